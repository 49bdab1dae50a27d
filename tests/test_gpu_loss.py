"""GPU: od_loss_fwd_bwd (csrc/loss.hip) where a detector actually lives -- saturated logits, gamma != 2, non-default alpha and
weights, row counts around the 256-row blocking, both row kernels (NC <= 74: od_loss_rows, NC > 74: od_loss_rows_wide) -- and
od_pred_grad_to_level (csrc/train.hip) on its own.

The reference is oracle/loss.py (f64, cancellation-free; checked against 400-digit arithmetic in tests/test_loss_host.py) fed
the same f32 pred and y.  Tolerances are those of test_gpu_train_ops.py::test_loss_matches_oracle: gradient rtol 1e-4 /
atol 1e-8, losses rtol 2e-5.  Every comparison first asserts that both sides are finite: assert_allclose alone accepts a NaN
opposite a NaN."""
import functools

import numpy as np
import pytest
import torch

from oracle import loss as oloss

pytestmark = pytest.mark.gpu

GAMMAS = [2.0, 0.0, 0.5, 1.0, 3.0]
GRAD_TOL = dict(rtol=1e-4, atol=1e-8)
LOSS_RTOL = 2e-5
MODES = {"smooth_l1": 0, "mse": 1}

# regime: (background margin mean, sd), (assigned-row margin mean, sd), (true-class boost, sd).  Margin d is in favour of the
# right answer: l_t = c + d/2, l_other = c - d/2, c ~ N(0, 1).
REGIMES = {
    "init": ((4.6, 0.3), (0.0, 2.0), (0.0, 1.0)),        # objectness bias set so that every prior starts at p = 0.01
    "trained": ((10.0, 3.0), (3.0, 2.0), (9.0, 1.0)),
    "late": ((14.0, 4.0), (4.7, 2.0), (14.0, 1.0)),
    "saturated": ((40.0, 20.0), (13.0, 2.0), (40.0, 1.0)),
    "wrong": ((-20.0, 10.0), (-3.3, 2.0), (-10.0, 1.0)),
    "extreme": ((0.0, 70.0), (0.0, 70.0), (0.0, 70.0)),
}


def _targets(rng, R, NC, pos_rows, ign_rows):
    y = np.zeros((R, NC + 6), np.float32)
    y[:, 0] = 1
    y[pos_rows, 0], y[pos_rows, 1] = 0, 1
    y[pos_rows, 2 + rng.integers(0, NC, len(pos_rows))] = 1
    y[pos_rows, -4:] = rng.normal(0, 1, (len(pos_rows), 4))
    y[ign_rows] = 0
    return y


def _logits(rng, y, regime):
    (bm, bs), (pm, ps), (cb, cs) = REGIMES[regime]
    R, NC = y.shape[0], y.shape[1] - 6
    pos = y[:, 1] > 0.5
    d = np.where(pos, rng.normal(pm, ps, R), rng.normal(bm, bs, R))
    c = rng.normal(0, 1, R)
    pred = np.empty(y.shape, np.float64)
    pred[:, 0] = np.where(pos, c - d / 2, c + d / 2)
    pred[:, 1] = np.where(pos, c + d / 2, c - d / 2)
    pred[:, 2:2 + NC] = rng.normal(0, 1, (R, NC)) + y[:, 2:2 + NC] * (cb + rng.normal(0, cs, (R, 1)))
    pred[:, -4:] = rng.normal(0, 1.5, (R, 4))
    return pred.astype(np.float32)


def _rows_case(seed, R, NC, regime, n_pos, n_ign):
    rng = np.random.default_rng(seed)
    perm = rng.permutation(R)
    y = _targets(rng, R, NC, np.sort(perm[:n_pos]), np.sort(perm[n_pos:n_pos + n_ign]))
    return _logits(rng, y, regime), y


@functools.lru_cache(maxsize=None)
def _regime_case(regime, NC):
    """B = 2, P = 1000: seven full 256-row workgroups and one of 208 rows; 40 assigned, 60 ignore, 1900 background rows."""
    pred, y = _rows_case(sorted(REGIMES).index(regime), 2000, NC, regime, 40, 60)
    pred, y = pred.reshape(2, 1000, NC + 6), y.reshape(2, 1000, NC + 6)
    pred.setflags(write=False)
    y.setflags(write=False)
    return pred, y


def _dev(a, cuda):
    return torch.tensor(a, device=cuda)  # a copy: the cached cases are read-only


def _check(losses, grad, rl, rg):
    losses, grad = losses.cpu().numpy(), grad.cpu().numpy()
    assert np.isfinite(rl).all() and np.isfinite(rg).all(), "reference not finite"
    assert np.isfinite(losses).all(), f"device losses {losses}"
    assert np.isfinite(grad).all(), f"{(~np.isfinite(grad)).sum()} non-finite device gradient elements"
    np.testing.assert_allclose(losses, rl, rtol=LOSS_RTOL)
    np.testing.assert_allclose(grad, rg, **GRAD_TOL)


# ---------------------------------------------------------------- a. regimes x gamma x both kernels

@pytest.mark.parametrize("NC", [20, 80])
@pytest.mark.parametrize("gamma", GAMMAS)
@pytest.mark.parametrize("regime", list(REGIMES))
def test_loss_regimes(cuda, regime, gamma, NC):
    from object_detector_amd import ops
    pred, y = _regime_case(regime, NC)
    rl, rg = oloss.loss_and_grad(pred, y, NC, gamma=gamma)
    assert np.isfinite(rl).all() and (rl != 0).all(), f"degenerate regime: {rl}"
    losses, grad = ops.loss_fwd_bwd(_dev(pred, cuda), _dev(y, cuda), NC, gamma=gamma)
    _check(losses, grad, rl, rg)


# ---------------------------------------------------------------- b. alpha, weights, box mode

@pytest.mark.parametrize("NC", [20, 80])
@pytest.mark.parametrize("box_mode", list(MODES))
@pytest.mark.parametrize("weights", [(2.0, 0.5, 3.0), (1.0, 0.0, 1.0)], ids=["w2-0.5-3", "w1-0-1"])
@pytest.mark.parametrize("alpha", [0.25, 0.5, 0.9])
def test_loss_parameters(cuda, alpha, weights, box_mode, NC):
    from object_detector_amd import ops
    pred, y = _regime_case("trained", NC)
    rl, rg = oloss.loss_and_grad(pred, y, NC, alpha=alpha, box_mode=box_mode, w=weights)
    losses, grad = ops.loss_fwd_bwd(_dev(pred, cuda), _dev(y, cuda), NC, alpha=alpha,
                                    box_mode=box_mode, weights=weights)
    _check(losses, grad, rl, rg)
    losses, grad = losses.cpu().numpy(), grad.cpu().numpy()
    assert losses[0] != 0 and losses[2] != 0
    if weights[1] == 0:  # a zero weight: exactly zero component and gradient columns
        assert losses[1] == 0 and (grad[..., 2:2 + NC] == 0).all()
        assert losses[3] == np.float32(losses[0] + losses[2])


# ---------------------------------------------------------------- c. row blocking, guards, the strided count / final sum

class _Guarded:
    """`rows` x `C` f32 in the middle of a larger device buffer: `G` guard rows on either side hold `fill`."""
    G = 4  # 4 rows = 16 * C bytes: the payload keeps the 16-byte alignment the vector copies need

    def __init__(self, dev, rows, Cc, fill, data=None):
        self.buf = torch.full(((rows + 2 * self.G) * Cc,), fill, dtype=torch.float32, device=dev)
        self.n, self.g = rows * Cc, self.G * Cc
        if data is not None:
            self.buf[self.g:self.g + self.n] = torch.tensor(np.asarray(data).reshape(-1), device=dev)
        self.before = self.guards()

    def ptr(self):
        return self.buf.data_ptr() + 4 * self.g

    def payload(self):
        return self.buf[self.g:self.g + self.n].cpu().numpy()

    def guards(self):
        b = self.buf.view(torch.int32)
        return torch.cat([b[:self.g], b[self.g + self.n:]]).cpu().numpy()

    def assert_guards_unchanged(self, what):
        assert np.array_equal(self.guards(), self.before), f"{what}: guard rows written"


def _abi_call(cuda, pred, y, NC, alpha=0.25, gamma=2.0, box_mode="smooth_l1", w=(1.0, 1.0, 1.0), B=1):
    """od_loss_fwd_bwd through the C ABI on guarded buffers, the workspace pre-filled with 0xFF.  pred / grad guards are NaN,
    y guards are 1.0 (an assigned row: reading one would move the normaliser).  -> (losses[4], grad[R, C]) as numpy."""
    from object_detector_amd import _lib
    from object_detector_amd.net import Context, _stream_ptr
    ctx = Context.get(cuda)
    R, Cc = y.shape
    assert R % B == 0 and Cc == NC + 6
    gp = _Guarded(cuda, R, Cc, float("nan"), pred)
    gy = _Guarded(cuda, R, Cc, 1.0, y)
    gg = _Guarded(cuda, R, Cc, float("nan"))
    gl = _Guarded(cuda, 1, 4, float("nan"))
    wsb = ctx.lib.od_loss_workspace_bytes(B, R // B)
    ws = torch.full((wsb + 256,), 0xFF, dtype=torch.uint8, device=cuda)
    _lib.check(ctx.lib.od_loss_fwd_bwd(ctx.handle, gp.ptr(), gy.ptr(), gg.ptr(), gl.ptr(), B, R // B, NC, float(alpha),
                                       float(gamma), MODES[box_mode], float(w[0]), float(w[1]), float(w[2]), ws.data_ptr(),
                                       wsb, _stream_ptr()), "od_loss_fwd_bwd")
    torch.cuda.synchronize()
    for g, what in ((gp, "pred"), (gy, "y"), (gg, "grad"), (gl, "losses")):
        g.assert_guards_unchanged(what)
    assert (ws[wsb:] == 0xFF).all(), "bytes after the workspace written"
    assert np.array_equal(gp.payload(), np.ascontiguousarray(pred).reshape(-1)), "pred modified"
    return gl.payload(), gg.payload().reshape(R, Cc)


def _check_np(losses, grad, rl, rg):
    assert np.isfinite(rl).all() and np.isfinite(rg).all(), "reference not finite"
    assert np.isfinite(losses).all() and np.isfinite(grad).all(), "device output not finite"
    np.testing.assert_allclose(losses, rl, rtol=LOSS_RTOL)
    np.testing.assert_allclose(grad, rg, **GRAD_TOL)


@pytest.mark.parametrize("NC", [1, 3, 74, 75])
@pytest.mark.parametrize("R", [1, 255, 256, 257, 513])
def test_loss_row_blocking_with_guards(cuda, R, NC):
    """C = NC + 6 odd and even, R * C mostly no multiple of 4 (scalar tail of the vector copies), NC = 74 | 75 either side of
    the od_loss_rows / od_loss_rows_wide switch; every buffer sits between poisoned guard rows."""
    n_pos = max(1, R // 9)
    pred, y = _rows_case(100 * R + NC, R, NC, "trained", n_pos, R // 13)
    if R > 1:
        y[-1] = y[np.nonzero(y[:, 1] > 0.5)[0][0]]  # the last row of the partial block is an assigned one
        pred[-1, 2:2 + NC] += 9 * y[-1, 2:2 + NC]
    for gamma in (2.0, 0.5):
        rl, rg = oloss.loss_and_grad(pred, y, NC, gamma=gamma)
        losses, grad = _abi_call(cuda, pred, y, NC, gamma=gamma)
        _check_np(losses, grad, rl, rg)
        assert rl[0] != 0 and rl[2] != 0


@pytest.mark.parametrize("where", ["everywhere", "tail_only"])
def test_loss_more_rows_than_one_count_pass(cuda, where):
    """R = 524288 + 300 rows of 7 floats: od_loss_count's grid stops at 2048 x 256 rows, so the last 300 rows are counted by
    its stride loop, and od_loss_final sums 2050 partials with 256 threads.  `tail_only` puts every assigned row at or beyond
    row 524288: dropping the second pass would leave the normaliser at 1."""
    NC, R = 1, 524288 + 300
    rng = np.random.default_rng(7)
    if where == "everywhere":
        pos = np.union1d(rng.choice(R, 1000, replace=False), [524288, 524400, R - 1])
    else:
        pos = np.sort(524288 + rng.choice(300, 37, replace=False))
    ign = np.setdiff1d(rng.choice(R, 2000, replace=False), pos)
    y = _targets(rng, R, NC, pos, ign)
    pred = _logits(rng, y, "trained")
    rl, rg = oloss.loss_and_grad(pred, y, NC)
    losses, grad = _abi_call(cuda, pred, y, NC)
    assert losses[1] == 0 and rl[1] == 0  # one class: q = 1
    _check_np(losses, grad, rl, rg)
    assert rl[0] != 0 and rl[2] != 0


# ---------------------------------------------------------------- d. workspace contents and determinism

@pytest.mark.parametrize("NC", [20, 80])
def test_loss_deterministic_on_a_dirty_workspace(cuda, NC):
    pred, y = _regime_case("late", NC)
    p2, y2 = pred.reshape(-1, NC + 6), y.reshape(-1, NC + 6)
    l1, g1 = _abi_call(cuda, p2, y2, NC, gamma=0.5, B=2)
    l2, g2 = _abi_call(cuda, p2, y2, NC, gamma=0.5, B=2)
    assert np.isfinite(l1).all() and np.isfinite(g1).all()
    assert np.array_equal(l1.view(np.int32), l2.view(np.int32)) and np.array_equal(g1.view(np.int32), g2.view(np.int32))
    rl, rg = oloss.loss_and_grad(p2, y2, NC, gamma=0.5)
    _check_np(l1, g1, rl, rg)


@pytest.mark.parametrize("gamma", [0.0, 0.5])
def test_loss_no_positives_other_gammas(cuda, gamma):
    """test_gpu_train_ops.py::test_loss_no_positives (normaliser 1, not 0) for plain cross-entropy and gamma < 1."""
    from object_detector_amd import ops
    rng = np.random.default_rng(3)
    y = np.zeros((2, 700, 26), np.float32)
    y[..., 0] = 1
    y[1, 5:40] = 0  # some ignore rows
    pred = _logits(rng, y.reshape(-1, 26), "late").reshape(y.shape)
    rl, rg = oloss.loss_and_grad(pred, y, gamma=gamma)
    losses, grad = ops.loss_fwd_bwd(_dev(pred, cuda), _dev(y, cuda), gamma=gamma)
    _check(losses, grad, rl, rg)
    assert rl[0] > 0 and rl[1] == 0 and rl[2] == 0


# ---------------------------------------------------------------- e. non-finite input stays visible

@functools.lru_cache(maxsize=None)
def _nonfinite_case(NC):
    R = 300  # two workgroups
    rng = np.random.default_rng(11)
    pos = np.array([3, 100, 255, 256, 299])
    ign = np.array([7, 200, 298])
    y = _targets(rng, R, NC, pos, ign)
    y[100, 2:2 + NC] = 0
    y[100, 2] = 1  # row 100: true class 0
    return _logits(rng, y, "trained"), y


@pytest.mark.parametrize("NC", [20, 80])
@pytest.mark.parametrize("bad", [np.inf, -np.inf, np.nan], ids=["+inf", "-inf", "nan"])
@pytest.mark.parametrize("gamma", GAMMAS)
def test_loss_nonfinite_input_reaches_the_gradient(cuda, gamma, bad, NC):
    """The trainer skips a step when od_grad_nonfinite sees a non-finite gradient (test_gpu_conv_exact.py), so an overflowed
    logit must not be turned into a finite number: the row's gradient and losses[3] become non-finite.  Ignore rows (all-zero
    target) still get an exactly zero gradient and add nothing."""
    from object_detector_amd import ops
    base, y = _nonfinite_case(NC)
    yd = _dev(y, cuda)[None]

    def run(pred, box_mode="smooth_l1"):
        losses, grad = ops.loss_fwd_bwd(torch.from_numpy(pred).to(cuda)[None], yd, NC, gamma=gamma, box_mode=box_mode)
        return losses.cpu().numpy(), grad.cpu().numpy()[0]

    pred = base.copy()
    pred[[7, 200, 298]] = bad  # ignore rows only
    losses, grad = run(pred)
    assert np.isfinite(losses).all() and np.isfinite(grad).all() and (grad[[7, 200, 298]] == 0).all()
    # (row, column, box mode): background rows 0 / 257, assigned rows 100 (true class 0) / 256 / 299
    spots = [(0, 0, "smooth_l1"), (257, 1, "smooth_l1"), (100, 0, "smooth_l1"), (256, 1, "smooth_l1"),
             (100, 2, "smooth_l1"), (100, 2 + NC - 1, "smooth_l1"), (299, 2 + NC // 2, "smooth_l1"),
             (299, 2 + NC, "smooth_l1"), (100, NC + 5, "smooth_l1"), (256, NC + 3, "mse")]
    for r, c, mode in spots:
        p2 = pred.copy()
        p2[r, c] = bad
        losses, grad = run(p2, mode)
        assert not np.isfinite(losses[3]), (r, c, mode, losses)
        assert not np.isfinite(grad[r]).all(), (r, c, mode, grad[r])
        assert (grad[[7, 200, 298]] == 0).all(), (r, c, mode)


# ---------------------------------------------------------------- f. od_pred_grad_to_level

def _level_grad(rng, B, P, Cc):
    g = rng.normal(0, 1, (B, P, Cc)).astype(np.float32)
    g *= np.float32(2.0) ** rng.integers(-30, 8, (B, P, Cc)).astype(np.float32)  # down to f16 denormals and below
    special = np.array([
        1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, -(1 + 2.0 ** -11), 1 + 2.0 ** -11 + 2.0 ** -20,  # ties (to even) and just above
        2.0 ** -24, 2.0 ** -25, 3 * 2.0 ** -25, -(2.0 ** -25), 2.0 ** -25 * (1 + 2.0 ** -10), 2.0 ** -14 - 2.0 ** -25,  # denormals
        65504.0, 65519.996, 65520.0, -65520.0, 65536.0, 1e5, -7e4, 3e38, np.inf, -np.inf,  # the f16 overflow threshold
        63.96875, 63.984375, 63.99, 64.0, -63.984375, 2.0 ** -34, 2.0 ** -35, 3 * 2.0 ** -35, 0.0, -0.0,  # the same after x 1024
    ], np.float32)
    flat = g.reshape(-1)
    idx = rng.choice(flat.size, 40 * len(special), replace=False)
    flat[idx] = np.tile(special, 40)
    for b in range(B):  # and at the very ends of the copied ranges
        g[b, 0, 0], g[b, -1, -1], g[b, 1200, 0] = 65520.0, -65520.0, 1e5
        g[b, 7, 0], g[b, 7, 1], g[b, 7, -1] = 2.0 ** -25, 65520.0, 65519.996
    return g


@pytest.mark.parametrize("scale", [1.0, 1024.0])
@pytest.mark.parametrize("row_off,rows", [(0, 1500), (1200, 300), (7, 1)])
def test_pred_grad_to_level(cuda, row_off, rows, scale):
    """f32 loss gradient rows [row_off, row_off + rows) of every image -> loss-scaled f16, bit-exact against numpy's
    round-to-nearest-even conversion: ties, denormals, and overflow to +-Inf (never clamped to 65504)."""
    from object_detector_amd import _lib
    from object_detector_amd.net import Context, _stream_ptr
    ctx = Context.get(cuda)
    B, P, Cc, G = 3, 1500, 26, 64
    g = _level_grad(np.random.default_rng(5), B, P, Cc)
    with np.errstate(over="ignore"):
        ref = (g[:, row_off:row_off + rows] * np.float32(scale)).astype(np.float16)
    assert np.isinf(ref).sum() > np.isinf(g[:, row_off:row_off + rows]).sum()  # some finite values do overflow
    gd = torch.from_numpy(g).to(cuda)
    n = B * rows * Cc
    dz = torch.full((n + 2 * G,), 0x5A5A, dtype=torch.int16, device=cuda)
    _lib.check(ctx.lib.od_pred_grad_to_level(ctx.handle, gd.data_ptr(), dz.data_ptr() + 2 * G, B, P, Cc, row_off, rows,
                                             scale, _stream_ptr()), "od_pred_grad_to_level")
    torch.cuda.synchronize()
    out = dz.cpu().numpy()
    assert (out[:G] == 0x5A5A).all() and (out[G + n:] == 0x5A5A).all(), "guard elements around dz written"
    assert np.array_equal(out[G:G + n].view(np.uint16), ref.reshape(-1).view(np.uint16))
    assert np.array_equal(gd.cpu().numpy().view(np.int32), g.view(np.int32))
    # a range that leaves the image is rejected before anything is launched
    assert ctx.lib.od_pred_grad_to_level(ctx.handle, gd.data_ptr(), dz.data_ptr() + 2 * G, B, P, Cc, P - rows + 1, rows,
                                         scale, _stream_ptr()) != 0
    assert ctx.lib.od_pred_grad_to_level(ctx.handle, gd.data_ptr(), dz.data_ptr() + 2 * G, B, P, Cc, -1, rows,
                                         scale, _stream_ptr()) != 0
    torch.cuda.synchronize()
    assert np.array_equal(dz.cpu().numpy(), out)
