"""GPU: box modes giou / diou / ciou of od_loss_fwd_bwd_iou (csrc/loss.hip) against tests/iou_loss_ref.py, whose gradient comes
from autograd in f64 and shares no algebra with the kernel's hand-derived one.

Shapes: B = 3, P = 300 (R = 900: three full 256-row workgroups and one of 132 rows; image boundaries inside workgroups, so
r % P wraps mid-block; P no multiple of 256 or 64), 300 random priors, 60 assigned rows (first / last rows of workgroups and of
images among them), 40 ignore rows.  Box gradients are compared PER ROW, as max_k |dg_k| <= 4 x (the f32 restatement's recorded
maximum for the case and mode) x max_k |g_ref_k|: an element-wise rtol is the wrong bound for components that cancel to near
zero against the row's largest.  The factor 4 covers the kernel's op order and its 1-ulp v_rcp_f32.  No row is left out: the
inputs are required to stay clear of every min / max / clamp tie instead (asserted here and in test_iou_loss_host.py)."""
import functools

import numpy as np
import pytest
import torch

import iou_loss_ref as R
from test_gpu_loss import LOSS_RTOL, _Guarded

pytestmark = pytest.mark.gpu

NCS = [20, 74, 75, 80]  # the LDS kernel, its last class count, the first streamed one, COCO


def _dev(a, cuda):
    return torch.tensor(np.asarray(a), device=cuda)  # a copy: the cached cases are read-only


def _run(cuda, pred, y, priors, NC, mode, **kw):
    from object_detector_amd import ops
    pr = None if priors is None else _dev(priors, cuda)
    losses, grad = ops.loss_fwd_bwd(_dev(pred, cuda), _dev(y, cuda), NC, box_mode=mode, priors=pr, loc_scale=R.LOC_SCALE, **kw)
    return losses.cpu().numpy(), grad.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _reference(regime, NC, mode, w=(1.0, 1.0, 1.0)):
    pred, y, priors = R.case(regime, NC)
    rl, rg = R.full_reference(pred, y, priors, NC, mode, R.LOC_SCALE, w=w)
    rg.setflags(write=False)
    return rl, rg


def _check_box(grad, rg, y, bound, what):
    """Per assigned row: max_k |dg_k| <= bound * max_k |g_ref_k|; every other row exactly zero.  Prints the worst row."""
    pos = y[..., 1] > 0.5
    g, r = grad[..., -4:], rg[..., -4:]
    assert np.isfinite(g).all(), f"{what}: non-finite box gradient"
    assert (g[~pos] == 0).all(), f"{what}: box gradient on a row that is not assigned"
    err = R.row_rel_err(g[pos], r[pos])
    print(f"{what}: worst row-relative box-gradient error {err.max():.3e}, bound {bound:.3e}")
    assert (err <= bound).all(), f"{what}: rows {np.nonzero(err > bound)[0]} of the assigned ones, errors {err[err > bound]}"


# ---------------------------------------------------------------- 1. parity

@pytest.mark.parametrize("regime", list(R.REGIMES))
@pytest.mark.parametrize("NC", NCS)
@pytest.mark.parametrize("mode", list(R.MODES))
def test_iou_loss_matches_reference(cuda, mode, NC, regime):
    pred, y, priors = R.case(regime, NC)
    assert (np.abs(R.case_margins(regime)) >= R.MARGIN_MIN).all(), "an input row sits on a min / max tie"
    rl, rg = _reference(regime, NC, mode)
    assert np.isfinite(rl).all() and np.isfinite(rg).all() and (rl[:3] != 0).all()
    losses, grad = _run(cuda, pred, y, priors, NC, mode)
    assert np.isfinite(losses).all(), losses
    print(f"{mode} NC {NC} {regime}: losses {losses}, reference {rl}")
    np.testing.assert_allclose(losses, rl, rtol=LOSS_RTOL)
    _check_box(grad, rg, y, 4 * R.F32_ROWREL_MAX[(regime, mode)], f"{mode} NC {NC} {regime}")
    # the other columns do not know about the box mode
    l0, g0 = _run(cuda, pred, y, None, NC, "smooth_l1")
    assert np.array_equal(losses[:2].view(np.int32), l0[:2].view(np.int32))
    assert np.array_equal(grad[..., :-4].view(np.int32), g0[..., :-4].view(np.int32))


# ---------------------------------------------------------------- 2. modes 0 / 1 through the new entry, 3. guards and poison

def _abi_call(cuda, pred, y, priors, NC, mode, w=(1.0, 1.0, 1.0), B=R.B, entry="od_loss_fwd_bwd_iou"):
    """The C ABI on guarded buffers (pred / grad / losses guards NaN, y guards 1.0 = an assigned row, prior-table guards NaN),
    the workspace pre-filled with 0xFF.  priors None -> NULL.  -> (losses [4], grad [R, C]) as numpy."""
    from object_detector_amd import _lib
    from object_detector_amd.net import Context, _stream_ptr
    from object_detector_amd.ops import BOX_MODES
    ctx = Context.get(cuda)
    R_, Cc = y.shape
    gp = _Guarded(cuda, R_, Cc, float("nan"), pred)
    gy = _Guarded(cuda, R_, Cc, 1.0, y)
    gg = _Guarded(cuda, R_, Cc, float("nan"))
    gl = _Guarded(cuda, 1, 4, float("nan"))
    gpr = None if priors is None else _Guarded(cuda, len(priors), 4, float("nan"), priors)
    wsb = ctx.lib.od_loss_workspace_bytes(B, R_ // B)
    ws = torch.full((wsb + 256,), 0xFF, dtype=torch.uint8, device=cuda)
    tail = (float(w[0]), float(w[1]), float(w[2]), ws.data_ptr(), wsb, _stream_ptr())
    if entry == "od_loss_fwd_bwd":
        rc = ctx.lib.od_loss_fwd_bwd(ctx.handle, gp.ptr(), gy.ptr(), gg.ptr(), gl.ptr(), B, R_ // B, NC, 0.25, 2.0,
                                     BOX_MODES[mode], *tail)
    else:
        rc = ctx.lib.od_loss_fwd_bwd_iou(ctx.handle, gp.ptr(), gy.ptr(), None if gpr is None else gpr.ptr(), gg.ptr(),
                                         gl.ptr(), B, R_ // B, NC, 0.25, 2.0, BOX_MODES[mode], R.LOC_SCALE, *tail)
    _lib.check(rc, entry)
    torch.cuda.synchronize()
    for g, what in ((gp, "pred"), (gy, "y"), (gg, "grad"), (gl, "losses")) + (() if gpr is None else ((gpr, "priors"),)):
        g.assert_guards_unchanged(what)
    assert (ws[wsb:] == 0xFF).all(), "bytes after the workspace written"
    assert np.array_equal(gp.payload().view(np.int32), np.ascontiguousarray(pred).reshape(-1).view(np.int32)), "pred modified"
    if gpr is not None:
        assert np.array_equal(gpr.payload(), np.ascontiguousarray(priors).reshape(-1)), "priors modified"
    return gl.payload(), gg.payload().reshape(R_, Cc)


@pytest.mark.parametrize("NC", [20, 80])
@pytest.mark.parametrize("mode", ["smooth_l1", "mse"])
def test_old_modes_through_the_new_entry_are_byte_identical(cuda, mode, NC):
    pred, y, _priors = R.case("sd1.5", NC)
    p2, y2 = pred.reshape(-1, NC + 6), y.reshape(-1, NC + 6)
    w = (2.0, 0.5, 3.0)
    l_old, g_old = _abi_call(cuda, p2, y2, None, NC, mode, w=w, entry="od_loss_fwd_bwd")
    l_new, g_new = _abi_call(cuda, p2, y2, None, NC, mode, w=w)
    assert np.isfinite(l_old).all() and (l_old[:3] != 0).all()
    assert l_old.tobytes() == l_new.tobytes() and g_old.tobytes() == g_new.tobytes()


def test_iou_entry_rejects_bad_arguments(cuda):
    from object_detector_amd.net import Context, _stream_ptr
    ctx = Context.get(cuda)
    pred, y, priors = R.case("sd1.5", 20)
    p, t, pr = _dev(pred, cuda), _dev(y, cuda), _dev(priors, cuda)
    g, l = torch.zeros_like(p), torch.zeros(4, device=cuda)
    wsb = ctx.lib.od_loss_workspace_bytes(R.B, R.P)
    ws = torch.zeros(wsb, dtype=torch.uint8, device=cuda)

    def call(prp, mode):
        return ctx.lib.od_loss_fwd_bwd_iou(ctx.handle, p.data_ptr(), t.data_ptr(), prp, g.data_ptr(), l.data_ptr(), R.B, R.P,
                                           20, 0.25, 2.0, mode, R.LOC_SCALE, 1.0, 1.0, 1.0, ws.data_ptr(), wsb, _stream_ptr())
    for mode in (2, 3, 4):
        assert call(None, mode) != 0  # an IoU mode needs the prior table
    assert call(pr.data_ptr(), 5) != 0 and call(pr.data_ptr(), -1) != 0
    assert call(pr.data_ptr() + 4, 2) != 0  # the 16-byte prior loads need an aligned table
    # od_loss_fwd_bwd still knows modes 0 and 1 only
    assert ctx.lib.od_loss_fwd_bwd(ctx.handle, p.data_ptr(), t.data_ptr(), g.data_ptr(), l.data_ptr(), R.B, R.P, 20, 0.25, 2.0,
                                   2, 1.0, 1.0, 1.0, ws.data_ptr(), wsb, _stream_ptr()) != 0
    torch.cuda.synchronize()
    assert not g.any() and not l.any()  # nothing was launched
    assert call(pr.data_ptr(), 2) == 0
    torch.cuda.synchronize()


@pytest.mark.parametrize("NC", [20, 80])
@pytest.mark.parametrize("mode", list(R.MODES))
def test_guards_and_poisoned_rows(cuda, mode, NC):
    """Every buffer and the prior table between guard rows, a dirty workspace, and NaN in the loc columns of every row that
    is not assigned (pred and target alike): guards unchanged, exactly zero box gradient on those rows, finite losses, the
    assigned rows as in the clean run."""
    pred, y, priors = R.case("sd1.5", NC)
    p2, y2 = pred.reshape(-1, NC + 6).copy(), y.reshape(-1, NC + 6).copy()
    pos = y2[:, 1] > 0.5
    p2[~pos, -4:] = np.nan
    y2[~pos, -4:] = np.nan  # (an ignore row is recognised by its first two columns)
    losses, grad = _abi_call(cuda, p2, y2, priors, NC, mode)
    assert np.isfinite(losses).all(), losses
    assert (grad[~pos, -4:] == 0).all() and np.isfinite(grad).all()
    rl, rg = _reference("sd1.5", NC, mode)
    np.testing.assert_allclose(losses, rl, rtol=LOSS_RTOL)
    _check_box(grad.reshape(y.shape), rg, y, 4 * R.F32_ROWREL_MAX[("sd1.5", mode)], f"guarded {mode} NC {NC}")
    l2, g2 = _abi_call(cuda, p2, y2, priors, NC, mode)  # deterministic, whatever the workspace held
    assert losses.tobytes() == l2.tobytes() and grad.tobytes() == g2.tobytes()


# ---------------------------------------------------------------- 4. non-finite input stays visible

@pytest.mark.parametrize("NC", [20, 80])
@pytest.mark.parametrize("bad", [np.inf, np.nan], ids=["+inf", "nan"])
@pytest.mark.parametrize("mode", list(R.MODES))
def test_nonfinite_loc_column_reaches_the_gradient(cuda, mode, bad, NC):
    pred, y, priors = R.case("sd1.5", NC)
    _l, clean = _run(cuda, pred, y, priors, NC, mode)
    pos = np.nonzero(y.reshape(-1, NC + 6)[:, 1] > 0.5)[0]
    for row, col in ((pos[0], 0), (pos[17], 3), (pos[-1], 2)):  # rows 0 and 899 among them, every kind of corner
        p2 = pred.reshape(-1, NC + 6).copy()
        p2[row, NC + 2 + col] = bad
        losses, grad = _run(cuda, p2.reshape(pred.shape), y, priors, NC, mode)
        grad = grad.reshape(-1, NC + 6)
        assert not np.isfinite(grad[row, -4:]).any(), (row, col, grad[row, -4:])
        assert np.isfinite(losses[:2]).all() and not np.isfinite(losses[2]) and not np.isfinite(losses[3]), losses
        others = np.arange(len(grad)) != row
        assert np.array_equal(grad[others].view(np.int32), clean.reshape(-1, NC + 6)[others].view(np.int32))
        assert np.array_equal(grad[row, :-4].view(np.int32), clean.reshape(-1, NC + 6)[row, :-4].view(np.int32))


# ---------------------------------------------------------------- 5. degenerate rows

@pytest.mark.parametrize("NC", [20, 80])
@pytest.mark.parametrize("mode", list(R.MODES))
def test_degenerate_rows_stay_finite(cuda, mode, NC):
    """A predicted box of zero width and a prediction equal to its target: finite loss and gradients.  Only finiteness is
    compared on these two rows (the derivative at an exact tie is a convention); they have a case of their own so that the
    parity test leaves nothing out."""
    pred, y, priors = R.case("sd1.5", NC)
    p2, y2 = pred.reshape(-1, NC + 6).copy(), y.reshape(-1, NC + 6)
    pos = np.nonzero(y2[:, 1] > 0.5)[0]
    zero_w, equal = pos[5], pos[40]
    p2[zero_w, -4:] = (5.0, 0.0, -5.0, 0.0)  # both x corners at the prior's centre
    p2[equal, -4:] = y2[equal, -4:]
    losses, grad = _run(cuda, p2.reshape(pred.shape), y, priors, NC, mode)
    assert np.isfinite(losses).all() and np.isfinite(grad).all(), losses
    grad, ref = grad.reshape(-1, NC + 6), _reference("sd1.5", NC, mode)[1].reshape(-1, NC + 6)
    rest = np.setdiff1d(pos, [zero_w, equal])
    err = R.row_rel_err(grad[rest, -4:], ref[rest, -4:])
    assert (err <= 4 * R.F32_ROWREL_MAX[("sd1.5", mode)]).all()
    # the second row alone: its loss is eps / area
    y1 = np.zeros_like(y2)
    y1[:, 0] = 1
    y1[equal] = y2[equal]
    l1, g1 = _run(cuda, p2.reshape(pred.shape), y1.reshape(y.shape), priors, NC, mode)
    assert np.isfinite(l1).all() and np.isfinite(g1).all()
    print(f"{mode} NC {NC}: loss of a prediction equal to its target {l1[2]:.3e}")
    assert 0 <= abs(l1[2]) <= 1e-5


# ---------------------------------------------------------------- 6. weights

@pytest.mark.parametrize("NC", [20, 80])
@pytest.mark.parametrize("mode", list(R.MODES))
def test_weights(cuda, mode, NC):
    pred, y, priors = R.case("sd1.5", NC)
    losses, grad = _run(cuda, pred, y, priors, NC, mode, weights=(1.0, 1.0, 0.0))
    assert np.isfinite(losses).all() and losses[2] == 0 and (grad[..., -4:] == 0).all()
    assert losses[3] == np.float32(losses[0] + losses[1]) and losses[0] != 0 and losses[1] != 0
    w = (2.0, 0.5, 3.0)
    rl, rg = _reference("sd1.5", NC, mode, w)
    losses, grad = _run(cuda, pred, y, priors, NC, mode, weights=w)
    assert np.isfinite(losses).all() and np.isfinite(grad).all()
    np.testing.assert_allclose(losses, rl, rtol=LOSS_RTOL)
    _check_box(grad, rg, y, 4 * R.F32_ROWREL_MAX[("sd1.5", mode)], f"weights {mode} NC {NC}")
    np.testing.assert_allclose(grad[..., :-4], rg[..., :-4], rtol=1e-4, atol=1e-8)


# ---------------------------------------------------------------- 7. Trainer plumbing, 8. sign of the whole chain

def test_trainer_passes_priors_scale_and_weights(cuda):
    from object_detector_amd import ops
    from object_detector_amd.trainer import Trainer
    from test_gpu_trainer import _setup
    Bs, Ss = 2, 96
    params, x, anns = _setup(cuda, Bs, Ss)
    w = (1.0, 1.0, 2.0)
    tr = Trainer(params, Bs, (Ss, Ss), device=cuda, lr=0.0, momentum=0.0, loss_scale=256.0, box_mode="ciou", loss_weights=w)
    y, _npos, _ = tr.pb.encode_batch(anns, return_device=True)
    tr.step(torch.from_numpy(x).to(cuda), annotations=anns)
    torch.cuda.synchronize()
    losses = tr.losses.cpu().numpy().copy()
    l2, g2 = ops.loss_fwd_bwd(tr.pred, y, tr.num_classes, box_mode="ciou", priors=tr.pb.priors_device,
                              loc_scale=tr.pb.loc_scale, weights=w)
    assert np.isfinite(losses).all() and losses[2] > 0
    assert losses.tobytes() == l2.cpu().numpy().tobytes() and torch.equal(tr.grad_pred.view(torch.int32), g2.view(torch.int32))
    rl, _rg = R.full_reference(tr.pred.cpu().numpy(), y.cpu().numpy(), tr.pb.pb_locs, tr.num_classes, "ciou", tr.pb.loc_scale,
                               w=w)
    np.testing.assert_allclose(losses, rl, rtol=LOSS_RTOL)
    with pytest.raises(ValueError, match="box_mode"):
        Trainer(params, Bs, (Ss, Ss), device=cuda, box_mode="iou")


def test_giou_training_lowers_the_box_loss(cuda):
    """30 steps on one fixed batch: a gradient with the wrong sign or in the wrong columns cannot lower the box loss."""
    from object_detector_amd.trainer import Trainer
    from test_gpu_trainer import _setup
    Bs, Ss = 2, 96
    params, x, anns = _setup(cuda, Bs, Ss)
    tr = Trainer(params, Bs, (Ss, Ss), device=cuda, lr=0.01, momentum=0.9, loss_scale=256.0, box_mode="giou")
    xt = torch.from_numpy(x).to(cuda)
    y, _n, _ = tr.pb.encode_batch(anns, return_device=True)

    def batches():
        while True:
            yield xt, y
    hist = tr.fit(batches(), 30)
    tr._poll_nonfinite(wait=True)
    assert np.isfinite(hist).all() and tr.skipped_steps == 0, f"{tr.skipped_steps} skipped steps"
    first, last = hist[:5, 2].mean(), hist[-5:, 2].mean()
    print(f"giou box loss: first 5 steps {first:.4f}, last 5 steps {last:.4f}, drop {first - last:.4f}")
    assert last < first
