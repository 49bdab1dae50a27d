"""GPU: the quality targets (csrc/quality.hip: od_quality_iou, od_quality_tal) and the quality-aware objectness terms of
od_loss_fwd_bwd_quality (csrc/loss.hip) against tests/quality_ref.py, on guarded, NaN-poisoned buffers; Trainer(objectness=...).

Quality targets: everything f32 is compared bit for bit (od_quality_iou whole; od_quality_tal's forced rows, the rows that carry
an object's umax, and the zeros); aligned rows of od_quality_tal within quality_ref.aligned_rtol of the f64 value.
Loss: the tolerances of test_gpu_loss.py (gradient rtol 1e-4 / atol 1e-8, losses rtol 2e-5); the general cases keep
|q - p| >= 1e-3 on every assigned row (asserted on the reference), a separate case goes to |q - p| in [1e-7, 1e-4]."""
import ctypes as C
import functools
import pathlib
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent))

import iou_loss_ref as IR  # noqa: E402
import lattice_ref as L  # noqa: E402
import quality_ref as qr  # noqa: E402
import tal_cases as tc  # noqa: E402
from object_detector_amd import priors as PR  # noqa: E402
from test_gpu_loss import GRAD_TOL, LOSS_RTOL, _Guarded, _rows_case  # noqa: E402

pytestmark = pytest.mark.gpu

NAN = float("nan")


def _lib_ctx(cuda):
    from object_detector_amd import _lib
    from object_detector_amd.net import Context, _stream_ptr
    return _lib, Context.get(cuda), _stream_ptr


# ---------------------------------------------------------------- od_quality_iou

def _anns(size, B, nc, seed):
    from object_detector_amd.pb import ObjectsAnnotation
    rng = np.random.default_rng(seed)
    anns = []
    for i in range(B):
        n = 0 if i == 1 else (6 if i == 0 else int(rng.integers(2, 6)))  # image 1 has no object, image 0 six
        c = rng.uniform(0.2, 0.8, (n, 2))
        wh = rng.uniform(0.15, 0.7, (n, 2))
        anns.append(ObjectsAnnotation(None, size[1], size[0], rng.integers(0, nc, n),
                                      np.clip(np.concatenate([c - wh / 2, c + wh / 2], 1), 0, 1).astype(np.float32)))
    return anns


@pytest.mark.parametrize("assigner", ["max-iou", "atss", "tal"])
@pytest.mark.parametrize("B,nc", [(4, 1), (3, 20), (2, 300)])
@pytest.mark.parametrize("size", [(64, 64), (96, 160)], ids=str)
def test_quality_iou_is_the_reference_bit_for_bit(cuda, size, B, nc, assigner):
    from object_detector_amd.pb import PriorBoxes
    _lib, ctx, _sp = _lib_ctx(cuda)
    seed = size[1] + 10 * B + nc
    anns = _anns(size, B, nc, seed)
    pb = PriorBoxes(size, nc, device=cuda, assigner=assigner)
    P = len(pb)
    rng = np.random.default_rng(seed + 1)
    pred = np.concatenate([rng.normal(0, 2, (B, P, 2 + nc)), rng.normal(0, 0.5, (B, P, 4))], 2).astype(np.float32)
    y, npos, _a = pb.encode_batch(anns, pred=torch.tensor(pred).to(cuda))
    assert npos[0] >= 5 and npos[1] == 0
    # crafted rows of image 0 (the target is ready-made from here on): a prediction with crossed corners, NaN / Inf offsets,
    # an ignored row (all-zero target) that holds NaN offsets too, a prediction that IS the target
    rows = np.nonzero(y[0, :, 1] > 0.5)[0]
    pri = pb.pb_locs
    pw = pri[rows[0], 2] - pri[rows[0], 0]
    pred[0, rows[0], -4:] = y[0, rows[0], -4:]
    pred[0, rows[0], -4] += 1.5 * (pri[rows[0], 2] - pri[rows[0], 0] + 1.0) / (0.1 * pw)  # x1 far beyond x2
    pred[0, rows[1], -3] = np.nan
    pred[0, rows[2], -1] = np.inf
    y[0, rows[3]] = 0
    pred[0, rows[3], -4:] = np.nan
    pred[0, rows[4], -4:] = y[0, rows[4], -4:]
    ref = qr.quality_iou(pred, y, pri)
    d = qr.decode(pred[0, rows[:1], -4:], pri[rows[:1]])
    assert d[0, 0] > d[0, 2], "the crafted row does not cross its corners"
    assert ref[0, rows[1]] == 0 and ref[0, rows[2]] == 0 and ref[0, rows[3]] == 0 and ref[0, rows[4]] > 0.999
    assert (ref[1] == 0).all() and ((ref > 0) & (ref < 0.999)).sum() >= 1 and ((ref >= 0) & (ref <= 1)).all()
    gq = L.Guarded((B, P), torch.float32, cuda)
    gq.t.fill_(NAN)
    dp, dy, dpr = (torch.tensor(v).to(cuda) for v in (pred, y, pri))
    _lib.check(ctx.lib.od_quality_iou(ctx.handle, dp.data_ptr(), dy.data_ptr(), dpr.data_ptr(), 0.1, B, P, nc,
                                      gq.t.data_ptr(), _sp()), "od_quality_iou")
    torch.cuda.synchronize()
    q = gq.numpy("q")
    assert q.tobytes() == ref.tobytes(), f"{(q.view(np.int32) != ref.view(np.int32)).sum()} rows differ"
    from object_detector_amd import ops
    assert ops.quality_targets(dp, dy, dpr).cpu().numpy().tobytes() == ref.tobytes()


# ---------------------------------------------------------------- od_quality_tal

def _tal_inputs(cuda, case):
    """the case's annotations and pred through od_assign_tal on the device -> device tensors (pred, y, priors, gt_boxes,
    assigned, metric) and their numpy copies"""
    from object_detector_amd.pb import PriorBoxes
    size, (B, nc, gmax), k, flagged = case
    anns, pred = tc.reference(case)[:2]
    pb = PriorBoxes(size, nc, device=cuda, assigner="tal", tal_topk=k, tal_alpha=tc.ALPHA, tal_beta=tc.BETA,
                    ignore_regions=flagged)
    dp = torch.tensor(pred).to(cuda)
    up = pb.upload_batch(anns)
    y, _npos, assigned = pb.encode_uploaded(up, return_device=True, pred=dp)
    dev = (dp, y, pb.priors_device, up[2].contiguous(), assigned, pb.last_metric)
    return dev, tuple(t.cpu().numpy() for t in dev)


def _quality_tal_abi(cuda, dev, nc, dirty, wsb=None, pred_ptr=None):
    _lib, ctx, _sp = _lib_ctx(cuda)
    dp, y, pri, gb, assigned, metric = dev
    B, P = assigned.shape
    gmax = gb.shape[1]
    need = ctx.lib.od_quality_tal_workspace_bytes(B, gmax)
    assert need == B * gmax * 8
    gq = L.Guarded((B, P), torch.float32, cuda)
    gws = L.Guarded((need,), torch.uint8, cuda)
    gq.t.fill_(NAN), gws.t.fill_(dirty)
    rc = ctx.lib.od_quality_tal(ctx.handle, dp.data_ptr() if pred_ptr is None else pred_ptr, y.data_ptr(), pri.data_ptr(), 0.1,
                                gb.data_ptr(), assigned.data_ptr(), metric.data_ptr(), B, P, gmax, nc, gq.t.data_ptr(),
                                gws.t.data_ptr(), need if wsb is None else wsb, _sp())
    torch.cuda.synchronize()
    gws.check("workspace")
    return rc, gq.numpy("q")


@pytest.mark.parametrize("case", tc.CASES, ids=str)
def test_quality_tal_against_the_reference(cuda, case):
    _lib, _ctx, _sp = _lib_ctx(cuda)
    size, (B, nc, gmax), k, flagged = case
    dev, host = _tal_inputs(cuda, case)
    ref = qr.quality_tal(*host)
    assert ref["aligned"].sum() > 0 and ref["forced"].sum() > 0, "the case shows no aligned or no forced row"
    assert (~ref["exact"]).sum() > 0 or k == 1
    rc, q = _quality_tal_abi(cuda, dev, nc, 0xA5)
    _lib.check(rc, "od_quality_tal")
    assert np.isfinite(q).all() and ((q >= 0) & (q <= 1)).all()
    ex = ref["exact"]
    want = ref["q"].astype(np.float32)
    assert ref["q"][ex].tobytes() == want[ex].astype(np.float64).tobytes()  # exact rows hold f32 numbers
    assert q[ex].tobytes() == want[ex].tobytes(), "a forced row, a umax row or a zero differs"
    err = np.abs(q[~ex].astype(np.float64) - ref["q"][~ex])
    tol = qr.aligned_rtol(ref["dl"][~ex]) * ref["q"][~ex]
    assert (err <= tol).all(), f"aligned rows off by up to {(err / np.maximum(tol, 1e-300)).max():.3g} x the tolerance"
    worst = float((err / np.maximum(tol, 1e-300)).max()) if err.size else 0.0
    print(f"{case}: max err / tolerance on aligned rows = {worst:.3g}")  # DESIGN.md records the largest of these
    rc2, q2 = _quality_tal_abi(cuda, dev, nc, 0x3C)  # another dirt in the workspace: same bytes
    assert rc2 == 0 and q2.tobytes() == q.tobytes()
    from object_detector_amd import ops
    q3 = ops.quality_targets(dev[0], dev[1], dev[2], mode="tal", assigned=dev[4], metric=dev[5], gt_boxes=dev[3])
    assert q3.cpu().numpy().tobytes() == q.tobytes()


def test_quality_tal_row_without_an_object_gets_zero(cuda):
    """od_assign_tal never writes it, but the entry takes any buffers: a row whose target says assigned while assigned_gt is
    negative or >= Gmax reads no box, touches no table slot and gets q = 0 (the documented rule); every other row keeps
    its value unless it shared an object with the rows taken out."""
    _lib, _ctx, _sp = _lib_ctx(cuda)
    case = ((64, 64), (4, 20, 7), 13, False)
    dev, host = _tal_inputs(cuda, case)
    assigned = host[4].copy()
    rows = np.argwhere((host[1][..., 1] > 0.5) & (host[5] < 0))  # aligned rows
    assert len(rows) >= 4
    for (b, p), g in zip(rows[:4], (7, 1 << 20, -1, -3)):
        assigned[b, p] = g
    dev2 = dev[:4] + (torch.tensor(assigned).to(cuda), dev[5])
    ref = qr.quality_tal(host[0], host[1], host[2], host[3], assigned, host[5])
    rc, q = _quality_tal_abi(cuda, dev2, 20, 0xA5)
    _lib.check(rc, "od_quality_tal")
    for b, p in rows[:4]:
        assert q[b, p] == 0 and ref["q"][b, p] == 0
    ex = ref["exact"]
    assert q[ex].tobytes() == ref["q"].astype(np.float32)[ex].tobytes()
    err = np.abs(q[~ex].astype(np.float64) - ref["q"][~ex])
    assert (err <= qr.aligned_rtol(ref["dl"][~ex]) * ref["q"][~ex]).all()


def test_quality_entries_refuse_bad_arguments(cuda):
    _lib, ctx, _sp = _lib_ctx(cuda)
    case = ((64, 64), (4, 20, 7), 13, False)
    dev, _host = _tal_inputs(cuda, case)
    dp, y, pri, gb, assigned, metric = dev
    B, P = assigned.shape
    rc, q = _quality_tal_abi(cuda, dev, 20, 0x11, wsb=B * 7 * 8 - 1)
    assert rc == -3 and np.isnan(q).all()  # OD_ERR_WORKSPACE, nothing written
    with pytest.raises(_lib.OdError, match="od_quality_tal: workspace"):
        _lib.check(rc, "od_quality_tal")
    rc, q = _quality_tal_abi(cuda, dev, 20, 0x11, pred_ptr=dp.data_ptr() + 4)
    assert rc == -1 and np.isnan(q).all()
    with pytest.raises(_lib.OdError, match="16-byte aligned"):
        _lib.check(rc, "od_quality_tal")
    for nc in (0, 1025):
        rc, q = _quality_tal_abi(cuda, dev, nc, 0x11)
        assert rc == -1 and np.isnan(q).all()
    out = torch.full((B, P), NAN, device=cuda)
    ws = torch.zeros(B * 7 * 8, dtype=torch.uint8, device=cuda)

    def iou(pred=dp.data_ptr(), yy=y.data_ptr(), pr=pri.data_ptr(), nc=20, qq=out.data_ptr()):
        return ctx.lib.od_quality_iou(ctx.handle, pred, yy, pr, 0.1, B, P, nc, qq, _sp())
    for kw in (dict(pred=None), dict(yy=None), dict(pr=None), dict(qq=None), dict(nc=0), dict(nc=1025),
               dict(pred=dp.data_ptr() + 4), dict(pr=pri.data_ptr() + 4)):
        assert iou(**kw) == -1, kw
        with pytest.raises(_lib.OdError, match="od_quality_iou"):
            _lib.check(-1, "od_quality_iou")
    for null in ("gb", "assigned", "metric", "ws"):
        ptrs = dict(gb=gb.data_ptr(), assigned=assigned.data_ptr(), metric=metric.data_ptr(), ws=ws.data_ptr())
        ptrs[null] = None
        assert ctx.lib.od_quality_tal(ctx.handle, dp.data_ptr(), y.data_ptr(), pri.data_ptr(), 0.1, ptrs["gb"], ptrs["assigned"],
                                      ptrs["metric"], B, P, 7, 20, out.data_ptr(), ptrs["ws"], ws.numel(), _sp()) == -1, null
    torch.cuda.synchronize()
    assert torch.isnan(out).all(), "a refused call wrote its output"


# ---------------------------------------------------------------- od_loss_fwd_bwd_quality

OBJ = {"focal": 0, "qfl": 1, "vfl": 2}
BOX = {"smooth_l1": 0, "mse": 1, "giou": 2, "diou": 3, "ciou": 4}
CRAFTED_Q = (0.0, 1.0, 1e-6)
CRAFTED_Z = (0.5, -1.0, 2.0)  # p = 0.62, 0.27, 0.88: every crafted q keeps |q - p| > 0.1


@functools.lru_cache(maxsize=None)
def _quality_case(regime, NC, R=2000, n_pos=40, n_ign=60):
    """test_gpu_loss.py's rows of the regime; three assigned rows get moderate objectness logits and the crafted qualities
    0, 1, 1e-6; every other row draws q uniformly, from the first seed that keeps |q - p| >= 1e-3 on every assigned row."""
    pred, y = _rows_case(17 + len(regime) + NC, R, NC, regime, n_pos, n_ign)
    pos = np.nonzero(y[:, 1] > 0.5)[0]
    for r, z in zip(pos[:3], CRAFTED_Z):
        pred[r, 0], pred[r, 1] = -z / 2, z / 2
    for seed in range(200):
        q = np.random.default_rng(1000 + seed).uniform(0, 1, R).astype(np.float32)
        q[pos[:3]] = CRAFTED_Q
        if qr.min_gap(pred, y, q) >= 1e-3:
            break
    assert qr.min_gap(pred, y, q) >= 1e-3
    for a in (pred, y, q):
        a.setflags(write=False)
    return pred, y, q


def _far_q(pred, seed):
    """q on the far side of 1/2 from p (p > 1/2: q in [0.12, 0.2]; p <= 1/2: q in [0.57, 0.95]): |q - p| >= 0.07 on every
    row without a seed search, at any row count"""
    z = pred[:, 1] - pred[:, 0]
    u = np.random.default_rng(seed).uniform(0.6, 1.0, len(pred))
    return (np.where(z > 0, 0.2, 0.95) * u).astype(np.float32)


def _abi_loss(cuda, pred, y, q, NC, mode, alpha=0.25, gamma=2.0, box_mode="smooth_l1", w=(1.0, 1.0, 1.0), B=1, priors=None,
              entry="quality"):
    """od_loss_fwd_bwd_quality (or od_loss_fwd_bwd_iou) through the C ABI on guarded buffers, the workspace pre-filled with
    0xFF -> (rc, losses [4], grad [R,C])"""
    _lib, ctx, _sp = _lib_ctx(cuda)
    R, Cc = y.shape
    gp = _Guarded(cuda, R, Cc, NAN, pred)
    gy = _Guarded(cuda, R, Cc, 1.0, y)
    gg = _Guarded(cuda, R, Cc, NAN)
    gl = _Guarded(cuda, 1, 4, NAN)
    gq = None if q is None else _Guarded(cuda, R, 1, NAN, q)
    dpr = None if priors is None else torch.tensor(priors).to(cuda)
    wsb = ctx.lib.od_loss_workspace_bytes(B, R // B)
    ws = torch.full((wsb + 256,), 0xFF, dtype=torch.uint8, device=cuda)
    head = (ctx.handle, gp.ptr(), gy.ptr(), None if dpr is None else dpr.data_ptr(), gg.ptr(), gl.ptr(), B, R // B, NC,
            float(alpha), float(gamma), BOX[box_mode], 0.1, float(w[0]), float(w[1]), float(w[2]))
    if entry == "quality":
        rc = ctx.lib.od_loss_fwd_bwd_quality(*head, None if gq is None else gq.ptr(), OBJ[mode], ws.data_ptr(), wsb, _sp())
    else:
        rc = ctx.lib.od_loss_fwd_bwd_iou(*head, ws.data_ptr(), wsb, _sp())
    torch.cuda.synchronize()
    for g, what in ((gp, "pred"), (gy, "y"), (gg, "grad"), (gl, "losses")) + (() if gq is None else ((gq, "quality"),)):
        g.assert_guards_unchanged(what)
    assert (ws[wsb:] == 0xFF).all(), "bytes after the workspace written"
    return rc, gl.payload(), gg.payload().reshape(R, Cc)


def _check(losses, grad, rl, rg):
    assert np.isfinite(rl).all() and np.isfinite(rg).all(), "reference not finite"
    assert np.isfinite(losses).all() and np.isfinite(grad).all(), "device output not finite"
    np.testing.assert_allclose(losses, rl, rtol=LOSS_RTOL)
    np.testing.assert_allclose(grad, rg.reshape(grad.shape), **GRAD_TOL)


@pytest.mark.parametrize("NC", [20, 80])
@pytest.mark.parametrize("gamma", [1.0, 2.0, 3.0])
@pytest.mark.parametrize("mode", ["qfl", "vfl"])
@pytest.mark.parametrize("regime", ["init", "trained", "saturated", "wrong"])
def test_loss_regimes(cuda, regime, mode, gamma, NC):
    """R = 2 x 1000: seven full 256-row workgroups and one of 208 rows; NC = 20 | 80: od_loss_rows | od_loss_rows_wide"""
    from object_detector_amd import ops
    pred, y, q = _quality_case(regime, NC)
    rl, rg = qr.loss_and_grad(pred, y, q, NC, mode, gamma=gamma)
    assert (rl != 0).all()
    shape = (2, 1000, NC + 6)
    losses, grad = ops.loss_fwd_bwd(torch.tensor(pred.reshape(shape)).to(cuda), torch.tensor(y.reshape(shape)).to(cuda), NC,
                                    gamma=gamma, objectness=mode, quality=torch.tensor(q.reshape(2, 1000)).to(cuda))
    _check(losses.cpu().numpy(), grad.cpu().numpy().reshape(-1, NC + 6), rl, rg)


@pytest.mark.parametrize("NC", [20, 80])
@pytest.mark.parametrize("mode", ["qfl", "vfl"])
@pytest.mark.parametrize("alpha,w,box_mode", [(0.5, (1.0, 1.0, 1.0), "smooth_l1"), (0.25, (2.0, 0.5, 3.0), "mse"),
                                              (0.5, (2.0, 0.5, 3.0), "giou")], ids=["alpha", "weights", "giou"])
def test_loss_parameters(cuda, alpha, w, box_mode, mode, NC):
    if box_mode == "giou":
        pred, y, priors = IR.case("sd1.5", NC)
        pred, y = pred.reshape(-1, NC + 6), y.reshape(-1, NC + 6)
        B = IR.B
        q = _far_q(pred, 5)
        assert qr.min_gap(pred, y, q) >= 1e-3
    else:
        pred, y, q = _quality_case("trained", NC)
        priors, B = None, 2
    rl, rg = qr.loss_and_grad(pred, y, q, NC, mode, alpha=alpha, box_mode=box_mode, w=w, priors=priors)
    rc, losses, grad = _abi_loss(cuda, pred, y, q, NC, mode, alpha=alpha, box_mode=box_mode, w=w, B=B, priors=priors)
    assert rc == 0
    if box_mode == "giou":
        # all four losses at LOSS_RTOL, objectness and class columns at GRAD_TOL; the box columns at test_gpu_iou_loss.py's
        # per-row bound (4 x the f32 restatement's row-relative error), every other row exactly zero
        _check(losses, grad[:, :2 + NC], rl, rg[:, :2 + NC])
        pos = y[:, 1] > 0.5
        assert np.isfinite(grad[:, -4:]).all() and (grad[~pos, -4:] == 0).all()
        err = IR.row_rel_err(grad[pos, -4:], rg[pos, -4:])
        bound = 4 * IR.F32_ROWREL_MAX[("sd1.5", "giou")]
        print(f"giou box columns under {mode}: worst row-relative error {err.max():.3e}, bound {bound:.3e}")
        assert (err <= bound).all()
    else:
        _check(losses, grad, rl, rg)


@pytest.mark.parametrize("NC", [20, 80])
@pytest.mark.parametrize("R", [1, 255, 256, 257, 513])
def test_loss_row_blocking_with_guards(cuda, R, NC):
    pred, y = _rows_case(100 * R + NC, R, NC, "trained", max(1, R // 9), R // 13)
    if R > 1:
        y[-1] = y[np.nonzero(y[:, 1] > 0.5)[0][0]]  # the last row of the partial block is an assigned one
    pos = y[:, 1] > 0.5
    q = _far_q(pred, R)
    assert qr.min_gap(pred, y, q) >= 1e-3 and pos.any()
    for mode, gamma in (("qfl", 2.0), ("qfl", 1.0), ("vfl", 2.0)):
        rl, rg = qr.loss_and_grad(pred, y, q, NC, mode, gamma=gamma)
        rc, losses, grad = _abi_loss(cuda, pred, y, q, NC, mode, gamma=gamma)
        assert rc == 0
        _check(losses, grad, rl, rg)


@pytest.mark.parametrize("NC", [20, 80])
@pytest.mark.parametrize("box_mode", ["smooth_l1", "giou"])
def test_mode_0_and_background_rows_are_the_focal_entrys_bits(cuda, box_mode, NC):
    if box_mode == "giou":
        pred, y, priors = IR.case("sd1.5", NC)
        pred, y, B = pred.reshape(-1, NC + 6), y.reshape(-1, NC + 6), IR.B
    else:
        pred, y, _q = _quality_case("trained", NC)
        priors, B = None, 2
    q = np.random.default_rng(9).uniform(0, 1, len(pred)).astype(np.float32)
    q[np.nonzero(y[:, 1] > 0.5)[0][:2]] = [0.0, np.nan]
    kw = dict(box_mode=box_mode, B=B, priors=priors, gamma=2.0)
    rc, fl, fg = _abi_loss(cuda, pred, y, None, NC, "focal", entry="iou", **kw)
    assert rc == 0 and np.isfinite(fl).all()
    for quality in (None, q):  # mode 0 does not read quality
        rc, l0, g0 = _abi_loss(cuda, pred, y, quality, NC, "focal", **kw)
        assert rc == 0 and l0.tobytes() == fl.tobytes() and g0.tobytes() == fg.tobytes()
    bg = y[:, 1] < 0.5
    for mode in ("qfl", "vfl"):
        rc, l1, g1 = _abi_loss(cuda, pred, y, q, NC, mode, **kw)
        assert rc == 0 and np.isfinite(l1).all()
        assert g1[bg].tobytes() == fg[bg].tobytes(), "a background row's gradient differs from the focal entry's"
        assert g1[:, 2:].tobytes() == fg[:, 2:].tobytes(), "class or box columns differ"
        assert l1[1:3].tobytes() == fl[1:3].tobytes()
        assert not np.array_equal(g1[~bg, :2], fg[~bg, :2])


@pytest.mark.parametrize("NC", [20, 80])
@pytest.mark.parametrize("gamma", [2.0, 3.0])
def test_loss_near_equality_of_quality_and_probability(cuda, gamma, NC):
    """assigned rows with |q - p| in [1e-7, 1e-4] (gamma >= 2: at gamma = 1 the sign of p - q decides the gradient): their
    objectness gradient within 1e-7 * w_obj / max(1, npos): the rounding of p, 2^-24, times the slope bound
    2 * 0.25 * log 2, with a margin of about 2.5."""
    pred, y = _rows_case(31 + NC, 600, NC, "init", 48, 20)
    pos = np.nonzero(y[:, 1] > 0.5)[0]
    _l, _g, p = qr.objectness(pred, y, np.zeros(len(pred)), "qfl")
    rng = np.random.default_rng(3)
    delta = np.exp(rng.uniform(np.log(2e-7), np.log(9e-5), len(pos))) * rng.choice([-1.0, 1.0], len(pos))
    q = np.zeros(len(pred), np.float32)
    q[pos] = (p[pos] + delta).astype(np.float32)
    gap = np.abs(q[pos].astype(np.float64) - p[pos])
    keep = (gap >= 1e-7) & (gap <= 1e-4) & (q[pos] > 0) & (q[pos] < 1)
    assert keep.sum() >= 40, keep.sum()
    near = pos[keep]
    w_obj = 2.0
    rl, rg = qr.loss_and_grad(pred, y, q, NC, "qfl", gamma=gamma, w=(w_obj, 1.0, 1.0))
    rc, losses, grad = _abi_loss(cuda, pred, y, q, NC, "qfl", gamma=gamma, w=(w_obj, 1.0, 1.0))
    assert rc == 0 and np.isfinite(grad).all() and np.isfinite(losses).all()
    atol = 1e-7 * w_obj / max(1, len(pos))
    err = np.abs(grad[near, :2] - rg[near, :2]).max()
    print(f"near-equality rows: max |g - ref| = {err:.3g} (bound {atol:.3g})")
    assert err <= atol
    np.testing.assert_allclose(losses, rl, rtol=LOSS_RTOL)
    rest = np.setdiff1d(np.arange(len(pred)), near)
    np.testing.assert_allclose(grad[rest], rg[rest], **GRAD_TOL)


@pytest.mark.parametrize("NC", [20, 80])
@pytest.mark.parametrize("mode", ["qfl", "vfl"])
@pytest.mark.parametrize("bad", [np.inf, -np.inf, np.nan], ids=["+inf", "-inf", "nan"])
def test_nonfinite_objectness_logit_stays_visible(cuda, bad, mode, NC):
    base, y, q = _quality_case("trained", NC, 300, 12, 6)
    pos = np.nonzero(y[:, 1] > 0.5)[0]
    bg = np.nonzero(y[:, 0] > 0.5)[0]
    ign = np.nonzero(y.sum(1) == 0)[0]
    qq = q.copy()
    qq[pos[4]] = 0.0  # an assigned row that varifocal sends through the background term
    pred = base.copy()
    pred[ign] = bad
    rc, losses, grad = _abi_loss(cuda, pred, y, qq, NC, mode)
    assert rc == 0 and np.isfinite(losses).all() and np.isfinite(grad).all() and (grad[ign] == 0).all()
    for r, c in ((pos[0], 0), (pos[3], 1), (pos[4], 1), (bg[0], 0), (bg[-1], 1)):
        p2 = pred.copy()
        p2[r, c] = bad
        rc, losses, grad = _abi_loss(cuda, p2, y, qq, NC, mode)
        assert rc == 0 and not np.isfinite(losses[3]), (r, c, losses)
        assert not np.isfinite(grad[r, :2]).any(), (r, c, grad[r, :2])
        assert np.isfinite(np.delete(grad, r, 0)).all() and (grad[ign] == 0).all()


def test_loss_entry_refuses_bad_arguments(cuda):
    _lib, _ctx, _sp = _lib_ctx(cuda)
    pred, y, q = _quality_case("trained", 20, 300, 12, 6)
    rc, losses, grad = _abi_loss(cuda, pred, y, q, 20, "qfl", gamma=0.5)
    assert rc == -1 and np.isnan(losses).all() and np.isnan(grad).all()
    with pytest.raises(_lib.OdError, match="focal_gamma >= 1"):
        _lib.check(rc, "od_loss_fwd_bwd_quality")
    for mode in ("qfl", "vfl"):
        rc, losses, grad = _abi_loss(cuda, pred, y, None, 20, mode)
        assert rc == -1 and np.isnan(losses).all() and np.isnan(grad).all()
        with pytest.raises(_lib.OdError, match="needs the quality targets"):
            _lib.check(rc, "od_loss_fwd_bwd_quality")
    OBJ["bad"] = 3
    try:
        rc, losses, grad = _abi_loss(cuda, pred, y, q, 20, "bad")
    finally:
        del OBJ["bad"]
    assert rc == -1 and np.isnan(grad).all()
    rc, losses, grad = _abi_loss(cuda, pred, y, q, 20, "vfl", gamma=0.5)  # varifocal takes any gamma >= 0
    assert rc == 0 and np.isfinite(losses).all()
    rl, rg = qr.loss_and_grad(pred, y, q, 20, "vfl", gamma=0.5)
    _check(losses, grad, rl, rg)


# ---------------------------------------------------------------- Trainer

def _trainer_setup(B=4, S=64, nc=3):
    from object_detector_amd import weights as W
    from oracle import network as onet
    params = W.random_init(2, num_classes=nc)
    x = onet.synthetic_images(B, S, seed=0)
    anns = _anns((S, S), B, nc, 4)
    return params, x, anns


@pytest.mark.parametrize("assigner,quality", [("max-iou", "iou"), ("tal", "tal")])
def test_trainer_steps_with_quality_targets(cuda, assigner, quality):
    from object_detector_amd.trainer import Trainer
    params, x, anns = _trainer_setup()
    tr = Trainer(params, 4, (64, 64), device=cuda, lr=1e-3, loss_scale=256.0, assigner=assigner, objectness="qfl",
                 quality=quality)
    assert tr.num_classes == 3 and tuple(tr.last_quality.shape) == (4, tr.P)
    xt = torch.from_numpy(x).to(cuda)
    for _ in range(3):
        tr.step(xt, annotations=anns)
        torch.cuda.synchronize()
        losses = tr.losses.cpu().numpy()
        q, y = tr.last_quality.cpu().numpy(), tr.last_target.cpu().numpy()
        assert np.isfinite(losses).all() and losses[0] > 0
        pos = y[..., 1] > 0.5
        assert pos.sum() > 0 and ((q >= 0) & (q <= 1)).all() and (q[~pos] == 0).all() and (q[pos] > 0).any()
        assert (q[1] == 0).all()  # the image without objects
    # the step's q is the reference's on the step's own pred and target
    pred = tr.pred.cpu().numpy()
    if quality == "iou":
        assert q.tobytes() == qr.quality_iou(pred, y, tr.pb.pb_locs, tr.pb.loc_scale).tobytes()
        tr.last_quality.fill_(NAN)  # forward() + loss(): loss() computes the quality of ITS pred and target itself
        tr.loss(tr.last_target)
        torch.cuda.synchronize()
        assert tr.last_quality.cpu().numpy().tobytes() == q.tobytes() and np.isfinite(tr.losses.cpu().numpy()).all()
    else:
        with pytest.raises(ValueError, match="tal_inputs"):
            tr.loss(tr.last_target)
    tr._poll_nonfinite(wait=True)
    assert tr.skipped_steps == 0


def test_trainer_focal_is_unchanged(cuda):
    from object_detector_amd.trainer import Trainer
    params, x, anns = _trainer_setup()
    xt = torch.from_numpy(x).to(cuda)
    a = Trainer(params, 4, (64, 64), device=cuda, lr=0.0, momentum=0.0, loss_scale=256.0)
    b = Trainer(params, 4, (64, 64), device=cuda, lr=0.0, momentum=0.0, loss_scale=256.0, objectness="focal", quality="iou")
    assert a.last_quality is None and b.last_quality is None
    a.step(xt, annotations=anns)
    b.step(xt, annotations=anns)
    torch.cuda.synchronize()
    assert a.grad_pred.cpu().numpy().tobytes() == b.grad_pred.cpu().numpy().tobytes()
    assert a.losses.cpu().numpy().tobytes() == b.losses.cpu().numpy().tobytes()
    assert np.isfinite(a.losses.cpu().numpy()).all()
