"""GPU parity of od_assign_tal (csrc/assign_tal.hip) against tests/tal_ref.py on the fixed cases of tests/tal_cases.py, under
the decided / undecided rule of tal_ref.check_image (u, v, claim order and rows exact; the metric within tau; only priors
within tau of a box's cut at rank topk may go either way); the raw C ABI on guarded buffers with garbage in the padding
slots; exact ties; determinism; the argument checks; Trainer(assigner="tal"); the static assigners left as they were; and
a short training run."""
import ctypes as C
import pathlib
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent))

import lattice_ref as L  # noqa: E402
import tal_cases as tc  # noqa: E402
import tal_ref  # noqa: E402
from object_detector_amd import priors as PR  # noqa: E402
from oracle import loss as oloss  # noqa: E402

pytestmark = pytest.mark.gpu


def _pb(cuda, case):
    from object_detector_amd.pb import PriorBoxes
    size, (B, nc, gmax), k, flagged = case
    return PriorBoxes(size, nc, device=cuda, assigner="tal", tal_topk=k, tal_alpha=tc.ALPHA, tal_beta=tc.BETA,
                      ignore_regions=flagged)


def _check(case, y, assigned, npos, metric):
    """the parity rule on every image of a case -> the largest relative metric error"""
    anns, _pred, refs, _shown = tc.reference(case)
    size, (B, nc, gmax), k, flagged = case
    pri = PR.make_priors(size)
    worst = 0.0
    for i, (a, r) in enumerate(zip(anns, refs)):
        worst = max(worst, tal_ref.check_image(r, a.bboxes, a.classes, pri, nc, y[i], assigned[i], npos[i],
                                               None if metric is None else metric[i]))
    return worst


@pytest.mark.parametrize("case", tc.CASES, ids=str)
def test_parity_with_the_reference(cuda, case):
    anns, pred, refs, shown = tc.reference(case)
    assert tc.expected(case) <= shown, f"the reference's output does not show {sorted(tc.expected(case) - shown)}"
    assert tc.undecided_share(refs) <= tc.UNDECIDED_CAP
    assert any(a.num_objects == 0 for a in anns)
    pb = _pb(cuda, case)
    y, npos, assigned = pb.encode_batch(anns, pred=torch.tensor(pred).to(cuda))
    worst = _check(case, y, assigned, npos, pb.last_metric.cpu().numpy())
    print(f"{case}: max |metric - l| / (1 + |l|) = {worst:.3g}")  # check_image asserted tau; DESIGN.md records this figure


# ---- the raw C ABI -------------------------------------------------------------------------------------------------------

def _pack(anns, gmax, rng, over=None):
    """boxes / classes / flags / counts as the C ABI takes them; every slot at or above an image's count holds NaN or
    garbage; counts[over] is raised above Gmax (the slots of that image are all real, so the clamp leaves them alone)."""
    B = len(anns)
    gb = np.full((B, gmax, 4), np.nan, np.float32)
    gb[:, :, 2:] = rng.uniform(-5, 5, (B, gmax, 2))  # half NaN, half garbage
    gc = rng.integers(-(2 ** 30), 2 ** 30, (B, gmax)).astype(np.int32)
    gf = rng.integers(-(2 ** 30), 2 ** 30, (B, gmax)).astype(np.int32)
    gn = np.zeros(B, np.int32)
    for i, a in enumerate(anns):
        n = a.num_objects
        gb[i, :n], gc[i, :n], gf[i, :n], gn[i] = a.bboxes, a.classes, a.difficults, n
    if over is not None:
        assert gn[over] == gmax
        gn[over] = gmax + 37
    return gb, gc, gf, gn


def _abi_call(cuda, case, with_assigned=True, with_metric=True, dirty=0xA5, zero_flags=False):
    """od_assign_tal on guarded y / assigned_gt / npos / metric / workspace (the workspace arrives dirty, the outputs hold
    garbage) -> numpy (y, assigned, npos, metric)"""
    from object_detector_amd import _lib
    from object_detector_amd.net import Context, _stream_ptr
    size, (B, nc, gmax), k, flagged = case
    anns, pred = tc.reference(case)[:2]
    ctx = Context.get(cuda)
    pri = PR.make_priors(size)
    P = len(pri)
    levels = PR.level_shapes(size)
    grid_hw = (C.c_int32 * (2 * len(levels)))(*[v for hw in levels for v in hw])
    gb, gc, gf, gn = _pack(anns, gmax, np.random.default_rng(8), over=0)
    if zero_flags:
        gf[:] = 0
    dev = [torch.tensor(v).to(cuda) for v in (pri, gb, gc, gf, gn, pred)]
    gy = L.Guarded((B, P, nc + 6), torch.float32, cuda)
    ga = L.Guarded((B, P), torch.int32, cuda)
    gm = L.Guarded((B, P), torch.float32, cuda)
    gnp = L.Guarded((B,), torch.int32, cuda)
    wsb = ctx.lib.od_assign_tal_workspace_bytes(B, P, gmax)
    assert wsb == B * P * 32 == ctx.lib.od_assign_tal_workspace_bytes(B, P, 1), "the workspace grows with B * P only"
    gws = L.Guarded((wsb,), torch.uint8, cuda)
    gy.t.fill_(float("nan")), ga.t.fill_(-77), gm.t.fill_(float("nan")), gnp.t.fill_(-77), gws.t.fill_(dirty)
    rc = ctx.lib.od_assign_tal(ctx.handle, dev[0].data_ptr(), grid_hw, len(levels), PR.NUM_PRIORS, dev[5].data_ptr(),
                               dev[1].data_ptr(), dev[2].data_ptr(), dev[4].data_ptr(),
                               dev[3].data_ptr() if flagged or zero_flags else None, 0.5, tc.ALPHA, tc.BETA, k, B, P, gmax, nc,
                               0.1, gy.t.data_ptr(), ga.t.data_ptr() if with_assigned else None, gnp.t.data_ptr(),
                               gm.t.data_ptr() if with_metric else None, gws.t.data_ptr(), wsb, _stream_ptr())
    _lib.check(rc, "od_assign_tal")
    torch.cuda.synchronize()
    gws.check("workspace")
    y, npos, assigned, metric = gy.numpy("y"), gnp.numpy("npos"), ga.numpy("assigned_gt"), gm.numpy("metric")
    if not with_assigned:
        assert (assigned == -77).all(), "assigned_gt = NULL, yet something wrote the buffer"
    if not with_metric:
        assert np.isnan(metric).all(), "metric = NULL, yet something wrote the buffer"
    return y, assigned, npos, metric


ABI_CASES = [((64, 64), (4, 20, 7), 13, True), ((96, 160), (3, 300, 128), 32, True), ((96, 160), (4, 1, 1), 1, False),
             ((64, 64), (3, 300, 128), 1, False)]


@pytest.mark.parametrize("case", ABI_CASES, ids=str)
def test_guarded_buffers_and_garbage_padding(cuda, case):
    assert case in tc.CASES
    y, assigned, npos, metric = _abi_call(cuda, case)
    _check(case, y, assigned, npos, metric)
    y2, _a2, n2, _m2 = _abi_call(cuda, case, with_assigned=False, with_metric=False, dirty=0x00)
    assert y2.tobytes() == y.tobytes() and (n2 == npos).all(), "NULL outputs or a clean workspace changed the rows"


def test_same_call_twice_gives_the_same_bytes(cuda):
    case = ((96, 160), (3, 300, 128), 13, True)  # conflicts on hundreds of priors: the claims race, the keys decide
    assert "conflict" in tc.reference(case)[3]
    a, b = _abi_call(cuda, case), _abi_call(cuda, case, dirty=0x3C)
    for u, v in zip(a, b):
        assert u.tobytes() == v.tobytes()


def test_null_flags_equal_all_zero_flags(cuda):
    case = ((64, 64), (4, 20, 7), 13, False)
    a, b = _abi_call(cuda, case), _abi_call(cuda, case, zero_flags=True)
    for u, v in zip(a, b):
        assert u.tobytes() == v.tobytes()


def test_exact_ties_go_to_the_lower_prior_index(cuda):
    """8 identical priors per cell with identical pred rows: l is bit-equal inside a cell whatever the device's exp / log, so
    the cut at topk = 13 is decided by the prior index alone: nothing is undecided, and the result is the reference's."""
    from object_detector_amd import _lib
    from object_detector_amd.net import Context, _stream_ptr
    size, nc, k = (64, 64), 5, 13
    pri, pred = tc.identical_cells(size, nc, seed=5)
    P = len(pri)
    boxes = np.array([[tc.BIG_BOX, [0.05, 0.1, 0.6, 0.45]]], np.float32)
    classes = np.array([[2, 4]], np.int32)
    ref = tal_ref.encode_truth(boxes[0], classes[0], pred, pri, PR.level_shapes(size), nc, topk=k)
    assert not ref["undecided"].any() and (ref["assigned"] >= 0).sum() > k
    ctx = Context.get(cuda)
    levels = PR.level_shapes(size)
    grid_hw = (C.c_int32 * (2 * len(levels)))(*[v for hw in levels for v in hw])
    dev = [torch.from_numpy(v).to(cuda) for v in (pri, boxes, classes, np.array([2], np.int32), pred[None])]
    y = torch.empty((1, P, nc + 6), device=cuda)
    assigned = torch.empty((1, P), dtype=torch.int32, device=cuda)
    metric = torch.empty((1, P), device=cuda)
    npos = torch.empty((1,), dtype=torch.int32, device=cuda)
    ws = torch.empty((ctx.lib.od_assign_tal_workspace_bytes(1, P, 2),), dtype=torch.uint8, device=cuda)
    _lib.check(ctx.lib.od_assign_tal(ctx.handle, dev[0].data_ptr(), grid_hw, len(levels), PR.NUM_PRIORS, dev[4].data_ptr(),
                                     dev[1].data_ptr(), dev[2].data_ptr(), dev[3].data_ptr(), None, 0.5, 1.0, 6.0, k, 1, P, 2, nc,
                                     0.1, y.data_ptr(), assigned.data_ptr(), npos.data_ptr(), metric.data_ptr(), ws.data_ptr(),
                                     ws.numel(), _stream_ptr()), "od_assign_tal")
    a = assigned.cpu().numpy()[0]
    assert (a == ref["assigned"]).all()
    tal_ref.check_image(ref, boxes[0], classes[0], pri, nc, y.cpu().numpy()[0], a, npos.cpu().numpy()[0],
                        metric.cpu().numpy()[0])


def test_bad_arguments_return_the_error_code(cuda):
    """argument checks only: nothing is launched (the outputs keep their poison)"""
    from object_detector_amd import _lib
    from object_detector_amd.net import Context, _stream_ptr
    ctx = Context.get(cuda)
    size, B, nc, gmax = (64, 64), 2, 3, 4
    pri = torch.from_numpy(PR.make_priors(size)).to(cuda)
    P = len(pri)
    levels = PR.level_shapes(size)
    gb = torch.zeros((B, 200, 4), device=cuda)
    gc = torch.zeros((B, 200), dtype=torch.int32, device=cuda)
    gn = torch.zeros((B,), dtype=torch.int32, device=cuda)
    pred = torch.zeros((B, P, 1024 + 8), device=cuda)
    y = torch.full((B, P, nc + 6), -7.0, device=cuda)
    metric = torch.full((B, P), -7.0, device=cuda)
    npos = torch.full((B,), -7, dtype=torch.int32, device=cuda)
    ws = torch.full((B * P * 32,), 0x5A, dtype=torch.uint8, device=cuda)

    def call(levels=levels, A=PR.NUM_PRIORS, topk=13, gmax=gmax, flags=None, ign_thr=0.5, wsb=None, alpha=1.0, beta=6.0, nc=nc,
             pred_ptr=pred.data_ptr()):
        grid_hw = (C.c_int32 * max(2, 2 * len(levels)))(*[v for hw in levels for v in hw])
        return ctx.lib.od_assign_tal(ctx.handle, pri.data_ptr(), grid_hw, len(levels), A, pred_ptr, gb.data_ptr(),
                                     gc.data_ptr(), gn.data_ptr(), flags, ign_thr, alpha, beta, topk, B, P, gmax, nc, 0.1,
                                     y.data_ptr(), None, npos.data_ptr(), metric.data_ptr(), ws.data_ptr(),
                                     ws.numel() if wsb is None else wsb, _stream_ptr())

    bad = {
        "levels do not add up to P": dict(levels=[(8, 8), (4, 4), (2, 3)]),
        "priors per cell do not add up to P": dict(A=7),
        "topk 0": dict(topk=0),
        "topk 33": dict(topk=33),
        "no level": dict(levels=[]),
        "five levels": dict(levels=[(8, 8), (4, 4), (2, 2), (1, 1), (1, 1)]),
        "Gmax 129": dict(gmax=129),
        "ign_thr 0 with flags": dict(flags=gc.data_ptr(), ign_thr=0.0),
        "ign_thr < 0 with flags": dict(flags=gc.data_ptr(), ign_thr=-1.0),
        "alpha 0": dict(alpha=0.0),
        "alpha < 0": dict(alpha=-1.0),
        "alpha NaN": dict(alpha=float("nan")),
        "alpha Inf": dict(alpha=float("inf")),
        "beta 0": dict(beta=0.0),
        "beta NaN": dict(beta=float("nan")),
        "beta Inf": dict(beta=float("inf")),
        "NC 0": dict(nc=0),
        "NC 1025": dict(nc=1025),
        "no pred": dict(pred_ptr=None),
    }
    for what, kw in bad.items():
        rc = call(**kw)
        assert rc == -1, what  # OD_ERR_INVALID
        with pytest.raises(_lib.OdError, match="od_assign_tal"):
            _lib.check(rc, "od_assign_tal")
    rc = call(wsb=B * P * 32 - 1)  # a short workspace is refused as well, with its own code
    assert rc == -3  # OD_ERR_WORKSPACE
    with pytest.raises(_lib.OdError, match="od_assign_tal: workspace"):
        _lib.check(rc, "od_assign_tal")
    torch.cuda.synchronize()
    assert (y == -7.0).all() and (npos == -7).all() and (metric == -7.0).all() and (ws == 0x5A).all(), \
        "a refused call wrote its outputs"
    assert call(flags=None, ign_thr=0.0) == 0  # without flags ign_thr is not read
    torch.cuda.synchronize()
    assert (y[:, :, 0] == 1).all() and (npos == 0).all() and (metric == 0).all()  # gt_counts are 0: every prior is background


# ---- Python layers ---------------------------------------------------------------------------------------------------------

def test_encode_batch_wants_a_device_pred_of_the_right_shape(cuda):
    case = ((64, 64), (4, 20, 7), 13, True)
    anns, pred = tc.reference(case)[:2]
    pb = _pb(cuda, case)
    good = torch.tensor(pred).to(cuda)
    for bad in (None, pred, good[:, :-1], good[:, :, :-1], good.double(), good.cpu()):
        with pytest.raises(ValueError, match="pred"):
            pb.encode_batch(anns, pred=bad)
    for call in (pb.encode_truth, pb.encode_truth_device):
        with pytest.raises(ValueError, match="Trainer.step"):
            call(anns)
    y, npos, assigned = pb.encode_batch(anns, return_device=True, pred=good)
    assert y.is_cuda and npos.is_cuda and assigned.is_cuda and tuple(pb.last_metric.shape) == tuple(assigned.shape)


def test_trainer_assigns_behind_the_forward_pass(cuda):
    """Trainer(assigner="tal").step(x, annotations=...): the target the step used is the reference's on tr.pred (decided
    rule), the loss is the oracle loss on that target, and a ready-made y_target is refused."""
    from object_detector_amd.trainer import Trainer
    from test_gpu_trainer import _setup
    Bs, Ss = 2, 96
    params, x, anns = _setup(cuda, Bs, Ss)
    tr = Trainer(params, Bs, (Ss, Ss), device=cuda, lr=0.0, momentum=0.0, loss_scale=256.0, assigner="tal", tal_topk=13,
                 tal_alpha=1.0, tal_beta=6.0)
    assert tr.pb.assigner == "tal" and (tr.pb.tal_topk, tr.pb.tal_alpha, tr.pb.tal_beta) == (13, 1.0, 6.0)
    xt = torch.from_numpy(x).to(cuda)
    with pytest.raises(ValueError, match="annotations"):
        tr.step(xt, y_target=torch.zeros((Bs, tr.P, tr.C), device=cuda))
    with pytest.raises(ValueError, match="annotations"):
        tr.step(xt)
    tr.step(xt, annotations=anns)
    torch.cuda.synchronize()
    pred = tr.pred.float().cpu().numpy()
    y, npos = tr.last_target.cpu().numpy(), tr.last_npos.cpu().numpy()
    assert tr.last_npos.is_cuda and npos.shape == (Bs,) and npos.sum() > 0
    levels = PR.level_shapes((Ss, Ss))
    for i, a in enumerate(anns):
        ref = tal_ref.encode_truth(a.bboxes, a.classes, pred[i], tr.pb.pb_locs, levels, tr.num_classes, topk=13,
                                   loc_scale=tr.pb.loc_scale)
        assert ref["undecided"].sum() <= max(1, tc.UNDECIDED_CAP * ref["claimed_any"].sum())
        dec = ~ref["undecided"]
        assert y[i][dec].tobytes() == ref["y"][dec].tobytes()
        assigned = np.where(y[i][:, 1] == 1, 0, -1)
        assert ref["claimed_sure"].sum() <= (assigned >= 0).sum() == npos[i] <= ref["claimed_any"].sum()
    losses = tr.losses.cpu().numpy().copy()
    rl, _rg = oloss.loss_and_grad(pred, y, tr.num_classes)
    np.testing.assert_allclose(losses, rl, rtol=2e-5)
    # the static assigners keep their order and count their positives too
    tr2 = Trainer(params, Bs, (Ss, Ss), device=cuda, lr=0.0, momentum=0.0, loss_scale=256.0)
    tr2.step(xt, annotations=anns)
    y2, n2, _ = tr2.pb.encode_batch(anns, return_device=True)
    assert torch.equal(tr2.last_npos, n2) and torch.equal(tr2.last_target, y2)
    tr2.step(xt, y_target=y2)
    assert tr2.last_npos is None


def test_static_assigners_ignore_pred(cuda):
    from object_detector_amd.pb import PriorBoxes
    case = ((96, 160), (4, 20, 7), 13, True)
    anns, pred = tc.reference(case)[:2]
    pt = torch.tensor(pred).to(cuda)
    outs = {}
    for name in ("max-iou", "atss"):
        pb = PriorBoxes((96, 160), 20, device=cuda, assigner=name, ignore_regions=True)
        a, b = pb.encode_batch(anns), pb.encode_batch(anns, pred=pt)
        for u, v in zip(a, b):
            assert u.tobytes() == v.tobytes()
        assert a[1].sum() > 0
        outs[name] = a[0]
    yt = _pb(cuda, case).encode_batch(anns, pred=pt)[0]
    assert yt.tobytes() != outs["max-iou"].tobytes() and yt.tobytes() != outs["atss"].tobytes()


def test_a_short_run_trains(cuda):
    """40 steps on generated shapes with assigner="tal": the generator yields annotation lists, every step assigns from its own
    predictions, every loss is finite, no step is skipped, the loss falls, and every step has positives."""
    sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent.parent / "scripts"))
    import _common
    import train as train_script
    from object_detector_amd import od_gen, weights as W
    from object_detector_amd.trainer import Trainer
    B, S, STEPS = 16, 160, 40
    X, y = _common.shapes_dataset(64, seed=0)
    params0 = train_script.init_for_training(W.random_init(2))
    tr = Trainer(params0, B, (S, S), device=cuda, lr=0.02, momentum=0.9, weight_decay=1e-4, lr_multipliers={"h.": 1.0 / 3.0},
                 assigner="tal")
    gen = od_gen.create_generator((S, S), preprocess_input=None, encode_truth=None, device=cuda, on_device=True,
                                  device_cache=True)
    batches, _ = gen.flow(X, y, batch_size=B, data_augmentation=True, shuffle=True, seed=0, prefetch=2)
    schedule = train_script.cosine_schedule(0.02, STEPS, 10)
    hist = torch.zeros((STEPS, 4), device=cuda)
    npos = torch.zeros((STEPS,), dtype=torch.int64, device=cuda)
    for i, (xb, anns) in zip(range(STEPS), batches):
        assert isinstance(anns, list)
        tr.lr = float(schedule(i))
        tr.step(xb, annotations=anns)
        hist[i].copy_(tr.losses)
        npos[i] = tr.last_npos.sum()
    batches.close()
    tr._poll_nonfinite(wait=True)
    hist, npos = hist.cpu().numpy(), npos.cpu().numpy()
    first, last = float(hist[:10, 3].mean()), float(hist[-10:, 3].mean())
    print(f"tal total loss {first:.3f} -> {last:.3f}, positives per image {npos.mean() / B:.1f}")
    assert np.isfinite(hist).all() and tr.skipped_steps == 0
    assert (npos > 0).all()
    assert last < first, (first, last)
