"""GPU parity of od_assign_atss (csrc/assign_atss.hip) against tests/atss_ref.py, bit for bit, on the fixed cases of
tests/atss_cases.py; the raw C ABI on guarded buffers with garbage in the padding slots; determinism; the argument checks;
Trainer(assigner="atss"); and the default assigner left as it was."""
import ctypes as C
import pathlib
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent))

import atss_cases as ac  # noqa: E402
import atss_ref  # noqa: E402
import lattice_ref as L  # noqa: E402
from object_detector_amd import priors as PR  # noqa: E402
from oracle import loss as oloss  # noqa: E402

pytestmark = pytest.mark.gpu


def _pb(cuda, case):
    from object_detector_amd.pb import PriorBoxes
    size, (B, nc, gmax), k, flagged = case
    return PriorBoxes(size, nc, device=cuda, assigner="atss", atss_topk=k, ignore_regions=flagged)


@pytest.mark.parametrize("case", ac.CASES, ids=str)
def test_bit_exact_against_the_reference(cuda, case):
    anns, ry, ra, rn, shown = ac.reference(case)
    assert ac.expected(case) <= shown, f"the reference's output does not show {sorted(ac.expected(case) - shown)}"
    assert any(a.num_objects == 0 for a in anns)
    y, npos, assigned = _pb(cuda, case).encode_batch(anns)
    assert (assigned == ra).all()
    assert y.tobytes() == ry.tobytes()
    assert (npos == rn).all()


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


def _abi_call(cuda, case, with_assigned=True, dirty=0xA5):
    """od_assign_atss on guarded y / assigned_gt / npos / workspace (the workspace arrives dirty) -> numpy (y, assigned, npos)"""
    from object_detector_amd import _lib
    from object_detector_amd.net import Context, _stream_ptr
    size, (B, nc, gmax), k, flagged = case
    anns = ac.reference(case)[0]
    ctx = Context.get(cuda)
    pri = PR.make_priors(size)
    P = len(pri)
    levels = PR.level_shapes(size)
    grid_hw = (C.c_int32 * (2 * len(levels)))(*[v for hw in levels for v in hw])
    gb, gc, gf, gn = _pack(anns, gmax, np.random.default_rng(8), over=0)
    dev = [torch.from_numpy(v).to(cuda) for v in (pri, gb, gc, gf, gn)]
    gy = L.Guarded((B, P, nc + 6), torch.float32, cuda)
    ga = L.Guarded((B, P), torch.int32, cuda)
    gnp = L.Guarded((B,), torch.int32, cuda)
    wsb = ctx.lib.od_assign_atss_workspace_bytes(B, P, gmax)
    assert wsb == B * P * 8
    gws = L.Guarded((wsb,), torch.uint8, cuda)
    gy.t.fill_(float("nan")), ga.t.fill_(-77), gnp.t.fill_(-77), gws.t.fill_(dirty)
    rc = ctx.lib.od_assign_atss(ctx.handle, dev[0].data_ptr(), grid_hw, len(levels), PR.NUM_PRIORS, dev[1].data_ptr(),
                                dev[2].data_ptr(), dev[4].data_ptr(), dev[3].data_ptr() if flagged else None, 0.5, k, B, P,
                                gmax, nc, 0.1, gy.t.data_ptr(), ga.t.data_ptr() if with_assigned else None,
                                gnp.t.data_ptr(), gws.t.data_ptr(), wsb, _stream_ptr())
    _lib.check(rc, "od_assign_atss")
    torch.cuda.synchronize()
    gws.check("workspace")
    y, npos, assigned = gy.numpy("y"), gnp.numpy("npos"), ga.numpy("assigned_gt")
    if not with_assigned:
        assert (assigned == -77).all(), "assigned_gt = NULL, yet something wrote the buffer"
    return y, assigned, npos


ABI_CASES = [((64, 64), (4, 20, 7), 9, True), ((96, 160), (3, 80, 128), 32, True), ((96, 160), (4, 1, 1), 1, False),
             ((64, 64), (3, 80, 128), 1, False)]


@pytest.mark.parametrize("case", ABI_CASES, ids=str)
def test_guarded_buffers_and_garbage_padding(cuda, case):
    assert case in ac.CASES
    _anns, ry, ra, rn, _shown = ac.reference(case)
    y, assigned, npos = _abi_call(cuda, case)
    assert (assigned == ra).all() and y.tobytes() == ry.tobytes() and (npos == rn).all()
    y2, _a2, n2 = _abi_call(cuda, case, with_assigned=False, dirty=0x00)
    assert y2.tobytes() == ry.tobytes() and (n2 == rn).all()


def test_same_call_twice_gives_the_same_bytes(cuda):
    case = ((96, 160), (3, 80, 128), 9, True)  # conflicts on hundreds of priors: the claims race, the keys decide
    assert "conflict" in ac.reference(case)[4]
    a, b = _abi_call(cuda, case), _abi_call(cuda, case)
    for u, v in zip(a, b):
        assert u.tobytes() == v.tobytes()


def test_bad_dimensions_return_the_error_code(cuda):
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
    y = torch.full((B, P, nc + 6), -7.0, device=cuda)
    npos = torch.full((B,), -7, dtype=torch.int32, device=cuda)
    ws = torch.empty((B * P * 8,), dtype=torch.uint8, device=cuda)

    def call(levels=levels, A=PR.NUM_PRIORS, topk=9, gmax=gmax, flags=None, ign_thr=0.5, wsb=None):
        grid_hw = (C.c_int32 * max(2, 2 * len(levels)))(*[v for hw in levels for v in hw])
        return ctx.lib.od_assign_atss(ctx.handle, pri.data_ptr(), grid_hw, len(levels), A, gb.data_ptr(), gc.data_ptr(),
                                      gn.data_ptr(), flags, ign_thr, topk, B, P, gmax, nc, 0.1, y.data_ptr(), None,
                                      npos.data_ptr(), ws.data_ptr(), ws.numel() if wsb is None else wsb, _stream_ptr())

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
    }
    for what, kw in bad.items():
        rc = call(**kw)
        assert rc != 0, what
        with pytest.raises(_lib.OdError, match="od_assign_atss"):
            _lib.check(rc, "od_assign_atss")
    assert call(wsb=B * P * 8 - 1) != 0  # a short workspace is refused as well
    torch.cuda.synchronize()
    assert (y == -7.0).all() and (npos == -7).all(), "a refused call wrote its outputs"
    assert call(flags=None, ign_thr=0.0) == 0  # without flags ign_thr is not read
    torch.cuda.synchronize()
    assert (y[:, :, 0] == 1).all() and (npos == 0).all()  # gt_counts are 0: every prior is background


# ---- Python layers ---------------------------------------------------------------------------------------------------------

def test_encode_truth_callbacks_route_through_atss(cuda):
    case = ((64, 64), (4, 20, 7), 9, True)
    anns, ry, _ra, _rn, _shown = ac.reference(case)
    pb = _pb(cuda, case)
    assert pb.encode_truth(anns).tobytes() == ry.tobytes()
    assert pb.encode_truth(anns[0]).tobytes() == ry[0].tobytes()
    assert pb.encode_truth_device(anns).cpu().numpy().tobytes() == ry.tobytes()


def test_trainer_follows_its_assigner(cuda):
    """Trainer(assigner="atss").step(x, annotations=...) encodes through od_assign_atss: the target equals the reference's and
    Trainer.loss on it equals the oracle loss on the reference's target."""
    from object_detector_amd.trainer import Trainer
    from test_gpu_trainer import _setup
    Bs, Ss = 2, 96
    params, x, anns = _setup(cuda, Bs, Ss)
    tr = Trainer(params, Bs, (Ss, Ss), device=cuda, lr=0.0, momentum=0.0, loss_scale=256.0, assigner="atss", atss_topk=9)
    assert tr.pb.assigner == "atss" and tr.pb.atss_topk == 9
    ref = [atss_ref.encode_truth(a.bboxes, a.classes, tr.pb.pb_locs, PR.level_shapes((Ss, Ss)), tr.num_classes, topk=9,
                                 loc_scale=tr.pb.loc_scale) for a in anns]
    ry, ra = np.stack([r[0] for r in ref]), np.stack([r[1] for r in ref])
    assert (ra >= 0).any()
    y, _npos, assigned = tr.pb.encode_batch(anns, return_device=True)
    assert y.cpu().numpy().tobytes() == ry.tobytes() and (assigned.cpu().numpy() == ra).all()
    tr.step(torch.from_numpy(x).to(cuda), annotations=anns)
    torch.cuda.synchronize()
    losses = tr.losses.cpu().numpy().copy()
    rl, _rg = oloss.loss_and_grad(tr.pred.float().cpu().numpy(), ry, tr.num_classes)
    np.testing.assert_allclose(losses, rl, rtol=2e-5)


def test_default_assigner_is_unchanged(cuda):
    from object_detector_amd.pb import PriorBoxes
    anns = ac.reference(((96, 160), (4, 20, 7), 9, True))[0]
    for ign in (False, True):
        y0, n0, a0 = PriorBoxes((96, 160), 20, device=cuda, ignore_regions=ign).encode_batch(anns)
        y1, n1, a1 = PriorBoxes((96, 160), 20, device=cuda, ignore_regions=ign, assigner="max-iou").encode_batch(anns)
        assert y0.tobytes() == y1.tobytes() and (a0 == a1).all() and (n0 == n1).all()
        assert n0.sum() > 0
    ya = PriorBoxes((96, 160), 20, device=cuda, assigner="atss").encode_batch(anns)[0]
    assert ya.tobytes() != y0.tobytes()  # the keyword does select another rule
