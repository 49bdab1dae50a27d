"""GPU parity of od_assign_anchors_ign (K9 with ignore regions) against tests/assign_ign_ref.py, bit for bit, and the
existing all-zero-row contract of the loss through the new producer."""
import pathlib
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent))

import assign_ign_ref as aref  # noqa: E402
from oracle import loss as oloss  # noqa: E402

pytestmark = pytest.mark.gpu


def _boxes(rng, n):
    c = rng.uniform(0, 1, (n, 2))
    wh = np.exp(rng.uniform(np.log(0.05), np.log(0.9), (n, 2)))
    return np.clip(np.concatenate([c - wh / 2, c + wh / 2], 1), 0, 1).astype(np.float32)


def make_case(seed, B, nc, gmax, flagged=True):
    """B annotations with up to gmax boxes; image 1 has no object at all and image 2 (and every image when flagged=False) no
    flagged box; the others flag about a third of their boxes, at least one where they have more than one."""
    from object_detector_amd.pb import ObjectsAnnotation
    rng = np.random.default_rng(seed)
    anns = []
    for i in range(B):
        n = 0 if i == 1 else (gmax if i == 0 else int(rng.integers(1, gmax + 1)))
        b = _boxes(rng, n)
        c = rng.integers(0, nc, n).astype(np.int32)
        f = rng.random(n) < 0.35
        if n > 1 and not f.any():
            f[int(rng.integers(0, n))] = True
        if n > 1 and f.all():
            f[int(rng.integers(0, n))] = False
        if not flagged or i == 2:
            f[:] = False
        anns.append(ObjectsAnnotation(None, 320, 320, c, b, f))
    return anns


def _reference(pb, anns, nc):
    ys, asg = [], []
    for a in anns:
        y, g = aref.encode_truth(a.bboxes, a.classes, pb.pb_locs, nc, flags=a.difficults.astype(np.int32), ign_thr=pb.ign_thr,
                                 pos_thr=pb.pos_thr, neg_thr=pb.neg_thr, loc_scale=pb.loc_scale)
        ys.append(y), asg.append(g)
    return np.stack(ys), np.stack(asg)


def check_case_is_not_vacuous(pb, anns, ref_assigned):
    """On the REFERENCE's output: a row ignored by a region, a positive prior whose centre lies inside a flagged box, and an
    image without any flagged box."""
    assert (ref_assigned == -3).any(), "no prior is ignored by a region"
    assert any(a.num_objects and not a.difficults.any() for a in anns), "no image without a flagged box"
    pr = pb.pb_locs
    cx, cy = (pr[:, 0] + pr[:, 2]) / 2, (pr[:, 1] + pr[:, 3]) / 2
    found = False
    for a, g in zip(anns, ref_assigned):
        for r in a.bboxes[a.difficults]:
            found |= bool(((g >= 0) & (cx >= r[0]) & (cx < r[2]) & (cy >= r[1]) & (cy < r[3])).any())
    assert found, "no positive prior inside a region"


SHAPES = [(6, 20, 10), (4, 1, 1), (4, 1, 7), (4, 20, 128), (4, 80, 7), (4, 80, 128), (3, 20, 1)]  # (B, NC, Gmax)
# seeds chosen on the CPU (no GPU needed) so that check_case_is_not_vacuous holds for each (size, shape) below
SEEDS = {(size, B, nc, gmax): 100 for size in (320, 512) for (B, nc, gmax) in SHAPES}


@pytest.mark.parametrize("size", [(320, 320), (512, 512)])
@pytest.mark.parametrize("B,nc,gmax", SHAPES)
def test_no_flags_equals_od_assign_anchors(cuda, size, B, nc, gmax):
    from object_detector_amd.pb import PriorBoxes
    anns = make_case(11 + gmax, B, nc, gmax, flagged=False)
    plain = PriorBoxes(size, nc, device=cuda)
    ign = PriorBoxes(size, nc, device=cuda, ignore_regions=True)
    y0, n0, a0 = plain.encode_batch(anns, return_device=True)
    y1, n1, a1 = ign.encode_batch(anns, return_device=True)
    assert torch.equal(y0.view(torch.int32), y1.view(torch.int32)) and torch.equal(a0, a1) and torch.equal(n0, n1)
    assert int(n0.sum()) > 0


def test_no_flags_equals_the_existing_assign_test_cases(cuda):
    """the shapes of tests/test_gpu_train_ops.py::test_encode_truth_bit_exact and its tie case"""
    from object_detector_amd.pb import ObjectsAnnotation, PriorBoxes
    from test_gpu_train_ops import _annotations
    tie = ObjectsAnnotation(None, 320, 320, [1, 2, 3], np.array([[0.2, 0.2, 0.6, 0.7], [0.2, 0.2, 0.6, 0.7],
                                                                [0.0, 0.0, 0.01, 0.01]], np.float32))
    for size in ((320, 320), (512, 512)):
        for anns in (_annotations(1, 6), [tie]):
            y0, n0, a0 = PriorBoxes(size, 20, device=cuda).encode_batch(anns)
            y1, n1, a1 = PriorBoxes(size, 20, device=cuda, ignore_regions=True).encode_batch(anns)
            assert y0.tobytes() == y1.tobytes() and (a0 == a1).all() and (n0 == n1).all()


@pytest.mark.parametrize("size", [(320, 320), (512, 512)])
@pytest.mark.parametrize("B,nc,gmax", [s for s in SHAPES if s[2] > 1])
def test_flags_equal_the_reference(cuda, size, B, nc, gmax):
    from object_detector_amd.pb import PriorBoxes
    pb = PriorBoxes(size, nc, device=cuda, ignore_regions=True)
    anns = make_case(SEEDS[(size[0], B, nc, gmax)], B, nc, gmax)
    ry, ra = _reference(pb, anns, nc)
    check_case_is_not_vacuous(pb, anns, ra)
    y, npos, assigned = pb.encode_batch(anns)
    for i, a in enumerate(anns):
        flagged = np.nonzero(a.difficults)[0]
        assert not np.isin(assigned[i], flagged).any(), "a flagged box owns a prior"
        assert npos[i] == (y[i][:, 1] == 1).sum()
        assert (y[i][assigned[i] == -3] == 0).all()
    assert (assigned == ra).all()
    assert y.tobytes() == ry.tobytes()
    assert (npos == (ra >= 0).sum(1)).all()


def test_single_flagged_box_and_threshold(cuda):
    """Gmax = 1 with the one box flagged: no positive at all, the priors inside it ignored; ign_thr moves the border."""
    from object_detector_amd.pb import ObjectsAnnotation, PriorBoxes
    a = ObjectsAnnotation(None, 320, 320, [0], np.array([[0.2, 0.3, 0.8, 0.9]], np.float32), [True])
    counts = []
    for thr in (0.5, 0.9):
        pb = PriorBoxes((320, 320), 1, device=cuda, ignore_regions=True, ign_thr=thr)
        y, npos, assigned = pb.encode_batch([a])
        ry, ra = _reference(pb, [a], 1)
        assert (assigned == ra).all() and y.tobytes() == ry.tobytes() and npos[0] == 0
        assert (assigned == -3).any() and not (assigned >= 0).any()
        counts.append(int((assigned == -3).sum()))
    assert counts[1] < counts[0]


@pytest.mark.parametrize("box_mode", ["smooth_l1", "mse"])
def test_loss_on_region_targets_matches_oracle_and_ignores_the_rows(cuda, box_mode):
    from object_detector_amd import ops
    from object_detector_amd.pb import PriorBoxes
    pb = PriorBoxes((320, 320), 20, device=cuda, ignore_regions=True)
    anns = make_case(SEEDS[(320, 6, 20, 10)], 6, 20, 10)
    y, npos, assigned = pb.encode_batch(anns, return_device=True)
    region = (assigned == -3).cpu().numpy()
    assert region.any()
    pred = np.random.default_rng(4).normal(0, 1.5, tuple(y.shape)).astype(np.float32)
    losses, grad = ops.loss_fwd_bwd(torch.from_numpy(pred).to(cuda), y, 20, box_mode=box_mode)
    torch.cuda.synchronize()
    rl, rg = oloss.loss_and_grad(pred, y.cpu().numpy(), 20, box_mode=box_mode)
    np.testing.assert_allclose(losses.cpu().numpy(), rl, rtol=2e-5)
    grad = grad.cpu().numpy()
    np.testing.assert_allclose(grad, rg, rtol=1e-4, atol=1e-8)
    assert (grad[region][:, :2] == 0).all(), "a row ignored by a region has an objectness gradient"
    assert (grad[region] == 0).all()


def test_trainer_follows_its_prior_boxes(cuda):
    """Trainer(ignore_regions=True).step(x, annotations=...) encodes through od_assign_anchors_ign: Trainer.loss on that
    target equals the oracle loss on the reference's target."""
    from object_detector_amd.trainer import Trainer
    from test_gpu_trainer import _setup
    Bs, Ss = 2, 96
    params, x, anns = _setup(cuda, Bs, Ss)
    for a in anns:
        if a.num_objects > 1:
            a.difficults[-1] = True
    assert any(a.difficults.any() for a in anns)
    tr = Trainer(params, Bs, (Ss, Ss), device=cuda, lr=0.0, momentum=0.0, loss_scale=256.0, ignore_regions=True)
    assert tr.pb.ignore_regions
    y, _npos, assigned = tr.pb.encode_batch(anns, return_device=True)
    ry, ra = _reference(tr.pb, anns, tr.num_classes)
    assert y.cpu().numpy().tobytes() == ry.tobytes() and (assigned.cpu().numpy() == ra).all()
    tr.step(torch.from_numpy(x).to(cuda), annotations=anns)
    torch.cuda.synchronize()
    losses = tr.losses.cpu().numpy().copy()
    rl, _rg = oloss.loss_and_grad(tr.pred.float().cpu().numpy(), ry, tr.num_classes)
    np.testing.assert_allclose(losses, rl, rtol=2e-5)
