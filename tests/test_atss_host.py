"""Host logic of the ATSS assigner: the numpy reference of od_assign_atss (tests/atss_ref.py) against a brute-force
restatement of the paper, its invariants, the constructor's argument checks and the non-vacuity of the fixed cases the GPU
tests compare bit for bit.  No GPU."""
import pathlib
import sys

import numpy as np
import pytest

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))

import atss_cases as ac  # noqa: E402
import atss_ref  # noqa: E402
from object_detector_amd import priors as PR  # noqa: E402
from oracle import assign as oassign  # noqa: E402
from oracle import postprocess as opp  # noqa: E402

MARGIN = 2.0 ** -18  # no candidate of the restatement's cases lies this close to its threshold


# ---- the reference against a second statement of the rule -----------------------------------------------------------

def brute_force(gt_boxes, priors, grid_hw, A, topk, flags):
    """ATSS as the paper states it: per level a FULL sort of the cells by distance to the box centre (ties: lower cell
    index), the first k cells' priors are candidates; threshold = mean + std of the candidates' IoUs, in f64 on the 2^-20
    lattice values; positive = IoU >= threshold and centre inside the box; no positive: the best candidate is forced;
    ownership box by box with explicit comparisons.  -> (assigned [P], smallest |IoU - threshold| over all candidates)"""
    f = np.float32
    P = len(priors)
    owner = {}  # prior -> (forced, v, g)
    margin = np.inf
    for g, box in enumerate(np.asarray(gt_boxes, f)):
        if flags is not None and flags[g] & 1:
            continue
        gx, gy = (box[0] + box[2]) * f(0.5), (box[1] + box[3]) * f(0.5)
        cand, base = [], 0
        for gh, gw in grid_hw:
            dist = []
            for yy in range(gh):
                for xx in range(gw):
                    cx, cy = (f(xx) + f(0.5)) / f(gw), (f(yy) + f(0.5)) / f(gh)
                    dx, dy = cx - gx, cy - gy
                    dist.append((float(f(f(dx * dx) + f(dy * dy))), yy * gw + xx, float(cx), float(cy)))
            dist.sort()
            for _d, cell, cx, cy in dist[:topk]:
                inside = box[0] < cx < box[2] and box[1] < cy < box[3]
                cand += [(base + cell * A + a, inside) for a in range(A)]
            base += gh * gw * A
        idx = np.array([p for p, _ in cand])
        v = oassign.iou_matrix(box[None], priors[idx])[0]
        lat = np.rint(v.astype(np.float64) * 2.0 ** 20) / 2.0 ** 20
        thr = lat.mean() + lat.std()
        margin = min(margin, float(np.abs(lat - thr).min()))
        claims = [(p, False, v[i]) for i, (p, inside) in enumerate(cand) if lat[i] >= thr and inside]
        if not claims and (v > 0).any():
            i = min((j for j in range(len(v)) if v[j] == v.max()), key=lambda j: idx[j])  # ties: the lowest prior index
            claims = [(int(idx[i]), True, v[i])]
        for p, forced, vv in claims:
            old = owner.get(p)
            if old is None or (forced, vv) > (old[0], old[1]):  # equal kind and IoU: the earlier (lower) box keeps it
                owner[p] = (forced, vv, g)
    assigned = np.full(P, -1, np.int32)
    for p, (_f, _v, g) in owner.items():
        assigned[p] = g
    return assigned, margin


def _random_boxes(rng, n):
    c = rng.uniform(0, 1, (n, 2))
    wh = np.exp(rng.uniform(np.log(0.05), np.log(0.9), (n, 2)))
    return np.clip(np.concatenate([c - wh / 2, c + wh / 2], 1), 0, 1).astype(np.float32)


# seeds fixed on the CPU so that the margin assertion below holds for every (size, topk)
RESTATEMENT_SEEDS = {(64, 64): 3, (96, 160): 4}


@pytest.mark.parametrize("size", [(64, 64), (96, 160)])
@pytest.mark.parametrize("topk", [1, 9, 32])
def test_reference_equals_the_brute_force_restatement(size, topk):
    rng = np.random.default_rng(RESTATEMENT_SEEDS[size])
    priors, grid_hw = PR.make_priors(size), PR.level_shapes(size)
    boxes = _random_boxes(rng, 8)
    boxes[0] = ac.CORNER_BOX  # distance ties: the full sort and the keyed selection must break them alike
    flags = np.array([0, 0, 1, 0, 0, 0, 1, 0], np.int32)
    for fl in (None, flags):
        want, margin = brute_force(boxes, priors, grid_hw, PR.NUM_PRIORS, topk, fl)
        assert margin > MARGIN, f"a candidate lies within 2^-18 of its threshold ({margin:.3g}): pick another seed"
        _y, got = atss_ref.encode_truth(boxes, np.zeros(8, np.int32), priors, grid_hw, 3, topk=topk, flags=fl)
        got = np.where(got == -3, -1, got)  # the region rule is assign_ign_ref's, not the paper's
        assert (got >= 0).sum() > 0 and (got == want).all()


def test_select_cells_breaks_ties_by_cell_index():
    cells, tie = atss_ref.select_cells(ac.CORNER_BOX, 8, 8, 1)  # centre (0.25, 0.25): cells (1,1) (1,2) (2,1) (2,2) tie
    assert tie and cells.tolist() == [1 * 8 + 1]
    cells, tie = atss_ref.select_cells(ac.CORNER_BOX, 8, 8, 3)
    assert tie and cells.tolist() == [9, 10, 17]
    cells, tie = atss_ref.select_cells(ac.CORNER_BOX, 2, 2, 9)  # fewer cells than k: all of them, nothing refused
    assert not tie and sorted(cells.tolist()) == [0, 1, 2, 3]


# ---- invariants ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", [c for c in ac.CASES if c[3] and c[1][2] > 1 and c[0] != (320, 320)], ids=str)
def test_reference_invariants(case):
    anns, y, assigned, npos, _shown = ac.reference(case)
    size, (B, nc, gmax), k, _ = case
    priors = PR.make_priors(size)
    for i, a in enumerate(anns):
        flagged = np.nonzero(a.difficults)[0]
        assert not np.isin(assigned[i], flagged).any(), "a flagged box owns a prior"
        assert not (assigned[i] == -2).any()
        assert npos[i] == (assigned[i] >= 0).sum() == (y[i][:, 1] == 1).sum()
        assert (y[i][assigned[i] == -3] == 0).all() and (y[i][assigned[i] == -1, 0] == 1).all()
        ps = np.nonzero(assigned[i] >= 0)[0]
        g = assigned[i][ps]
        assert (y[i][ps, 2 + a.classes[g]] == 1).all() and (y[i][ps, 2:2 + nc].sum(1) == 1).all()
        # ((g - p) / w) / s and back: four roundings of 2^-24 relative on |g - p| < 2, plus the result's: below 2e-6
        np.testing.assert_allclose(opp.decode_locs(y[i][ps, -4:], priors[ps]), a.bboxes[g], rtol=0, atol=2e-6)


def test_reference_without_boxes_is_all_background():
    priors = PR.make_priors((64, 64))
    y, a = atss_ref.encode_truth(np.zeros((0, 4), np.float32), [], priors, PR.level_shapes((64, 64)), 5)
    assert (a == -1).all() and (y[:, 0] == 1).all() and (y[:, 1:] == 0).all()


# ---- the constructor's checks: before anything touches the GPU ----------------------------------------------------------------

@pytest.mark.parametrize("kw", [{"assigner": "iou"}, {"assigner": None}, {"assigner": "atss", "atss_topk": 0},
                                {"assigner": "atss", "atss_topk": 33}, {"atss_topk": 33}, {"assigner": "atss", "atss_topk": 2.5}])
def test_bad_assigner_arguments_raise_value_error(kw):
    from object_detector_amd import _lib
    from object_detector_amd.pb import PriorBoxes
    loaded = _lib._lib
    with pytest.raises(ValueError):
        PriorBoxes((64, 64), 3, **kw)
    assert _lib._lib is loaded, "the check loaded the library"


def test_trainer_checks_the_assigner_before_the_device():
    from object_detector_amd.trainer import Trainer
    for kw in ({"assigner": "iou"}, {"assigner": "atss", "atss_topk": 0}, {"assigner": "atss", "atss_topk": 33}):
        with pytest.raises(ValueError, match="assigner|atss_topk"):
            Trainer({}, 2, (64, 64), device="cuda:0", **kw)  # no parameters, no GPU: the check comes first


def test_assigner_arguments_are_kept():
    from object_detector_amd.pb import PriorBoxes
    pb = PriorBoxes((64, 64), 3)
    assert pb.assigner == "max-iou" and pb.atss_topk == 9
    pb = PriorBoxes((64, 64), 3, assigner="atss", atss_topk=32)
    assert pb.assigner == "atss" and pb.atss_topk == 32 and pb._ctx is None


# ---- non-vacuity of the fixed cases -------------------------------------------------------------------------------------------

def test_fixed_cases_show_what_they_are_there_for():
    seen = set()
    for case in ac.CASES:
        shown, want = ac.reference(case)[4], ac.expected(case)
        assert want <= shown, f"{case}: the reference's output does not show {sorted(want - shown)}"
        seen |= want
        assert any(a.num_objects == 0 for a in ac.reference(case)[0]), "no image without a box"
    assert seen == set(ac.PROPERTIES)
    for prop in ac.PROPERTIES:  # each property on its own, where the issue names a case for it
        assert any(prop in ac.expected(c) for c in ac.CASES if c[0] == (64, 64)), prop
