"""Host logic of the task-aligned assigner: the numpy reference of od_assign_tal (tests/tal_ref.py) against a brute-force,
per-box restatement of the rule, the cap on the priors the reference leaves undecided, the non-vacuity of the fixed cases,
and the constructors' argument checks.  No GPU."""
import math
import pathlib
import sys

import numpy as np
import pytest

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))

import tal_cases as tc  # noqa: E402
import tal_ref  # noqa: E402
from object_detector_amd import priors as PR  # noqa: E402
from oracle import postprocess as opp  # noqa: E402


# ---- the reference against a second statement of the rule -----------------------------------------------------------

def _iou(a, c):
    """iou_f32 of csrc/assign_common.h on numpy f32 scalars"""
    f = np.float32
    iw = max(min(a[2], c[2]) - max(a[0], c[0]), f(0))
    ih = max(min(a[3], c[3]) - max(a[1], c[1]), f(0))
    inter = f(iw * ih)
    uni = f(f(f((a[2] - a[0]) * (a[3] - a[1])) + f((c[2] - c[0]) * (c[3] - c[1]))) - inter)
    return f(inter / uni) if uni > 0 else f(0)


def brute_force(gt_boxes, gt_classes, flags, pred, priors, grid_hw, nc, topk, alpha, beta, loc_scale=0.1, A=8):
    """The rule with explicit loops: box by box, level by level, cell by cell, prior by prior; Python's math in f64 for the
    metric; a full sort per box; ownership by explicit comparisons.  -> (assigned [P] with -1 for every unowned prior,
    metric [P])"""
    f = np.float32
    P = len(priors)
    owner = {}  # prior -> (forced, v, g, l)
    for g, box in enumerate(np.asarray(gt_boxes, f)):
        if flags is not None and flags[g] & 1:
            continue
        cand, base = [], 0
        for gh, gw in grid_hw:
            for yy in range(gh):
                for xx in range(gw):
                    cx, cy = (f(xx) + f(0.5)) / f(gw), (f(yy) + f(0.5)) / f(gh)
                    if not (box[0] < cx < box[2] and box[1] < cy < box[3]):
                        continue
                    for a in range(A):
                        p = base + (yy * gw + xx) * A + a
                        row, pr = pred[p], priors[p]
                        if not np.isfinite(row[:2]).all() or np.isnan(row[2:2 + nc]).any() or np.isposinf(row[2:2 + nc]).any() \
                                or np.isneginf(row[2:2 + nc]).all():
                            continue  # la or lse would not be finite
                        pw, ph = pr[2] - pr[0], pr[3] - pr[1]
                        d = [pr[0] + f(row[2 + nc] * f(loc_scale)) * pw, pr[1] + f(row[3 + nc] * f(loc_scale)) * ph,
                             pr[2] + f(row[4 + nc] * f(loc_scale)) * pw, pr[3] + f(row[5 + nc] * f(loc_scale)) * ph]
                        if not np.isfinite(d).all():
                            continue
                        pb = [min(d[0], d[2]), min(d[1], d[3]), max(d[0], d[2]), max(d[1], d[3])]
                        u = _iou(box, pb)
                        if not u > 0:
                            continue
                        z0, z1 = float(row[0]), float(row[1])
                        la = z1 - (max(z0, z1) + math.log(math.exp(z0 - max(z0, z1)) + math.exp(z1 - max(z0, z1))))
                        zc = [float(v) for v in row[2:2 + nc]]
                        mc = max(zc)
                        lse = mc + math.log(sum(math.exp(v - mc) for v in zc))
                        c = int(gt_classes[g])
                        l = alpha * (la + zc[c] - lse if 0 <= c < nc else la) + beta * math.log(float(u))
                        cand.append((-l, p, u))
            base += gh * gw * A
        cand.sort()
        claims = [(p, False, u, -nl) for nl, p, u in cand[:topk]]
        if not cand:
            best = None
            for p in range(P):
                v = _iou(box, priors[p])
                if v > 0 and (best is None or v > best[1]):
                    best = (p, v)
            claims = [(best[0], True, best[1], 0.0)] if best else []
        for p, forced, v, l in claims:
            old = owner.get(p)
            if old is None or (forced, v) > (old[0], old[1]):  # equal kind and IoU: the earlier (lower) box keeps it
                owner[p] = (forced, v, g, l)
    assigned, metric = np.full(P, -1, np.int32), np.zeros(P)
    for p, (forced, _v, g, l) in owner.items():
        assigned[p], metric[p] = g, 0.0 if forced else l
    return assigned, metric


@pytest.mark.parametrize("case", [((64, 64), (4, 20, 7), 1, True), ((64, 64), (4, 20, 7), 13, True),
                                  ((64, 64), (4, 20, 7), 32, False), ((64, 64), (4, 1, 1), 13, False)], ids=str)
def test_reference_equals_the_brute_force_restatement(case):
    assert case in tc.CASES
    size, (B, nc, gmax), k, flagged = case
    anns, pred, refs, _shown = tc.reference(case)
    priors, grid_hw = PR.make_priors(size), PR.level_shapes(size)
    for i, (a, r) in enumerate(zip(anns, refs)):
        assert not r["undecided"].any(), "pick a case whose cut is clear in f64: the two statements sum in different orders"
        want, metric = brute_force(a.bboxes, a.classes, a.difficults.astype(np.int32) if flagged else None, pred[i], priors,
                                   grid_hw, nc, k, tc.ALPHA, tc.BETA)
        got = np.where(r["assigned"] == -3, -1, r["assigned"])  # the region rule is assign_ign_ref's
        assert (got == want).all()
        np.testing.assert_allclose(r["metric"], metric, rtol=0, atol=1e-9)
    assert sum((r["assigned"] >= 0).sum() for r in refs) > 0


def test_exact_ties_are_decided_by_the_prior_index():
    """8 identical priors per cell with identical pred rows: l is bit-equal inside a cell on any exp / log, so the cut at
    topk = 13 = 8 + 5 takes the five lowest priors of the second cell, and nothing is undecided."""
    size, nc = (64, 64), 5
    priors, pred = tc.identical_cells(size, nc, seed=5)
    box = np.array([tc.BIG_BOX], np.float32)
    r = tal_ref.encode_truth(box, [2], pred, priors, PR.level_shapes(size), nc, topk=13)
    own = np.nonzero(r["assigned"] == 0)[0]
    assert len(own) == 13 and not r["undecided"].any()
    cells = sorted({int(p) // 8 for p in own})
    assert len(cells) == 2
    per = {c: sorted(int(p) % 8 for p in own if p // 8 == c) for c in cells}
    assert sorted(per.values(), key=len) == [[0, 1, 2, 3, 4], list(range(8))]


# ---- the cap on undecided priors, and what the cases show ------------------------------------------------------------

def test_fixed_cases_show_what_they_are_there_for_and_stay_under_the_undecided_cap():
    seen = set()
    for case in tc.CASES:
        anns, _pred, refs, shown = tc.reference(case)
        want = tc.expected(case)
        assert want <= shown, f"{case}: the reference's output does not show {sorted(want - shown)}"
        seen |= want
        assert anns[1].num_objects == 0, "image 1 has no box"
        share = tc.undecided_share(refs)
        assert share <= tc.UNDECIDED_CAP, f"{case}: {share:.2%} of the claimed priors are undecided: pick another seed"
    assert seen == set(tc.PROPERTIES)
    for case in tc.CASES:  # every case with more than one box per image and topk > 1 shows every property it can
        if case[1][2] > 1 and case[2] > 1:
            assert tc.expected(case) >= set(tc.PROPERTIES) - {"region_row"}


@pytest.mark.parametrize("case", [c for c in tc.CASES if c[3] and c[1][2] > 1 and c[0] != (320, 320)], ids=str)
def test_reference_invariants(case):
    anns, _pred, refs, _shown = tc.reference(case)
    size, (B, nc, gmax), k, _ = case
    priors = PR.make_priors(size)
    for a, r in zip(anns, refs):
        assigned, y = r["assigned"], r["y"]
        assert not np.isin(assigned, np.nonzero(a.difficults)[0]).any(), "a flagged box owns a prior"
        assert not (assigned == -2).any()
        assert (y[assigned == -3] == 0).all() and (y[assigned == -1, 0] == 1).all()
        for g in np.nonzero(~a.difficults)[0]:
            normal = [p for p, gg, _v, forced, _l, kind in r["claims"] if gg == g and not forced and kind != "maybe_out"]
            assert len(normal) == min(k, len(r["cands"][g])) and set(normal) <= set(r["cands"][g].tolist())
        assert (r["metric"][r["normal"]] <= 0).all() and (r["metric"][~r["normal"]] == 0).all()
        assert r["claimed_sure"].sum() <= (assigned >= 0).sum() <= r["claimed_any"].sum()
        ps = np.nonzero(assigned >= 0)[0]
        g = assigned[ps]
        assert (y[ps, 2 + a.classes[g]] == 1).all() and (y[ps, 2:2 + nc].sum(1) == 1).all()
        np.testing.assert_allclose(opp.decode_locs(y[ps, -4:], priors[ps]), a.bboxes[g], rtol=0, atol=2e-6)


def test_reference_without_boxes_is_all_background():
    priors = PR.make_priors((64, 64))
    pred = np.zeros((len(priors), 11), np.float32)
    r = tal_ref.encode_truth(np.zeros((0, 4), np.float32), [], pred, priors, PR.level_shapes((64, 64)), 5)
    assert (r["assigned"] == -1).all() and (r["y"][:, 0] == 1).all() and (r["y"][:, 1:] == 0).all()


def test_a_class_outside_the_range_drops_the_class_term():
    size, nc = (64, 64), 4
    priors = PR.make_priors(size)
    rng = np.random.default_rng(11)
    pred = np.concatenate([rng.normal(0, 2, (len(priors), 2 + nc)), rng.normal(0, 0.5, (len(priors), 4))], 1).astype(np.float32)
    box = np.array([tc.BIG_BOX], np.float32)
    r = tal_ref.encode_truth(box, [nc], pred, priors, PR.level_shapes(size), nc, topk=5, alpha=2.0, beta=3.0)
    la, _lse, pbox, _raw, _valid = r["pp"]
    own = np.nonzero(r["assigned"] == 0)[0]
    assert len(own) == 5 and (r["y"][own, 2:2 + nc] == 0).all()
    from oracle import assign as oassign
    u = oassign.iou_matrix(box, pbox[own])[0].astype(np.float64)
    np.testing.assert_allclose(r["metric"][own], 2.0 * la[own] + 3.0 * np.log(u), rtol=0, atol=1e-12)


# ---- the constructors' checks: before anything touches the GPU -------------------------------------------------------

BAD = [{"tal_topk": 0}, {"tal_topk": 33}, {"tal_topk": 2.5}, {"tal_topk": True}, {"tal_alpha": 0.0}, {"tal_alpha": -1.0},
       {"tal_alpha": float("nan")}, {"tal_alpha": float("inf")}, {"tal_beta": 0}, {"tal_beta": -6.0},
       {"tal_beta": float("inf")}, {"tal_beta": float("nan")}, {"tal_beta": "6"}, {"tal_alpha": None}]


@pytest.mark.parametrize("kw", BAD, ids=str)
def test_bad_tal_arguments_raise_value_error(kw):
    from object_detector_amd import _lib
    from object_detector_amd.pb import PriorBoxes, check_tal
    loaded = _lib._lib
    with pytest.raises(ValueError, match="tal_"):
        PriorBoxes((64, 64), 3, assigner="tal", **kw)
    with pytest.raises(ValueError, match="tal_"):
        check_tal(**{"tal_topk": 13, "tal_alpha": 1.0, "tal_beta": 6.0, **kw})
    assert _lib._lib is loaded, "the check loaded the library"


def test_check_assigner_knows_tal():
    from object_detector_amd.pb import ASSIGNERS, check_assigner
    assert "tal" in ASSIGNERS and check_assigner("tal", 9) == ("tal", 9)
    with pytest.raises(ValueError):
        check_assigner("task-aligned", 9)


def test_trainer_checks_the_tal_arguments_before_the_device():
    from object_detector_amd.trainer import Trainer
    for kw in ({"tal_topk": 0}, {"tal_topk": 33}, {"tal_alpha": 0.0}, {"tal_beta": float("nan")}):
        with pytest.raises(ValueError, match="tal_"):
            Trainer({}, 2, (64, 64), device="cuda:0", assigner="tal", **kw)  # no parameters, no GPU: the check comes first


def test_tal_arguments_are_kept_and_the_truth_callbacks_refuse():
    from object_detector_amd import _lib
    from object_detector_amd.pb import ObjectsAnnotation, PriorBoxes
    loaded = _lib._lib
    pb = PriorBoxes((64, 64), 3)
    assert pb.assigner == "max-iou" and (pb.tal_topk, pb.tal_alpha, pb.tal_beta) == (13, 1.0, 6.0)
    pb = PriorBoxes((64, 64), 3, assigner="tal", tal_topk=32, tal_alpha=0.5, tal_beta=4)
    assert pb.assigner == "tal" and (pb.tal_topk, pb.tal_alpha, pb.tal_beta) == (32, 0.5, 4.0) and pb._ctx is None
    ann = ObjectsAnnotation(None, 64, 64, [1], [tc.BIG_BOX])
    for call in (pb.encode_truth, pb.encode_truth_device):
        for arg in (ann, [ann]):
            with pytest.raises(ValueError, match="Trainer.step"):
                call(arg)
    with pytest.raises(ValueError, match="pred"):  # no predictions, and a host array is none either
        pb.encode_batch([ann])
    with pytest.raises(ValueError, match="pred"):
        pb.encode_batch([ann], pred=np.zeros((1, len(pb), 9), np.float32))
    assert pb._ctx is None and _lib._lib is loaded, "a refused call touched the device"
