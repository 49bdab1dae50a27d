"""The fixed cases of the task-aligned assigner's tests (host and GPU): annotations, a seeded `pred`, their reference results
(computed once per process, never modified) and the properties each case must SHOW on the reference's output, so that the
comparison on it is not vacuous.  TEST INFRASTRUCTURE ONLY.

Gaussian logits and offsets never reach the corners of the rule, so image 0 of every case starts with crafted boxes and
crafted pred rows (make_case).  A case with Gmax = 1 has one box per image and cannot show what needs two boxes in an image
(a conflict, the identical pair, a forced claim over a normal one, a box with fewer candidates than topk beside the others);
topk = 1 cannot show a box with fewer candidates than topk that still has one.  expected() says so, from the parameters."""
from __future__ import annotations

import functools

import numpy as np

import tal_ref
from object_detector_amd import priors as PR
from oracle import assign as oassign

PROPERTIES = ("conflict", "identical_pair", "forced", "forced_beats_normal", "owns_nothing", "short", "crossed", "nan_row",
              "inf_row", "nonfinite_forced", "region_row")

SIZES = [(64, 64), (96, 160)]             # P = 672: the top level has 2 x 2 cells; P = 2520: gh != gw
SHAPES = [(4, 1, 1), (4, 20, 7), (3, 300, 128)]  # (B, NC, Gmax); image 1 of every batch has no box; NC = 300: the wide read
TOPKS = [1, 13, 32]
CASES = [(size, shape, k, flagged) for size in SIZES for shape in SHAPES for k in TOPKS for flagged in (False, True)]
CASES.append(((320, 320), (3, 80, 128), 13, True))  # the one real size
ALPHA, BETA = 1.0, 6.0
UNDECIDED_CAP = 0.02

BIG_BOX = [0.3, 0.3, 0.8, 0.8]
EMPTY_BOX = [0.5, 0.5, 0.5, 0.5]  # zero area: every IoU is 0, it owns nothing
REGION_BOX = [0.1, 0.1, 0.6, 0.6]  # the region of the flagged Gmax = 1 cases


def between_centres(size, fx, fy):
    """a box inside one cell of the finest level that holds no cell centre of any level (the coarser levels' centres are
    whole cells of the finest): it has no candidate, so it forces a prior"""
    gh, gw = PR.level_shapes(size)[0]
    kx, ky = round(fx * gw), round(fy * gh)
    return [(kx + 0.6) / gw, (ky + 0.6) / gh, (kx + 0.9) / gw, (ky + 0.9) / gh]


def one_centre(size, fx, fy):
    """a box around exactly one cell centre of the finest level: 8 candidates at most"""
    gh, gw = PR.level_shapes(size)[0]
    kx, ky = round(fx * gw), round(fy * gh)
    return [(kx + 0.3) / gw, (ky + 0.3) / gh, (kx + 0.7) / gw, (ky + 0.7) / gh]


def _boxes(rng, n):
    c = rng.uniform(0, 1, (n, 2))
    wh = np.exp(rng.uniform(np.log(0.05), np.log(0.9), (n, 2)))
    return np.clip(np.concatenate([c - wh / 2, c + wh / 2], 1), 0, 1).astype(np.float32)


def case_seed(case):
    (size, (B, nc, gmax), k, flagged) = case
    return 2000 + size[1] + 7 * gmax + 3 * k


def _forced_prior(box, priors):
    v = oassign.iou_matrix(np.asarray(box, np.float32)[None], priors)[0]
    return int(np.nonzero(v == v.max())[0][0])


def _favour(row, nc, cls, prior, box, loc_scale=0.1):
    """a pred row that is sure of `box` with class `cls`: high objectness, high class logit, offsets that decode to the box"""
    f = np.float32
    row[0], row[1] = -4.0, 4.0
    row[2 + cls] = 6.0
    pw, ph = prior[2] - prior[0], prior[3] - prior[1]
    row[2 + nc:] = ((np.asarray(box, f) - prior) / np.array([pw, ph, pw, ph], f)) / f(loc_scale)


def make_case(case):
    """-> (annotations, pred f32 [B,P,NC+6]).  Image 1 has no box.  With Gmax >= 7 image 0 has Gmax boxes and starts with
    BIG, BIG again (same class), two boxes between cell centres inside BIG, the zero-area box and a one-centre box; with
    Gmax = 1 image 0 has BIG, image 2 a box between centres and image 3 the zero-area box (unflagged cases) or a region
    (flagged ones).  With flags about a third of the random boxes are regions (crafted boxes: never).
    Crafted pred rows: the forced prior of the first between-centres box is sure of BIG (a normal claim the forced one
    beats), that of the second has a NaN objectness logit; in the cell at BIG's centre prior 0 decodes with crossed corners,
    prior 1 has a NaN offset and prior 2 an Inf class logit."""
    from object_detector_amd.pb import ObjectsAnnotation
    (size, (B, nc, gmax), k, flagged) = case
    rng = np.random.default_rng(case_seed(case))
    pri = PR.make_priors(size)
    P = len(pri)
    t1, t2 = between_centres(size, 0.4, 0.4), between_centres(size, 0.65, 0.65)
    crafted = [BIG_BOX, BIG_BOX, t1, t2, EMPTY_BOX, one_centre(size, 0.1, 0.1)]
    anns = []
    for i in range(B):
        n = 0 if i == 1 else (gmax if i == 0 else int(rng.integers(min(2, gmax), gmax + 1)))
        b = _boxes(rng, n)
        f = rng.random(n) < 0.35
        c = rng.integers(0, nc, n).astype(np.int32)
        if gmax == 1:
            if i == 0:
                b[0], f[0] = BIG_BOX, False
            if i == 2:
                b[0], f[0] = t2, False
            if i == 3:
                b[0], f[0] = (REGION_BOX, True) if flagged else (EMPTY_BOX, False)
        else:
            if i == 0:
                b[:len(crafted)], f[:len(crafted)] = crafted, False
                c[1] = c[0]
            if i == 2:
                f[int(rng.integers(0, n))] = True
            if n > 1 and f.all():
                f[int(rng.integers(0, n))] = False
        if not flagged:
            f[:] = False
        anns.append(ObjectsAnnotation(None, size[1], size[0], c, b, f))
    pred = np.concatenate([rng.normal(0, 2, (B, P, 2 + nc)), rng.normal(0, 0.5, (B, P, 4))], 2).astype(np.float32)
    gh, gw = PR.level_shapes(size)[0]
    cell = (int(0.55 * gh) * gw + int(0.55 * gw)) * PR.NUM_PRIORS  # the finest level's cell at BIG's centre
    c0 = int(anns[0].classes[0])
    _favour(pred[0, cell], nc, c0, pri[cell], [BIG_BOX[2], BIG_BOX[1], BIG_BOX[0], BIG_BOX[3]])  # x1 beyond x2: crossed
    pred[0, cell + 1, 2 + nc + 1] = np.nan
    pred[0, cell + 2, 2 + (nc - 1)] = np.inf
    p1, p2 = _forced_prior(t1, pri), _forced_prior(t2, pri)
    assert len({p1, p2, cell, cell + 1, cell + 2}) == 5
    if gmax > 1:
        _favour(pred[0, p1], nc, c0, pri[p1], BIG_BOX)
        pred[0, p1, :2], pred[0, p1, 2 + c0] = [-6.0, 6.0], 9.0  # BIG's first choice for every topk
        pred[0, p2, 1] = np.nan
    else:
        pred[2, p2, 1] = np.nan
    return anns, pred


def identical_cells(size, nc, seed):
    """-> (priors [P,4], pred [P,NC+6]) whose 8 priors of a cell are one and the same prior with one and the same pred row:
    whatever exp / log a device has, l is bit-equal inside a cell, so only the prior index can order it"""
    pri = PR.make_priors(size).reshape(-1, PR.NUM_PRIORS, 4)
    pri = np.ascontiguousarray(np.repeat(pri[:, 4:5], PR.NUM_PRIORS, 1).reshape(-1, 4))
    rng = np.random.default_rng(seed)
    cells = len(pri) // PR.NUM_PRIORS
    rows = np.concatenate([rng.normal(0, 2, (cells, 2 + nc)), rng.normal(0, 0.5, (cells, 4))], 1).astype(np.float32)
    return pri, np.ascontiguousarray(np.repeat(rows, PR.NUM_PRIORS, 0))


def shown(case, anns, refs, pred):
    """the PROPERTIES the reference's output for this case shows"""
    (size, (B, nc, gmax), k, flagged) = case
    out = set()
    cx, cy = tal_ref.prior_centres(PR.level_shapes(size), PR.NUM_PRIORS)
    for a, r, pr in zip(anns, refs, pred):
        la, lse, pbox, raw, valid = r["pp"]
        by_prior, normal_of = {}, {}
        for p, g, v, forced, l, kind in r["claims"]:
            if kind != "maybe_out":
                by_prior.setdefault(p, []).append((g, forced, v))
            if not forced:
                normal_of.setdefault(g, []).append(p)
        for p, cl in by_prior.items():
            if len({g for g, _, _ in cl}) > 1:
                out.add("conflict")
            fv = [v for _, forced, v in cl if forced]
            nv = [v for _, forced, v in cl if not forced]
            if fv and nv and max(nv) > max(fv) and any(forced and g == r["assigned"][p] for g, forced, _ in cl):
                out.add("forced_beats_normal")  # the larger IoU loses to the forced claim
            if fv:
                out.add("forced")
                if not valid[p]:
                    out.add("nonfinite_forced")  # a row that is no candidate is still taken through its static IoU
        for g in range(a.num_objects):
            for h in range(g + 1, a.num_objects):
                if (a.bboxes[g] == a.bboxes[h]).all() and a.classes[g] == a.classes[h] and not a.difficults[g] \
                        and not a.difficults[h] and normal_of.get(g) and sorted(normal_of[g]) == sorted(normal_of.get(h, [])) \
                        and all(r["assigned"][p] != h for p in normal_of[g]):
                    out.add("identical_pair")  # equal l and u on every prior: the lower box keeps them
            if not a.difficults[g]:
                if not (r["assigned"] == g).any():
                    out.add("owns_nothing")
                if 0 < len(r["cands"][g]) < k:
                    out.add("short")
                inside = (cx > a.bboxes[g][0]) & (cx < a.bboxes[g][2]) & (cy > a.bboxes[g][1]) & (cy < a.bboxes[g][3])
                normal = set(normal_of.get(g, []))
                if any(raw[p, 0] > raw[p, 2] or raw[p, 1] > raw[p, 3] for p in r["cands"][g]):
                    out.add("crossed")  # a candidate whose decoded corners had to be sorted
                bad = np.nonzero(inside & ~valid)[0]
                assert not (set(bad.tolist()) & normal), "a non-finite row was claimed as a candidate"
                if np.isnan(pr[bad]).any():
                    out.add("nan_row")
                if np.isinf(pr[bad]).any():
                    out.add("inf_row")
        if (r["assigned"] == -3).any():
            out.add("region_row")
    return out


@functools.lru_cache(maxsize=None)
def reference(case):
    """-> (anns, pred [B,P,C], list of tal_ref.encode_truth results per image, shown properties); read-only"""
    (size, (B, nc, gmax), k, flagged) = case
    anns, pred = make_case(case)
    pri = PR.make_priors(size)
    refs = [tal_ref.encode_truth(a.bboxes, a.classes, pred[i], pri, PR.level_shapes(size), nc, topk=k, alpha=ALPHA, beta=BETA,
                                 flags=a.difficults.astype(np.int32) if flagged else None) for i, a in enumerate(anns)]
    pred.setflags(write=False)
    for r in refs:
        for v in r.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
    return anns, pred, refs, shown(case, anns, refs, pred)


def undecided_share(refs):
    """undecided priors as a share of the priors with any claimant, over the images of a case"""
    return sum(int(r["undecided"].sum()) for r in refs) / max(1, sum(int(r["claimed_any"].sum()) for r in refs))


def expected(case):
    """The properties the case must show, from its parameters alone (see the module docstring for what Gmax = 1 and topk = 1
    cannot show)."""
    (size, (B, nc, gmax), k, flagged) = case
    want = {"forced", "crossed", "nan_row", "inf_row", "nonfinite_forced"}
    if gmax > 1:
        want |= {"conflict", "identical_pair", "forced_beats_normal", "owns_nothing"}
        if k > 1:
            want.add("short")
    elif not flagged:
        want.add("owns_nothing")
    if flagged:
        want.add("region_row")
    return want
