"""The fixed cases of the ATSS tests (host and GPU), their reference results (computed once per process, never modified) and
the properties each case must SHOW on the reference's output, so that a bit-exact comparison on it is not vacuous.
TEST INFRASTRUCTURE ONLY."""
from __future__ import annotations

import functools

import numpy as np

import atss_ref
from object_detector_amd import priors as PR

PROPERTIES = ("conflict", "forced_beats_passed", "tie", "short_level", "owns_nothing", "region_row")

SIZES = [(64, 64), (96, 160)]            # P = 672: the top level has 4 cells; P = 2520: gh != gw
SHAPES = [(4, 1, 1), (4, 20, 7), (3, 80, 128)]  # (B, NC, Gmax); image 1 of every batch has no box
TOPKS = [1, 9, 32]
CASES = [(size, shape, k, flagged) for size in SIZES for shape in SHAPES for k in TOPKS for flagged in (False, True)]
CASES.append(((320, 320), (3, 80, 128), 9, True))  # the one real size

CORNER_BOX = [0.125, 0.125, 0.375, 0.375]  # centred on a cell corner of every level at 64x64: exact distance ties
CORNER_BOX_2 = [0.25, 0.25, 0.5, 0.5]
BIG_BOX, TINY_BOX = [0.3, 0.3, 0.8, 0.8], [0.548, 0.548, 0.552, 0.552]  # about 0.004 of the image, at the other's centre
EMPTY_BOX = [0.5, 0.5, 0.5, 0.5]  # zero area: every IoU is 0


def _boxes(rng, n):
    c = rng.uniform(0, 1, (n, 2))
    wh = np.exp(rng.uniform(np.log(0.05), np.log(0.9), (n, 2)))
    return np.clip(np.concatenate([c - wh / 2, c + wh / 2], 1), 0, 1).astype(np.float32)


def case_seed(case):
    (size, (B, nc, gmax), k, flagged) = case
    return 1000 + size[1] + 7 * gmax


def make_case(case):
    """B annotations with up to Gmax boxes.  Image 0 has Gmax boxes and starts with the crafted ones, image 1 has none; with
    flags about a third of the random boxes are regions (image 2: at least one; crafted boxes: never)."""
    from object_detector_amd.pb import ObjectsAnnotation
    (size, (B, nc, gmax), k, flagged) = case
    rng = np.random.default_rng(case_seed(case))
    crafted = [CORNER_BOX, BIG_BOX, TINY_BOX, CORNER_BOX_2, EMPTY_BOX]
    anns = []
    for i in range(B):
        n = 0 if i == 1 else (gmax if i == 0 else int(rng.integers(min(2, gmax), gmax + 1)))
        b = _boxes(rng, n)
        f = rng.random(n) < 0.35
        if i == 0:
            m = min(n, len(crafted))
            b[:m], f[:m] = crafted[:m], False
        if i == 2:
            f[int(rng.integers(0, n))] = True
        if n > 1 and f.all():
            f[int(rng.integers(0, n))] = False
        if gmax == 1 and i == 3:
            b[0], f[0] = EMPTY_BOX, False
        if not flagged:
            f[:] = False
        c = rng.integers(0, nc, n).astype(np.int32)
        anns.append(ObjectsAnnotation(None, size[1], size[0], c, b, f))
    return anns


def shown(case, anns, infos, assigned):
    """the PROPERTIES the reference's output for this case shows"""
    (size, (B, nc, gmax), k, flagged) = case
    out = set()
    for a, info, asg in zip(anns, infos, assigned):
        by_prior = {}
        for p, g, forced, v in info["claims"]:
            by_prior.setdefault(p, []).append((g, forced, v))
        for cl in by_prior.values():
            if len({g for g, _, _ in cl}) > 1:
                out.add("conflict")
            fv = [v for _, forced, v in cl if forced]
            pv = [v for _, forced, v in cl if not forced]
            if fv and pv and max(pv) > max(fv):  # the larger IoU loses to the forced claim
                out.add("forced_beats_passed")
        if info["tie"]:
            out.add("tie")
        if any(not a.difficults[g] and not (asg == g).any() for g in range(a.num_objects)):
            out.add("owns_nothing")
        if (asg == -3).any():
            out.add("region_row")
    if any(h * w < k for h, w in PR.level_shapes(size)):
        out.add("short_level")
    return out


@functools.lru_cache(maxsize=None)
def reference(case):
    """-> (anns, y [B,P,C], assigned [B,P], npos [B], shown properties); shared by the tests: treat as read-only"""
    (size, (B, nc, gmax), k, flagged) = case
    anns = make_case(case)
    pri = PR.make_priors(size)
    ys, asg, infos = [], [], []
    for a in anns:
        info = {}
        y, g = atss_ref.encode_truth(a.bboxes, a.classes, pri, PR.level_shapes(size), nc, topk=k,
                                     flags=a.difficults.astype(np.int32) if flagged else None, info=info)
        ys.append(y), asg.append(g), infos.append(info)
    y, assigned = np.stack(ys), np.stack(asg)
    for arr in (y, assigned):
        arr.setflags(write=False)
    return anns, y, assigned, (assigned >= 0).sum(1).astype(np.int32), shown(case, anns, infos, assigned)


def expected(case):
    """The properties the case must show, from its parameters alone (checked on the CPU for every case, seeds fixed):
    a distance tie needs the exact cell centres of 64x64; a short level needs k above a level's cell count; a box left with
    nothing needs the zero-area box or a lost prior; conflicts need several boxes and more than the one nearest cell per
    level, or many boxes; a forced claim over a larger passed one needs many boxes on a small grid; a -3 row needs a region."""
    (size, (B, nc, gmax), k, flagged) = case
    want = set()
    if size == (64, 64):
        want.add("tie")
        if k > 4:
            want.add("short_level")
    if gmax == 1 or gmax >= 7:
        want.add("owns_nothing")
    if gmax == 128 or (gmax >= 7 and k > 1):
        want.add("conflict")
    if gmax == 128 and k > 1 and size in SIZES:
        want.add("forced_beats_passed")
    if flagged:
        want.add("region_row")
    return want
