"""Reference for od_assign_atss (csrc/assign_atss.hip): the frozen ATSS rule in numpy, f32 where the rule says f32 and Python
integers for the sums => bit-exact.  TEST INFRASTRUCTURE ONLY.

  1. per unflagged box and level (gh x gw cells, A priors per cell, priors in row order (level, y, x, prior)):
     gx = (x1 + x2) * 0.5f; cx = ((float)x + 0.5f) / (float)gw (same in y); d2 = dx*dx + dy*dy; the min(k, gh*gw) cells with
     the smallest key (d2 bits as u32, cell index) are chosen; all A priors of a chosen cell are candidates (n in all)
  2. v = iou_f32(box, prior); q = rint(v * 2^20); S1 = sum q; S2 = sum q^2; D = n*S2 - S1^2; L = n*q - S1; a candidate
     passes when L >= 0, L^2 >= D and its cell centre lies strictly inside the box
  3. a box with no passing candidate forces its candidate of the largest v > 0 (ties: lowest prior index)
  4. a prior claimed more than once goes to a forced claim, then to the larger v, then to the lower box index
  5. owned priors get oracle.assign's row; the others are background; flagged boxes (bit 0) take no part in 1-4 and turn the
     background priors they cover by >= ign_thr into all-zero rows, assigned -3 (tests/assign_ign_ref.py's rule)"""
from __future__ import annotations

import numpy as np

from assign_ign_ref import IGN_THR, cover_matrix
from oracle import assign as oassign

SCALE = np.float32(1048576.0)


def cell_centres(gh, gw):
    """f32 (cx [gh*gw], cy [gh*gw]) in cell-index order y*gw + x"""
    f = np.float32
    cx = (np.arange(gw, dtype=f) + f(0.5)) / f(gw)
    cy = (np.arange(gh, dtype=f) + f(0.5)) / f(gh)
    return np.tile(cx, gh), np.repeat(cy, gw)


def select_cells(box, gh, gw, topk):
    """-> (chosen cell indices in ascending key order, True when the last chosen and the first refused cell have the same
    d2 bits, so that the cell index decided)"""
    f = np.float32
    box = np.asarray(box, f)
    gx = (box[0] + box[2]) * f(0.5)
    gy = (box[1] + box[3]) * f(0.5)
    cx, cy = cell_centres(gh, gw)
    dx, dy = cx - gx, cy - gy
    d2 = (dx * dx + dy * dy).astype(f)
    key = (d2.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.arange(gh * gw, dtype=np.uint64)
    order = np.argsort(key, kind="stable")
    n = min(int(topk), gh * gw)
    tie = n < gh * gw and (key[order[n - 1]] >> np.uint64(32)) == (key[order[n]] >> np.uint64(32))
    return order[:n].astype(np.int64), bool(tie)


def box_claims(box, priors, grid_hw, A, topk):
    """claims of one box: (prior indices, v f32, forced flag) and whether a distance tie decided a level's choice"""
    f = np.float32
    box = np.asarray(box, f)
    cand, inside, tie, base = [], [], False, 0
    for gh, gw in grid_hw:
        cells, t = select_cells(box, gh, gw, topk)
        tie |= t
        cx, cy = cell_centres(gh, gw)
        ins = (cx[cells] > box[0]) & (cx[cells] < box[2]) & (cy[cells] > box[1]) & (cy[cells] < box[3])
        cand.append((base + cells[:, None] * A + np.arange(A)[None, :]).reshape(-1))
        inside.append(np.repeat(ins, A))
        base += gh * gw * A
    cand, inside = np.concatenate(cand), np.concatenate(inside)
    v = oassign.iou_matrix(box[None], priors[cand])[0]
    q = [int(t) for t in np.rint(v * SCALE).astype(np.int64)]
    n, S1, S2 = len(q), sum(q), sum(t * t for t in q)
    D = n * S2 - S1 * S1
    passed = np.array([n * t - S1 >= 0 and (n * t - S1) ** 2 >= D for t in q], bool) & inside
    if passed.any():
        return cand[passed], v[passed], False, tie
    best = None
    for p, t in zip(cand, v):
        if t > 0 and (best is None or (t, -p) > (best[1], -best[0])):
            best = (p, t)
    if best is None:
        return cand[:0], v[:0], True, tie
    return np.array([best[0]]), np.array([best[1]], f), True, tie


def encode_truth(gt_boxes, gt_classes, priors, grid_hw, num_classes=20, topk=9, flags=None, ign_thr=IGN_THR, loc_scale=0.1,
                 priors_per_cell=8, info=None):
    """-> (y f32 [P, 2+NC+4], assigned i32 [P]: GT index / -1 background / -3 region ignore).  info (a dict) receives
    `claims` (list of (prior, box, forced, v)) and `tie` (a distance tie decided some level's choice)."""
    f = np.float32
    priors = np.asarray(priors, f)
    P, A = len(priors), int(priors_per_cell)
    grid_hw = [(int(h), int(w)) for h, w in grid_hw]
    assert sum(h * w * A for h, w in grid_hw) == P
    gt_boxes = np.asarray(gt_boxes, f).reshape(-1, 4)
    gt_classes = np.asarray(gt_classes, np.int64).reshape(-1)
    flagged = np.zeros(len(gt_boxes), bool) if flags is None else (np.asarray(flags, np.int64).reshape(-1) & 1).astype(bool)
    best = {}  # prior -> (forced, v bits, -g): the largest wins
    claims, tie = [], False
    for g in np.nonzero(~flagged)[0]:
        ps, vs, forced, t = box_claims(gt_boxes[g], priors, grid_hw, A, topk)
        tie |= t
        for p, v in zip(ps, vs):
            claims.append((int(p), int(g), forced, f(v)))
            k = (forced, int(f(v).view(np.uint32)), -int(g))
            if int(p) not in best or k > best[int(p)]:
                best[int(p)] = k
    assigned = np.full(P, -1, np.int32)
    for p, k in best.items():
        assigned[p] = -k[2]
    if flagged.any():
        cov = cover_matrix(gt_boxes[flagged], priors)
        assigned[(cov >= f(ign_thr)).any(0) & (assigned == -1)] = -3
    y = np.zeros((P, 2 + num_classes + 4), f)
    y[assigned == -1, 0] = 1
    ps = np.nonzero(assigned >= 0)[0]
    if len(ps):  # oracle.assign.encode_truth's row
        g = assigned[ps]
        y[ps, 1] = 1
        cls = gt_classes[g]
        ok = (cls >= 0) & (cls < num_classes)
        y[ps[ok], 2 + cls[ok]] = 1
        pr = priors[ps]
        pw = pr[:, 2] - pr[:, 0]; ph = pr[:, 3] - pr[:, 1]
        y[ps, -4:] = ((gt_boxes[g] - pr) / np.stack([pw, ph, pw, ph], 1)) / f(loc_scale)
    if info is not None:
        info["claims"], info["tie"] = claims, tie
    return y, assigned
