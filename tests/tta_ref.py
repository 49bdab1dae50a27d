"""Numpy restatement of od_tta_merge (DESIGN.md "Flip test-time augmentation"), one image at a time, as plain loops in
np.float32: one rounding per operation, no contraction.  The suppression / membership predicate is oracle.nms's.

A view is a dict: keys u64 [K] (sorted descending, the first `count` valid), count, boxes f32 [P,4], flip.
"""
from __future__ import annotations

import numpy as np

from oracle import nms as onms

F = np.float32
LOW = np.uint64(0xFFFFFFFF)


def mirror_box(box):
    """(x1, y1, x2, y2) of a mirrored view -> the box in the original frame: (1 - x2, y1, 1 - x1, y2)."""
    box = np.asarray(box, F)
    return np.array([F(1) - box[2], box[1], F(1) - box[0], box[3]], F)


def candidates(views, NC):
    """Step 1: every candidate of every view as (conf_bits, view, flat, cls, box), in view / list order."""
    out = []
    for v, vw in enumerate(views):
        boxes = np.asarray(vw["boxes"], F)
        for r in range(int(vw["count"])):
            key = np.uint64(vw["keys"][r])
            bits = int(key >> np.uint64(32))
            flat = int(LOW - (key & LOW))
            p, c = flat // NC, flat % NC
            box = boxes[p].copy()
            if vw["flip"]:
                box = mirror_box(box)
            out.append((bits, v, flat, c, box))
    return out


def merged_order(cands, K):
    """Step 2: conf bits descending, then view ascending, then flat ascending; the first min(K, len) are kept."""
    return sorted(cands, key=lambda t: (-t[0], t[1], t[2]))[:K]


def _table(merged):
    n = len(merged)
    bits = np.array([m[0] for m in merged], np.uint32)
    cls = np.array([m[3] for m in merged], np.int64)
    boxes = np.array([m[4] for m in merged], F).reshape(n, 4)
    return bits, cls, boxes


def nms(merged, iou_threshold, strict, max_det):
    """Step 3: greedy NMS over the merged list -> kept merged ranks (rank order, at most max_det).  The loop of
    oracle.nms.nms_image, with its predicate (one row of pairs at a time, elementwise f32)."""
    _, cls, boxes = _table(merged)
    n = len(merged)
    removed = np.zeros(n, bool)
    keep = []
    for i in range(n):
        if removed[i]:
            continue
        keep.append(i)
        if i + 1 < n:
            sup = onms.suppress_matrix_row(boxes[i], boxes[i + 1:], iou_threshold)
            if not strict:
                sup &= cls[i + 1:] == cls[i]
            removed[i + 1:] |= sup
    return keep[:max_det]


def vote(merged, i, vote_iou, table=None):
    """Step 4: the voted box of kept merged rank i: members in ascending rank, multiply and add rounded separately."""
    bits, cls, boxes = table if table is not None else _table(merged)
    a = boxes[i]
    if not vote_iou > 0:
        return a.copy()
    member = onms.suppress_matrix_row(a, boxes, vote_iou) & (cls == cls[i])
    member[i] = True
    conf = bits.view(F)
    sw = F(0)
    s = [F(0), F(0), F(0), F(0)]
    for j in np.nonzero(member)[0]:
        w = conf[j]
        sw = F(sw + w)
        for k in range(4):
            s[k] = F(s[k] + F(w * boxes[j, k]))
    return np.array([F(s[k] / sw) for k in range(4)], F)


def merge_image(views, NC, K, iou_threshold=0.45, strict=False, max_det=200, vote_iou=0.5):
    """-> dict(src i32 [n,2] (view, flat), cls i32 [n], conf_bits u32 [n], boxes f32 [n,4]) of the kept detections."""
    merged = merged_order(candidates(views, NC), K)
    keep = nms(merged, iou_threshold, strict, max_det)
    table = _table(merged)
    n = len(keep)
    return {
        "src": np.array([[merged[i][1], merged[i][2]] for i in keep], np.int32).reshape(n, 2),
        "cls": np.array([merged[i][3] for i in keep], np.int32),
        "conf_bits": np.array([merged[i][0] for i in keep], np.uint32),
        "boxes": np.array([vote(merged, i, vote_iou, table) for i in keep], F).reshape(n, 4),
    }
