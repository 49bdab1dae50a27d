"""Numpy restatement of the soft scan (DESIGN.md "Soft-NMS"), one image at a time, in np.float32: one rounding per operation,
no contraction.  inter / uni are oracle.nms's predicate ops (suppress_matrix_row's, term by term); the merged variants reuse
tests/tta_ref.py (candidates, merged order, box voting).

    HARD, LINEAR, GAUSSIAN = 0, 1, 2
    exp_neg(x)                       od_exp_neg: the fixed-order f32 exp(-x), x >= 0
    scan(boxes, cls, conf, ...)      -> (emitted ranks, their scores at emission)
    soft_nms_image(boxes, keys, ...) -> (keep_flat, keep_conf) of od_soft_nms for one image's sorted keys
    merge_cands(cands, K, ...)       -> tta_ref.merge_image's dict with the soft scan in place of the greedy one
    crowded_image(seed, ...)         -> the generated candidate lists of the host and GPU tests
"""
from __future__ import annotations

import numpy as np

import tta_ref

F = np.float32
HARD, LINEAR, GAUSSIAN = 0, 1, 2
METHODS = {"hard": HARD, "linear": LINEAR, "gaussian": GAUSSIAN}
LOW = np.uint64(0xFFFFFFFF)

_C = [F(1.9875691500e-4), F(1.3981999507e-3), F(8.3334519073e-3), F(4.1665795894e-2), F(1.6666665459e-1), F(5.0000001201e-1)]


def exp_neg(x):
    """od_exp_neg elementwise on an f32 array (any shape), every multiply and add rounded on its own."""
    x = np.asarray(x, F)
    big = x > F(80)
    x = np.where(big, F(0), x)  # the result there is 0, whatever the polynomial would give
    n = np.rint(F(1.44269504) * x)
    r = (x - n * F(0.693359375)) - n * F(-2.12194440e-4)
    y = -r
    p = np.full_like(y, _C[0])
    for c in _C[1:]:
        p = p * y + c
    e = ((p * (y * y)) + y) + F(1)
    scale = ((127 - n.astype(np.int64)).astype(np.uint32) << np.uint32(23)).view(F)
    return np.where(big, F(0), e * scale).astype(F)


def inter_union(a, boxes):
    """oracle.nms.suppress_matrix_row's inter and uni of row a against boxes [m,4], op for op."""
    ix1 = np.maximum(a[0], boxes[:, 0]); iy1 = np.maximum(a[1], boxes[:, 1])
    ix2 = np.minimum(a[2], boxes[:, 2]); iy2 = np.minimum(a[3], boxes[:, 3])
    iw = np.maximum(ix2 - ix1, F(0)); ih = np.maximum(iy2 - iy1, F(0))
    inter = iw * ih
    area_a = (a[2] - a[0]) * (a[3] - a[1])
    area_b = (boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1])
    uni = (area_a + area_b) - inter
    return inter, uni


def scan(boxes, cls, conf, method, thr, strict, max_det, sigma=0.5, min_conf=1e-6):
    """boxes f32 [n,4], cls int [n], conf f32 [n] in rank order -> (ranks int64 [k], scores f32 [k]) in emission order."""
    boxes = np.asarray(boxes, F).reshape(-1, 4)
    cls = np.asarray(cls, np.int64)
    s = np.asarray(conf, F).copy()
    n = len(s)
    thr, sigma, min_conf = F(thr), F(sigma), F(min_conf)
    live = np.ones(n, bool)
    ranks, scores = [], []
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        while len(ranks) < max_det and live.any():
            cand = np.where(live, s, F(-np.inf))
            i = int(np.argmax(cand))  # the first (smallest rank) of the largest score
            if not cand[i] > min_conf:
                break
            ranks.append(i)
            scores.append(s[i])
            live[i] = False
            sel = live.copy()
            if not strict:
                sel &= cls == cls[i]
            idx = np.nonzero(sel)[0]
            if len(idx) == 0:
                continue
            inter, uni = inter_union(boxes[i], boxes[idx])
            pos = inter > F(0)
            over = pos & (inter > thr * uni)
            if method == HARD:
                live[idx[over]] = False
            elif method == LINEAR:
                w = F(1) - inter / uni
                s[idx[over]] = (s[idx] * w)[over]
            else:
                iou = inter / uni
                w = exp_neg((iou * iou) / sigma)
                s[idx[pos]] = (s[idx] * w)[pos]
    return np.asarray(ranks, np.int64), np.asarray(scores, F)


def soft_nms_image(boxes, sorted_keys, num_classes, method, thr=0.45, strict=False, max_det=200, sigma=0.5, min_conf=1e-6):
    """boxes f32 [P,4]; sorted_keys u64 descending (valid ones only) -> (keep_flat i32 [k], keep_conf f32 [k], boxes [k,4])."""
    boxes = np.asarray(boxes, F)
    keys = np.asarray(sorted_keys, np.uint64)
    flat = (LOW - (keys & LOW)).astype(np.int64)
    conf = (keys >> np.uint64(32)).astype(np.uint32).view(F)
    cb = boxes[flat // num_classes].reshape(-1, 4)
    ranks, scores = scan(cb, flat % num_classes, conf, method, thr, strict, max_det, sigma, min_conf)
    return flat[ranks].astype(np.int32), scores, cb[ranks]


def det_rows(keep_flat, keep_conf, kept_boxes, max_det):
    """One image's record block f32 [1 + 6*max_det] as the soft scan writes it (u32 view for a bit-for-bit comparison)."""
    out = np.zeros(1 + 6 * max_det, F)
    w = out.view(np.int32)
    k = len(keep_flat)
    w[0] = k
    w[1::6] = -1
    w[1:1 + 6 * k:6] = keep_flat
    out[2:2 + 6 * k:6] = keep_conf
    for e in range(4):
        out[3 + e:3 + e + 6 * k:6] = kept_boxes[:, e]
    return out.view(np.uint32)


def merge_cands(cands, K, method, thr=0.45, strict=False, max_det=200, vote_iou=0.5, sigma=0.5, min_conf=1e-6):
    """The merged variants for one image: cands = tta_ref.candidates(views, NC) (od_tta_merge_soft) or
    slice_ref.candidates(...)[0] (od_slice_merge_soft).  tta_ref.merge_image with the soft scan in place of the greedy one:
    the votes weigh the ORIGINAL confidences; conf_bits are the rescored ones, in emission order."""
    merged = tta_ref.merged_order(cands, K)
    table = tta_ref._table(merged)
    bits, cls, boxes = table
    keep, scores = scan(boxes, cls, bits.view(F), method, thr, strict, min(max_det, K), sigma, min_conf)
    n = len(keep)
    return {
        "src": np.array([[merged[i][1], merged[i][2]] for i in keep], np.int32).reshape(n, 2),
        "cls": np.array([merged[i][3] for i in keep], np.int32),
        "conf_bits": scores.view(np.uint32).copy(),
        "boxes": np.array([tta_ref.vote(merged, i, vote_iou, table) for i in keep], F).reshape(n, 4),
    }


# ---- the generator the host test puts its conditions on and the GPU test runs -------------------------------------------
GEN_THR, GEN_SIGMA, GEN_MIN_CONF = 0.3, 0.5, 0.05


def crowded_image(seed, n=128, NC=3, P=256, clusters=12, jitter=0.01):
    """n candidates on P priors drawn from `clusters` box clusters (corner jitter N(0, jitter)), classes 0..NC-1,
    confidences uniform(0.05, 1) -> (boxes f32 [P,4], keys u64 [n] sorted descending)."""
    rng = np.random.default_rng(seed)
    c = rng.uniform(0.2, 0.8, (clusters, 2))
    wh = rng.uniform(0.1, 0.3, (clusters, 2))
    base = np.concatenate([c - wh / 2, c + wh / 2], 1)
    boxes = np.clip(base[rng.integers(0, clusters, P)] + rng.normal(0, jitter, (P, 4)), 0, 1).astype(F)
    flat = rng.choice(P * NC, n, replace=n > P * NC).astype(np.uint64)  # more candidates than slots: exact duplicates
    conf = np.nextafter(rng.uniform(0.05, 1.0, n).astype(F), F(2))  # strictly above 0.05
    keys = (conf.view(np.uint32).astype(np.uint64) << np.uint64(32)) | (LOW - flat)
    return boxes, np.sort(keys)[::-1].copy()


# ---- crafted lists: one decision each -----------------------------------------------------------------------------------
CRAFTED = {
    # exact duplicates: the linear weight is 1 - 1 = 0, the candidate is dropped; the Gaussian one is exp(-1 / sigma)
    "duplicates": ([[0.25, 0.25, 0.75, 0.5]] * 3, [0.9, 0.8, 0.7]),
    # zero-area boxes inside a kept box: inter == 0, never rescored, never removed
    "zero_area": ([[0.25, 0.25, 0.75, 0.75], [0.5, 0.25, 0.5, 0.75], [0.5, 0.25, 0.5, 0.75], [0.25, 0.5, 0.75, 0.5]],
                  [0.9, 0.8, 0.7, 0.6]),
    # two equal-confidence candidates mirror images about a third (dyadic corners: equal inter and uni, bit for bit) and
    # disjoint from each other: their rescored scores tie, the lower rank must be emitted first
    "tie": ([[0.25, 0.25, 0.75, 0.75], [0.0, 0.25, 0.5, 0.75], [0.5, 0.25, 1.0, 0.75]], [0.9, 0.625, 0.625]),
    # a strip covered by three disjoint kept boxes (IoU 1/3 each): decayed three times before it is emitted
    "chain": ([[0.0, 0.0, 0.3, 0.3], [0.3, 0.0, 0.6, 0.3], [0.6, 0.0, 0.9, 0.3], [0.0, 0.0, 0.9, 0.3]], [0.9, 0.8, 0.7, 0.6]),
}


def crafted(name, P=256, NC=3):
    """-> (boxes f32 [P,4], keys u64 [n] sorted descending, NC): candidate k sits on prior 10 + 7k, class 1."""
    bx, conf = CRAFTED[name]
    boxes = np.zeros((P, 4), F)
    boxes[:] = F(0.9), F(0.9), F(0.95), F(0.95)
    pri = 10 + 7 * np.arange(len(bx))
    boxes[pri] = np.asarray(bx, F)
    flat = (pri * NC + 1).astype(np.uint64)
    keys = (np.asarray(conf, F).view(np.uint32).astype(np.uint64) << np.uint64(32)) | (LOW - flat)
    assert (np.sort(keys)[::-1] == keys).all()
    return boxes, keys, NC
