"""Reference for od_assign_anchors_ign (csrc/assign.hip): oracle/assign.py's rule plus ignore regions, numpy f32, op for op
the kernel's sequence => bit-exact.  TEST INFRASTRUCTURE ONLY.

  * a flagged GT box (flags bit 0) never owns a prior: it is left out of the per-prior argmax, of the per-GT force-take and
    of the positives' count; GT indices keep their numbering
  * a prior that came out as background becomes an all-zero row, assigned -3, when inter(prior, r) / area(prior) >= ign_thr
    for any flagged box r; positives stay positive, rows ignored by the IoU band keep -2
  * flags=None (or all zero) is oracle.assign.encode_truth"""
from __future__ import annotations

import numpy as np

from oracle import assign as oassign

IGN_THR = np.float32(0.5)


def cover_matrix(regions, priors):
    """f32 [R,P]: share of each prior's area inside each region, op for op cover_f32 of assign.hip."""
    f = np.float32
    a = regions[:, None, :].astype(f)
    c = priors[None, :, :].astype(f)
    ix1 = np.maximum(a[..., 0], c[..., 0]); iy1 = np.maximum(a[..., 1], c[..., 1])
    ix2 = np.minimum(a[..., 2], c[..., 2]); iy2 = np.minimum(a[..., 3], c[..., 3])
    iw = np.maximum(ix2 - ix1, f(0)); ih = np.maximum(iy2 - iy1, f(0))
    inter = iw * ih
    area_c = np.broadcast_to((c[..., 2] - c[..., 0]) * (c[..., 3] - c[..., 1]), inter.shape)
    with np.errstate(divide="ignore", invalid="ignore"):
        out = np.where(area_c > 0, inter / area_c, f(0))
    return out.astype(f)


def encode_truth(gt_boxes, gt_classes, priors, num_classes=20, flags=None, ign_thr=IGN_THR, pos_thr=oassign.POS_THR,
                 neg_thr=oassign.NEG_THR, loc_scale=0.1):
    """-> (y f32 [P, 2+NC+4], assigned i32 [P]: GT index / -1 background / -2 IoU-band ignore / -3 region ignore)"""
    f = np.float32
    priors = np.asarray(priors, f)
    gt_boxes = np.asarray(gt_boxes, f).reshape(-1, 4)
    gt_classes = np.asarray(gt_classes, np.int64).reshape(-1)
    flagged = np.zeros(len(gt_boxes), bool) if flags is None else (np.asarray(flags, np.int64).reshape(-1) & 1).astype(bool)
    own = np.nonzero(~flagged)[0]  # the boxes that take part in steps 1 and 2, in ascending order
    y, assigned = oassign.encode_truth(gt_boxes[own], gt_classes[own], priors, num_classes, pos_thr, neg_thr, loc_scale)
    pos = assigned >= 0
    assigned[pos] = own[assigned[pos]].astype(np.int32)  # back to the caller's numbering
    if flagged.any():
        cov = cover_matrix(gt_boxes[flagged], priors)
        hit = (cov >= f(ign_thr)).any(0) & (assigned == -1)
        assigned[hit] = -3
        y[hit] = 0
    return y, assigned
