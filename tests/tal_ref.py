"""Reference for od_assign_tal (csrc/assign_tal.hip): the frozen task-aligned rule in numpy.  u, v, pbox and the claim order
are f32 op for op (bit-exact); the metric l is computed in f64 from them, and the one place where the device's logf / expf
can matter, the cut at rank topk, is reported as SURE and MAYBE claims.  TEST INFRASTRUCTURE ONLY.

  1. per prior, from its pred row (z0, z1, NC class logits, 4 offsets): la = (z1 - m) - log(exp(z0 - m) + exp(z1 - m)) with
     m = max(z0, z1); lse = mc + log(sum exp(z_c - mc)) with mc = max z_c; pbox = od_decode_locs' formula in f32, no clip,
     corners sorted.  A prior with a non-finite pbox coordinate, la or lse is no candidate.
  2. per unflagged box: candidates = priors whose cell centre ((x + .5f) / gw, (y + .5f) / gh) lies strictly inside the box
     and whose u = iou_f32(box, pbox) > 0;  l = alpha * ((la + z_cls) - lse) + beta * log(u), the class term dropped for a
     class outside 0..NC-1;  the box claims its min(topk, n) candidates of the largest l (ties: lower prior index)
  3. a box without a candidate forces the prior of the largest static iou_f32(box, prior) > 0 (ties: lowest index)
  4. a prior claimed more than once goes to a forced claim, then to the larger v (u, or the static IoU of a forced claim;
     f32 bits), then to the lower box
  5. rows, ignore regions, assigned (never -2): atss_ref's step 5

The cut: tau = 1e-4 * (1 + |l|).  l is a handful of f32 log / exp results plus a max-subtracted sum of at most 1024 terms,
each good to a few 2^-23 relative, so a device's l lies within about 1e-6 * (1 + |l|) of the f64 value; tau is 100 times that.
A claim inside the top topk is SURE when it beats every refused candidate by more than tau, MAYBE otherwise; a refused
candidate within tau of a chosen one is a MAYBE claim too.  Candidates whose inputs (la, lse, z_cls, u) are all equal have
bit-equal l on any device: the prior index decides between them, they never make each other MAYBE."""
from __future__ import annotations

import numpy as np

from assign_ign_ref import IGN_THR, cover_matrix
from atss_ref import cell_centres
from oracle import assign as oassign

TAU = 1e-4


def tau(l):
    return TAU * (1.0 + np.abs(l))


def per_prior(pred, priors, num_classes, loc_scale=0.1):
    """pred f32 [P, 2+NC+4] -> (la f64 [P], lse f64 [P], pbox f32 [P,4], raw decode f32 [P,4], valid bool [P])"""
    f = np.float32
    pred = np.asarray(pred, f)
    priors = np.asarray(priors, f)
    nc = int(num_classes)
    with np.errstate(all="ignore"):
        z = pred.astype(np.float64)
        m = np.fmax(z[:, 0], z[:, 1])
        la = (z[:, 1] - m) - np.log(np.exp(z[:, 0] - m) + np.exp(z[:, 1] - m))
        zc = z[:, 2:2 + nc]
        mc = np.fmax.reduce(zc, axis=1)
        lse = mc + np.log(np.exp(zc - mc[:, None]).sum(1))
        loc = pred[:, 2 + nc:]
        pw, ph = priors[:, 2] - priors[:, 0], priors[:, 3] - priors[:, 1]
        s = f(loc_scale)
        d = np.stack([priors[:, 0] + (loc[:, 0] * s) * pw, priors[:, 1] + (loc[:, 1] * s) * ph,
                      priors[:, 2] + (loc[:, 2] * s) * pw, priors[:, 3] + (loc[:, 3] * s) * ph], 1).astype(f)
        sx, sy = d[:, 0] <= d[:, 2], d[:, 1] <= d[:, 3]
        pbox = np.stack([np.where(sx, d[:, 0], d[:, 2]), np.where(sy, d[:, 1], d[:, 3]),
                         np.where(sx, d[:, 2], d[:, 0]), np.where(sy, d[:, 3], d[:, 1])], 1).astype(f)
        valid = np.isfinite(pbox).all(1) & np.isfinite(la.astype(f)) & np.isfinite(lse.astype(f))
    return la, lse, pbox, d, valid


def prior_centres(grid_hw, A):
    """f32 (cx [P], cy [P]): the cell centre of every prior, in prior row order (level, y, x, prior)"""
    cxs, cys = [], []
    for gh, gw in grid_hw:
        cx, cy = cell_centres(gh, gw)
        cxs.append(np.repeat(cx, A)), cys.append(np.repeat(cy, A))
    return np.concatenate(cxs), np.concatenate(cys)


def box_claims(box, cls, pp, pred, priors, centres, num_classes, topk, alpha, beta):
    """claims of one box -> list of (prior, v f32, forced, l f64 | None, kind) with kind "sure" | "maybe_in" | "maybe_out"
    (maybe_out: refused by the f64 order, within tau of the cut), and the candidates' prior indices"""
    f = np.float32
    la, lse, pbox, _d, valid = pp
    box = np.asarray(box, f)
    cx, cy = centres
    with np.errstate(all="ignore"):
        idx = np.nonzero((cx > box[0]) & (cx < box[2]) & (cy > box[1]) & (cy < box[3]) & valid)[0]
        u = oassign.iou_matrix(box[None], pbox[idx])[0].astype(f) if len(idx) else np.zeros(0, f)
        idx, u = idx[u > 0], u[u > 0]
    if len(idx) == 0:
        with np.errstate(all="ignore"):
            v = oassign.iou_matrix(box[None], priors)[0].astype(f)
        if not (v > 0).any():
            return [], idx
        p = int(np.nonzero(v == v[v > 0].max())[0][0])
        return [(p, v[p], True, None, "sure")], idx
    has = 0 <= int(cls) < num_classes
    zc = pred[idx, 2 + int(cls)].astype(np.float64) if has else np.zeros(len(idx))
    a, b = float(f(alpha)), float(f(beta))
    l = a * ((la[idx] + zc) - lse[idx] if has else la[idx]) + b * np.log(u.astype(np.float64))
    order = np.lexsort((idx, -l))
    idx, u, l, zc = idx[order], u[order], l[order], zc[order]
    n, k = len(idx), min(int(topk), len(idx))
    same = lambda i, j: (la[idx[i]] == la[idx[j]] and lse[idx[i]] == lse[idx[j]] and zc[i] == zc[j] and u[i] == u[j])  # noqa: E731
    kind = ["sure"] * k + [None] * (n - k)
    for i in range(k - 1, -1, -1):  # chosen, from the cut upwards
        if k == n or l[i] - l[k] > tau(l[i]):
            break  # sorted: everything above beats every refused candidate by more as well
        if any(l[i] - l[j] <= tau(l[i]) and not same(i, j) for j in range(k, n) if l[i] - l[j] <= tau(l[i])):
            kind[i] = "maybe_in"
    for j in range(k, n):  # refused, from the cut downwards
        if l[k - 1] - l[j] > tau(l[j]):
            break
        if any(l[i] - l[j] <= tau(l[j]) and not same(i, j) for i in range(k - 1, -1, -1) if l[i] - l[j] <= tau(l[j])):
            kind[j] = "maybe_out"
    return [(int(idx[i]), u[i], False, float(l[i]), kind[i]) for i in range(n) if kind[i]], np.sort(idx)


def rows_for(assigned, gt_boxes, gt_classes, priors, num_classes, loc_scale=0.1):
    """the target rows of an ownership table (GT index / -1 background / -3 region): oracle.assign.encode_truth's row"""
    f = np.float32
    priors = np.asarray(priors, f)
    gt_boxes = np.asarray(gt_boxes, f).reshape(-1, 4)
    gt_classes = np.asarray(gt_classes, np.int64).reshape(-1)
    y = np.zeros((len(priors), 2 + num_classes + 4), f)
    y[assigned == -1, 0] = 1
    ps = np.nonzero(assigned >= 0)[0]
    if len(ps):
        g = assigned[ps]
        y[ps, 1] = 1
        cls = gt_classes[g]
        ok = (cls >= 0) & (cls < num_classes)
        y[ps[ok], 2 + cls[ok]] = 1
        pr = priors[ps]
        pw = pr[:, 2] - pr[:, 0]; ph = pr[:, 3] - pr[:, 1]
        y[ps, -4:] = ((gt_boxes[g] - pr) / np.stack([pw, ph, pw, ph], 1)) / f(loc_scale)
    return y


def encode_truth(gt_boxes, gt_classes, pred, priors, grid_hw, num_classes=20, topk=13, alpha=1.0, beta=6.0, flags=None,
                 ign_thr=IGN_THR, loc_scale=0.1, priors_per_cell=8):
    """One image -> dict:
      assigned i32 [P], y f32 [P,C], metric f64 [P], normal bool [P] (the owner's claim is a normal one): the result under
      the f64 order (every MAYBE resolved as f64 says)
      undecided bool [P]: the prior is in some box's MAYBE set;  allowed: {undecided prior: set of owners a device may report}
      claimed_sure / claimed_any bool [P]: priors with a sure (or forced) claimant / with any claimant
      bg i32 [P]: what an unowned prior is (-1 background, -3 inside a region)
      claims: list of (prior, box, v f32, forced, l, kind);  cands: {box: its candidates' prior indices};  pp: per_prior's tuple"""
    f = np.float32
    priors = np.asarray(priors, f)
    pred = np.asarray(pred, f)
    P, A = len(priors), int(priors_per_cell)
    grid_hw = [(int(h), int(w)) for h, w in grid_hw]
    assert sum(h * w * A for h, w in grid_hw) == P and pred.shape == (P, num_classes + 6)
    gt_boxes = np.asarray(gt_boxes, f).reshape(-1, 4)
    gt_classes = np.asarray(gt_classes, np.int64).reshape(-1)
    flagged = np.zeros(len(gt_boxes), bool) if flags is None else (np.asarray(flags, np.int64).reshape(-1) & 1).astype(bool)
    pp = per_prior(pred, priors, num_classes, loc_scale)
    centres = prior_centres(grid_hw, A)
    claims, cands = [], {}
    best = {}  # prior -> ((forced, v bits, -g), l): the largest key wins, among the claims the f64 order makes
    sure, anyc, undecided, allowed = np.zeros(P, bool), np.zeros(P, bool), np.zeros(P, bool), {}
    for g in np.nonzero(~flagged)[0]:
        cl, cands[int(g)] = box_claims(gt_boxes[g], gt_classes[g], pp, pred, priors, centres, num_classes, topk, alpha, beta)
        for p, v, forced, l, kind in cl:
            claims.append((p, int(g), f(v), forced, l, kind))
            anyc[p] = True
            allowed.setdefault(p, set()).add(int(g))
            if kind == "sure":
                sure[p] = True
            else:
                undecided[p] = True
            if kind != "maybe_out":
                k = (forced, int(f(v).view(np.uint32)), -int(g))
                if p not in best or k > best[p][0]:
                    best[p] = (k, l)
    assigned = np.full(P, -1, np.int32)
    metric, normal = np.zeros(P, np.float64), np.zeros(P, bool)
    for p, (k, l) in best.items():
        assigned[p] = -k[2]
        if not k[0]:
            metric[p], normal[p] = l, True
    bg = np.full(P, -1, np.int32)
    if flagged.any():
        cov = cover_matrix(gt_boxes[flagged], priors)
        bg[(cov >= f(ign_thr)).any(0)] = -3
    assigned[assigned == -1] = bg[assigned == -1]
    for p in list(allowed):
        if not undecided[p]:
            del allowed[p]
        elif not sure[p]:
            allowed[p].add(int(bg[p]))
    return {"assigned": assigned, "y": rows_for(assigned, gt_boxes, gt_classes, priors, num_classes, loc_scale),
            "metric": metric, "normal": normal, "undecided": undecided, "allowed": allowed, "claimed_sure": sure, "claimed_any": anyc, "bg": bg,
            "claims": claims, "cands": cands, "pp": pp}


def check_image(ref, gt_boxes, gt_classes, priors, num_classes, y, assigned, npos, metric=None, loc_scale=0.1):
    """The parity rule on one image of a device's result (y [P,C], assigned [P], npos scalar, metric [P] or None):
    decided priors: equal owner, byte-identical row, |metric - l| <= tau for a normal claim and metric == 0 otherwise;
    undecided priors: an owner from `allowed`, and the row that owner implies; npos between the sure and the any count.
    -> the largest |metric - l| / (1 + |l|) over the decided normal claims"""
    dec = ~ref["undecided"]
    assert (assigned[dec] == ref["assigned"][dec]).all(), "a decided prior has another owner"
    for p, ok in ref["allowed"].items():
        assert int(assigned[p]) in ok, f"prior {p}: owner {int(assigned[p])} is none of {sorted(ok)}"
    assert not (assigned == -2).any()
    want = rows_for(assigned, gt_boxes, gt_classes, priors, num_classes, loc_scale)
    assert y.tobytes() == want.tobytes(), "a row is not the row of its owner"
    assert y[dec].tobytes() == ref["y"][dec].tobytes()
    assert int(npos) == int((assigned >= 0).sum())
    assert int(ref["claimed_sure"].sum()) <= int(npos) <= int(ref["claimed_any"].sum())
    worst = 0.0
    if metric is not None:
        assert np.isfinite(metric[dec]).all()
        normal = dec & ref["normal"]
        err = np.abs(metric[normal].astype(np.float64) - ref["metric"][normal])
        assert (err <= tau(ref["metric"][normal])).all(), f"metric off by {err.max():.3g}"
        assert (metric[dec & ~normal] == 0).all(), "background, ignored and forced rows have metric 0"
        if normal.any():
            worst = float((err / (1.0 + np.abs(ref["metric"][normal]))).max())
    return worst
