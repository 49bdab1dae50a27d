"""Reference for the quality targets (csrc/quality.hip: od_quality_iou, od_quality_tal) and for the quality-aware objectness
terms of od_loss_fwd_bwd_quality (csrc/loss.hip).  TEST INFRASTRUCTURE ONLY.

Quality targets: the decode, the corner sort, u, the static IoU and the maxima are f32 op for op (bit-exact against the
device); expf(l - lmax) is taken in f64, so aligned rows of the "tal" mode are compared by tolerance (aligned_rtol).

Objectness (f64, in forms without cancellation; z = l1 - l0, e = exp(-|z|), p = {1, e} / (1 + e), 1 - p = {e, 1} / (1 + e),
sp(t) = max(t, 0) + log1p(e), CE = q sp(-z) + (1 - q) sp(z), p - q taken as (1 - q) - (1 - p) where p > 1/2):
  focal: oracle/loss.py
  qfl:   assigned rows L = alpha |q - p|^gamma CE;  dL/dz = alpha (gamma d^(gamma-1) sgn(p - q) p (1 - p) CE + d^gamma (p - q))
  vfl:   assigned rows with q > 0: L = q CE, dL/dz = q (p - q);  with q == 0: focal's background term (1 - alpha included)
Background rows take focal's background term and ignore rows nothing, in every mode; q is clamped to [0,1] (NaN -> 0).  Class
and box terms come from oracle/loss.py and tests/iou_loss_ref.py."""
from __future__ import annotations

import numpy as np

import iou_loss_ref
from oracle import loss as oloss

OBJ_MODES = ("focal", "qfl", "vfl")


# ---------------------------------------------------------------- quality targets

def iou_rows(a, c):
    """f32 [n]: iou_f32 (csrc/assign_common.h) of the box pairs a[i], c[i], op for op (fmaxf / fminf drop a NaN)."""
    f = np.float32
    a, c = np.asarray(a, f).reshape(-1, 4), np.asarray(c, f).reshape(-1, 4)
    with np.errstate(all="ignore"):
        ix1, iy1 = np.fmax(a[:, 0], c[:, 0]), np.fmax(a[:, 1], c[:, 1])
        ix2, iy2 = np.fmin(a[:, 2], c[:, 2]), np.fmin(a[:, 3], c[:, 3])
        iw, ih = np.fmax(ix2 - ix1, f(0)), np.fmax(iy2 - iy1, f(0))
        inter = iw * ih
        area_a = (a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1])
        area_c = (c[:, 2] - c[:, 0]) * (c[:, 3] - c[:, 1])
        uni = (area_a + area_c) - inter
        out = np.where(uni > 0, inter / np.where(uni > 0, uni, f(1)), f(0))
    return out.astype(f)


def decode(loc, pr, loc_scale=0.1):
    """od_decode_one without clip, f32 op for op: loc, pr [n,4] -> [n,4]"""
    f = np.float32
    loc, pr = np.asarray(loc, f), np.asarray(pr, f)
    s = f(loc_scale)
    with np.errstate(all="ignore"):
        pw, ph = pr[:, 2] - pr[:, 0], pr[:, 3] - pr[:, 1]
        return np.stack([pr[:, 0] + (loc[:, 0] * s) * pw, pr[:, 1] + (loc[:, 1] * s) * ph,
                         pr[:, 2] + (loc[:, 2] * s) * pw, pr[:, 3] + (loc[:, 3] * s) * ph], 1).astype(f)


def pbox(loc, pr, loc_scale=0.1):
    """-> (predicted boxes with sorted corners f32 [n,4], every coordinate finite [n])"""
    d = decode(loc, pr, loc_scale)
    sx, sy = d[:, 0] <= d[:, 2], d[:, 1] <= d[:, 3]
    b = np.stack([np.where(sx, d[:, 0], d[:, 2]), np.where(sy, d[:, 1], d[:, 3]),
                  np.where(sx, d[:, 2], d[:, 0]), np.where(sy, d[:, 3], d[:, 1])], 1).astype(np.float32)
    return b, np.isfinite(b).all(1)


def _clamp(q):
    with np.errstate(invalid="ignore"):
        return np.fmin(np.fmax(q, q.dtype.type(0)), q.dtype.type(1))


def quality_iou(pred, y, priors, loc_scale=0.1):
    """pred, y [B,P,C], priors [P,4] -> q f32 [B,P], the bytes od_quality_iou writes"""
    pred, y = np.asarray(pred, np.float32), np.asarray(y, np.float32)
    B, P, _ = pred.shape
    p2, y2 = pred.reshape(B * P, -1), y.reshape(B * P, -1)
    q = np.zeros(B * P, np.float32)
    rows = np.nonzero(y2[:, 1] > 0.5)[0]
    if len(rows):
        pr = np.asarray(priors, np.float32)[rows % P]
        b, ok = pbox(p2[rows, -4:], pr, loc_scale)
        g = decode(y2[rows, -4:], pr, loc_scale)
        q[rows] = np.where(ok, _clamp(iou_rows(g, b)), np.float32(0))
    return q.reshape(B, P)


def quality_tal(pred, y, priors, gt_boxes, assigned, metric, loc_scale=0.1):
    """pred, y [B,P,C], priors [P,4], gt_boxes [B,Gmax,4], assigned i32 [B,P], metric f32 [B,P] (od_assign_tal's) -> dict:
      q f64 [B,P]: the value of every row (exact f32 numbers on forced rows and on rows with l == lmax)
      aligned / forced bool [B,P];  exact bool [B,P]: rows whose q the device must give bit for bit (everything but aligned
      rows with l < lmax);  dl f64 [B,P]: l - lmax on aligned rows (<= 0);  u f32 [B,P];
      lmax, umax f32 [B,Gmax] (NaN where an object has no aligned row)"""
    f = np.float32
    pred, y = np.asarray(pred, f), np.asarray(y, f)
    gt_boxes, metric = np.asarray(gt_boxes, f), np.asarray(metric, f)
    assigned = np.asarray(assigned)
    B, P, _ = pred.shape
    G = gt_boxes.shape[1]
    q = np.zeros((B, P), np.float64)
    u = np.zeros((B, P), f)
    dl = np.zeros((B, P), np.float64)
    aligned, forced = np.zeros((B, P), bool), np.zeros((B, P), bool)
    lmax, umax = np.full((B, G), np.nan, f), np.full((B, G), np.nan, f)
    pri = np.asarray(priors, f)
    for b in range(B):
        rows = np.nonzero((y[b, :, 1] > 0.5) & (assigned[b] >= 0) & (assigned[b] < G))[0]
        if not len(rows):
            continue
        g = assigned[b, rows]
        pb, ok = pbox(pred[b, rows, -4:], pri[rows], loc_scale)
        ub = np.where(ok, iou_rows(gt_boxes[b, g], pb), f(0)).astype(f)
        u[b, rows] = ub
        with np.errstate(invalid="ignore"):
            al = metric[b, rows] < 0
        aligned[b, rows[al]], forced[b, rows[~al]] = True, True
        for o in np.unique(g[al]):
            m = al & (g == o)
            lmax[b, o], umax[b, o] = metric[b, rows[m]].max(), ub[m].max()
        ra, ga = rows[al], g[al]
        d = metric[b, ra].astype(np.float64) - lmax[b, ga].astype(np.float64)
        dl[b, ra] = d
        q[b, ra] = _clamp(np.exp(d) * umax[b, ga].astype(np.float64))
        rf, gf = rows[~al], g[~al]
        q[b, rf] = _clamp(np.fmax(ub[~al], iou_rows(gt_boxes[b, gf], pri[rf])))
    exact = ~aligned | (dl == 0)
    return {"q": q, "aligned": aligned, "forced": forced, "exact": exact, "dl": dl, "u": u, "lmax": lmax, "umax": umax}


def aligned_rtol(dl):
    """Tolerance of an aligned row's q against the f64 value: one f32 subtraction (half an ulp of |l - lmax|), expf within
    2 ulp, one multiply: about 2e-7 (1 + |l - lmax|); 1e-5 (1 + |l - lmax|) leaves a margin of about 50."""
    return 1e-5 * (1.0 + np.abs(dl))


# ---------------------------------------------------------------- objectness

def clamp_quality(q):
    q = np.asarray(q, np.float64)
    return np.where(np.isnan(q), 0.0, np.clip(np.where(np.isnan(q), 0.0, q), 0.0, 1.0))


def objectness(pred, y, quality, mode, alpha=0.25, gamma=2.0):
    """pred, y [..., C], quality [...] -> (loss per row, d loss / d z per row, p per row) in f64, unnormalised and unweighted;
    z = l1 - l0.  mode "focal" ignores quality."""
    assert mode in OBJ_MODES
    pred, y = np.asarray(pred, np.float64), np.asarray(y, np.float64)
    t0, t1 = y[..., 0], y[..., 1]
    pos = t1 > 0.5
    active = (t0 + t1) > 0
    q = np.where(pos, clamp_quality(quality), 0.0) if mode != "focal" else np.zeros(pos.shape)
    with np.errstate(all="ignore"):
        z = pred[..., 1] - pred[..., 0]
        nf = z * 0.0
        e = np.exp(-np.abs(z))
        p = np.where(z >= 0, 1.0, e) / (1.0 + e)
        om = np.where(z >= 0, e, 1.0) / (1.0 + e)
        l1p = np.log1p(e)
        spn, spp = np.maximum(-z, 0.0) + l1p, np.maximum(z, 0.0) + l1p  # sp(-z) = -log p, sp(z) = -log(1 - p)
        # focal, as oracle/loss.py: the target's probability pt, om_t = 1 - pt
        fpos = pos if mode == "focal" else np.zeros(pos.shape, bool)  # soft modes: only background-like rows come here
        pt, omt, lpt = np.where(fpos, p, om), np.where(fpos, om, p), -np.where(fpos, spn, spp)
        a = np.where(fpos, alpha, 1.0 - alpha)
        mod = omt ** gamma
        ratio = np.where(omt > 0, lpt / np.where(omt > 0, omt, 1.0), -1.0)
        lf = -a * mod * lpt + nf
        gt = -a * mod * (1.0 - gamma * pt * ratio) * omt + nf  # d loss / d l_t
        gf = np.where(fpos, gt, -gt)  # d loss / d z
        # soft rows
        ce = q * spn + (1.0 - q) * spp
        pmq = np.where(z >= 0, (1.0 - q) - om, p - q)
        d = np.abs(pmq)
        if mode == "qfl":
            soft = pos
            ls = alpha * d ** gamma * ce + nf
            gs = alpha * (gamma * d ** (gamma - 1.0) * np.sign(pmq) * (p * om) * ce + d ** gamma * pmq) + nf
        elif mode == "vfl":
            soft = pos & (q > 0)
            ls, gs = q * ce + nf, q * pmq + nf
        else:
            soft, ls, gs = np.zeros(pos.shape, bool), lf, gf
        loss = np.where(soft, ls, np.where(active, lf, 0.0))
        dz = np.where(soft, gs, np.where(active, gf, 0.0))
    return loss, dz, p


def loss_and_grad(pred, y, quality, num_classes, mode, alpha=0.25, gamma=2.0, box_mode="smooth_l1", w=(1.0, 1.0, 1.0),
                  priors=None, loc_scale=0.1):
    """The full reference of od_loss_fwd_bwd_quality: (losses [4], grad like pred) in f64.  Class and box terms from
    oracle/loss.py (box_mode "smooth_l1" | "mse") or tests/iou_loss_ref.py ("giou" | "diou" | "ciou", needs priors); the
    objectness columns and losses[0] from objectness()."""
    pred32, y32 = np.asarray(pred, np.float32), np.asarray(y, np.float32)
    if box_mode in iou_loss_ref.MODES:
        rl, rg = iou_loss_ref.full_reference(pred32, y32, priors, num_classes, box_mode, loc_scale, w=w, alpha=alpha, gamma=gamma)
    else:
        rl, rg = oloss.loss_and_grad(pred32, y32, num_classes, alpha=alpha, gamma=gamma, box_mode=box_mode, w=w)
    n = max(1, int((y32[..., 1] > 0.5).sum()))
    lo, dz, _p = objectness(pred32, y32, quality, mode, alpha, gamma)
    rg = np.array(rg, np.float64)
    rg[..., 1] = dz * w[0] / n
    rg[..., 0] = -dz * w[0] / n
    losses = np.array([lo.sum() * w[0] / n, rl[1], rl[2]])
    return np.append(losses, losses.sum()), rg


def min_gap(pred, y, quality):
    """min |q - p| over the assigned rows (f64): the general GPU cases keep it >= 1e-3"""
    y = np.asarray(y)
    pos = y[..., 1] > 0.5
    _l, _g, p = objectness(pred, y, quality, "qfl")
    return float(np.abs(clamp_quality(quality) - p)[pos].min()) if pos.any() else np.inf
