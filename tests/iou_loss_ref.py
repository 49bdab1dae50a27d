"""Reference for the IoU-family box losses (box modes giou / diou / ciou of od_loss_fwd_bwd_iou, csrc/loss.hip), and the inputs
of the GPU cases in test_gpu_iou_loss.py.

`loss_and_grad` is a torch-CPU function of (pred_loc, y_loc, priors, loc_scale, mode): it builds each row's loss from the
published formulas and takes the gradient from autograd, so the kernel's hand-derived gradient is checked against something
that shares none of its algebra.  float64 is the reference; the same function in float32 (`loss_and_grad_f32`, the "f32
restatement") says how far f32 arithmetic alone moves a row's gradient, which sets the tolerance of the GPU test.

Placement of eps = 1e-9 (normalised image units; real boxes have areas >= 2e-6), which the kernel mirrors:
  b = prior + (pred_loc * loc_scale) * [pw, ph, pw, ph],  g likewise from y_loc                 (od_decode_one, no clip)
  x1, x2 = min / max (bx1, bx2),  y1, y2 likewise;  wb = x2 - x1, hb = y2 - y1, wg, hg of g      (GIoU paper, Algorithm 2)
  iw = max(0, min(x2, gx2) - max(x1, gx1)), ih likewise;  inter = iw * ih
  union = ((wb * hb + wg * hg) - inter) + eps;  IoU = inter / union
  cw = max(x2, gx2) - min(x1, gx1), ch likewise
  giou:  C = cw * ch + eps;                 m = IoU - (C - union) / C
  diou:  D = (cw^2 + ch^2) + eps;           m = IoU - rho2 / D,  rho2 = dx^2 + dy^2,  dx = ((x1 + x2) - (gx1 + gx2)) / 2
  ciou:  v = (4 / pi^2) * (atan2(wg, hg + eps) - atan2(wb, hb + eps))^2
         alpha = v / (((1 - IoU) + v) + eps), constant in the gradient;  m = diou - alpha * v
  loss = 1 - m
A zero-size predicted box leaves every denominator positive: union >= wg * hg, C and D >= those of g, and atan2's
derivative divides by wb^2 + (hb + eps)^2 >= eps^2.

`margins` returns the signed differences behind every min / max / clamp of a row.  Within f32 coordinate rounding (<= 6e-8)
of a tie, f32 and f64 may take different branches and the gradient legitimately jumps, so the GPU cases are REQUIRED to keep
every margin of every assigned row at or above MARGIN_MIN in absolute value; no row is ever left out of a comparison.
"""
from __future__ import annotations

import functools
import math

import numpy as np
import torch

from oracle import loss as oloss

EPS = 1e-9
MODES = {"giou": 2, "diou": 3, "ciou": 4}
MARGIN_MIN = 1e-5
MARGIN_NAMES = ("bx1-bx2", "by1-by2", "x1-gx1", "y1-gy1", "x2-gx2", "y2-gy2", "iw", "ih")


def _decode(loc, pr, loc_scale):
    pw, ph = pr[:, 2] - pr[:, 0], pr[:, 3] - pr[:, 1]
    return (pr[:, 0] + (loc[:, 0] * loc_scale) * pw, pr[:, 1] + (loc[:, 1] * loc_scale) * ph,
            pr[:, 2] + (loc[:, 2] * loc_scale) * pw, pr[:, 3] + (loc[:, 3] * loc_scale) * ph)


def _forward(pl, yl, pr, loc_scale, mode, alpha_fixed=None):
    """-> (loss [n], alpha [n] or None, margins [n, 8]); torch tensors of pl's dtype."""
    b0, b1, b2, b3 = _decode(pl, pr, loc_scale)
    g0, g1, g2, g3 = _decode(yl, pr, loc_scale)
    x1, x2 = torch.minimum(b0, b2), torch.maximum(b0, b2)
    y1, y2 = torch.minimum(b1, b3), torch.maximum(b1, b3)
    wb, hb, wg, hg = x2 - x1, y2 - y1, g2 - g0, g3 - g1
    iwr = torch.minimum(x2, g2) - torch.maximum(x1, g0)
    ihr = torch.minimum(y2, g3) - torch.maximum(y1, g1)
    iw, ih = torch.clamp(iwr, min=0), torch.clamp(ihr, min=0)
    inter = iw * ih
    union = ((wb * hb + wg * hg) - inter) + EPS
    iou = inter / union
    cw = torch.maximum(x2, g2) - torch.minimum(x1, g0)
    ch = torch.maximum(y2, g3) - torch.minimum(y1, g1)
    alpha = None
    if mode == "giou":
        c = cw * ch + EPS
        m = iou - (c - union) / c
    else:
        dx = ((x1 + x2) - (g0 + g2)) * 0.5
        dy = ((y1 + y2) - (g1 + g3)) * 0.5
        m = iou - (dx * dx + dy * dy) / ((cw * cw + ch * ch) + EPS)
        if mode == "ciou":
            da = torch.atan2(wg, hg + EPS) - torch.atan2(wb, hb + EPS)
            v = (4.0 / math.pi ** 2) * (da * da)
            alpha = (v / (((1.0 - iou) + v) + EPS)).detach() if alpha_fixed is None else alpha_fixed
            m = m - alpha * v
        elif mode != "diou":
            raise ValueError(mode)
    marg = torch.stack([b0 - b2, b1 - b3, x1 - g0, y1 - g1, x2 - g2, y2 - g3, iwr, ihr], 1)
    return 1.0 - m, alpha, marg


def _tensors(pred_loc, y_loc, priors, dtype):
    # inputs are f32 data: both precisions start from the same numbers
    return tuple(torch.tensor(np.asarray(a, np.float32).reshape(-1, 4), dtype=dtype) for a in (pred_loc, y_loc, priors))


def loss_and_grad(pred_loc, y_loc, priors, loc_scale, mode, dtype=torch.float64):
    """Rows [n,4] of loc columns and their priors -> (loss [n], d loss / d pred_loc [n,4]) as f64 numpy, computed in `dtype`;
    the gradient comes from autograd with alpha detached."""
    pl, yl, pr = _tensors(pred_loc, y_loc, priors, dtype)
    pl.requires_grad_(True)
    loss, _a, _m = _forward(pl, yl, pr, float(loc_scale), mode)
    loss.sum().backward()
    return loss.detach().double().numpy(), pl.grad.double().numpy()


def loss_and_grad_f32(pred_loc, y_loc, priors, loc_scale, mode):
    """The f32 restatement: the same function evaluated in float32."""
    return loss_and_grad(pred_loc, y_loc, priors, loc_scale, mode, dtype=torch.float32)


def loss_values(pred_loc, y_loc, priors, loc_scale, mode, alpha_fixed=None):
    """f64 losses [n] only; alpha_fixed [n] freezes ciou's alpha (finite differences of what the gradient differentiates)."""
    _pl, yl, pr = _tensors(pred_loc, y_loc, priors, torch.float64)
    pl = torch.tensor(np.asarray(pred_loc, np.float64).reshape(-1, 4))  # not rounded to f32: the caller perturbs it
    af = None if alpha_fixed is None else torch.tensor(np.asarray(alpha_fixed, np.float64))
    return _forward(pl, yl, pr, float(loc_scale), mode, af)[0].numpy()


def ciou_alpha(pred_loc, y_loc, priors, loc_scale):
    pl, yl, pr = _tensors(pred_loc, y_loc, priors, torch.float64)
    return _forward(pl, yl, pr, float(loc_scale), "ciou")[1].numpy()


def margins(pred_loc, y_loc, priors, loc_scale):
    """Decision margins [n, 8] (MARGIN_NAMES) in f64."""
    pl, yl, pr = _tensors(pred_loc, y_loc, priors, torch.float64)
    return _forward(pl, yl, pr, float(loc_scale), "giou")[2].numpy()


def row_rel_err(g, g_ref):
    """Per row: max_k |g_k - g_ref_k| / max_k |g_ref_k| over the four box columns."""
    g, g_ref = np.asarray(g, np.float64), np.asarray(g_ref, np.float64)
    return np.abs(g - g_ref).max(-1) / np.abs(g_ref).max(-1)


def full_reference(pred, y, priors, num_classes, mode, loc_scale, w=(1.0, 1.0, 1.0), alpha=0.25, gamma=2.0):
    """pred, y [B,P,C] (or [R,C] with R a multiple of P), priors [P,4] -> (losses [4], grad like pred), f64: objectness and
    class columns from oracle.loss.loss_and_grad, box columns and losses[2] from this module with the same
    w_box / max(1, #assigned)."""
    pred = np.asarray(pred, np.float32)
    y = np.asarray(y, np.float32)
    shape = pred.shape
    P = len(priors)
    p2, y2 = pred.reshape(-1, shape[-1]), y.reshape(-1, shape[-1])
    assert p2.shape[0] % P == 0
    pos = np.nonzero(y2[:, 1] > 0.5)[0]
    clean = p2.copy()
    clean[:, -4:] = 0  # the oracle's own box term is replaced: keep whatever these columns hold out of it
    yc = y2.copy()
    yc[:, -4:] = 0
    rl, rg = oloss.loss_and_grad(clean, yc, num_classes, alpha=alpha, gamma=gamma, w=w)
    n = max(1, len(pos))
    rg = rg.copy()
    rg[:, -4:] = 0
    lb = 0.0
    if len(pos):
        l, g = loss_and_grad(p2[pos, -4:], y2[pos, -4:], np.asarray(priors)[pos % P], loc_scale, mode)
        rg[pos, -4:] = g * w[2] / n
        lb = l.sum() * w[2] / n
    losses = np.array([rl[0], rl[1], lb])
    return np.append(losses, losses.sum()), rg.reshape(shape)


# ---------------------------------------------------------------- inputs of the GPU cases (test_gpu_iou_loss.py)

B, P = 3, 300          # R = 900: three full 256-row workgroups and one of 132 rows; image boundaries inside workgroups
LOC_SCALE = 0.1
REGIMES = {"sd1.5": 1.5, "sd0.2": 0.2, "sd8": 8.0}  # sd of (pred_loc - y_loc) on assigned rows
# first / last rows of workgroups (0 | 255, 256 | 511, 512 | 767, 768 | 899), last / first rows of images (299 | 300, 599 | 600)
EDGE_ROWS = (0, 255, 256, 299, 300, 511, 512, 599, 600, 767, 768, 899)
N_ASSIGNED, N_IGNORE = 60, 40
# seeds chosen so that every assigned row keeps every decision margin >= MARGIN_MIN (asserted in test_iou_loss_host.py and
# again in test_gpu_iou_loss.py)
CASE_SEEDS = {"sd1.5": 1, "sd0.2": 2, "sd8": 3}


@functools.lru_cache(maxsize=None)
def case_rows(regime):
    """-> (priors f32 [P,4], assigned rows, ignore rows, y_loc f32 [60,4], pred_loc f32 [60,4]): the same for every NC."""
    rng = np.random.default_rng(CASE_SEEDS[regime])
    c = rng.uniform(0.1, 0.9, (P, 2))
    wh = np.exp(rng.uniform(np.log(0.03), np.log(0.9), (P, 2)))
    priors = np.concatenate([c - wh / 2, c + wh / 2], 1).astype(np.float32)  # random well-formed boxes, not a grid
    rest = np.setdiff1d(np.arange(B * P), EDGE_ROWS)
    perm = rng.permutation(rest)
    pos = np.sort(np.concatenate([EDGE_ROWS, perm[:N_ASSIGNED - len(EDGE_ROWS)]]))
    ign = np.sort(perm[N_ASSIGNED - len(EDGE_ROWS):][:N_IGNORE])
    y_loc = rng.normal(0, 1, (len(pos), 4)).astype(np.float32)
    pred_loc = (y_loc + rng.normal(0, REGIMES[regime], (len(pos), 4))).astype(np.float32)
    for a in (priors, pos, ign, y_loc, pred_loc):
        a.setflags(write=False)
    return priors, pos, ign, y_loc, pred_loc


@functools.lru_cache(maxsize=None)
def case(regime, NC):
    """-> (pred f32 [B,P,NC+6], y f32 [B,P,NC+6], priors f32 [P,4]), read-only."""
    priors, pos, ign, y_loc, pred_loc = case_rows(regime)
    rng = np.random.default_rng(1000 + NC)
    R = B * P
    y = np.zeros((R, NC + 6), np.float32)
    y[:, 0] = 1
    y[pos, 0], y[pos, 1] = 0, 1
    y[pos, 2 + rng.integers(0, NC, len(pos))] = 1
    y[pos, -4:] = y_loc
    y[ign] = 0
    pred = rng.normal(0, 1, (R, NC + 6)).astype(np.float32)
    pred[:, 2:2 + NC] += 4 * y[:, 2:2 + NC]
    pred[:, -4:] = rng.normal(0, 1.5, (R, 4))
    pred[pos, -4:] = pred_loc
    pred, y = pred.reshape(B, P, NC + 6), y.reshape(B, P, NC + 6)
    pred.setflags(write=False)
    y.setflags(write=False)
    return pred, y, priors


def case_margins(regime):
    priors, pos, _ign, y_loc, pred_loc = case_rows(regime)
    return margins(pred_loc, y_loc, priors[pos % P], LOC_SCALE)


def case_f32_rowrel(regime, mode):
    """max over the assigned rows of the case of the f32 restatement's row-relative gradient error against f64."""
    priors, pos, _ign, y_loc, pred_loc = case_rows(regime)
    pr = priors[pos % P]
    _l, g64 = loss_and_grad(pred_loc, y_loc, pr, LOC_SCALE, mode)
    _l, g32 = loss_and_grad_f32(pred_loc, y_loc, pr, LOC_SCALE, mode)
    return float(row_rel_err(g32, g64).max())


# Recorded maxima of case_f32_rowrel (torch CPU, rounded up to two digits); test_iou_loss_host.py re-measures them.  The GPU
# test allows 4 x these per row.  They are smaller than the 1.6e-5 .. 1.6e-4 a 200 000-row sample reaches: the maximum over
# 60 rows sits lower in the same distribution, and the bound belongs to the rows that are compared.
F32_ROWREL_MAX = {
    ("sd1.5", "giou"): 1.7e-06,  # measured 1.640e-06
    ("sd1.5", "diou"): 1.9e-06,  # measured 1.807e-06
    ("sd1.5", "ciou"): 1.8e-06,  # measured 1.738e-06
    ("sd0.2", "giou"): 3.0e-06,  # measured 2.942e-06
    ("sd0.2", "diou"): 3.4e-06,  # measured 3.322e-06
    ("sd0.2", "ciou"): 3.4e-06,  # measured 3.382e-06
    ("sd8", "giou"): 7.7e-07,  # measured 7.617e-07
    ("sd8", "diou"): 1.7e-06,  # measured 1.634e-06
    ("sd8", "ciou"): 1.3e-06,  # measured 1.286e-06
}
