"""Oracle: detection loss + gradient (reference docs/MODEL.md:33-52), numpy f64 so that it also serves as the
high-precision check of the f32 kernel; tests cross-check it against 60-digit arithmetic and by finite differences.

  objectness: 2-class softmax focal loss, alpha_t = alpha (object) / 1-alpha (background), gamma   [:33-37]
  class:      softmax cross-entropy on assigned priors                                              [:39-44]
  box:        smooth-L1 (beta 1; north_star) or MSE = mean_4 d^2 (reference doc) on assigned priors  [:46-52]
  total = (w_obj*sum_obj + w_cls*sum_cls + w_box*sum_box) / max(1, #assigned)
[BUILD-DEFINED]: alpha 0.25, gamma 2 (RetinaNet paper cited at :37), unit weights, normaliser, all-zero row = ignore.

No term is formed as a difference of nearly equal numbers, so every output keeps f64 relative precision at any logit margin:
  objectness, x = l_other - l_t:  log p_t = -max(x, 0) - log1p(exp(-|x|)),  log(1 - p_t) = min(x, 0) - log1p(exp(-|x|));
    d loss / d log p_t = -a * om^g * (1 - g * p_t * (log p_t / om)), the ratio taken as its limit -1 where om underflows to 0
    (finite for every gamma >= 0, gamma = 0 is plain cross-entropy);  d log p_t / d l_t = om = -d log p_t / d l_other.
  class:  log q_c = (l_c - max) - log1p(sum over c != first argmax of exp(l_c - max));  q_c - 1 = expm1(log q_c).
Non-finite input stays visible (the trainer's skip-step logic depends on it): a non-finite objectness logit of a
non-ignored row, or a non-finite class / box column of an assigned row, makes that row's gradient in those columns and the
loss component NaN (an infinite box loss may stay infinite).  Ignore rows contribute nothing whatever they hold.
"""
from __future__ import annotations

import numpy as np


def loss_and_grad(pred, y, num_classes=20, alpha=0.25, gamma=2.0, box_mode="smooth_l1", w=(1.0, 1.0, 1.0)):
    pred = np.asarray(pred, np.float64)
    y = np.asarray(y, np.float64)
    NC = num_classes
    grad = np.zeros_like(pred)
    t0, t1 = y[..., 0], y[..., 1]
    pos = t1 > 0.5
    active = (t0 + t1) > 0
    n = max(1, int(pos.sum()))
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        # objectness
        x = np.where(pos, pred[..., 0] - pred[..., 1], pred[..., 1] - pred[..., 0])  # l_other - l_t
        nf = x * 0.0  # 0, or NaN where a logit is not finite
        lg = np.log1p(np.exp(-np.abs(x)))
        lpt = -np.maximum(x, 0.0) - lg
        pt = np.exp(lpt)
        om = np.exp(np.minimum(x, 0.0) - lg)
        a = np.where(pos, alpha, 1 - alpha)
        mod = om ** gamma  # 0 ** 0 = 1
        ratio = np.where(om > 0, lpt / np.where(om > 0, om, 1.0), -1.0)
        l_obj = np.where(active, -a * mod * lpt + nf, 0.0)
        gt = -a * mod * (1.0 - gamma * pt * ratio) * om + nf  # d loss / d l_t = -(d loss / d l_other)
        g1 = np.where(pos, gt, -gt)
        grad[..., 0] = np.where(active, -g1, 0.0) * w[0] / n
        grad[..., 1] = np.where(active, g1, 0.0) * w[0] / n
        # class
        cl = pred[..., 2:2 + NC]
        imax = np.argmax(np.where(np.isnan(cl), -np.inf, cl), -1)[..., None]  # first maximum
        mx = np.take_along_axis(cl, imax, -1)
        ex = np.exp(cl - mx)
        np.put_along_axis(ex, imax, 0.0, -1)
        nfc = (mx + cl.min(-1, keepdims=True)) * 0.0
        lq = (cl - mx) - (np.log1p(ex.sum(-1, keepdims=True)) + nfc)
        tc = y[..., 2:2 + NC]
        l_cls = np.where(pos, -(tc * lq).sum(-1), 0.0)
        gq = np.where(tc == 1.0, np.expm1(lq), np.exp(lq) - tc)
        grad[..., 2:2 + NC] = np.where(pos[..., None], gq, 0.0) * w[1] / n
        # box
        d = pred[..., -4:] - y[..., -4:]
        if box_mode == "smooth_l1":
            ad = np.abs(d)
            lb = np.where(ad < 1, 0.5 * d * d, ad - 0.5)
            gb = np.where(ad < 1, d, np.sign(d))
        else:
            lb = 0.25 * d * d
            gb = 0.5 * d
        l_box = np.where(pos, lb.sum(-1), 0.0)
        grad[..., -4:] = np.where(pos[..., None], gb + d * 0.0, 0.0) * w[2] / n
    losses = np.array([l_obj.sum() * w[0] / n, l_cls.sum() * w[1] / n, l_box.sum() * w[2] / n])
    return np.append(losses, losses.sum()), grad
