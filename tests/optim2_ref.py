"""Restated reference of the optimizer path beyond plain momentum SGD (csrc/optim.hip), in numpy, without a GPU:

  od_grad_stats -> od_optim_prepare -> od_optim_step_multi (OD_OPT_SGD | OD_OPT_NESTEROV | OD_OPT_ADAMW)

As in optim_ref.py: optim.hip is built with -ffp-contract=off, every f32 expression of these kernels is a sequence of
correctly rounded IEEE operations (division and square root included), and numpy float32 arithmetic is the same sequence,
so the GPU tests compare `uint32` views with no tolerance.  The one f64 quantity is the sum of squares; the GPU tests that
compare it bit for bit use inputs whose sum is exact in f64 in any order.

Every function takes `dt` (default float32): test_optim2_ref_host.py runs the same code in float64 against torch.optim,
where the only difference left is f64 rounding.
"""
from __future__ import annotations

import numpy as np

F32 = np.float32
OD_OPT_SGD, OD_OPT_NESTEROV, OD_OPT_ADAMW = 0, 1, 2
KINDS = {"sgd": OD_OPT_SGD, "nesterov": OD_OPT_NESTEROV, "adamw": OD_OPT_ADAMW}


def nesterov_ref(w, m, g, lr, momentum, wd, inv, dt=F32):
    """grad = g*inv + wd*w; mv = momentum*m + grad; m = mv; u = grad + momentum*mv; w = w - lr*u.  -> new (w, m)"""
    for a in (w, m, g):
        assert a.dtype == dt
    lr, momentum, wd, inv = dt(lr), dt(momentum), dt(wd), dt(inv)
    grad = g * inv + wd * w
    mv = momentum * m + grad
    u = grad + momentum * mv
    out = w - lr * u
    assert out.dtype == dt and mv.dtype == dt
    return out, mv


def adamw_ref(w, m, v, g, lr, beta1, beta2, eps, wd, inv, bc1, bc2, dt=F32):
    """gh = g*inv; m = beta1*m + (1-beta1)*gh; v = beta2*v + (1-beta2)*(gh*gh); mh = m/bc1; vh = v/bc2;
    den = sqrt(vh) + eps; u = mh/den; w = w - lr*(u + wd*w).  bc1 / bc2 come from prepare_ref.  -> new (w, m, v)"""
    for a in (w, m, v, g):
        assert a.dtype == dt
    lr, beta1, beta2, eps, wd, inv, bc1, bc2 = (dt(x) for x in (lr, beta1, beta2, eps, wd, inv, bc1, bc2))
    omb1, omb2 = dt(1.0) - beta1, dt(1.0) - beta2
    gh = g * inv
    m1 = beta1 * m + omb1 * gh
    v1 = beta2 * v + omb2 * (gh * gh)
    mh = m1 / bc1
    vh = v1 / bc2
    den = np.sqrt(vh) + eps
    u = mh / den
    out = w - lr * (u + wd * w)
    assert out.dtype == dt and m1.dtype == dt and v1.dtype == dt
    return out, m1, v1


def grad_stats_ref(g):
    """-> (flag, s): flag = 1 when any element is Inf / NaN; s = the f64 sum of the squares of the elements widened to f64
    (numpy's pairwise order: the kernel's equals it exactly only where the sum is exact, and within n * 2**-53 otherwise)."""
    assert g.dtype == F32
    g64 = g.astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        return int(not np.isfinite(g).all()), np.float64(np.sum(g64 * g64))


def new_state():
    """The od_optim_state the host starts from (the fields prepare writes before anything reads them are zero)."""
    return dict(step=0, b1pow=F32(1), b2pow=F32(1), grad_norm=F32(0), clip_coef=F32(0), inv_scale_eff=F32(0), bc1=F32(0),
                bc2=F32(0))


def prepare_ref(state, s, flag, inv_loss_scale, max_grad_norm, beta1, beta2, dt=F32):
    """od_optim_prepare on a state dict (new_state()), the f64 sum of squares `s` and the non-finite flag.  -> new dict."""
    inv, mx, beta1, beta2 = dt(inv_loss_scale), dt(max_grad_norm), dt(beta1), dt(beta2)
    st = dict(state)
    with np.errstate(over="ignore", invalid="ignore"):
        norm_raw = np.sqrt(dt(np.float64(s)))
        st["grad_norm"] = norm_raw * inv
        st["clip_coef"] = np.fmin(dt(1.0), mx / (st["grad_norm"] + dt(1e-6))) if mx > 0 else dt(1.0)
        st["inv_scale_eff"] = inv * st["clip_coef"]
    if flag == 0:
        st["step"] = state["step"] + 1
        st["b1pow"] = dt(state["b1pow"]) * beta1
        st["b2pow"] = dt(state["b2pow"]) * beta2
        st["bc1"] = dt(1.0) - st["b1pow"]
        st["bc2"] = dt(1.0) - st["b2pow"]
    for k, x in st.items():
        assert k == "step" or x.dtype == dt, k
    return st


def step_ref(kind, w, m, v, g, lr, momentum, beta2, eps, wd, st):
    """One segment's od_optim_step_multi with the scalars of the prepared state `st`.  -> new (w, m, v); v passes through
    for the SGD kinds (None there)."""
    import optim_ref
    inv = st["inv_scale_eff"]
    if kind == OD_OPT_SGD:
        return optim_ref.sgd_ref(w, m, g, lr, momentum, wd, inv) + (v,)
    if kind == OD_OPT_NESTEROV:
        return nesterov_ref(w, m, g, lr, momentum, wd, inv) + (v,)
    assert kind == OD_OPT_ADAMW
    return adamw_ref(w, m, v, g, lr, momentum, beta2, eps, wd, inv, st["bc1"], st["bc2"])
