"""Restated reference of the weight average (od_sgd_step_multi_ema / od_ema_update of csrc/optim.hip and
trainer.ema_decay_at), in numpy, without a GPU.

The update is three separately rounded f32 operations, d = w - e; p = omd * d; e = e + p (optim.hip is built with
-ffp-contract=off), which numpy float32 arithmetic reproduces one rounding per operation: the GPU tests compare uint32 views
with no tolerance.  This form, not decay * e + omd * w, is the contract: it leaves e bitwise unchanged where w == e.
With the inputs of optim_ref.values (|x| in [1e-6, 1e3]) no intermediate is subnormal for the omd values the tests use.

test_ema_host.py checks this file itself against float64.
"""
from __future__ import annotations

import numpy as np

F32 = np.float32


def ema_ref(e, w, omd):
    """-> the new average.  e, w: np.float32 arrays; omd = 1 - decay, rounded to f32 as ctypes c_float rounds it."""
    assert e.dtype == F32 and w.dtype == F32
    omd = F32(omd)
    d = w - e
    p = omd * d
    assert d.dtype == F32 and p.dtype == F32
    return e + p


def ema_decay_ref(n, decay, warmup=True):
    """Decay of update number n (the count of optimizer steps attempted before it), in float64: with warm-up
    min(decay, (1 + n) / (10 + n)), else decay."""
    return min(float(decay), (1.0 + n) / (10.0 + n)) if warmup else float(decay)


def omd_ref(n, decay, warmup=True):
    """The kernel argument of update n: 1 - decay in float64, rounded once to f32."""
    return F32(1.0 - ema_decay_ref(n, decay, warmup))
