"""Restated reference of the weight-update path (csrc/optim.hip; the re-pack and the casts: csrc/train.hip), in numpy,
without a GPU:

  od_grad_nonfinite -> od_sgd_step[_multi] -> od_copy_if_nonzero -> od_pack_weights[_multi] -> host loss-scale control

Both files are compiled with -ffp-contract=off, so every f32 expression of these kernels is a sequence of correctly rounded
IEEE operations.  numpy `float32` arithmetic is the same sequence, one rounding per operation, so the GPU tests compare
results as integer views (`uint32` / `uint16`) with no tolerance; signed zeros count.

Input magnitudes: the callers keep |values| in [1e-6, 1e3] and lr <= 0.1, so that no input, intermediate or result is
subnormal in f32 (a flush-to-zero mode of either side would otherwise show as a bit difference that is no arithmetic
error).  `values()` draws such numbers: a random sign times 10 ** uniform(lo, hi).

test_optim_ref_host.py checks this file itself: `sgd_ref` against torch.optim.SGD in float64, `bf16_ref` against torch's
CPU cast, `pack_ref` against a plain triple loop.
"""
from __future__ import annotations

import numpy as np

F32 = np.float32
F16_NAN = 0x7e00  # the fill of the pack tests: an f16 quiet NaN no conversion of a finite weight produces


def values(rng, n, lo=-6.0, hi=3.0):
    """n f32 values, random sign, magnitude 10 ** uniform(lo, hi): none is zero or subnormal."""
    mag = 10.0 ** rng.uniform(lo, hi, n)
    return (mag * rng.choice([-1.0, 1.0], n)).astype(F32)


def sgd_ref(w, m, g, lr, momentum, wd, inv):
    """`sgd_update` of csrc/optim.hip: grad = g*inv + wd*w; mv = momentum*m + grad; m = mv; w = w - lr*mv, each operation
    rounded once to f32.  Arrays and scalars are np.float32 (the scalars as ctypes c_float rounds them).  -> new (w, m)."""
    for a in (w, m, g):
        assert a.dtype == F32
    lr, momentum, wd, inv = F32(lr), F32(momentum), F32(wd), F32(inv)
    grad = g * inv + wd * w
    mv = momentum * m + grad
    assert grad.dtype == F32 and mv.dtype == F32
    return w - lr * mv, mv


def pack_dims(Cout, Cin, k):
    """(cout_pad, kpad, cin_pad, kpad_t) of the forward [cout_pad][kpad] and backward-data [cin_pad][kpad_t] packs: rows in
    whole 256-channel pads, columns in whole 64-element pads (od_conv_weight_dims)."""
    up = lambda a, b: (a + b - 1) // b * b
    return up(Cout, 256), up(k * k * Cin, 64), up(Cin, 256), up(k * k * Cout, 64)


def pack_ref(w_master, Cout, Cin, k, cout_pad, kpad, cin_pad, kpad_t, fill):
    """f32 masters [Cout, k*k*Cin] (column = tap*Cin + ci) -> (wf [cout_pad, kpad], wt [cin_pad, kpad_t]) as uint16 views of
    f16: wf[co][tap*Cin + ci] = f16(w[co][tap*Cin + ci]); wt[ci][(k*k-1-tap)*Cout + co] the same value (taps flipped,
    channels swapped).  Every other element keeps `fill`."""
    taps = k * k
    w16 = np.asarray(w_master, F32).reshape(Cout, taps, Cin).astype(np.float16).view(np.uint16)
    wf = np.full((cout_pad, kpad), fill, np.uint16)
    wt = np.full((cin_pad, kpad_t), fill, np.uint16)
    wf[:Cout, :taps * Cin] = w16.reshape(Cout, taps * Cin)
    # wt[ci][(taps-1-tap)][co] = w16[co][tap][ci]
    wt[:Cin, :taps * Cout] = w16[:, ::-1, :].transpose(2, 1, 0).reshape(Cin, taps * Cout)
    return wf, wt


def add_f16_ref(a, b):
    """od_add_f16: f16(f32(a) + f32(b))"""
    assert a.dtype == np.float16 and b.dtype == np.float16
    with np.errstate(over="ignore", invalid="ignore"):
        return (a.astype(F32) + b.astype(F32)).astype(np.float16)


def down2_ref(d, base=None):
    """od_down2_sum_add: d f16 [B, 2*Hh, 2*Wh, C] -> f16 [B, Hh, Wh, C].  f32 accumulation in the kernel's order (base first
    when given, then the 2x2 block as (0,0), (0,1), (1,0), (1,1)), then one rounding to f16."""
    assert d.dtype == np.float16
    d32 = d.astype(F32)
    acc = np.zeros((d.shape[0], d.shape[1] // 2, d.shape[2] // 2, d.shape[3]), F32) if base is None else base.astype(F32)
    with np.errstate(over="ignore", invalid="ignore"):
        for dy, dx in ((0, 0), (0, 1), (1, 0), (1, 1)):
            acc = acc + d32[:, dy::2, dx::2, :]
        return acc.astype(np.float16)


def bf16_ref(x):
    """f32 -> bf16 bit patterns (uint16): round to nearest even on the bit pattern; NaN stays NaN with the quiet bit set."""
    u = np.ascontiguousarray(x, F32).view(np.uint32).astype(np.uint64)
    nan = (u & 0x7fffffff) > 0x7f800000
    r = (u + 0x7fff + ((u >> 16) & 1)) >> 16
    return np.where(nan, (u >> 16) | 0x40, r).astype(np.uint16)


def bf16_widen_ref(b):
    """bf16 bit patterns (uint16) -> f32: the pattern in the high half, zeros below."""
    return (np.ascontiguousarray(b, np.uint16).astype(np.uint32) << 16).view(F32)


def lr_mult_ref(name):
    """Per-layer learning-rate multiplier of docs/MODEL.md:84-90: the base network at 1/100, the layers shared by the three
    pyramid levels at 1 / (times shared), everything else at the full rate."""
    if name.startswith("b."):
        return 0.01
    if name.startswith("h."):
        return 1.0 / 3.0
    return 1.0


def loss_scale_ref(flags, lag, scale0, interval, dynamic=True, steps=None):
    """The host loss-scale control as a function of the non-finite flags alone.  -> for every step i in range(steps)
    (default len(flags)) the (loss_scale, skipped_steps, good_steps, consecutive_skips) that step i STARTS with: the flags
    of steps 0 .. i - lag have been applied, in order, and no other.  Each entry is computed from scratch, without a queue.

    The rule: a non-zero flag (any value) counts one skipped step and one more consecutive skip, forgets the clean steps
    counted so far and halves the scale, never below 1; a zero flag ends the consecutive skips and counts one clean step,
    and when `interval` of them have come in a row the scale doubles, never above 65536, and the count starts again.
    dynamic=False: the scale stays, skipped_steps and consecutive_skips move as before, and good_steps counts the clean
    flags since the last bad one without starting again (nothing doubles).  steps > len(flags): the run goes on with no new flags, so entry
    len(flags) + lag - 1 has every flag applied (what a drain at the end of the run leaves)."""
    flags = [int(f) for f in flags]
    out = []
    for i in range(len(flags) if steps is None else steps):
        scale, skipped, good, consecutive = float(scale0), 0, 0, 0
        for f in flags[:max(0, i - lag + 1)]:
            if f != 0:
                skipped, consecutive, good = skipped + 1, consecutive + 1, 0
                if dynamic and scale > 1.0:
                    scale = max(scale / 2.0, 1.0)
            else:
                consecutive, good = 0, good + 1
                if dynamic and good == interval:
                    good = 0
                    if scale < 65536.0:
                        scale = min(scale * 2.0, 65536.0)
        out.append((scale, skipped, good, consecutive))
    return out
