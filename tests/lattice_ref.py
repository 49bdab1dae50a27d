"""Exact-arithmetic ("lattice") inputs and references for the convolution kernels.

Why: with Gaussian f16 data the f32 accumulation order of a kernel is visible in the result, so a test needs a tolerance,
and that tolerance hides dropped pixels, a wrong rounding mode or a second rounding.  Here the inputs are chosen so that
f32 accumulation is EXACT: activations and weights are small integers (or multiples of one power of two), scales are
powers of two, biases and residuals are dyadic.  Every partial sum is then an integer multiple of a fixed quantum below
2^24 quanta, so the f32 result is the same in any summation order, any split-K / slab / atomic schedule and with or
without FMA contraction; it equals the float64 reference exactly, and an f16 output must equal ref.astype(float16) bit
for bit.

This module is the generator and the reference only (numpy / torch-CPU; nothing here needs the library).  The reference
functions ASSERT the conditions that make the claim above true, on the reference alone, before any device result is
looked at:
  1. sum|a||b| / quantum < 2^24 for every accumulation (a-priori bound n_terms * max|a| * max|b|; when that is too
     coarse, the convolution of the absolute values);
  2. the float32 epilogue, evaluated in the kernel's op order, equals the float64 one on every element
     (ELU: on the elements with a positive pre-activation; slope 0.1: see below);
  3. |v| < 65504 unless the case is meant to overflow;
  4. f16 outputs with K >= 576: >= 50 % of the elements are not representable in f16 and >= 1 % are exact ties, so
     the case cannot quietly lose its rounding content.

LeakyReLU slope 0.1 (the product's value) is not dyadic: v * 0.1f is ONE IEEE f32 multiply, which numpy float32
reproduces, so for those (single-layer) cases the float32 evaluation IS the reference and condition 2 does not apply.
ELU's negative branch goes through od_expm1_fast (1e-6 relative) followed by one f16 rounding: such an element must be
f16(ref) or one of its two f16 neighbours (1e-6 << 2^-11: a bound from the formats, not a measurement).  So that a
residual cannot cancel the ELU value and amplify that 1e-6, ELU cases draw their residual from the even integers.
"""
from __future__ import annotations

import types
import zlib

import numpy as np
import torch
import torch.nn.functional as F

LIM = float(2 ** 24)
F16_MAX = 65504.0
F16_NAN_BITS = 0x7E00     # poison of the f16 input guards
U8_POISON = 255           # poison of the u8 input guards
SENTINEL = 0xA5           # byte the output allocations are filled with (f16 -0.02205, f32 -2.9e-16: off every lattice)
GUARD_BYTES = 4096
SLOPE = 0.125             # the dyadic leaky slope of the lattice cases


def seed_of(*key) -> int:
    """A seed that depends on the case only (not on PYTHONHASHSEED): the CPU test checks the tensors the GPU test runs."""
    return zlib.crc32(repr(key).encode())


def out_hw(H, W, stride):
    return (H + stride - 1) // stride, (W + stride - 1) // stride


def quantum_of(a) -> float:
    """Largest power of two q <= 1 such that every element of a is an integer multiple of q."""
    a = np.asarray(a, np.float64)
    for n in range(0, 26):
        q = 2.0 ** -n
        if np.array_equal(np.round(a / q) * q, a):
            return q
    raise AssertionError("not on a dyadic lattice of 2^-25 or coarser")


# ------------------------------------------------------------------------------------------------ convolutions (CPU)
def _nchw(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).permute(0, 3, 1, 2)


def _conv_dtype(work, exact_in_f32):
    # float64 unless the case is large AND condition 1 has shown that a float32 sum is exact in any order
    return torch.float32 if (exact_in_f32 and work > 4e9) else torch.float64


def conv_nhwc(x, w, stride, dtype=torch.float64):
    """x [B,H,W,Cin], w [Cout,k,k,Cin] -> float64 [B,Ho,Wo,Cout], 'same' padding (k // 2)."""
    k = w.shape[1]
    y = F.conv2d(_nchw(x, dtype), _nchw(w, dtype), stride=stride, padding=k // 2)
    return y.permute(0, 2, 3, 1).contiguous().numpy().astype(np.float64)


def conv_int64(x, w, stride):
    """The same convolution by direct integer arithmetic (int64, tap by tap): the check of conv_nhwc on small cases.
    x and w must hold integers."""
    xi, wi = np.asarray(x).astype(np.int64), np.asarray(w).astype(np.int64)
    assert np.array_equal(xi, np.asarray(x, np.float64)) and np.array_equal(wi, np.asarray(w, np.float64))
    B, H, W, Cin = xi.shape
    Cout, k = wi.shape[0], wi.shape[1]
    p = k // 2
    Ho, Wo = out_hw(H, W, stride)
    xp = np.zeros((B, H + 2 * p + stride, W + 2 * p + stride, Cin), np.int64)
    xp[:, p:p + H, p:p + W] = xi
    out = np.zeros((B, Ho, Wo, Cout), np.int64)
    for dy in range(k):
        for dx in range(k):
            win = xp[:, dy:dy + (Ho - 1) * stride + 1:stride, dx:dx + (Wo - 1) * stride + 1:stride]
            out += win @ wi[:, dy, dx, :].T
    return out


def _check_accumulation(a, b, n_terms, what, absconv=None):
    """Condition 1.  a, b: the two operand tensors of an accumulation of n_terms products per output element."""
    qa, qb = quantum_of(a), quantum_of(b)
    bound = n_terms * float(np.abs(a).max()) * float(np.abs(b).max()) / (qa * qb)
    if bound >= LIM and absconv is not None:
        bound = float(absconv().max()) / (qa * qb)
    assert bound < LIM, f"{what}: sum|a||b| / quantum = {bound:.3g} >= 2^24: f32 accumulation is not exact"
    return bound


# ------------------------------------------------------------------------------------------------ epilogue
def _act64(v, act, alpha):
    if act == "leaky":
        return np.where(v > 0, v, v * np.float64(np.float32(alpha)))
    if act == "elu":
        return np.where(v > 0, v, alpha * np.expm1(np.minimum(v, 0)))
    return v


def _act32(v, act, alpha):
    a = np.float32(alpha)
    if act == "leaky":
        return np.maximum(v, v * a)                  # od_leaky: fmaxf(v, v * alpha)
    if act == "elu":
        return np.where(v > 0, v, a * np.expm1(np.minimum(v, np.float32(0)))).astype(np.float32)
    return v


def _up2(r):
    return np.repeat(np.repeat(r, 2, axis=1), 2, axis=2)


def rounding_content(v):
    """(fraction of v not representable in f16, fraction that are exact ties between two f16 values)."""
    v = np.asarray(v, np.float64)
    with np.errstate(over="ignore"):
        r16 = v.astype(np.float16)
    r = r16.astype(np.float64)
    inexact = r != v
    with np.errstate(over="ignore", invalid="ignore"):
        other = np.nextafter(r16, np.where(v > r, np.inf, -np.inf).astype(np.float16)).astype(np.float64)
        tie = inexact & np.isfinite(other) & (np.abs(v - r) == np.abs(other - v))
    return float(inexact.mean()), float(tie.mean())


def epilogue(acc, scale, bias, act=None, alpha=0.0, res=None, up2=False, out_f32=False, overflow=False, K=0,
             what="epilogue", rounding=True):
    """acc float64 (exact) -> the reference of  act(acc * scale + bias) (+ res), with conditions 2-4 asserted.
    Returns a namespace: v (float64, or the float32 evaluation for a non-dyadic slope), pre (the pre-activation),
    ref16 / ref32 (the expected stored tensor), act."""
    scale, bias = np.asarray(scale, np.float32), np.asarray(bias, np.float32)
    a32 = acc.astype(np.float32)
    assert np.array_equal(a32.astype(np.float64), acc), f"{what}: accumulator not exact in f32"
    pre64 = acc * scale.astype(np.float64) + bias.astype(np.float64)
    prod32 = a32 * scale
    assert np.array_equal(prod32.astype(np.float64), acc * scale.astype(np.float64)), \
        f"{what}: acc * scale is not exact in f32 (an FMA would then differ from mul + add)"
    pre32 = prod32 + bias
    v64, v32 = _act64(pre64, act, alpha), _act32(pre32, act, alpha)
    if res is not None:
        r = _up2(res) if up2 else res
        v64 = v64 + r.astype(np.float64)
        v32 = v32 + r.astype(np.float32)
    dyadic_slope = act != "leaky" or quantum_ok(alpha)
    if act == "elu":
        sel = pre64 > 0
        assert np.array_equal(v32[sel].astype(np.float64), v64[sel]), f"{what}: f32 epilogue != f64 epilogue"
        v = v64
    elif dyadic_slope:
        assert np.array_equal(v32.astype(np.float64), v64), f"{what}: f32 epilogue != f64 epilogue"
        v = v64
    else:
        assert np.array_equal(pre32.astype(np.float64), pre64), f"{what}: f32 pre-activation != f64"
        v = v32.astype(np.float64)   # one IEEE multiply (+ one add): the f32 op order is the definition
    finite = np.abs(v) < F16_MAX
    if overflow:
        assert not finite.all(), f"{what}: the case is meant to overflow and does not"
    else:
        assert finite.all(), f"{what}: |v| reaches {np.abs(v).max()}"
    with np.errstate(over="ignore"):
        ref16 = v.astype(np.float16)
    if rounding and not out_f32 and K >= 576 and not overflow:
        # ELU: counted over the elements that are compared for equality (a saturated negative branch is -1 + integer)
        inexact, ties = rounding_content(v[pre64 > 0] if act == "elu" else v)
        assert inexact >= 0.5 and ties >= 0.01, f"{what}: only {inexact:.1%} inexact / {ties:.2%} ties in f16"
    return types.SimpleNamespace(v=v, pre=pre64, ref16=ref16, ref32=v.astype(np.float32), act=act)


def quantum_ok(alpha) -> bool:
    """True when alpha is a power of two (times a small integer): a multiply by it is exact on the lattice."""
    a = float(np.float32(alpha))
    return a == 0.0 or (a * 1024.0).is_integer()


# ------------------------------------------------------------------------------------------------ generators
def _ints(rng, amp, shape):
    return rng.integers(-amp, amp + 1, shape)


def amp_for_integer_output(K, sigma=7000.0):
    """Amplitude a of x and w for a layer whose output is the bare integer sum (scale 1): that integer must pass 2048 on
    most elements to be rounded at all by the f16 store, and stay below 65504.  Uniform integers in [-a, a] have variance
    a (a + 1) / 3, so the sum of K products has a standard deviation of sqrt(K) a (a + 1) / 3; it is aimed at 7000
    (6 sigma = 42000)."""
    return max(1, int(round((3.0 * sigma / K ** 0.5) ** 0.5)))


def gen_first_grad(key, B, H, W):
    """u8 image and dz [B,H,W,32] in [-3, 3] for the first layer's weight gradient: the widest image range of
    (255, 63, 15, 3) -- at training size {0, 1} with dz in [-1, 1] -- whose B*H*W-term sums, plus the dw they are
    accumulated into, stay below 2^24 quanta."""
    rng = np.random.default_rng(seed_of("first_grad", key))
    n = B * H * W
    xmax, amp = next((m, a) for m, a in ((255, 3), (63, 3), (15, 3), (3, 3), (1, 1)) if n * m * a + 4096 * 256 < LIM / 2)
    g = types.SimpleNamespace()
    g.x = rng.integers(0, xmax + 1, (B, H, W, 3)).astype(np.uint8)
    g.dz = _ints(rng, amp, (B, H, W, 32)).astype(np.float16)
    g.dw0 = rng.integers(-4096, 4097, (32, 27)).astype(np.float32)
    return g


def gen_conv(key, B, H, W, Cin, Cout, k, stride=1, res_mode="none", act=None, amp=8, Cout2=0, lift=False, integer=False):
    """Lattice tensors of one fused conv layer: x f16 and w f32 integers in [-amp, amp]; scale in {1, 1/2, 1/4}; bias a
    multiple of 2^-7 in [-8, 8]; residual a multiple of 2^-3 in [-256, 256] (ELU: an even integer).  Cout2 > 0 adds the
    consuming 1x1 layer (w2 integers in [-2, 2], scale2 in {2^-6, 2^-5}, bias2 a multiple of 2^-5).
    integer: the recipe for a layer whose f16 output is the operand of a second accumulation -- scale in {1, 2}, integer
    bias and residual.  The output is then an integer of up to ~14 bits (rounded to f16's 11: plenty of inexact values and
    ties) whose f16 rounding is a multiple of 1/8 (1/8: the leaky slope on the negative side), which keeps the SECOND sum
    below 2^24 quanta; the fractional recipe would leave a quantum of 2^-10 under values of a few thousand."""
    rng = np.random.default_rng(seed_of("conv", key))
    g = types.SimpleNamespace()
    g.x = _ints(rng, amp, (B, H, W, Cin)).astype(np.float16)
    g.w = _ints(rng, amp, (Cout, k, k, Cin)).astype(np.float32)
    g.scale = (2.0 ** -rng.integers(0, 3, Cout)).astype(np.float32)
    g.bias = (rng.integers(-1024, 1025, Cout) / 128.0).astype(np.float32)
    if integer:
        g.scale = (2.0 ** rng.integers(0, 2, Cout)).astype(np.float32)
        g.bias = rng.integers(-8, 9, Cout).astype(np.float32)
    Ho, Wo = out_hw(H, W, stride)
    g.res = None
    if res_mode != "none":
        shp = (B, Ho, Wo, Cout) if res_mode == "same" else (B, Ho // 2, Wo // 2, Cout)
        if act == "elu" or integer:
            g.res = (2 * rng.integers(-128, 129, shp)).astype(np.float16)
        else:
            g.res = (rng.integers(-2048, 2049, shp) / 8.0).astype(np.float16)
    if lift:
        # an ELU layer whose output feeds a second layer on the lattice: an INTEGER bias that keeps every pre-activation
        # positive (ELU's identity branch), so the first output is exact and integer-spaced wherever it is >= 1/4
        top = np.abs(conv_nhwc(g.x, g.w, stride)).max((0, 1, 2)) * g.scale
        g.bias = (np.ceil(top) + 1.0 + np.abs(np.round(g.bias))).astype(np.float32)
    if Cout2:
        g.w2 = _ints(rng, 2, (Cout2, 1, 1, Cout)).astype(np.float32)
        g.scale2 = (2.0 ** -rng.integers(5, 7, Cout2)).astype(np.float32)
        g.bias2 = (rng.integers(-256, 257, Cout2) / 32.0).astype(np.float32)
    return g


def gen_bneck(key, B, H, W, C, act):
    """The chained recipe of the fused residual block: x, w1, w3 in [-4, 4]; s1 in {1/8, 1/4}; b1 a multiple of 2^-4;
    s3 in {1/16, 1/8, 1/4}; b3 a multiple of 2^-5.  ELU: b1 lifts every first-layer pre-activation above zero, so the
    middle tensor (which never leaves the chip) stays exact and only the OUTPUT has ELU's negative branch."""
    rng = np.random.default_rng(seed_of("bneck", key))
    g = types.SimpleNamespace()
    g.x = _ints(rng, 4, (B, H, W, C)).astype(np.float16)
    g.w1 = _ints(rng, 4, (C // 2, 1, 1, C)).astype(np.float32)
    g.w3 = _ints(rng, 4, (C, 3, 3, C // 2)).astype(np.float32)
    g.s1 = (2.0 ** -rng.integers(2, 4, C // 2)).astype(np.float32)
    g.b1 = (rng.integers(-64, 65, C // 2) / 16.0).astype(np.float32)
    g.s3 = (2.0 ** -rng.integers(2, 5, C)).astype(np.float32)
    g.b3 = (rng.integers(-256, 257, C) / 32.0).astype(np.float32)
    if act == "elu":
        lift = np.abs(conv_nhwc(g.x, g.w1, 1)).max((0, 1, 2)) * g.s1
        g.b1 = (np.ceil(lift) + 1.0 + np.abs(g.b1)).astype(np.float32)
    return g


def gen_stem(key, B, H, W, act):
    """u8 image (full range) -> conv 3 -> 32 -> stride-2 conv 32 -> 64.  w0, w3 in [-4, 4]; s0 = 2^-9 (the image
    normalisation folded into a power of two); b0 a multiple of 2^-4; s3 in {1/8, 1/4}; b3 a multiple of 2^-5.  ELU as in
    gen_bneck: b0 keeps the first layer positive."""
    rng = np.random.default_rng(seed_of("stem", key))
    g = types.SimpleNamespace()
    g.x = rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)
    g.w0 = _ints(rng, 4, (32, 3, 3, 3)).astype(np.float32)
    g.w3 = _ints(rng, 4, (64, 3, 3, 32)).astype(np.float32)
    g.s0 = np.full(32, 2.0 ** -9, np.float32)
    g.b0 = (rng.integers(-32, 33, 32) / 16.0).astype(np.float32)
    g.s3 = (2.0 ** -rng.integers(2, 4, 64)).astype(np.float32)
    g.b3 = (rng.integers(-256, 257, 64) / 32.0).astype(np.float32)
    if act == "elu":
        lift = np.abs(conv_nhwc(g.x, g.w0, 1)).max((0, 1, 2)) * g.s0
        g.b0 = (np.ceil(lift) + 1.0 + np.abs(g.b0)).astype(np.float32)
    return g


def gen_grad(key, B, H, W, Cin, Cout, k, stride, amp=3, bwd_data=False):
    """x [B,H,W,Cin] and dz [B,Ho,Wo,Cout] integers in [-amp, amp] (f16) and a master weight w [Cout,k,k,Cin] in [-8, 8].
    bwd_data: the tensors of a backward-data case instead.  dx is the bare sum (identity epilogue), so it must pass 2048 on
    most elements to be rounded at all: w in [-a, a] and dz HALF-integers in [-a, a] with a = amp_for_integer_output of the
    terms per dx element, k*k*Cout / stride^2 (stride 2: the four parity classes of dx have 1, 2, 2 and 4 taps of the nine, so
    their standard deviations are 0.67 .. 1.33 of the 7000 aimed at; 7 sigma of the widest is still below 65504)."""
    rng = np.random.default_rng(seed_of("grad", key))
    Ho, Wo = out_hw(H, W, stride)
    g = types.SimpleNamespace()
    g.x = _ints(rng, amp, (B, H, W, Cin)).astype(np.float16)
    g.dz = _ints(rng, amp, (B, Ho, Wo, Cout)).astype(np.float16)
    g.w = _ints(rng, 8, (Cout, k, k, Cin)).astype(np.float32)
    if bwd_data:
        a = amp_for_integer_output(k * k * Cout / (stride * stride))
        g.dz = (_ints(rng, 2 * a, (B, Ho, Wo, Cout)) / 2.0).astype(np.float16)
        g.w = _ints(rng, a, (Cout, k, k, Cin)).astype(np.float32)
    g.acc = (rng.integers(-2048, 2049, (B, H, W, Cin)) / 8.0).astype(np.float16)      # an existing dx to accumulate into
    g.dw0 = rng.integers(-4096, 4097, (Cout, k * k * Cin)).astype(np.float32)         # an existing dw to accumulate into
    return g


# ------------------------------------------------------------------------------------------------ references
def ref_forward(x, w, scale, bias, stride=1, act=None, alpha=0.0, res=None, up2=False, out_f32=False, overflow=False,
                what="forward", rounding=True):
    """One fused conv layer.  x may be f16 on any dyadic lattice (the f16 output of a previous layer), w integers."""
    k, Cin = w.shape[1], w.shape[3]
    K = k * k * Cin
    _check_accumulation(x, w, K, what, lambda: conv_nhwc(np.abs(x), np.abs(w), stride))
    B, H, W, _ = x.shape
    acc = conv_nhwc(x, w, stride, _conv_dtype(2.0 * B * H * W * K * w.shape[0] / (stride * stride), True))
    return epilogue(acc, scale, bias, act, alpha, res, up2, out_f32, overflow, K, what, rounding)


def ref_forward_pw(g, stride, act, alpha, res_mode, act2, alpha2, what="forward + 1x1"):
    """The layer of gen_conv(..., Cout2) and the 1x1 layer that consumes its rounded f16 output -> (ref of out, ref of out2)."""
    r1 = ref_forward(g.x, g.w, g.scale, g.bias, stride, act, alpha, g.res, res_mode == "up2", what=what + " [1]")
    r2 = ref_forward(r1.ref16, g.w2, g.scale2, g.bias2, 1, act2, alpha2, what=what + " [2]")
    return r1, r2


def ref_bneck(g, act, alpha, what="bottleneck"):
    """out = x + act(s3 * conv3x3(f16(act(s1 * conv1x1(x) + b1))) + b3): one rounding of the middle tensor, one of the output."""
    r1 = ref_forward(g.x, g.w1, g.s1, g.b1, 1, act, alpha, what=what + " [1x1]")
    if act == "elu":
        assert (r1.pre > 0).all(), f"{what}: the first layer must stay on ELU's identity branch"
    return ref_forward(r1.ref16, g.w3, g.s3, g.b3, 1, act, alpha, res=g.x, what=what + " [3x3]")


def ref_conv_first(x_u8, w0, s0, b0, act, alpha, what="first layer"):
    return ref_forward(x_u8.astype(np.float32), w0, s0, b0, 1, act, alpha, what=what)


def ref_stem(g, act, alpha, what="stem"):
    r1 = ref_conv_first(g.x, g.w0, g.s0, g.b0, act, alpha, what + " [3->32]")
    if act == "elu":
        assert (r1.pre > 0).all(), f"{what}: the first layer must stay on ELU's identity branch"
    return ref_forward(r1.ref16, g.w3, g.s3, g.b3, 2, act, alpha, what=what + " [32->64 s2]")


def ref_bwd_data(dz, w, x_shape, stride, acc=None, overflow=False, what="backward-data", both=False, rounding=True):
    """dx = conv^T(dz, w) (+ acc): w [Cout,k,k,Cin] is the FORWARD master weight.  Stride 2 is the transposed form.
    both: -> (reference without acc, reference with acc) from one transposed convolution."""
    Cout, k, _, Cin = w.shape
    _check_accumulation(dz, w, k * k * Cout, what)
    B, H, W, _ = x_shape
    dt = _conv_dtype(2.0 * B * H * W * k * k * Cin * Cout / (stride * stride), True)
    dx = torch.nn.grad.conv2d_input((B, Cin, H, W), _nchw(w, dt), _nchw(dz, dt), stride=stride, padding=k // 2)
    dx = dx.permute(0, 2, 3, 1).contiguous().numpy().astype(np.float64)
    one, zero = np.ones(Cin, np.float32), np.zeros(Cin, np.float32)
    K = k * k * Cout  # condition 4 applies to the plain dx and to dx + acc alike
    if both:
        return (epilogue(dx, one, zero, overflow=overflow, K=K, what=what, rounding=rounding),
                epilogue(dx, one, zero, res=acc, overflow=overflow, K=K, what=what + " + acc", rounding=rounding))
    return epilogue(dx, one, zero, None, 0.0, acc, False, False, overflow, K, what, rounding)


def ref_bwd_weight(x, dz, k, stride, dw0=None, in_scale=1.0, what="weight gradient"):
    """dw [Cout, k*k*Cin] = in_scale * sum over pixels of dz^T . shifted(x) (+ dw0), as float32 holding exact values."""
    B, H, W, Cin = x.shape
    Ho, Wo, Cout = dz.shape[1], dz.shape[2], dz.shape[3]
    n = B * Ho * Wo
    bound = _check_accumulation(x, dz, n, what)
    dt = _conv_dtype(2.0 * n * k * k * Cin * Cout, True)
    dw = torch.nn.grad.conv2d_weight(_nchw(x, dt), (Cout, Cin, k, k), _nchw(dz, dt), stride=stride, padding=k // 2)
    dw = dw.permute(0, 2, 3, 1).reshape(Cout, k * k * Cin).numpy().astype(np.float64)
    assert np.array_equal(np.round(dw), dw)
    assert float(np.float32(in_scale)) == in_scale and np.log2(in_scale).is_integer(), "in_scale must be a power of two"
    dw = dw * in_scale
    if dw0 is not None:
        q = min(quantum_of(dw0), in_scale)
        assert (bound * in_scale + float(np.abs(dw0).max())) / q < LIM, f"{what}: dw0 + dw leaves the exact range"
        dw = dw + dw0.astype(np.float64)
    out = dw.astype(np.float32)
    assert np.array_equal(out.astype(np.float64), dw)
    return out


def ref_bn_sums(z16, what="bn_partials"):
    """(sum z, sum z^2) per channel of the STORED f16 z, exact, as float32; asserts that any f32 summation order is exact."""
    z = z16.astype(np.float64).reshape(-1, z16.shape[-1])
    q = quantum_of(z)
    assert float(np.abs(z).sum(0).max()) / q < LIM, f"{what}: sum|z| leaves the exact f32 range"
    assert float((z * z).sum(0).max()) / (q * q) < LIM, f"{what}: sum z^2 leaves the exact f32 range"
    assert float((z * z).max()) / (q * q) < LIM
    return z.sum(0).astype(np.float32), (z * z).sum(0).astype(np.float32)


BN_TILE_MAX = 256  # pixels of the largest m-tile of any conv kernel (the 8-wave kernel's BM): one bn_partials row sums at most that many


def gen_bn(key, B, H, W, Cin, Cout, k, stride, per_row=False):
    """x, w for the raw (identity-epilogue) training forward whose epilogue also sums z and z^2.
    Default: the largest amplitude of (4, 2, 1) for which the sums over the WHOLE tensor stay exact in f32, so that
    od_bn_stats_from_partials' own row sum is exact too (small maps).
    per_row: only every partial ROW must be exact -- a row covers one m-tile of at most BN_TILE_MAX pixels, so |z| < 256
    keeps sum z and sum z^2 of a row below 2^24 in any order; the rows are then added in float64 on the host, exactly, at
    any pixel count (the training shards).  Amplitudes (2, 1), then x thinned to every 4th element.
    Condition 4 cannot hold with an exact sum of z^2 and is waived (rounding=False in the caller): a z that needs more than
    f16's 11 bits has a z^2 of more than 22, and 128 or more of them need more than 24.  gen_bn_rounded covers sum z of a
    ROUNDED z."""
    tries = ((2, 1), (1, 1), (1, 4)) if per_row else ((4, 1), (2, 1), (1, 1))
    work = 2.0 * B * H * W * k * k * Cin * Cout / (stride * stride)
    for amp, thin in tries:
        g = gen_conv(("bn", key, amp, thin), B, H, W, Cin, Cout, k, stride, amp=amp)
        if thin > 1:
            keep = np.random.default_rng(seed_of("bn thin", key)).integers(0, thin, g.x.shape) == 0
            g.x = (g.x * keep).astype(np.float16)
        g.scale, g.bias = np.ones(Cout, np.float32), np.zeros(Cout, np.float32)
        z = conv_nhwc(g.x, g.w, stride, _conv_dtype(work, True)).reshape(-1, Cout)  # integers far below 2^24: f32 is exact
        if per_row:
            if np.abs(z).max() < 256:
                return g
        elif np.abs(z).max() < 2048 and (z * z).sum(0).max() < LIM and np.abs(z).sum(0).max() < LIM:
            return g
    raise AssertionError(f"no amplitude keeps the statistics of {key} exact")


def ref_bn_row_sums(z16, what="bn_partials"):
    """(sum z, sum z^2) per channel of the stored f16 z as float64, for a comparison with the float64 sum of the partial
    ROWS; asserts that every row (<= BN_TILE_MAX pixels) is exact in f32 in any order."""
    z = z16.astype(np.float64).reshape(-1, z16.shape[-1])
    q = quantum_of(z)
    assert BN_TILE_MAX * float(np.abs(z).max()) / q < LIM and BN_TILE_MAX * float((z * z).max()) / (q * q) < LIM, \
        f"{what}: a partial row may leave the exact f32 range"
    return z.sum(0), (z * z).sum(0)


def gen_bn_rounded(key, B, H, W, Cin, Cout, k, stride):
    """The same launch with a z that IS rounded by the f16 store (amp_for_integer_output: |z| mostly beyond 2048), to tell
    'sums of the f16 values it stores' from sums of the f32 values before the cast.  Only sum z is exact then."""
    g = gen_conv(("bn rounded", key), B, H, W, Cin, Cout, k, stride, amp=amp_for_integer_output(k * k * Cin))
    g.scale, g.bias = np.ones(Cout, np.float32), np.zeros(Cout, np.float32)
    return g


def ref_bn_rounded_sum(r, what="bn_partials (rounded z)"):
    """sum z per channel (float64) of the stored f16 z of reference r.  A row sums at most BN_TILE_MAX integers (or even
    integers) of magnitude < 65504: 256 * 65504 < 2^24, exact in f32 in any order.  Also asserts that the case can tell the
    stored values from the unrounded ones."""
    z = r.ref16.astype(np.float64).reshape(-1, r.ref16.shape[-1])
    assert quantum_of(z) >= 1.0 and BN_TILE_MAX * float(np.abs(z).max()) < LIM, f"{what}: a partial row may be inexact"
    s_stored, s_unrounded = z.sum(0), r.v.reshape(z.shape).sum(0)
    assert (s_stored != s_unrounded).mean() > 0.5, f"{what}: the sums of stored and unrounded z do not differ"
    return s_stored


# ------------------------------------------------------------------------------------------------ comparison
def _first_diff(bad, got, ref):
    idx = tuple(int(i) for i in np.argwhere(bad)[0])
    return f"{int(bad.sum())} of {bad.size} elements differ; first at {idx}: got {got[idx]!r}, expected {ref[idx]!r}"


def assert_equal(got, ref, what=""):
    """Bit-for-bit (by value: +0 == -0, Inf == Inf, NaN equals nothing)."""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape and got.dtype == ref.dtype, (what, got.shape, ref.shape, got.dtype, ref.dtype)
    bad = ~(got == ref)
    assert not bad.any(), f"{what}: {_first_diff(bad, got, ref)}"


def assert_matches(got16, r, what=""):
    """got16 (numpy f16) against the namespace epilogue() returned: equality; for ELU, elements with a non-positive
    pre-activation may also be one of the two f16 neighbours of f16(ref)."""
    got16 = np.asarray(got16)
    assert got16.dtype == np.float16 and got16.shape == r.ref16.shape, (what, got16.dtype, got16.shape, r.ref16.shape)
    bad = ~(got16 == r.ref16)
    if r.act == "elu":
        up = np.nextafter(r.ref16, np.float16(np.inf))
        dn = np.nextafter(r.ref16, np.float16(-np.inf))
        bad &= ~((r.pre <= 0) & ((got16 == up) | (got16 == dn)))
    assert not bad.any(), f"{what}: {_first_diff(bad, got16, r.ref16)}"


def assert_matches32(got32, r, what=""):
    """An f32 output against the namespace epilogue() returned: equality.  An element on ELU's negative branch has no f16
    rounding to absorb od_expm1_fast's error (relative < 1e-6, as its source states): it must lie within
    1e-6 * |expm1(pre)| plus one f32 ulp of the result -- again a bound from the formats and the stated accuracy."""
    got32 = np.asarray(got32)
    assert got32.dtype == np.float32 and got32.shape == r.ref32.shape, (what, got32.dtype, got32.shape, r.ref32.shape)
    bad = ~(got32 == r.ref32)
    if r.act == "elu":
        lim = 1e-6 * np.abs(np.expm1(np.minimum(r.pre, 0))) + 2.0 ** -23 * np.abs(r.v)
        bad &= ~((r.pre <= 0) & (np.abs(got32.astype(np.float64) - r.v) <= lim))
    assert not bad.any(), f"{what}: {_first_diff(bad, got32, r.ref32)}"


# ------------------------------------------------------------------------------------------------ guarded device tensors
_TORCH_DT = {np.dtype(np.float16): torch.float16, np.dtype(np.float32): torch.float32, np.dtype(np.uint8): torch.uint8}


def poisoned(arr, device):
    """arr as a 16-byte-aligned device view in the MIDDLE of one larger allocation whose remainder (>= 4 KiB on each
    side) holds f16 NaN patterns (u8 data: 255).  A read outside the tensor that reaches a result makes it NaN / wrong;
    the stray access itself lands in mapped memory.  A stray read whose value is discarded stays invisible."""
    a = np.ascontiguousarray(arr)
    n = a.nbytes
    body = (n + 15) // 16 * 16
    if a.dtype == np.uint8:
        host = np.full(2 * GUARD_BYTES + body, U8_POISON, np.uint8)
    else:
        host = np.full((2 * GUARD_BYTES + body) // 2, F16_NAN_BITS, np.uint16).view(np.uint8)
    host[GUARD_BYTES:GUARD_BYTES + n] = a.reshape(-1).view(np.uint8)
    base = torch.from_numpy(host).to(device)
    view = base[GUARD_BYTES:GUARD_BYTES + n].view(_TORCH_DT[a.dtype]).view(a.shape)
    assert view.data_ptr() % 16 == 0
    return view


class Guarded:
    """An output tensor as a view inside a sentinel-filled allocation (>= 4 KiB of guard on each side)."""

    def __init__(self, shape, dtype, device, init=None):
        numel = int(np.prod(shape))
        n = numel * torch.empty((), dtype=dtype).element_size()
        self.lo, self.hi = GUARD_BYTES, GUARD_BYTES + n
        self.base = torch.full((2 * GUARD_BYTES + (n + 15) // 16 * 16,), SENTINEL, dtype=torch.uint8, device=device)
        self.t = self.base[self.lo:self.hi].view(dtype).view(shape)
        if init is not None:
            self.t.copy_(torch.from_numpy(np.ascontiguousarray(init)))
        assert self.t.data_ptr() % 16 == 0

    def check(self, what=""):
        assert bool((self.base[:self.lo] == SENTINEL).all()) and bool((self.base[self.hi:] == SENTINEL).all()), \
            f"{what}: guard band overwritten"

    def numpy(self, what=""):
        self.check(what)
        return self.t.cpu().numpy()
