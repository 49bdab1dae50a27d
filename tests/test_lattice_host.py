"""CPU checks of the exact-arithmetic tier (tests/lattice_ref.py): no GPU, no library.

1. The reference's convolution (torch-CPU float64) against a direct int64 convolution, and the gradient references
   against sums written out tap by tap, on the small cases.
2. The conditions that make f32 accumulation exact (lattice_ref's docstring, 1-4) for EVERY case the GPU files run:
   building a case's reference asserts them, so each build_* call below is that check.
3. The helper notices what it is there to notice: a truncating cast, a residual added after the cast, a lattice that is
   too wide for f32, a NaN guard that reaches a result.
"""
import pathlib
import sys

import numpy as np
import pytest

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))

import lattice_ref as L  # noqa: E402
import test_gpu_conv_exact as E  # noqa: E402

SMALL = 3e8  # multiply-adds up to which the int64 restatement is run


def _work(B, H, W, Cin, Cout, k, stride):
    return B * H * W * Cin * Cout * k * k / (stride * stride)


@pytest.mark.parametrize("case", [c for c in E.tc.CASES if _work(*c[:7]) <= SMALL], ids=str)
def test_reference_convolution_is_the_integer_convolution(case):
    B, H, W, Cin, Cout, k, stride = case[:7]
    g = L.gen_conv(("fwd", case[:9]), B, H, W, Cin, Cout, k, stride)
    ref = L.conv_nhwc(g.x, g.w, stride)
    direct = L.conv_int64(g.x, g.w, stride)
    assert ref.shape == direct.shape and np.array_equal(ref, direct.astype(np.float64))
    import torch
    assert np.array_equal(L.conv_nhwc(g.x, g.w, stride, torch.float32), ref)  # what the large cases use


@pytest.mark.parametrize("case", [c for c in E.tk.CONV_CASES if _work(*c) <= SMALL], ids=str)
def test_gradient_references_are_the_integer_sums(case):
    B, H, W, Cin, Cout, k, stride = case
    g = L.gen_grad(("wgrad", case), B, H, W, Cin, Cout, k, stride)
    Ho, Wo = L.out_hw(H, W, stride)
    p = k // 2
    xi, dzi, wi = g.x.astype(np.int64), g.dz.astype(np.int64), g.w.astype(np.int64)
    xp = np.zeros((B, H + 2 * p + stride, W + 2 * p + stride, Cin), np.int64)
    xp[:, p:p + H, p:p + W] = xi
    dw = np.zeros((Cout, k, k, Cin), np.int64)
    dxp = np.zeros_like(xp)
    for dy in range(k):
        for dx in range(k):
            sl = (slice(None), slice(dy, dy + (Ho - 1) * stride + 1, stride), slice(dx, dx + (Wo - 1) * stride + 1, stride))
            dw[:, dy, dx, :] = np.einsum("bhwo,bhwi->oi", dzi, xp[sl])
            dxp[sl] += dzi @ wi[:, dy, dx, :]
    assert np.array_equal(L.ref_bwd_weight(g.x, g.dz, k, stride), dw.reshape(Cout, -1).astype(np.float32))
    r = L.ref_bwd_data(g.dz, g.w, g.x.shape, stride, rounding=False)  # small integers: the transposed conv itself is checked
    assert np.array_equal(r.v, dxp[:, p:p + H, p:p + W].astype(np.float64))


# ---- the conditions, for every case list of the GPU files ------------------------------------------------------------
@pytest.mark.parametrize("case", E.tc.CASES + E.SPLITK_CASES, ids=str)
def test_conditions_forward(case):
    g, r = E.build_fwd(case)
    assert r.ref16.dtype == np.float16 and np.isfinite(r.ref16).all()


@pytest.mark.parametrize("case", E.tc.RDIRECT_CASES, ids=str)
def test_conditions_weights_resident(case):
    E.build_rdirect(case)


@pytest.mark.parametrize("case", E.tc.PW_CASES, ids=str)
def test_conditions_consuming_pointwise(case):
    E.build_pw(case)


@pytest.mark.parametrize("case", E.GROUPED_CASES, ids=str)
def test_conditions_grouped(case):
    E.build_grouped(case)


def test_conditions_f32_strided():
    E.build_fwd((2, 10, 10, 256, 208, 3, 1, None, "none", -1), out_f32=True)


@pytest.mark.parametrize("case", E.tb.CASES, ids=str)
def test_conditions_bottleneck(case):
    E.build_bneck(case)


@pytest.mark.parametrize("case", E.STEM_CASES, ids=str)
def test_conditions_stem(case):
    E.build_stem(case)


@pytest.mark.parametrize("shape", E.FIRST_CASES, ids=str)
def test_conditions_first_layer(shape):
    E.build_first(shape)


@pytest.mark.parametrize("case", E.BWD_CASES, ids=str)
def test_conditions_backward_data(case):
    E.build_bwd(case)


@pytest.mark.parametrize("case", E.WGRAD_CASES + E.W8_WGRAD_CASES, ids=str)
def test_conditions_weight_gradient(case):
    E.build_wgrad(case)


@pytest.mark.parametrize("case", E.FIRST_WGRAD_CASES, ids=str)
def test_conditions_first_layer_weight_gradient(case):
    E.build_first_wgrad(case)


@pytest.mark.parametrize("case", E.BN_CASES, ids=str)
def test_conditions_bn_partials(case):
    E.build_bn(case)
    E.build_bn_rows(case)
    if case[5] * case[5] * case[3] >= 576:
        E.build_bn_rounded(case)  # asserts condition 4 on z and that stored and unrounded sums differ


# the shapes of the plan file nearest the limits (Darknet53 at the 32 x 320^2 / 16 x 640^2 shards: host arithmetic only):
# the widest pixel sums of the weight gradients, the image layer falling back to a {0, 1} image, the largest backward-data
# map, per-row bn sums at M = 819 200 and at the longest K
@pytest.mark.parametrize("case", [(16, 640, 640, 32, 64, 3, 2), (16, 320, 320, 64, 32, 1, 1)], ids=str)
def test_conditions_shard_weight_gradient(case):
    E.build_wgrad(case)


@pytest.mark.parametrize("case", [(32, 320, 320), (16, 640, 640)], ids=str)
def test_conditions_shard_first_layer_weight_gradient(case):
    g, _dw = E.build_first_wgrad(case)
    assert g.x.max() == 1 and np.abs(g.dz).max() == 1


def test_conditions_shard_backward_data():
    E.build_bwd((32, 320, 320, 32, 64, 3, 2))


@pytest.mark.parametrize("case", [(32, 320, 320, 32, 64, 3, 2), (16, 20, 20, 512, 1024, 3, 1)], ids=str)
def test_conditions_shard_bn_partial_rows(case):
    E.build_bn_rows(case)


@pytest.mark.parametrize("case", E.OVERFLOW_FWD, ids=str)
def test_conditions_forward_overflow(case):
    g, r = E.build_fwd(case, overflow=True)
    assert np.isinf(r.ref16).any() and np.isfinite(r.ref16).any()


@pytest.mark.parametrize("case", E.OVERFLOW_BWD, ids=str)
def test_conditions_backward_overflow(case):
    g, r, racc = E.build_bwd(case, overflow=True)
    assert np.isinf(r.ref16).any() and np.isfinite(r.ref16).any()


@pytest.mark.parametrize("args", [(600, 256, 1, 0, 0, 0, True), (2 * 8 * 12, 64, 0, 0, 0, 0, True), (2 * 8 * 12, 64, 1, 1, 8, 12, True),
                                  (100, 128, 0, 0, 0, 0, False)], ids=str)
def test_conditions_wide_add(args):
    import test_gpu_conv_exact_plan as P
    y, res, v32, hi, hilo = P.build_wide(*args)
    assert hilo.shape == (args[0], 2 * args[1]) and hilo.dtype == np.float16
    # [hi | lo] carries v to ~22 bits: hi + lo differs from v by at most half an ulp of lo
    back = hilo[:, :args[1]].astype(np.float64) + hilo[:, args[1]:].astype(np.float64)
    assert np.abs(back - v32).max() <= 2.0 ** -11 * np.abs(hilo[:, args[1]:].astype(np.float64)).max()


# ---- the helper bites------------------------------------------------------------------------------------------------
def _trunc16(v):
    r = v.astype(np.float16)
    over = np.abs(r.astype(np.float64)) > np.abs(v)
    return np.where(over, np.nextafter(r, np.float16(0)), r).astype(np.float16)


def test_equality_notices_truncation_a_second_rounding_and_a_dropped_term():
    case = (2, 12, 12, 64, 128, 3, 1, "leaky", "same", 0)
    g, r = E.build_fwd(case)
    L.assert_matches(r.ref16.copy(), r, "identity")
    with pytest.raises(AssertionError, match="elements differ"):
        L.assert_matches(_trunc16(r.v), r, "truncating cast")
    early = ((r.v - g.res.astype(np.float64)).astype(np.float16).astype(np.float64) + g.res).astype(np.float16)
    assert (early != r.ref16).mean() > 0.05
    with pytest.raises(AssertionError, match="elements differ"):
        L.assert_matches(early, r, "residual added after the cast")
    x1 = g.x.copy()
    x1[1, 5, 7, 3] = 0  # one dropped input element
    r1 = L.ref_forward(x1, g.w, g.scale, g.bias, 1, "leaky", L.SLOPE, g.res)
    with pytest.raises(AssertionError, match="elements differ"):
        L.assert_matches(r1.ref16, r, "dropped term")


def test_conditions_reject_a_lattice_too_wide_for_f32_and_one_without_rounding():
    rng = np.random.default_rng(0)
    x = rng.integers(-2048, 2049, (1, 6, 6, 512)).astype(np.float16)
    w = rng.integers(-2048, 2049, (64, 3, 3, 512)).astype(np.float32)
    with pytest.raises(AssertionError, match="2\\^24"):
        L.ref_forward(x, w, np.ones(64, np.float32), np.zeros(64, np.float32))
    x = rng.integers(-1, 2, (1, 8, 8, 64)).astype(np.float16)
    w = rng.integers(-1, 2, (64, 3, 3, 64)).astype(np.float32)
    with pytest.raises(AssertionError, match="inexact"):  # every output is a small integer: nothing is rounded
        L.ref_forward(x, w, np.ones(64, np.float32), np.zeros(64, np.float32))
    with pytest.raises(AssertionError, match="reaches"):
        L.ref_forward(x * np.float16(64), w * 64, np.full(64, 64, np.float32), np.zeros(64, np.float32))


def test_elu_neighbour_rule_is_one_ulp_on_the_negative_branch_only():
    case = (3, 10, 10, 128, 64, 1, 1, "elu", "none", 0)
    g, r = E.build_fwd(case)
    neg, pos = np.argwhere(r.pre < 0)[0], np.argwhere(r.pre > 0)[0]
    for idx, steps, ok in ((neg, 1, True), (neg, 2, False), (pos, 1, False)):
        got = r.ref16.copy()
        for _ in range(steps):
            got[tuple(idx)] = np.nextafter(got[tuple(idx)], np.float16(np.inf))
        if ok:
            L.assert_matches(got, r, "one neighbour")
        else:
            with pytest.raises(AssertionError, match="elements differ"):
                L.assert_matches(got, r, "too far")


def test_poison_patterns():
    nan16 = np.array([L.F16_NAN_BITS], np.uint16).view(np.float16)
    assert np.isnan(nan16).all() and np.isnan(nan16.astype(np.float32) * 0.0).all()  # garbage * 0 is NaN, not 0
    s16 = np.array([L.SENTINEL * 257], np.uint16).view(np.float16)
    s32 = np.array([L.SENTINEL * 0x01010101], np.uint32).view(np.float32)
    assert np.isfinite(s16).all() and np.isfinite(s32).all()
    assert L.quantum_of(s16) == 2.0 ** -16  # finer than any lattice used here (>= 2^-13): never an expected value
    with pytest.raises(AssertionError, match="elements differ"):
        L.assert_equal(np.array([np.nan], np.float32), np.array([np.nan], np.float32), "NaN equals nothing")


# ---- the persistent-walk cases of test_gpu_conv_exact.WALKS: their rule and their references, without a GPU
@pytest.mark.parametrize("num_cu", [64, 228, 256, 304], ids=str)
def test_walk_shapes_hold_their_rule_on_any_part(num_cu):
    for name, (units, per_cu, trips, _kernel, _make) in E.WALKS.items():
        workers = per_cu * num_cu
        E.assert_walks(E.walk_batch(units, workers, trips) * units, workers, trips, f"{name} on {num_cu} CUs")
    with pytest.raises(AssertionError, match="not a walk"):
        E.assert_walks(33 * 4, num_cu, 4, "the old (33, 32, 32, 64) case")  # 132 tiles: one each on 256 CUs, 2 on 64


def test_fullsize_cases_walk_on_256_cus():
    """What the full-size cases of the stream kernels give a 256-CU part (work, workers, least trips).  The two ring kernels
    get 25 tiles per workgroup, the same for all: unequal trip counts come from the WALKS cases alone."""
    B, Hs, Ws = E.TCONV_STREAM_CASES[-1]  # od_tconv_64_32: 4 x 16 dZ tiles, 2 workgroups per CU, ring of 3
    E.assert_walks(B * (Hs // 4) * (Ws // 16), 2 * 256, 5, "od_tconv_64_32 (32, 160, 160)", uneven=False)
    B, Hs, Ws = E.TCONV_RDIRECT_CASES[-1]  # od_tconv_rdirect: 16 dZ pixels of a row per item, 8 waves per CU
    E.assert_walks(B * Hs * (Ws // 16), 8 * 256, 4, "od_tconv_rdirect (32, 80, 80)")
    B, H, W = E.tc.CASES[-1][:3]  # od_conv_stream3<32, 64, 1>: 4 x 16 output tiles, 2 workgroups per CU
    E.assert_walks(B * (H // 4) * (W // 16), 2 * 256, 5, "od_conv_stream3 (32, 160, 160)", uneven=False)
    for c in E.tc.RDIRECT_CASES[-2:]:  # the pointwise od_conv_rdirect forms: 2 workgroups per CU x 8 waves
        E.assert_walks(c[0] * c[1] * (c[2] // 16), 2 * 8 * 256, 3, f"od_conv_rdirect {c}")


@pytest.mark.parametrize("walk", sorted(E.WALKS), ids=str)
def test_walk_case_references_are_exact(walk):
    units, per_cu, trips, _kernel, make = E.WALKS[walk]
    case = make(E.walk_batch(units, per_cu * 16, trips))  # a 16-CU part's shape: the conditions do not depend on the batch
    build = {"bneck64": E.build_bneck, "stem": E.build_stem, "rdirect3x3": E.build_rdirect, "tconv_rdirect": E.build_bwd,
             "tconv_64_32": E.build_bwd}.get(walk, E.build_fwd)
    build(case)
