"""Every convolution kernel family, bit for bit, on exact-arithmetic inputs with poisoned surroundings.

The case lists are those of test_gpu_conv.py, test_gpu_bneck.py, test_gpu_stem.py and test_gpu_train_kernels.py (imported,
not copied).  Those tests feed Gaussian data and need a tolerance for the f32 accumulation order; here the inputs come
from tests/lattice_ref.py, for which f32 accumulation is exact in any order, so every comparison is an EQUALITY with the
float64 reference rounded once (the only exception: an element on ELU's negative branch may be one f16 neighbour off,
see lattice_ref).  A dropped pixel, a truncating cast, a second rounding or a wrong tap then fails, whatever the size.

Poisoned surroundings: every f16 input (x, res, dz) is a view in the middle of one larger allocation filled with f16 NaN
patterns (u8 inputs: 255), every output a view inside a sentinel-filled allocation whose guards (>= 4 KiB on each side)
must stay intact.  A read outside a tensor that REACHES a result (e.g. K or M padding done by multiplying with zero
weights) turns it into NaN and fails the equality.  A stray read whose value is discarded stays invisible to this
technique; nothing here tries to catch it.

The build_* functions produce the inputs and the reference of a case and need no GPU: tests/test_lattice_host.py runs
them for every case below, so the conditions that make the arithmetic exact are checked on a machine without a GPU.
"""
import ctypes as C
import pathlib
import sys

import numpy as np
import pytest
import torch

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))

import lattice_ref as L  # noqa: E402
import test_gpu_bneck as tb  # noqa: E402
import test_gpu_conv as tc  # noqa: E402
import test_gpu_stem as ts  # noqa: E402
import test_gpu_train_kernels as tk  # noqa: E402

pytestmark = pytest.mark.gpu


def params_of(fn, name=None):
    """The case list of an existing parametrised test (the argument of its @pytest.mark.parametrize)."""
    marks = [m for m in fn.pytestmark if m.name == "parametrize" and (name is None or m.args[0] == name)]
    assert len(marks) == 1
    return list(marks[0].args[1])


def _alpha(act, slope=L.SLOPE):
    return slope if act == "leaky" else 1.0


SPLITK_CASES = params_of(tc.test_conv_split_k)
GROUPED_CASES = params_of(tc.test_conv_grouped_over_pyramid_levels)
FIRST_CASES = params_of(tc.test_conv_first_matches_oracle)
STEM_CASES = [(s, a) for s in params_of(ts.test_stem_matches_oracle, "shape") for a in params_of(ts.test_stem_matches_oracle, "act")]
SLAB_CASES = params_of(tk.test_weight_gradient_slab_path_many_splits)
WGRAD_CASES = list(dict.fromkeys(tk.CONV_CASES + SLAB_CASES))
# The 8-wave 256 x 256 weight-gradient kernel (od_conv_wgrad_w8) is selected only with >= 60 pixel chunks in each of >= 160
# workgroups: ~50 GFLOP is the floor on a 256-CU part, so its cases live here (a few ms on the GPU, seconds for the integer
# reference) and not in the torch-f64 tests.  The smallest shapes the rule admits:
W8_WGRAD_CASES = [
    (16, 20, 20, 512, 1024, 3, 1),   # whole tiles, a trainer shape of 16 x 640^2: M = 6400, 3 splits x 72 tiles, 67 chunks each
    (11, 70, 70, 256, 208, 3, 1),    # ragged Cout, one tap over two half-tiles, ragged last chunk (M = 53900 = 32 q + 12): 28 x 9, 61
    (5, 148, 148, 128, 1024, 3, 2),  # stride 2, ragged Ktot (4.5 column tiles), M = 27380 = 32 q + 20: 12 splits x 20 tiles, 72
]
# (its 1x1 form needs a 250 MB dZ at the smallest admissible shape and no trainer shape selects it: left out)
W8_WGRAD_KERNEL = {c: "od_conv_wgrad_w8" for c in W8_WGRAD_CASES}
ALL_WGRAD_KERNELS = {"od_conv_wgrad", "od_conv_wgrad_w8", tk.WGRAD_THIN1, tk.WGRAD_THIN2}
TCONV_STREAM_CASES = params_of(tk.test_first_downsample_backward_data_streaming_kernel)
TCONV_RDIRECT_CASES = params_of(tk.test_second_downsample_backward_data_weights_resident_kernel)
FIRST_WGRAD_CASES = params_of(tk.test_first_layer_weight_gradient)
BN_CASES = params_of(tk.test_bn_statistics_from_the_conv_epilogue)
# backward-data: (B, H, W, Cin, Cout, k, stride) of the FORWARD layer; the two special kernels take dZ 64 -> dX 32 and
# dZ 128 -> dX 64 of a 3x3 stride-2 layer, their cases give the dZ map
BWD_CASES = list(dict.fromkeys(
    tk.CONV_CASES + [(B, 2 * h, 2 * w, 32, 64, 3, 2) for B, h, w in TCONV_STREAM_CASES]
    + [(B, 2 * h, 2 * w, 64, 128, 3, 2) for B, h, w in TCONV_RDIRECT_CASES]))
# overflow: pre-activations beyond the f16 range must become +-Inf exactly where the reference's cast does
OVERFLOW_FWD = [(2, 12, 12, 64, 128, 3, 1, "leaky", "same", -1), (2, 10, 10, 512, 256, 3, 1, None, "none", tc.NE8),
                (3, 10, 10, 128, 64, 1, 1, "leaky", "none", 2)]
OVERFLOW_BWD = [(2, 12, 12, 64, 128, 3, 1), (2, 12, 12, 64, 128, 3, 2), (2, 6, 10, 1024, 512, 1, 1), (2, 16, 32, 32, 64, 3, 2)]


# ------------------------------------------------------------------------------------------------ inputs + references (CPU)
_FWD_CACHE = {}  # references of the small cases: the table configs of one shape differ in tile_cfg only


def build_fwd(case, slope=L.SLOPE, out_f32=False, overflow=False):
    B, H, W, Cin, Cout, k, stride, act, resm, _cfg = case[:10]
    ck = (case[:9], slope, out_f32, overflow)
    if ck in _FWD_CACHE:
        return _FWD_CACHE[ck]
    g = L.gen_conv(("fwd", case[:9]), B, H, W, Cin, Cout, k, stride, resm, act)
    if overflow:  # scale and bias x 2^8: |acc| of a few hundred and more leaves the f16 range; an integer residual keeps the f32 sum exact
        g.scale, g.bias = g.scale * np.float32(256.0), g.bias * np.float32(256.0)
        g.res = None if g.res is None else g.res * np.float16(8.0)
    r = L.ref_forward(g.x, g.w, g.scale, g.bias, stride, act, _alpha(act, slope), g.res, resm == "up2", out_f32, overflow,
                      what=f"fwd {case}")
    if r.ref16.size <= (1 << 21):
        _FWD_CACHE[ck] = (g, r)
    return g, r


def build_rdirect(case):
    B, H, W, Cin, Cout, k, stride, act, with_res = case
    c = (B, H, W, Cin, Cout, k, stride, act, "same" if with_res else "none", -1)
    return build_fwd(c, slope=0.1)  # single layer: the product's slope (one IEEE multiply, see lattice_ref)


def build_pw(case):
    """ELU first layers are lifted onto ELU's identity branch by their bias (lattice_ref.gen_conv, lift): the second layer
    can then be checked against the chained reference, exactly.  The price: in the ELU PW_CASES the negative branch of the
    FIRST layer inside the fused epilogue is never executed by this tier, and `out` of those cases carries no ELU content
    (the single-layer ELU cases of CASES do; out2's own ELU negative branch is exercised)."""
    B, H, W, Cin, Cout, k, stride, act, resm, act2, _cfg = case
    # ELU, lifted above zero by its bias: amplitude 8 at scale 1 or 2
    amp = 8 if act == "elu" else L.amp_for_integer_output(k * k * Cin)
    g = L.gen_conv(("pw", case[:10]), B, H, W, Cin, Cout, k, stride, resm, act, amp=amp, Cout2=Cout // 2,
                   lift=act == "elu", integer=True)
    if act != "elu":
        g.scale = np.ones(Cout, np.float32)
    r1, r2 = L.ref_forward_pw(g, stride, act, _alpha(act), resm, act2, _alpha(act2), what=f"pw {case}")
    return g, r1, r2


def build_grouped(case):
    B, dims, Cin, Cout, act, out_f32, _cfg = case
    g = L.gen_conv(("grp", B, Cin, Cout, act), B, 1, 1, Cin, Cout, 3, 1, "none", act)
    rng = np.random.default_rng(L.seed_of("grpx", case[:4]))
    xs = [rng.integers(-8, 9, (B, h, w, Cin)).astype(np.float16) for h, w in dims]
    rs = [L.ref_forward(x, g.w, g.scale, g.bias, 1, act, _alpha(act), out_f32=out_f32, what=f"grouped {case}") for x in xs]
    return g, xs, rs


def build_bneck(case):
    B, H, W, Cc, act = case
    g = L.gen_bneck(case, B, H, W, Cc, act)
    return g, L.ref_bneck(g, act, _alpha(act), what=f"bneck {case}")


def build_stem(case):
    (B, H, W), act = case
    g = L.gen_stem(case, B, H, W, act)
    return g, L.ref_stem(g, act, _alpha(act), what=f"stem {case}")


def build_first(shape):
    B, H, W = shape
    g = L.gen_stem(("first", shape), B, H, W, "leaky")
    return g, L.ref_conv_first(g.x, g.w0, g.s0, g.b0, "leaky", 0.1, what=f"first {shape}")  # single layer: slope 0.1


def build_bwd(case, overflow=False):
    B, H, W, Cin, Cout, k, stride = case
    g = L.gen_grad(("bwd", case), B, H, W, Cin, Cout, k, stride, bwd_data=True)
    if overflow:  # sigma 7000 -> 28000: a few per cent of dx pass 65504
        g.dz = g.dz * np.float16(4.0)
    r, racc = L.ref_bwd_data(g.dz, g.w, g.x.shape, stride, g.acc, overflow, what=f"bwd-data {case}", both=True)
    return g, r, racc


def build_wgrad(case):
    B, H, W, Cin, Cout, k, stride = case
    g = L.gen_grad(("wgrad", case), B, H, W, Cin, Cout, k, stride, amp=3)
    dw = L.ref_bwd_weight(g.x, g.dz, k, stride, what=f"wgrad {case}")
    dw_acc = (dw.astype(np.float64) + g.dw0).astype(np.float32)
    assert np.array_equal(dw_acc.astype(np.float64), dw.astype(np.float64) + g.dw0)
    return g, dw, dw_acc


FIRST_IN_SCALE = 2.0 ** -8


def build_first_wgrad(case):
    B, H, W = case
    g = L.gen_first_grad(case, B, H, W)
    dw = L.ref_bwd_weight(g.x.astype(np.float32), g.dz, 3, 1, g.dw0, FIRST_IN_SCALE, what=f"first wgrad {case}")
    return g, dw


def build_bn(case):
    B, H, W, Cin, Cout, k, stride = case
    g = L.gen_bn(case, B, H, W, Cin, Cout, k, stride)
    r = L.ref_forward(g.x, g.w, g.scale, g.bias, stride, what=f"bn {case}", rounding=False)
    return g, r, L.ref_bn_sums(r.ref16, what=f"bn {case}")


def build_bn_rows(case):
    """Exact per partial row only (any pixel count): -> g, reference of z, (sum z, sum z^2) as float64."""
    B, H, W, Cin, Cout, k, stride = case
    g = L.gen_bn(case, B, H, W, Cin, Cout, k, stride, per_row=True)
    r = L.ref_forward(g.x, g.w, g.scale, g.bias, stride, what=f"bn rows {case}", rounding=False)
    return g, r, L.ref_bn_row_sums(r.ref16, what=f"bn rows {case}")


def build_bn_rounded(case):
    """A z that the f16 store rounds: -> g, reference of z, sum of the STORED z as float64."""
    B, H, W, Cin, Cout, k, stride = case
    g = L.gen_bn_rounded(case, B, H, W, Cin, Cout, k, stride)
    r = L.ref_forward(g.x, g.w, g.scale, g.bias, stride, what=f"bn rounded {case}")
    return g, r, L.ref_bn_rounded_sum(r, what=f"bn rounded {case}")


# ------------------------------------------------------------------------------------------------ device side
def _ctx(cuda):
    from object_detector_amd.net import Context
    return Context.get(cuda)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def _packed(w, scale, bias, cuda):
    from object_detector_amd.net import pack_conv_weight, pad_vec
    wp = _dev(pack_conv_weight(w), cuda)
    return wp, _dev(pad_vec(np.asarray(scale, np.float32), wp.shape[0]), cuda), \
        _dev(pad_vec(np.asarray(bias, np.float32), wp.shape[0]), cuda)


def run_conv(cuda, x, w, scale, bias, stride=1, act=None, alpha=0.0, res=None, resm="none", cfg=-1, splitk=1, out_f32=False,
             second=None, bn=False):
    """od_conv2d_fwd on poisoned inputs into guarded outputs -> numpy out (, out2) (, partial rows)."""
    from object_detector_amd import _lib
    ctx = _ctx(cuda)
    B, H, W, Cin = x.shape
    Cout, k = w.shape[0], w.shape[1]
    Ho, Wo = L.out_hw(H, W, stride)
    keep = [L.poisoned(x, cuda), _packed(w, scale, bias, cuda)]
    out = L.Guarded((B, Ho, Wo, Cout), torch.float32 if out_f32 else torch.float16, cuda)
    d = _lib.ConvDesc()
    d.x, d.out = keep[0].data_ptr(), out.t.data_ptr()
    d.w, d.scale, d.bias = (t.data_ptr() for t in keep[1])
    if res is not None:
        keep.append(L.poisoned(res, cuda))
        d.res = keep[-1].data_ptr()
    d.B, d.H, d.W, d.Cin, d.Cout, d.ksize, d.stride = B, H, W, Cin, Cout, k, stride
    d.act, d.alpha = _lib.ACT_ENUM[act], float(alpha)
    d.res_mode = {"none": _lib.OD_RES_NONE, "same": _lib.OD_RES_SAME, "up2": _lib.OD_RES_UP2}[resm]
    d.out_dtype = _lib.OD_DT_F32 if out_f32 else _lib.OD_DT_F16
    d.tile_cfg, d.splitk = cfg, splitk
    if splitk != 1:
        keep.append(torch.empty(32 * B * Ho * Wo * Cout, dtype=torch.float32, device=cuda))
        d.splitk_workspace, d.splitk_workspace_bytes = keep[-1].data_ptr(), keep[-1].numel() * 4
    out2 = part = None
    if second is not None:
        w2, scale2, bias2, act2, alpha2 = second
        keep.append(_packed(w2, scale2, bias2, cuda))
        out2 = L.Guarded((B, Ho, Wo, w2.shape[0]), torch.float16, cuda)
        d.w2, d.scale2, d.bias2 = (t.data_ptr() for t in keep[-1])
        d.out2, d.Cout2, d.act2, d.alpha2 = out2.t.data_ptr(), w2.shape[0], _lib.ACT_ENUM[act2], float(alpha2)
    rows = 0
    if bn:
        M = B * Ho * Wo
        part = L.Guarded((((M + 63) // 64) * 2 * Cout,), torch.float32, cuda)
        d.bn_partials, d.bn_partials_bytes = part.t.data_ptr(), part.t.numel() * 4
        rows = ctx.lib.od_conv2d_fwd_bn_rows(ctx.handle, C.byref(d))
        assert 0 < rows <= (M + 63) // 64
    _lib.check(ctx.lib.od_conv2d_fwd(ctx.handle, C.byref(d), _stream()), "od_conv2d_fwd")
    torch.cuda.synchronize()
    res_ = [out.numpy("out")]
    if out2 is not None:
        res_.append(out2.numpy("out2"))
    if part is not None:
        res_.append((part, rows))
    return res_[0] if len(res_) == 1 else tuple(res_)


# ------------------------------------------------------------------------------------------------ od_conv2d_fwd
@pytest.mark.parametrize("case", tc.CASES, ids=str)
def test_fwd_every_table_config(cuda, case):
    act, resm, cfg = case[7:10]
    g, r = build_fwd(case)
    got = run_conv(cuda, g.x, g.w, g.scale, g.bias, case[6], act, _alpha(act), g.res, resm, cfg)
    L.assert_matches(got, r, f"fwd {case}")


@pytest.mark.parametrize("case", tc.RDIRECT_CASES, ids=str)
def test_fwd_weights_resident_kernels(cuda, case, monkeypatch):
    monkeypatch.setenv("OD_CONV_RDIRECT_MIN_PIXELS", "0")
    B, H, W, Cin, Cout, k, stride, act, with_res = case
    g, r = build_rdirect(case)
    got = run_conv(cuda, g.x, g.w, g.scale, g.bias, stride, act, _alpha(act, 0.1), g.res, "same" if with_res else "none", -1)
    L.assert_matches(got, r, f"rdirect {case}")


@pytest.mark.parametrize("case", tc.PW_CASES, ids=str)
def test_fwd_with_consuming_pointwise_layer(cuda, case):
    """out AND out2 against the chained reference (out2 of the reference's own rounded out)."""
    B, H, W, Cin, Cout, k, stride, act, resm, act2, cfg = case
    g, r1, r2 = build_pw(case)
    out, out2 = run_conv(cuda, g.x, g.w, g.scale, g.bias, stride, act, _alpha(act), g.res, resm, cfg,
                         second=(g.w2, g.scale2, g.bias2, act2, _alpha(act2)))
    L.assert_matches(out, r1, f"pw out {case}")
    L.assert_matches(out2, r2, f"pw out2 {case}")


@pytest.mark.parametrize("case", SPLITK_CASES, ids=str)
def test_fwd_split_k(cuda, case):
    act, resm, cfg, sk = case[7:11]
    g, r = build_fwd(case)
    got = run_conv(cuda, g.x, g.w, g.scale, g.bias, case[6], act, _alpha(act), g.res, resm, cfg, splitk=sk)
    L.assert_matches(got, r, f"split-K {case}")


@pytest.mark.parametrize("case", GROUPED_CASES, ids=str)
def test_fwd_grouped_over_pyramid_levels(cuda, case):
    from object_detector_amd import _lib
    B, dims, Cin, Cout, act, out_f32, cfg = case
    g, xs, rs = build_grouped(case)
    ctx = _ctx(cuda)
    wp, sc, bi = _packed(g.w, g.scale, g.bias, cuda)
    xd = [L.poisoned(x, cuda) for x in xs]
    outs = [L.Guarded((B, h, w, Cout), torch.float32 if out_f32 else torch.float16, cuda) for h, w in dims]
    d = _lib.ConvDesc()
    d.w, d.scale, d.bias = wp.data_ptr(), sc.data_ptr(), bi.data_ptr()
    d.B, d.Cin, d.Cout, d.ksize, d.stride = B, Cin, Cout, 3, 1
    d.act, d.alpha = _lib.ACT_ENUM[act], _alpha(act)
    d.out_dtype = _lib.OD_DT_F32 if out_f32 else _lib.OD_DT_F16
    d.tile_cfg, d.nseg = cfg, len(dims)
    for i, (x, o, (h, w)) in enumerate(zip(xd, outs, dims)):
        d.seg_x[i], d.seg_out[i], d.seg_H[i], d.seg_W[i] = x.data_ptr(), o.t.data_ptr(), h, w
    _lib.check(ctx.lib.od_conv2d_fwd(ctx.handle, C.byref(d), _stream()), "od_conv2d_fwd(grouped)")
    torch.cuda.synchronize()
    for i, (o, r) in enumerate(zip(outs, rs)):
        if out_f32:
            L.assert_equal(o.numpy(f"segment {i}"), r.ref32, f"grouped {case} segment {i}")
        else:
            L.assert_matches(o.numpy(f"segment {i}"), r, f"grouped {case} segment {i}")


def test_fwd_f32_into_strided_slice(cuda):
    """The prediction conv: Cout = 208, f32 logits into a slice of pred[B, P, 26]: equality, and the gaps between the images'
    slices, the rest of pred and the guards untouched."""
    from object_detector_amd import _lib
    case = (2, 10, 10, 256, 208, 3, 1, None, "none", -1)
    B, H, W, Cin, Cout = case[:5]
    P_total, Cc, off = 3000, 26, 400
    g, r = build_fwd(case, out_f32=True)
    ctx = _ctx(cuda)
    wp, sc, bi = _packed(g.w, g.scale, g.bias, cuda)
    x = L.poisoned(g.x, cuda)
    pred = L.Guarded((B, P_total, Cc), torch.float32, cuda, init=np.full((B, P_total, Cc), 7.0, np.float32))
    d = _lib.ConvDesc()
    d.x, d.w, d.scale, d.bias = x.data_ptr(), wp.data_ptr(), sc.data_ptr(), bi.data_ptr()
    d.out = pred.t.data_ptr() + off * Cc * 4
    d.B, d.H, d.W, d.Cin, d.Cout, d.ksize, d.stride = B, H, W, Cin, Cout, 3, 1
    d.out_dtype, d.tile_cfg, d.splitk = _lib.OD_DT_F32, -1, 1
    d.out_batch_stride, d.out_pix_stride = P_total * Cc, Cout
    _lib.check(ctx.lib.od_conv2d_fwd(ctx.handle, C.byref(d), _stream()), "od_conv2d_fwd")
    torch.cuda.synchronize()
    got = pred.numpy("pred")
    rows = H * W * Cout // Cc
    L.assert_equal(got[:, off:off + rows], r.ref32.reshape(B, rows, Cc), "f32 strided output")
    assert (got[:, :off] == 7.0).all() and (got[:, off + rows:] == 7.0).all(), "pred written outside the level's slice"


# ------------------------------------------------------------------------------------------------ fused blocks, first layer
@pytest.mark.parametrize("case", tb.CASES, ids=str)
def test_bottleneck(cuda, case):
    from object_detector_amd import _lib
    from object_detector_amd.net import pack_conv_weight, pad_vec
    B, H, W, Cc, act = case
    g, r = build_bneck(case)
    ctx = _ctx(cuda)
    x = L.poisoned(g.x, cuda)
    out = L.Guarded((B, H, W, Cc), torch.float16, cuda)
    w1p, w3p = _dev(pack_conv_weight(g.w1), cuda), _dev(pack_conv_weight(g.w3), cuda)
    v = [_dev(pad_vec(a, n), cuda) for a, n in ((g.s1, w1p.shape[0]), (g.b1, w1p.shape[0]), (g.s3, w3p.shape[0]),
                                               (g.b3, w3p.shape[0]))]
    d = _lib.BneckDesc()
    d.x, d.out, d.w1, d.w3 = x.data_ptr(), out.t.data_ptr(), w1p.data_ptr(), w3p.data_ptr()
    d.scale1, d.bias1, d.scale3, d.bias3 = (t.data_ptr() for t in v)
    d.B, d.H, d.W, d.C, d.act, d.alpha = B, H, W, Cc, _lib.ACT_ENUM[act], _alpha(act)
    _lib.check(ctx.lib.od_bottleneck_fwd(ctx.handle, C.byref(d), _stream()), "od_bottleneck_fwd")
    torch.cuda.synchronize()
    L.assert_matches(out.numpy("out"), r, f"bneck {case}")


@pytest.mark.parametrize("case", STEM_CASES, ids=str)
def test_stem(cuda, case):
    from object_detector_amd import _lib
    from object_detector_amd.net import pack_conv_weight, pack_first_weight, pad_vec
    (B, H, W), act = case
    g, r = build_stem(case)
    ctx = _ctx(cuda)
    x = L.poisoned(g.x, cuda)
    out = L.Guarded((B, H // 2, W // 2, 64), torch.float16, cuda)
    w0p, w3p = _dev(pack_first_weight(g.w0), cuda), _dev(pack_conv_weight(g.w3), cuda)
    v = [_dev(g.s0, cuda), _dev(g.b0, cuda), _dev(pad_vec(g.s3, w3p.shape[0]), cuda), _dev(pad_vec(g.b3, w3p.shape[0]), cuda)]
    d = _lib.StemDesc()
    d.x, d.out, d.w0, d.w3 = x.data_ptr(), out.t.data_ptr(), w0p.data_ptr(), w3p.data_ptr()
    d.scale0, d.bias0, d.scale3, d.bias3 = (t.data_ptr() for t in v)
    d.B, d.H, d.W, d.act, d.alpha = B, H, W, _lib.ACT_ENUM[act], _alpha(act)
    _lib.check(ctx.lib.od_stem_fwd(ctx.handle, C.byref(d), _stream()), "od_stem_fwd")
    torch.cuda.synchronize()
    L.assert_matches(out.numpy("out"), r, f"stem {case}")


@pytest.mark.parametrize("shape", FIRST_CASES, ids=str)
def test_conv_first(cuda, shape):
    from object_detector_amd import _lib
    from object_detector_amd.net import pack_first_weight
    B, H, W = shape
    g, r = build_first(shape)
    ctx = _ctx(cuda)
    x = L.poisoned(g.x, cuda)
    out = L.Guarded((B, H, W, 32), torch.float16, cuda)
    wp, sc, bi = _dev(pack_first_weight(g.w0), cuda), _dev(g.s0, cuda), _dev(g.b0, cuda)
    _lib.check(ctx.lib.od_conv_first_fwd(ctx.handle, x.data_ptr(), wp.data_ptr(), sc.data_ptr(), bi.data_ptr(),
                                         out.t.data_ptr(), B, H, W, 32, _lib.OD_ACT_LEAKY, 0.1, _stream()), "od_conv_first_fwd")
    torch.cuda.synchronize()
    L.assert_matches(out.numpy("out"), r, f"first {shape}")


# ------------------------------------------------------------------------------------------------ backward-data
def check_backward_data(cuda, case, overflow=False):
    """od_conv2d_bwd_data: plain, accumulating into a second tensor, and in place (dx_accumulate aliases dx)."""
    from object_detector_amd import _lib, train_ops as T
    B, H, W, Cin, Cout, k, stride = case
    g, r, racc = build_bwd(case, overflow)
    ctx = _ctx(cuda)
    Ho, Wo = L.out_hw(H, W, stride)
    # the w_bwd pack comes from od_pack_weights: a wrong flip or channel swap cannot hide
    wf, wb = T.pack_weights(_dev(g.w.reshape(Cout, -1), cuda), Cout, Cin, k)
    L.assert_equal(wf.cpu().numpy()[:Cout, :k * k * Cin], g.w.reshape(Cout, -1).astype(np.float16), "forward pack")
    dz = L.poisoned(g.dz, cuda)

    def run(acc, dx):
        _lib.check(ctx.lib.od_conv2d_bwd_data(ctx.handle, dz.data_ptr(), wb.data_ptr(), acc, dx.t.data_ptr(), B, Ho, Wo, Cin,
                                              Cout, k, stride, _stream()), "od_conv2d_bwd_data")
        torch.cuda.synchronize()
        return dx.numpy("dx")
    L.assert_matches(run(None, L.Guarded((B, H, W, Cin), torch.float16, cuda)), r, f"bwd-data {case}")
    acc = L.poisoned(g.acc, cuda)
    L.assert_matches(run(acc.data_ptr(), L.Guarded((B, H, W, Cin), torch.float16, cuda)), racc, f"bwd-data + acc {case}")
    inplace = L.Guarded((B, H, W, Cin), torch.float16, cuda, init=g.acc)  # dx_accumulate aliases dx
    L.assert_matches(run(inplace.t.data_ptr(), inplace), racc, f"bwd-data in place {case}")


@pytest.mark.parametrize("case", BWD_CASES, ids=str)
def test_backward_data(cuda, case, monkeypatch):
    monkeypatch.setenv("OD_CONV_RDIRECT_MIN_PIXELS", "0")  # small maps reach the weights-resident kernel too
    check_backward_data(cuda, case)


@pytest.mark.parametrize("case", OVERFLOW_BWD, ids=str)
def test_backward_data_overflow_becomes_inf(cuda, case, monkeypatch):
    """The trainer's skip-step logic (od_grad_nonfinite) rests on overflow becoming Inf, not a saturated finite value."""
    monkeypatch.setenv("OD_CONV_RDIRECT_MIN_PIXELS", "0")
    check_backward_data(cuda, case, overflow=True)


@pytest.mark.parametrize("case", OVERFLOW_FWD, ids=str)
def test_forward_overflow_becomes_inf(cuda, case):
    act, resm, cfg = case[7:10]
    g, r = build_fwd(case, overflow=True)
    assert np.isinf(r.ref16).any()
    got = run_conv(cuda, g.x, g.w, g.scale, g.bias, case[6], act, _alpha(act), g.res, resm, cfg)
    L.assert_matches(got, r, f"overflow fwd {case}")


# ------------------------------------------------------------------------------------------------ weight gradient
@pytest.mark.parametrize("case", WGRAD_CASES, ids=str)
def test_weight_gradient(cuda, case):
    """Atomics and slabs + fixed-order reduce, from zero and into a non-zero dw: all == the integer reference."""
    check_weight_gradient(cuda, case, table=tk.WGRAD_KERNEL)


@pytest.mark.parametrize("case", W8_WGRAD_CASES, ids=str)
def test_weight_gradient_256_wide_kernel(cuda, case):
    """od_conv_wgrad_w8: its atomic epilogue from zero and into a non-zero dw, and its slab epilogue == the integer reference."""
    check_weight_gradient(cuda, case, table=W8_WGRAD_KERNEL)


def test_every_weight_gradient_kernel_is_exercised(cuda):
    """The exact case lists reach all four kernels (what the library selects, not what the tables say)."""
    ctx = _ctx(cuda)
    reached = {tk.wgrad_kernel(ctx.lib, ctx.handle, c, slabs) for c in WGRAD_CASES + W8_WGRAD_CASES for slabs in (0, 1)}
    assert reached == ALL_WGRAD_KERNELS, f"never exercised: {sorted(ALL_WGRAD_KERNELS - reached)}, unknown: {sorted(reached - ALL_WGRAD_KERNELS)}"


def check_weight_gradient(cuda, case, atomics=True, table=None):
    from object_detector_amd import _lib
    B, H, W, Cin, Cout, k, stride = case
    ctx = _ctx(cuda)
    lib, h = ctx.lib, ctx.handle
    for slabs in ((False, True) if atomics else (True,)) if table else ():  # before anything is built or launched
        tk.assert_wgrad_kernel(lib, h, case, slabs, table)
    g, dw_ref, dw_acc_ref = build_wgrad(case)
    x, dz = L.poisoned(g.x, cuda), L.poisoned(g.dz, cuda)
    count = Cout * k * k * Cin
    for init, ref in ((np.zeros_like(g.dw0), dw_ref), (g.dw0, dw_acc_ref)) if atomics else ():
        dw = L.Guarded((Cout, k * k * Cin), torch.float32, cuda, init=init)
        _lib.check(lib.od_conv2d_bwd_weight(h, x.data_ptr(), dz.data_ptr(), dw.t.data_ptr(), B, H, W, Cin, Cout, k, stride,
                                            _stream()), "od_conv2d_bwd_weight")
        torch.cuda.synchronize()
        L.assert_equal(dw.numpy("dw"), ref, f"wgrad (atomics) {case}")
    sp = lib.od_conv2d_bwd_weight_splits(h, B, H, W, Cin, Cout, k, stride)
    assert sp >= 1
    slabs = L.Guarded((sp * count,), torch.float32, cuda, init=np.full(sp * count, np.nan, np.float32))
    _lib.check(lib.od_conv2d_bwd_weight_slabs(h, x.data_ptr(), dz.data_ptr(), slabs.t.data_ptr(), B, H, W, Cin, Cout, k, stride,
                                              _stream()), "od_conv2d_bwd_weight_slabs")
    e = _lib.WgradRed()
    e.dw_offset, e.count, e.slabs, e.nslabs = 0, count, slabs.t.data_ptr(), sp
    tbl = torch.frombuffer(bytearray(bytes(e)), dtype=torch.uint8).to(cuda)
    grad = L.Guarded((count,), torch.float32, cuda)
    _lib.check(lib.od_wgrad_reduce_multi(h, tbl.data_ptr(), 1, grad.t.data_ptr(), _stream()), "od_wgrad_reduce_multi")
    torch.cuda.synchronize()
    slabs.check("slabs")
    L.assert_equal(grad.numpy("grad").reshape(Cout, -1), dw_ref, f"wgrad (slabs, {sp} splits) {case}")


@pytest.mark.parametrize("case", FIRST_WGRAD_CASES, ids=str)
def test_first_layer_weight_gradient(cuda, case):
    """Both forms (streaming: W % 32 == 0; widened copy: W = 48), in_scale a power of two, into a non-zero dw."""
    check_first_layer_weight_gradient(cuda, case)


def check_first_layer_weight_gradient(cuda, case):
    from object_detector_amd import _lib
    B, H, W = case
    g, ref = build_first_wgrad(case)
    ctx = _ctx(cuda)
    lib, h = ctx.lib, ctx.handle
    x, dz = L.poisoned(g.x, cuda), L.poisoned(g.dz, cuda)
    nb = lib.od_conv_first_bwd_weight_workspace_bytes(h, B, H, W)
    assert nb > 0
    ws = torch.full((nb,), 0xFF, dtype=torch.uint8, device=cuda)
    dw = L.Guarded((32, 27), torch.float32, cuda, init=g.dw0)
    _lib.check(lib.od_conv_first_bwd_weight(h, x.data_ptr(), dz.data_ptr(), dw.t.data_ptr(), B, H, W, 32, FIRST_IN_SCALE,
                                            ws.data_ptr(), nb, _stream()), "od_conv_first_bwd_weight")
    torch.cuda.synchronize()
    L.assert_equal(dw.numpy("dw"), ref, f"first-layer wgrad {case}")


# ------------------------------------------------------------------------------------------------ bn_partials
@pytest.mark.parametrize("case", BN_CASES, ids=str)
def test_bn_partials_are_the_sums_of_the_stored_z(cuda, case):
    """The conv epilogue's statistics, after the fixed-order row sum of od_bn_stats_from_partials' first step, equal the
    integer sums of the stored f16 z; z itself equals the reference."""
    B, H, W, Cin, Cout, k, stride = case
    g, r, (s1, s2) = build_bn(case)
    z, (part, rows) = run_conv(cuda, g.x, g.w, g.scale, g.bias, stride, bn=True)
    L.assert_matches(z, r, f"bn z {case}")
    p = part.numpy("bn_partials")[:rows * 2 * Cout].reshape(rows, 2, Cout)
    assert np.isfinite(p).all()
    # every row holds exact integers and so does every partial sum of the rows: the f32 row sum is exact in any order
    tot = p.astype(np.float64).sum(0)
    L.assert_equal(tot[0].astype(np.float32), s1, f"sum z {case}")
    L.assert_equal(tot[1].astype(np.float32), s2, f"sum z^2 {case}")
    # and through od_bn_stats_from_partials: mean = sum z / M with gamma = 1, beta = 0 -> shift = -mean * scale
    from object_detector_amd import _lib, weights as Wt
    ctx = _ctx(cuda)
    M = z.size // Cout
    one, zero = torch.ones(Cout, device=cuda), torch.zeros(Cout, device=cuda)
    got = [torch.empty(Cout, device=cuda) for _ in range(4)]
    _lib.check(ctx.lib.od_bn_stats_from_partials(ctx.handle, part.t.data_ptr(), rows, M, Cout, one.data_ptr(), zero.data_ptr(),
                                                 Wt.BN_EPS, *(t.data_ptr() for t in got), None, None, 0.99, _stream()))
    torch.cuda.synchronize()
    # its row sum is exact (integers), and the mean is ONE IEEE f32 multiply of that sum by 1.f / M
    L.assert_equal(got[0].cpu().numpy(), s1 * (np.float32(1.0) / np.float32(M)), f"mean {case}")


def check_bn_partial_rows(cuda, case, rounded=False):
    """The partial rows the epilogue writes, added in float64 on the host (every row holds exact values, see lattice_ref):
    == the sums of the stored f16 z.  rounded: a z the f16 store rounds, sum z only."""
    B, H, W, Cin, Cout, k, stride = case
    g, r, sums = build_bn_rounded(case) if rounded else build_bn_rows(case)
    z, (part, rows) = run_conv(cuda, g.x, g.w, g.scale, g.bias, stride, bn=True)
    L.assert_matches(z, r, f"bn z {case}")
    p = part.numpy("bn_partials")[:rows * 2 * Cout].reshape(rows, 2, Cout).astype(np.float64)
    assert np.isfinite(p).all()
    tot = p.sum(0)
    if rounded:
        L.assert_equal(tot[0], sums, f"sum of the stored (rounded) z {case}")
    else:
        L.assert_equal(tot[0], sums[0], f"sum z {case}")
        L.assert_equal(tot[1], sums[1], f"sum z^2 {case}")


@pytest.mark.parametrize("case", [c for c in BN_CASES if c[5] * c[5] * c[3] >= 576], ids=str)
def test_bn_partials_sum_the_rounded_values_they_store(cuda, case):
    """'partial sums of the f16 values it stores' (include/odhip.h): with a z that the store rounds, sum z must be the sum
    of the ROUNDED values -- the sum of the f32 values before the cast is a different number on most channels."""
    check_bn_partial_rows(cuda, case, rounded=True)


# ------------------------------------------------------------------------------------------------ persistent tile walks
# The direct kernels (csrc/conv_direct.h) are persistent: a workgroup -- in od_conv_rdirect / od_tconv_rdirect a wave --
# walks several tiles, with the next windows in flight.  On a 256-CU part none of the small cases above makes a workgroup
# take a second tile, so the second window buffer, the loader waves' steady state, the counted vmcnt waits and the `xb`
# half of the ping-pong were reached by the tolerance-based full-size tests only.  The shapes here are built from the
# device's CU count and the grid rules of the *_prepare functions so that, on whatever part this runs,
#   every worker takes at least NBUF + 2 tiles (4 where there is no ring): prologue, steady state and drain all run;
#   the work is no whole multiple of the workers: trip counts differ between them.
# (The pointwise od_conv_rdirect forms reach this with the (8, 160, 160, ...) cases of tc.RDIRECT_CASES: 12 800 items for
# 2 x 256 x 8 waves; od_bneck<128> runs one tile per workgroup.)
DIRECT_KERNELS = ({f"od_stem_k<{a}>" for a in range(3)} | {f"od_bneck<{c}, {a}>" for c in (64, 128) for a in range(3)}
                  | {f"od_conv_rdirect<{kc}, {nc}, 1, 1>" for kc, nc in ((64, 32), (32, 64), (128, 64), (64, 128))}
                  | {"od_conv_rdirect<64, 128, 2, 3>", "od_tconv_rdirect<128, 64>", "od_tconv_64_32"}
                  | {"od_conv_stream3<64, 32, 1>", "od_conv_stream3<32, 64, 1>", "od_conv_stream3<32, 64, 2>"})
DIRECT_PREFIXES = ("od_stem_k", "od_bneck", "od_conv_rdirect", "od_tconv_rdirect", "od_conv_stream3", "od_tconv_64_32")
# name -> (units of work per image, workers per CU, least trips per worker, kernel, case builder from the batch)
WALKS = {
    # od_bottleneck_prepare: grid = min(num_cu, tiles), 16 x 16 tiles, two x-window buffers
    "bneck64": (4, 1, 4, "od_bneck<64, 1>", lambda B: (B, 32, 32, 64, "leaky")),
    # od_stem_prepare: grid = min(num_cu, tiles), 32 x 32 input pixels per tile, two uint8 window buffers
    "stem": (4, 1, 4, "od_stem_k<1>", lambda B: ((B, 64, 64), "leaky")),
    # od_conv_rdirect_prepare, 3x3: num_cu workgroups x 8 waves, item = 16 output pixels of a row (Ho = 64, Wo = 16)
    "rdirect3x3": (64, 8, 4, "od_conv_rdirect<64, 128, 2, 3>", lambda B: (B, 128, 32, 64, 128, 3, 2, "leaky", False)),
    # the same grid; item = 16 dZ pixels of a row (dZ 64 x 16); the case is the forward layer's
    "tconv_rdirect": (64, 8, 4, "od_tconv_rdirect<128, 64>", lambda B: (B, 128, 32, 64, 128, 3, 2)),
    # od_conv_stream3_prepare: grid = min(2 num_cu, tiles), 4 x 16 output tiles (Ho = 16, Wo = 32), ring of 3 or 2
    "stream3_64_32": (8, 2, 5, "od_conv_stream3<64, 32, 1>", lambda B: (B, 16, 32, 64, 32, 3, 1, None, "none", -1)),
    "stream3_32_64": (8, 2, 5, "od_conv_stream3<32, 64, 1>", lambda B: (B, 16, 32, 32, 64, 3, 1, "leaky", "none", -1)),
    "stream3_32_64_s2": (8, 2, 5, "od_conv_stream3<32, 64, 2>", lambda B: (B, 32, 64, 32, 64, 3, 2, "elu", "none", -1)),
    # od_tconv_small_prepare: grid = min(2 num_cu, tiles), 4 x 16 dZ tiles (dZ 16 x 32), ring of 3
    "tconv_64_32": (8, 2, 5, "od_tconv_64_32", lambda B: (B, 32, 64, 32, 64, 3, 2)),
}


def walk_batch(units_per_image, workers, trips):
    """The smallest batch whose work gives each of `workers` at least `trips` units and is no multiple of `workers`."""
    assert units_per_image % workers != 0, "an image is a whole number of rounds: no batch gives unequal trip counts"
    B = -(-(trips * workers + 1) // units_per_image)
    while B * units_per_image % workers == 0:
        B += 1
    return B


def assert_walks(work, workers, trips, what, uneven=True):
    assert work > workers and work // workers >= trips and (work % workers != 0 or not uneven), \
        f"{what}: {work} units over {workers} workers is not a walk of >= {trips} units each" + " with unequal trip counts" * uneven


def _plan_kernel(cuda, fill):
    """The kernel a one-op plan resolves to (creation only: nothing is launched, the tensors are one dummy buffer)."""
    from object_detector_amd import _lib
    ctx = _ctx(cuda)
    dummy = torch.zeros(4096, dtype=torch.uint8, device=cuda)
    op = _lib.PlanOp()
    fill(op, dummy.data_ptr())
    h = C.c_void_p()
    _lib.check(ctx.lib.od_plan_create(ctx.handle, (_lib.PlanOp * 1)(op), 1, C.byref(h)), "od_plan_create (one op)")
    try:
        return ctx.lib.od_plan_op_kernel_name(h, 0).decode()
    finally:
        ctx.lib.od_plan_destroy(h)


def conv_kernel(cuda, B, H, W, Cin, Cout, k, stride, act=None, resm="none", cfg=-1, transposed=False):
    from object_detector_amd import _lib

    def fill(op, ptr):
        op.kind, d = _lib.OD_OP_CONV, op.conv
        d.x = d.w = d.scale = d.bias = d.out = ptr
        d.res = ptr if resm != "none" else None
        d.B, d.H, d.W, d.Cin, d.Cout, d.ksize, d.stride = B, H, W, Cin, Cout, k, stride
        d.act, d.alpha = _lib.ACT_ENUM[act], _alpha(act)
        d.res_mode = {"none": _lib.OD_RES_NONE, "same": _lib.OD_RES_SAME, "up2": _lib.OD_RES_UP2}[resm]
        d.out_dtype, d.tile_cfg, d.splitk, d.transposed = _lib.OD_DT_F16, cfg, 1, int(transposed)
    return _plan_kernel(cuda, fill)


def bneck_kernel(cuda, case):
    from object_detector_amd import _lib
    B, H, W, Cc, act = case

    def fill(op, ptr):
        op.kind, d = _lib.OD_OP_BNECK, op.bneck
        d.x = d.w1 = d.scale1 = d.bias1 = d.w3 = d.scale3 = d.bias3 = d.out = ptr
        d.B, d.H, d.W, d.C, d.act, d.alpha = B, H, W, Cc, _lib.ACT_ENUM[act], _alpha(act)
    return _plan_kernel(cuda, fill)


def stem_kernel(cuda, case):
    from object_detector_amd import _lib
    (B, H, W), act = case

    def fill(op, ptr):
        op.kind, d = _lib.OD_OP_STEM, op.stem
        d.x = d.w0 = d.scale0 = d.bias0 = d.w3 = d.scale3 = d.bias3 = d.out = ptr
        d.B, d.H, d.W, d.act, d.alpha = B, H, W, _lib.ACT_ENUM[act], _alpha(act)
    return _plan_kernel(cuda, fill)


def bwd_data_kernel(cuda, case):
    """Backward-data of the forward layer `case`: stride 2 is the transposed launch over the dZ map, stride 1 a forward
    launch with the channels swapped (od_conv2d_bwd_data)."""
    B, H, W, Cin, Cout, k, stride = case
    if stride == 2:
        return conv_kernel(cuda, B, H // 2, W // 2, Cout, Cin, k, 2, transposed=True)
    return conv_kernel(cuda, B, H, W, Cout, Cin, k, 1)


@pytest.mark.parametrize("walk", sorted(WALKS), ids=str)
def test_persistent_walk_takes_several_tiles_per_worker(cuda, walk, monkeypatch):
    monkeypatch.setenv("OD_CONV_RDIRECT_MIN_PIXELS", "0")
    units, per_cu, trips, kernel, make = WALKS[walk]
    workers = per_cu * torch.cuda.get_device_properties(cuda).multi_processor_count
    B = walk_batch(units, workers, trips)
    case = make(B)
    assert_walks(B * units, workers, trips, f"{walk} {case}")  # before anything is built or launched
    if walk == "bneck64":
        assert bneck_kernel(cuda, case) == kernel
        test_bottleneck(cuda, case)
    elif walk == "stem":
        assert stem_kernel(cuda, case) == kernel
        test_stem(cuda, case)
    elif walk == "rdirect3x3":
        assert conv_kernel(cuda, *case[:7], act=case[7]) == kernel
        test_fwd_weights_resident_kernels(cuda, case, monkeypatch)
    elif walk.startswith("stream3"):
        assert conv_kernel(cuda, *case[:7], act=case[7]) == kernel
        test_fwd_every_table_config(cuda, case)
    else:
        assert bwd_data_kernel(cuda, case) == kernel
        check_backward_data(cuda, case)


def test_every_direct_kernel_is_exercised(cuda, monkeypatch):
    """The exact case lists reach all 19 direct kernels: what the library selects for each case, not what a table says."""
    monkeypatch.setenv("OD_CONV_RDIRECT_MIN_PIXELS", "0")
    reached = {bneck_kernel(cuda, c) for c in tb.CASES} | {stem_kernel(cuda, c) for c in STEM_CASES}
    reached |= {conv_kernel(cuda, *c[:7], act=c[7], resm=c[8], cfg=c[9]) for c in tc.CASES}
    reached |= {conv_kernel(cuda, *c[:7], act=c[7], resm="same" if c[8] else "none") for c in tc.RDIRECT_CASES}
    reached |= {bwd_data_kernel(cuda, c) for c in BWD_CASES}
    reached = {n for n in reached if n.startswith(DIRECT_PREFIXES)}
    assert reached == DIRECT_KERNELS, f"never exercised: {sorted(DIRECT_KERNELS - reached)}, unknown: {sorted(reached - DIRECT_KERNELS)}"
