"""The only writer of the descriptor structs that cross the C ABI (od_conv_desc, od_bneck_desc, od_stem_desc,
od_wide_desc, od_plan_op of include/odhip.h).  Plain functions: every argument lands in exactly one field, and a field
no argument names stays zero.  Tensor arguments may be torch tensors, raw integer addresses or None.

A new od_conv_desc field is added in _lib.ConvDesc, in conv() here and in tests/test_desc_host.py, nowhere else."""
from __future__ import annotations

from . import _lib

RES_MODES = {"none": _lib.OD_RES_NONE, "same": _lib.OD_RES_SAME, "up2": _lib.OD_RES_UP2}
_OP_MEMBER = {_lib.OD_OP_CONV: "conv", _lib.OD_OP_CONV_FIRST: "conv", _lib.OD_OP_BNECK: "bneck", _lib.OD_OP_STEM: "stem",
              _lib.OD_OP_WIDE: "wide"}


def ptr(t):
    """None -> None, an int (a raw address) -> itself, a tensor -> its data pointer."""
    return t if t is None or isinstance(t, int) else t.data_ptr()


def pad_to(n: int, m: int) -> int:
    """n rounded up to a multiple of m."""
    return (n + m - 1) // m * m


def act_pair(act, alpha=None):
    """None | "linear" | "leaky" | "elu" with an explicit alpha, or a (name, alpha) tuple -> (OD_ACT_* enum, float)."""
    if isinstance(act, (tuple, list)):
        act, alpha = act
    if act not in _lib.ACT_ENUM:
        raise ValueError(f"activation must be one of {sorted(k for k in _lib.ACT_ENUM if k)} or None, got {act!r}")
    return _lib.ACT_ENUM[act], float(alpha or 0.0)


def res_code(mode) -> int:
    """"none" | "same" | "up2" (or the OD_RES_* enum itself) -> OD_RES_* enum."""
    if mode in RES_MODES:
        return RES_MODES[mode]
    if isinstance(mode, int) and mode in RES_MODES.values():
        return mode
    raise ValueError(f"res_mode must be one of {sorted(RES_MODES)}, got {mode!r}")


def set_splitk(d, n, workspace, workspace_bytes):
    """Split-K of a conv descriptor: n partial slabs (0 = the library chooses) in the caller's f32 workspace."""
    d.splitk, d.splitk_workspace, d.splitk_workspace_bytes = n, ptr(workspace), workspace_bytes


def conv(x, w, scale, bias, out, B, H, W, Cin, Cout, ksize, stride=1, act=None, alpha=None, res=None, res_mode="none",
         out_f32=False, out_batch_stride=0, out_pix_stride=0, tile_cfg=-1, transposed=False, then=None, splitk=None,
         bn_partials=None):
    """od_conv_desc of one layer.  then = (w2, scale2, bias2, out2, Cout2, act2[, alpha2]): the pointwise layer that
    consumes `out`; splitk = (n, workspace, workspace_bytes); bn_partials = (ptr, bytes)."""
    d = _lib.ConvDesc()
    d.x, d.w, d.scale, d.bias, d.res, d.out = ptr(x), ptr(w), ptr(scale), ptr(bias), ptr(res), ptr(out)
    d.B, d.H, d.W, d.Cin, d.Cout, d.ksize, d.stride = B, H, W, Cin, Cout, ksize, stride
    d.act, d.alpha = act_pair(act, alpha)
    d.res_mode = res_code(res_mode)
    d.out_dtype = _lib.OD_DT_F32 if out_f32 else _lib.OD_DT_F16
    d.out_batch_stride, d.out_pix_stride = out_batch_stride, out_pix_stride
    d.tile_cfg, d.transposed = tile_cfg, int(transposed)
    if then is not None:
        w2, scale2, bias2, out2, d.Cout2, *act2 = then
        d.w2, d.scale2, d.bias2, d.out2 = ptr(w2), ptr(scale2), ptr(bias2), ptr(out2)
        d.act2, d.alpha2 = act_pair(*act2)
    if splitk is not None:
        set_splitk(d, *splitk)
    if bn_partials is not None:
        d.bn_partials, d.bn_partials_bytes = ptr(bn_partials[0]), bn_partials[1]
    return d


def conv_grouped(xs, dims, outs, w, scale, bias, B, Cin, Cout, act=None, alpha=None, out_f32=False, out_batch_stride=0,
                 out_pix_stride=0, tile_cfg=-1, ksize=3):
    """od_conv_desc of one stride-1 layer over len(xs) <= 3 maps (nseg): xs / outs per map, dims = [(H, W)]."""
    d = _lib.ConvDesc()
    d.w, d.scale, d.bias = ptr(w), ptr(scale), ptr(bias)
    d.B, d.Cin, d.Cout, d.ksize, d.stride = B, Cin, Cout, ksize, 1
    d.act, d.alpha = act_pair(act, alpha)
    d.out_dtype = _lib.OD_DT_F32 if out_f32 else _lib.OD_DT_F16
    d.out_batch_stride, d.out_pix_stride = out_batch_stride, out_pix_stride
    d.tile_cfg = tile_cfg
    d.nseg = len(xs)
    for i, (x, (h, wd), o) in enumerate(zip(xs, dims, outs)):
        d.seg_x[i], d.seg_out[i], d.seg_H[i], d.seg_W[i] = ptr(x), ptr(o), h, wd
    return d


def bneck(x, w1, scale1, bias1, w3, scale3, bias3, out, B, H, W, C, act=None, alpha=None):
    d = _lib.BneckDesc()
    d.x, d.out = ptr(x), ptr(out)
    d.w1, d.scale1, d.bias1 = ptr(w1), ptr(scale1), ptr(bias1)
    d.w3, d.scale3, d.bias3 = ptr(w3), ptr(scale3), ptr(bias3)
    d.B, d.H, d.W, d.C = B, H, W, C
    d.act, d.alpha = act_pair(act, alpha)
    return d


def stem(x, w0, scale0, bias0, w3, scale3, bias3, out, B, H, W, act=None, alpha=None):
    d = _lib.StemDesc()
    d.x, d.out = ptr(x), ptr(out)
    d.w0, d.scale0, d.bias0 = ptr(w0), ptr(scale0), ptr(bias0)
    d.w3, d.scale3, d.bias3 = ptr(w3), ptr(scale3), ptr(bias3)
    d.B, d.H, d.W = B, H, W
    d.act, d.alpha = act_pair(act, alpha)
    return d


def wide(y, res, out32, out16, out_hilo, M, C, H, W, res_f32=False, up2=False):
    d = _lib.WideDesc()
    d.y, d.res, d.out32, d.out16, d.out_hilo = ptr(y), ptr(res), ptr(out32), ptr(out16), ptr(out_hilo)
    d.M, d.C, d.res_f32 = M, C, int(bool(res_f32))
    d.res_up2, d.H, d.W = int(bool(up2)), H, W
    return d


def plan_op(kind, desc):
    """od_plan_op of `kind` (OD_OP_*) holding a copy of its descriptor."""
    op = _lib.PlanOp()
    op.kind = kind
    setattr(op, _OP_MEMBER[kind], desc)
    return op
