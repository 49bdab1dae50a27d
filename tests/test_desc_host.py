"""object_detector_amd/desc.py is the only writer of the descriptor structs: every case here fills the struct by hand, field
by field as the call sites did before they shared the builder, and asserts the builder returns the same bytes -- the
fields a site left at zero included.  ctypes only: no GPU, no library."""
import pytest

from object_detector_amd import _lib, desc

X, WT, SC, BI, RES, OUT = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000  # made-up addresses
W2, SC2, BI2, OUT2, WS, PART = 0x70000, 0x80000, 0x90000, 0xA0000, 0xB0000, 0xC0000


class _Tensor:  # what desc.ptr() needs of a tensor
    def __init__(self, addr):
        self.addr = addr

    def data_ptr(self):
        return self.addr


def same(hand, built):
    assert type(hand) is type(built)
    assert bytes(hand) == bytes(built)


def _plain(stride=1):
    d = _lib.ConvDesc()
    d.x, d.w, d.scale, d.bias = X, WT, SC, BI
    d.res = None
    d.out = OUT
    d.B, d.H, d.W, d.Cin, d.Cout = 2, 12, 20, 64, 128
    d.ksize, d.stride = 3, stride
    d.act, d.alpha = _lib.OD_ACT_LEAKY, float(0.1)
    d.res_mode = _lib.OD_RES_NONE
    d.out_dtype = _lib.OD_DT_F16
    d.out_batch_stride, d.out_pix_stride = 0, 0
    d.tile_cfg = -1
    return d


def test_ptr_pad_to():
    assert desc.ptr(None) is None and desc.ptr(0x1234) == 0x1234 and desc.ptr(_Tensor(0x77)) == 0x77
    assert [desc.pad_to(n, 4) for n in (0, 1, 3, 4, 5, 8)] == [0, 4, 4, 4, 8, 8]
    assert [desc.pad_to(n, 256) for n in (1, 256, 257)] == [256, 256, 512]
    assert desc.pad_to(3200, 64) == 3200 and desc.pad_to(3201, 64) == 3264


def test_act_pair_every_spelling():
    assert desc.act_pair(None) == (_lib.OD_ACT_LINEAR, 0.0)
    assert desc.act_pair(None, 0.0) == (_lib.OD_ACT_LINEAR, 0.0)
    assert desc.act_pair("linear") == (_lib.OD_ACT_LINEAR, 0.0)
    assert desc.act_pair("leaky", 0.1) == (_lib.OD_ACT_LEAKY, 0.1)
    assert desc.act_pair("elu", 1) == (_lib.OD_ACT_ELU, 1.0) and isinstance(desc.act_pair("elu", 1)[1], float)
    assert desc.act_pair(("leaky", 0.1)) == (_lib.OD_ACT_LEAKY, 0.1)
    assert desc.act_pair(("elu", 1.0)) == (_lib.OD_ACT_ELU, 1.0)
    for bad in ("relu", "LEAKY", 1, ("relu", 0.1)):
        with pytest.raises(ValueError):
            desc.act_pair(bad, 0.1)


def test_res_code_strings_and_enums():
    assert desc.RES_MODES == {"none": _lib.OD_RES_NONE, "same": _lib.OD_RES_SAME, "up2": _lib.OD_RES_UP2}
    for name, enum in desc.RES_MODES.items():
        assert desc.res_code(name) == enum and desc.res_code(enum) == enum
    for bad in ("down2", 3, -1, None):
        with pytest.raises(ValueError):
            desc.res_code(bad)


@pytest.mark.parametrize("stride", [1, 2])
def test_conv_plain(stride):
    same(_plain(stride), desc.conv(X, WT, SC, BI, OUT, 2, 12, 20, 64, 128, 3, stride, "leaky", 0.1))
    # the (name, alpha) tuple of net.py, tensors instead of addresses, the residual mode as an enum
    same(_plain(stride), desc.conv(_Tensor(X), _Tensor(WT), _Tensor(SC), _Tensor(BI), _Tensor(OUT), 2, 12, 20, 64, 128, 3,
                                   stride, ("leaky", 0.1), res_mode=_lib.OD_RES_NONE))


@pytest.mark.parametrize("mode,enum", [("same", _lib.OD_RES_SAME), ("up2", _lib.OD_RES_UP2)])
def test_conv_residual(mode, enum):
    d = _plain()
    d.res = RES
    d.res_mode = enum
    same(d, desc.conv(X, WT, SC, BI, OUT, 2, 12, 20, 64, 128, 3, 1, "leaky", 0.1, res=RES, res_mode=mode))
    same(d, desc.conv(X, WT, SC, BI, OUT, 2, 12, 20, 64, 128, 3, 1, ("leaky", 0.1), res=_Tensor(RES), res_mode=enum))


def test_conv_f32_into_pred_slice():
    """The prediction conv: f32 logits with batch / pixel strides into a level's rows of pred, `out` a raw address;
    linear activation whose alpha stays zero."""
    P, Cc, off = 1512, 26, 1152
    d = _lib.ConvDesc()
    d.x, d.w = X, WT
    d.scale, d.bias = SC, BI
    d.out = OUT + off * Cc * 4
    d.B, d.H, d.W, d.Cin, d.Cout, d.ksize, d.stride = 2, 6, 6, 256, 208, 3, 1
    d.act, d.res_mode, d.tile_cfg = _lib.OD_ACT_LINEAR, _lib.OD_RES_NONE, -1
    d.out_dtype = _lib.OD_DT_F32
    d.out_batch_stride, d.out_pix_stride = P * Cc, 208
    same(d, desc.conv(X, WT, SC, BI, OUT + off * Cc * 4, 2, 6, 6, 256, 208, 3, 1, out_f32=True, out_batch_stride=P * Cc,
                      out_pix_stride=208))
    d.tile_cfg = -2  # the inference plan beside other batches in flight
    same(d, desc.conv(X, WT, SC, BI, OUT + off * Cc * 4, 2, 6, 6, 256, 208, 3, 1, None, out_f32=True,
                      out_batch_stride=P * Cc, out_pix_stride=208, tile_cfg=-2))


def test_conv_transposed():
    d = _lib.ConvDesc()
    d.x, d.w, d.scale, d.bias, d.out = X, WT, SC, BI, OUT
    d.res = RES
    d.B, d.H, d.W, d.Cin, d.Cout = 2, 6, 6, 128, 64
    d.ksize, d.stride = 3, 2
    d.act, d.alpha = _lib.OD_ACT_LINEAR, float(0.0)
    d.res_mode = 1
    d.out_dtype = _lib.OD_DT_F16
    d.tile_cfg = -1
    d.transposed = int(True)
    same(d, desc.conv(X, WT, SC, BI, OUT, 2, 6, 6, 128, 64, 3, 2, None, 0.0, res=RES, res_mode="same", transposed=True))


def test_conv_then():
    d = _plain()
    d.w2, d.scale2, d.bias2, d.out2 = W2, SC2, BI2, OUT2
    d.Cout2 = 64
    d.act2, d.alpha2 = _lib.OD_ACT_LEAKY, float(0.1)
    same(d, desc.conv(X, WT, SC, BI, OUT, 2, 12, 20, 64, 128, 3, 1, ("leaky", 0.1),
                      then=(_Tensor(W2), _Tensor(SC2), _Tensor(BI2), _Tensor(OUT2), 64, ("leaky", 0.1))))
    same(d, desc.conv(X, WT, SC, BI, OUT, 2, 12, 20, 64, 128, 3, 1, "leaky", 0.1, then=(W2, SC2, BI2, OUT2, 64, "leaky", 0.1)))
    d.act2, d.alpha2 = _lib.OD_ACT_LINEAR, 0.0  # a linear second layer: alpha2 and pad2_ stay zero
    same(d, desc.conv(X, WT, SC, BI, OUT, 2, 12, 20, 64, 128, 3, 1, "leaky", 0.1, then=(W2, SC2, BI2, OUT2, 64, None)))


def test_conv_splitk():
    d = _plain()
    same(d, desc.conv(X, WT, SC, BI, OUT, 2, 12, 20, 64, 128, 3, 1, "leaky", 0.1, splitk=None))  # splitk stays 0, not 1
    assert d.splitk == 0 and not d.splitk_workspace and d.splitk_workspace_bytes == 0
    d.splitk, d.splitk_workspace, d.splitk_workspace_bytes = 4, WS, 1 << 20
    same(d, desc.conv(X, WT, SC, BI, OUT, 2, 12, 20, 64, 128, 3, 1, "leaky", 0.1, splitk=(4, _Tensor(WS), 1 << 20)))
    d.splitk = 0  # the inference plan: the library chooses, the workspace is set once the largest layer is known
    built = desc.conv(X, WT, SC, BI, OUT, 2, 12, 20, 64, 128, 3, 1, "leaky", 0.1)
    desc.set_splitk(built, 0, WS, 1 << 20)
    same(d, built)


def test_conv_bn_partials():
    d = _lib.ConvDesc()
    d.x, d.w = X, WT
    d.scale, d.bias = SC, BI
    d.out = OUT
    d.B, d.H, d.W, d.Cin, d.Cout, d.ksize, d.stride = 2, 12, 12, 128, 256, 3, 2
    d.act, d.res_mode, d.tile_cfg = _lib.OD_ACT_LINEAR, _lib.OD_RES_NONE, -1
    d.out_dtype = _lib.OD_DT_F16
    d.out_batch_stride, d.out_pix_stride = 0, 0
    d.bn_partials, d.bn_partials_bytes = PART, 4096 * 4
    same(d, desc.conv(X, WT, SC, BI, OUT, 2, 12, 12, 128, 256, 3, 2, bn_partials=(_Tensor(PART), 4096 * 4)))


def test_conv_first_layer_form():
    """The image layer as a plan op: Cin 3, and neither tile_cfg nor the output fields are set."""
    d = _lib.ConvDesc()
    d.x, d.w, d.scale, d.bias, d.out = (X, WT, SC, BI, OUT)
    d.B, d.H, d.W, d.Cin, d.Cout = 2, 96, 96, 3, 32
    d.ksize, d.stride = 3, 1
    d.act, d.alpha = _lib.OD_ACT_LEAKY, float(0.1)
    assert d.tile_cfg == 0
    same(d, desc.conv(X, WT, SC, BI, OUT, 2, 96, 96, 3, 32, 3, 1, ("leaky", 0.1), tile_cfg=0))


@pytest.mark.parametrize("nseg", [3, 2])
def test_conv_grouped(nseg):
    xs, outs, dims = [X, X + 0x100, X + 0x200][:nseg], [OUT, OUT + 0x100, OUT + 0x200][:nseg], [(12, 12), (6, 6), (3, 3)][:nseg]
    d = _lib.ConvDesc()
    d.w, d.scale, d.bias = WT, SC, BI
    d.B, d.Cin, d.Cout, d.ksize, d.stride = 2, 256, 208, 3, 1
    d.act, d.alpha = _lib.OD_ACT_ELU, float(1.0)
    d.out_dtype = _lib.OD_DT_F32
    d.out_batch_stride, d.out_pix_stride = 1512 * 26, 208
    d.tile_cfg = -2
    d.nseg = nseg
    for i, (x, (h, w), o) in enumerate(zip(xs, dims, outs)):
        d.seg_x[i], d.seg_out[i], d.seg_H[i], d.seg_W[i] = x, o, h, w
    if nseg == 2:  # the unused third segment stays zero
        assert not d.seg_x[2] and not d.seg_out[2] and d.seg_H[2] == 0 and d.seg_W[2] == 0
    assert not d.x and not d.out and d.H == 0 and d.W == 0
    same(d, desc.conv_grouped([_Tensor(x) for x in xs], dims, outs, WT, SC, BI, 2, 256, 208, ("elu", 1.0), out_f32=True,
                              out_batch_stride=1512 * 26, out_pix_stride=208, tile_cfg=-2))
    # the per-op wrapper's form: dense f16 outputs, the kernel size taken from the weights
    e = _lib.ConvDesc()
    e.w, e.scale, e.bias = WT, SC, BI
    e.B, e.Cin, e.Cout, e.ksize, e.stride = 2, 256, 208, 1, 1
    e.act, e.alpha = _lib.OD_ACT_LINEAR, float(0.0)
    e.out_dtype = _lib.OD_DT_F16
    e.tile_cfg = -1
    e.nseg = nseg
    for i, (x, (h, w), o) in enumerate(zip(xs, dims, outs)):
        e.seg_x[i], e.seg_out[i], e.seg_H[i], e.seg_W[i] = x, o, h, w
    same(e, desc.conv_grouped(xs, dims, [_Tensor(o) for o in outs], WT, SC, BI, 2, 256, 208, None, 0.0, ksize=1))


def _bneck():
    d = _lib.BneckDesc()
    d.x, d.out = X, OUT
    d.w1, d.scale1, d.bias1 = WT, SC, BI
    d.w3, d.scale3, d.bias3 = W2, SC2, BI2
    d.B, d.H, d.W, d.C = 2, 48, 48, 64
    d.act, d.alpha = _lib.OD_ACT_LEAKY, float(0.1)
    return d


def _stem():
    d = _lib.StemDesc()
    d.x, d.out = X, OUT
    d.w0, d.scale0, d.bias0 = WT, SC, BI
    d.w3, d.scale3, d.bias3 = W2, SC2, BI2
    d.B, d.H, d.W = 2, 96, 64
    d.act, d.alpha = _lib.OD_ACT_LEAKY, float(0.1)
    return d


def _wide(res, res_f32, up2):
    d = _lib.WideDesc()
    d.y = X
    d.res = res
    d.out32 = OUT
    d.out16 = None
    d.out_hilo = OUT2
    d.M, d.C, d.res_f32 = 2 * 6 * 10, 512, int(bool(res_f32))
    d.res_up2, d.H, d.W = int(bool(up2)), 6, 10
    return d


def test_bneck_stem():
    same(_bneck(), desc.bneck(X, WT, SC, BI, W2, SC2, BI2, OUT, 2, 48, 48, 64, ("leaky", 0.1)))
    same(_bneck(), desc.bneck(_Tensor(X), WT, SC, BI, W2, SC2, BI2, _Tensor(OUT), 2, 48, 48, 64, "leaky", 0.1))
    same(_stem(), desc.stem(X, WT, SC, BI, W2, SC2, BI2, OUT, 2, 96, 64, ("leaky", 0.1)))
    same(_stem(), desc.stem(_Tensor(X), WT, SC, BI, W2, SC2, BI2, _Tensor(OUT), 2, 96, 64, "leaky", 0.1))


@pytest.mark.parametrize("res,res_f32,up2", [(None, True, False), (RES, False, False), (RES, True, False), (RES, True, True)])
def test_wide(res, res_f32, up2):
    same(_wide(res, res_f32, up2), desc.wide(X, res, _Tensor(OUT), None, OUT2, 120, 512, 6, 10, res_f32=res_f32, up2=up2))


def test_plan_op_every_kind():
    hand = []
    op = _lib.PlanOp()
    op.kind = _lib.OD_OP_CONV
    op.conv = _plain()
    hand.append((op, _plain()))
    op = _lib.PlanOp()
    op.kind = _lib.OD_OP_CONV_FIRST
    op.conv = _plain(2)
    hand.append((op, _plain(2)))
    op = _lib.PlanOp()
    op.kind = _lib.OD_OP_BNECK
    op.bneck = _bneck()
    hand.append((op, _bneck()))
    op = _lib.PlanOp()
    op.kind = _lib.OD_OP_STEM
    op.stem = _stem()
    hand.append((op, _stem()))
    op = _lib.PlanOp()
    op.kind = _lib.OD_OP_WIDE
    op.wide = _wide(RES, True, True)
    hand.append((op, _wide(RES, True, True)))
    assert [op.kind for op, _d in hand] == [1, 2, 3, 4, 5]
    for op, d in hand:
        same(op, desc.plan_op(op.kind, d))
    with pytest.raises(KeyError):
        desc.plan_op(0, _plain())
