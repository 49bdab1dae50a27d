"""The launches the product actually issues, bit for bit on exact-arithmetic inputs.

tests/test_gpu_conv_exact.py proves each kernel under an explicit tile_cfg.  This file proves the kernel THE LIBRARY
SELECTS at the real shapes: Net is built at the BASELINE inference configs, its ops are de-duplicated by descriptor, and
every distinct op is copied, pointed at lattice tensors (tests/lattice_ref.py) in guard-banded allocations, run as a
ONE-OP PLAN (od_plan_create / od_plan_run: the selection is the plan's own) and compared in full with the float64
reference -- equality, or the one-neighbour rule on ELU's negative branch.  An op keeps its activation (the fused kernels
are compiled per activation); a leaky slope, a run-time field, becomes the dyadic 0.125 except in the single-layer first
convolution.  The kernel names the one-op plans report must be exactly the names the full plans report, so an op type
this file forgot fails instead of being skipped.
"""
import collections
import ctypes as C
import pathlib
import sys

import numpy as np
import pytest
import torch

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))

import lattice_ref as L  # noqa: E402
import test_gpu_conv_exact as E  # noqa: E402

pytestmark = pytest.mark.gpu

# batch, size, overlapped (tile_cfg -2: the throughput pipelines), precision, OD_FUSE_BLOCKS
CONFIGS = [(32, 320, True, "f16", "1"), (16, 640, True, "f16", "1"), (1, 320, False, "f16", "1"),
           (32, 320, True, "f16", "0"), (16, 640, True, "f16", "0"), (1, 320, False, "f16", "0"),
           (32, 320, True, "mixed", "1")]
ACT = {0: None, 1: "leaky", 2: "elu"}
RES = {0: "none", 1: "same", 2: "up2"}
_VERIFIED = {}  # descriptor key -> kernel name: an op verified under one config is not RUN again under another (its
#                 kernel is still resolved under every config's own Net and must be the one that was verified)


def _conv_key(d):
    segs = tuple((d.seg_H[i], d.seg_W[i]) for i in range(d.nseg))
    return ("conv", d.B, d.H, d.W, d.Cin, d.Cout, d.ksize, d.stride, d.act, d.res_mode, d.out_dtype, d.out_batch_stride,
            d.out_pix_stride, bool(d.w2), d.Cout2, d.act2, d.nseg, segs, d.tile_cfg, d.splitk, bool(d.splitk_workspace),
            d.transposed)


def _key(op):
    from object_detector_amd import _lib
    if op.kind == _lib.OD_OP_CONV:
        return _conv_key(op.conv)
    if op.kind == _lib.OD_OP_CONV_FIRST:
        d = op.conv
        return ("first", d.B, d.H, d.W, d.Cout, d.act)
    if op.kind == _lib.OD_OP_BNECK:
        d = op.bneck
        return ("bneck", d.B, d.H, d.W, d.C, d.act)
    if op.kind == _lib.OD_OP_STEM:
        d = op.stem
        return ("stem", d.B, d.H, d.W, d.act)
    d = op.wide
    return ("wide", d.M, d.C, d.res_f32, d.res_up2, d.H if d.res_up2 else 0, d.W if d.res_up2 else 0, bool(d.res),
            bool(d.out32), bool(d.out16), bool(d.out_hilo))


def _run_one(net, op):
    """The op as a plan of its own -> the device kernel the plan resolved it to."""
    from object_detector_amd import _lib
    arr = (_lib.PlanOp * 1)(op)
    h = C.c_void_p()
    _lib.check(net.lib.od_plan_create(net.ctx.handle, arr, 1, C.byref(h)), "od_plan_create (one op)")
    try:
        name = net.lib.od_plan_op_kernel_name(h, 0).decode()
        _lib.check(net.lib.od_plan_run(h, E._stream()), "od_plan_run (one op)")
        torch.cuda.synchronize()
    finally:
        net.lib.od_plan_destroy(h)
    return name


def _resolve(net, op):
    """The kernel the plan resolves the op to under THIS net (creation only, nothing is launched)."""
    from object_detector_amd import _lib
    arr = (_lib.PlanOp * 1)(op)
    h = C.c_void_p()
    _lib.check(net.lib.od_plan_create(net.ctx.handle, arr, 1, C.byref(h)), "od_plan_create (one op)")
    try:
        return net.lib.od_plan_op_kernel_name(h, 0).decode()
    finally:
        net.lib.od_plan_destroy(h)


def _copy(op):
    from object_detector_amd import _lib
    return _lib.PlanOp.from_buffer_copy(bytes(op))


def _slope(act):
    return L.SLOPE if act == "leaky" else 1.0


class _Pred:
    """A stand-in for Net.pred (f32 [B, P, C], guarded, pre-filled) for the ops that write their slice of it."""

    def __init__(self, net, cuda):
        self.net, self.g = net, None
        self.lo, self.hi = net.pred.data_ptr(), net.pred.data_ptr() + net.pred.numel() * 4
        self.cuda = cuda
        self.written = []

    def holds(self, ptr):
        return self.lo <= ptr < self.hi

    def map(self, ptr, rows):
        if self.g is None:
            shape = tuple(self.net.pred.shape)
            self.g = L.Guarded(shape, torch.float32, self.cuda)
            self.g.t.fill_(7.0)
        off = (ptr - self.lo) // 4
        assert off % self.net.C == 0
        self.written.append((off // self.net.C, rows))
        return self.g.t.data_ptr() + off * 4

    def check(self, refs, what):
        got = self.g.numpy(what)
        mask = np.ones(got.shape[1], bool)
        for (row0, rows), ref in zip(self.written, refs):
            L.assert_equal(got[:, row0:row0 + rows], ref.reshape(got.shape[0], rows, got.shape[2]), what)
            mask[row0:row0 + rows] = False
        assert (got[:, mask] == 7.0).all(), f"{what}: pred written outside the op's rows"


def _verify_conv(net, op, cuda):
    from object_detector_amd import _lib
    d = op.conv
    act, resm, out_f32 = ACT[d.act], RES[d.res_mode], d.out_dtype == _lib.OD_DT_F32
    assert not d.transposed and not d.bn_partials
    if act == "leaky":
        d.alpha = L.SLOPE
    keep = []
    pred = _Pred(net, cuda)
    if d.nseg > 1:
        dims = [(d.seg_H[i], d.seg_W[i]) for i in range(d.nseg)]
        g, xs, rs = E.build_grouped((d.B, dims, d.Cin, d.Cout, act, out_f32, d.tile_cfg))
        keep.append(E._packed(g.w, g.scale, g.bias, cuda))
        d.w, d.scale, d.bias = (t.data_ptr() for t in keep[-1])
        outs = []
        for i, (x, (h, w)) in enumerate(zip(xs, dims)):
            keep.append(L.poisoned(x, cuda))
            d.seg_x[i] = keep[-1].data_ptr()
            if pred.holds(d.seg_out[i]):
                assert out_f32
                d.seg_out[i] = pred.map(d.seg_out[i], h * w * d.Cout // net.C)
                outs.append(None)
            else:
                outs.append(L.Guarded((d.B, h, w, d.Cout), torch.float32 if out_f32 else torch.float16, cuda))
                d.seg_out[i] = outs[-1].t.data_ptr()
        name = _run_one(net, op)
        if pred.g is not None:
            pred.check([r.ref32 for r in rs], f"{name} grouped into pred")
        for i, (o, r) in enumerate(zip(outs, rs)):
            if o is not None:
                (L.assert_matches32 if out_f32 else L.assert_matches)(o.numpy(), r, f"{name} segment {i}")
        return name
    case = (d.B, d.H, d.W, d.Cin, d.Cout, d.ksize, d.stride, act, resm)
    if d.w2:
        act2 = ACT[d.act2]
        assert d.Cout2 == d.Cout // 2 and not out_f32
        if act2 == "leaky":
            d.alpha2 = L.SLOPE
        g, r, r2 = E.build_pw(case + (act2, d.tile_cfg))
        keep.append(E._packed(g.w2, g.scale2, g.bias2, cuda))
        d.w2, d.scale2, d.bias2 = (t.data_ptr() for t in keep[-1])
        out2 = L.Guarded(r2.ref16.shape, torch.float16, cuda)
        d.out2 = out2.t.data_ptr()
    else:
        g, r = E.build_fwd(case + (d.tile_cfg,), out_f32=out_f32)
    keep.append(E._packed(g.w, g.scale, g.bias, cuda))
    d.w, d.scale, d.bias = (t.data_ptr() for t in keep[-1])
    keep.append(L.poisoned(g.x, cuda))
    d.x = keep[-1].data_ptr()
    if g.res is not None:
        keep.append(L.poisoned(g.res, cuda))
        d.res = keep[-1].data_ptr()
    out = None
    if pred.holds(d.out or 0):
        assert out_f32
        d.out = pred.map(d.out, r.ref32.shape[1] * r.ref32.shape[2] * d.Cout // net.C)
    else:
        assert d.out_batch_stride == 0 and d.out_pix_stride == 0
        out = L.Guarded(r.ref16.shape, torch.float32 if out_f32 else torch.float16, cuda)
        d.out = out.t.data_ptr()
    name = _run_one(net, op)
    what = f"{name} {case} cfg {d.tile_cfg}"
    if out is None:
        pred.check([r.ref32], what)
    elif out_f32:
        L.assert_matches32(out.numpy(what), r, what)
    else:
        L.assert_matches(out.numpy(what), r, what)
    if d.w2:
        L.assert_matches(out2.numpy(what), r2, what + " out2")
    return name


def _verify_first(net, op, cuda):
    from object_detector_amd.net import pack_first_weight
    d = op.conv
    assert ACT[d.act] == "leaky" and abs(d.alpha - 0.1) < 1e-6 and d.Cout == 32  # a single layer: the product's slope stays
    g, r = E.build_first((d.B, d.H, d.W))
    keep = [L.poisoned(g.x, cuda), E._dev(pack_first_weight(g.w0), cuda), E._dev(g.s0, cuda), E._dev(g.b0, cuda)]
    out = L.Guarded(r.ref16.shape, torch.float16, cuda)
    d.x, d.w, d.scale, d.bias, d.out = (t.data_ptr() for t in keep + [out.t])
    name = _run_one(net, op)
    L.assert_matches(out.numpy(name), r, f"{name} {(d.B, d.H, d.W)}")
    return name


def _verify_bneck(net, op, cuda):
    from object_detector_amd.net import pack_conv_weight, pad_vec
    d = op.bneck
    act = ACT[d.act]
    d.alpha = _slope(act)
    g, r = E.build_bneck((d.B, d.H, d.W, d.C, act))
    w1p, w3p = E._dev(pack_conv_weight(g.w1), cuda), E._dev(pack_conv_weight(g.w3), cuda)
    v = [E._dev(pad_vec(a, n), cuda) for a, n in ((g.s1, w1p.shape[0]), (g.b1, w1p.shape[0]), (g.s3, w3p.shape[0]),
                                                 (g.b3, w3p.shape[0]))]
    x = L.poisoned(g.x, cuda)
    out = L.Guarded(r.ref16.shape, torch.float16, cuda)
    d.x, d.out, d.w1, d.w3 = x.data_ptr(), out.t.data_ptr(), w1p.data_ptr(), w3p.data_ptr()
    d.scale1, d.bias1, d.scale3, d.bias3 = (t.data_ptr() for t in v)
    name = _run_one(net, op)
    L.assert_matches(out.numpy(name), r, f"{name} {(d.B, d.H, d.W, d.C, act)}")
    return name


def _verify_stem(net, op, cuda):
    from object_detector_amd.net import pack_conv_weight, pack_first_weight, pad_vec
    d = op.stem
    act = ACT[d.act]
    d.alpha = _slope(act)
    g, r = E.build_stem(((d.B, d.H, d.W), act))
    w0p, w3p = E._dev(pack_first_weight(g.w0), cuda), E._dev(pack_conv_weight(g.w3), cuda)
    v = [E._dev(g.s0, cuda), E._dev(g.b0, cuda), E._dev(pad_vec(g.s3, w3p.shape[0]), cuda), E._dev(pad_vec(g.b3, w3p.shape[0]), cuda)]
    x = L.poisoned(g.x, cuda)
    out = L.Guarded(r.ref16.shape, torch.float16, cuda)
    d.x, d.out, d.w0, d.w3 = x.data_ptr(), out.t.data_ptr(), w0p.data_ptr(), w3p.data_ptr()
    d.scale0, d.bias0, d.scale3, d.bias3 = (t.data_ptr() for t in v)
    name = _run_one(net, op)
    L.assert_matches(out.numpy(name), r, f"{name} {(d.B, d.H, d.W, act)}")
    return name


def build_wide(M, Cc, res_f32, res_up2, H, W, has_res):
    """od_wide_add on the lattice: y (and an f32 residual) multiples of 2^-7 up to 4096 -- 20 significant bits, so the
    [hi | lo] split has a real low half -- an f16 residual a multiple of 2^-3 up to 256.  The f32 sum is exact (21 bits);
    hi = f16(v) and lo = f16(v - hi) are exact by definition (v - hi is exact in f32)."""
    rng = np.random.default_rng(L.seed_of("wide", M, Cc, res_f32, res_up2, H, W, has_res))
    y = (rng.integers(-(1 << 19), (1 << 19) + 1, (M, Cc)) / 128.0).astype(np.float32)
    res = None
    v = y.astype(np.float64)
    if has_res:
        rshape = (M // (H * W), H // 2, W // 2, Cc) if res_up2 else (M, Cc)
        if res_f32:
            res = (rng.integers(-(1 << 19), (1 << 19) + 1, rshape) / 128.0).astype(np.float32)
        else:
            res = (rng.integers(-2048, 2049, rshape) / 8.0).astype(np.float16)
        r = res.astype(np.float64)
        if res_up2:
            r = L._up2(r).reshape(M, Cc)
        v = v + r
    v32 = v.astype(np.float32)
    assert np.array_equal(v32.astype(np.float64), v), "the f32 sum must be exact"
    with np.errstate(over="ignore"):
        hi = v32.astype(np.float16)
    assert np.isfinite(hi).all()
    lo32 = v32 - hi.astype(np.float32)
    assert np.array_equal(lo32.astype(np.float64), v - hi.astype(np.float64))
    lo = lo32.astype(np.float16)
    assert (lo != 0).mean() > 0.5
    return y, res, v32, hi, np.concatenate([hi, lo], axis=1)


def _verify_wide(net, op, cuda):
    d = op.wide
    y, res, v32, hi, hilo = build_wide(d.M, d.C, d.res_f32, d.res_up2, d.H, d.W, bool(d.res))
    yg = L.Guarded(y.shape, torch.float32, cuda, init=y)   # f32 input: inside a sentinel-filled allocation
    d.y = yg.t.data_ptr()
    keep = [yg]
    if res is not None:
        keep.append(L.Guarded(res.shape, torch.float32, cuda, init=res).t if d.res_f32 else L.poisoned(res, cuda))
        d.res = keep[-1].data_ptr()
    outs = {}
    for fld, ref, dt in (("out32", v32, torch.float32), ("out16", hi, torch.float16), ("out_hilo", hilo, torch.float16)):
        if getattr(d, fld):
            outs[fld] = (L.Guarded(ref.shape, dt, cuda), ref)
            setattr(d, fld, outs[fld][0].t.data_ptr())
    name = _run_one(net, op)
    for fld, (o, ref) in outs.items():
        L.assert_equal(o.numpy(fld), ref, f"{name} {fld} M={d.M} C={d.C}")
    return name


@pytest.mark.parametrize("config", CONFIGS, ids=str)
def test_every_distinct_op_of_the_inference_plan(cuda, config, monkeypatch):
    from object_detector_amd import _lib, weights as Wt
    from object_detector_amd.net import Net
    B, S, overlapped, precision, fuse = config
    monkeypatch.setenv("OD_FUSE_BLOCKS", fuse)
    monkeypatch.delenv("OD_PRECISION", raising=False)
    net = Net(Wt.random_init(2), B, (S, S), device=cuda, overlapped=overlapped, precision=precision)
    verify = {_lib.OD_OP_CONV: _verify_conv, _lib.OD_OP_CONV_FIRST: _verify_first, _lib.OD_OP_BNECK: _verify_bneck,
              _lib.OD_OP_STEM: _verify_stem, _lib.OD_OP_WIDE: _verify_wide}
    reached = collections.Counter()
    distinct = {}
    for op in net.ops:
        distinct.setdefault(_key(op), op)
    for key, op in distinct.items():
        if key not in _VERIFIED:
            _VERIFIED[key] = verify[op.kind](net, _copy(op), cuda)
        else:
            assert _resolve(net, op) == _VERIFIED[key], f"{key}: resolved to another kernel than the one verified"
        reached[_VERIFIED[key]] += 1
    print(f"\n{config}: {len(net.ops)} ops, {len(distinct)} distinct")
    for name, n in sorted(reached.items()):
        print(f"  {name}: {n} distinct ops")
    full = set(net.time_ops()[1])
    assert set(reached) == full, f"kernels never exercised: {sorted(full - set(reached))}; unexpected: {sorted(set(reached) - full)}"


# ------------------------------------------------------------------------------------------------ the training step
TRAIN_SHARDS = [(32, 320), (16, 640)]  # one rank's share of batch 256 at 320^2 and of batch 128 at 640^2


def _verify_train_forward(tr, n, cuda):
    """The raw (identity-epilogue) forward convolution as Trainer.forward issues it: z f16, or for the prediction conv f32
    logits with a bias into the level's rows of pred."""
    from object_detector_amd import _lib
    B = tr.B
    pred = n.pred_off is not None
    case = (B, n.H, n.W, n.Cin, n.Cout, n.k, n.stride, None, "none", -1)
    g = L.gen_conv(("train fwd", case[:7]), B, n.H, n.W, n.Cin, n.Cout, n.k, n.stride,
                   amp=L.amp_for_integer_output(n.k * n.k * n.Cin))  # identity epilogue: z is the bare integer sum
    g.scale = np.ones(n.Cout, np.float32)
    if not pred:
        g.bias = np.zeros(n.Cout, np.float32)
    r = L.ref_forward(g.x, g.w, g.scale, g.bias, n.stride, out_f32=pred, what=f"train fwd {n.name} {case[:7]}")
    keep = [L.poisoned(g.x, cuda), E._packed(g.w, g.scale, g.bias, cuda)]
    if pred:
        out = L.Guarded((B, tr.P, tr.C), torch.float32, cuda)
        out.t.fill_(7.0)
        out_ptr = out.t.data_ptr() + n.pred_off * tr.C * 4
    else:
        out = L.Guarded(r.ref16.shape, torch.float16, cuda)
        out_ptr = out.t.data_ptr()
    # the Trainer's own descriptor of this node; only the pointers are replaced, by the guarded buffers
    d = tr._fwd_desc(n, keep[0], out_ptr, bias=keep[1][2] if pred else None)
    d.x, d.out = keep[0].data_ptr(), out_ptr
    d.w, d.scale, d.bias = (t.data_ptr() for t in keep[1])
    _lib.check(tr.lib.od_conv2d_fwd(tr.ctx.handle, C.byref(d), E._stream()), f"conv fwd {n.name}")
    torch.cuda.synchronize()
    got = out.numpy(n.name)
    if pred:
        L.assert_equal(got[:, n.pred_off:n.pred_off + n.pred_rows], r.ref32.reshape(B, n.pred_rows, tr.C), f"train fwd {n.name}")
        got[:, n.pred_off:n.pred_off + n.pred_rows] = 7.0
        assert (got == 7.0).all(), f"{n.name}: pred written outside the level's rows"
    else:
        L.assert_matches(got, r, f"train fwd {n.name} {case[:7]}")


def _verify_train_first(tr, n, cuda):
    """The image layer: od_conv_first_fwd with a linear epilogue (in_scale a power of two here) and its weight gradient."""
    from object_detector_amd import _lib
    from object_detector_amd.net import pack_first_weight
    B = tr.B
    g = L.gen_stem(("train first", B, n.H, n.W), B, n.H, n.W, None)
    s0, b0 = np.full(32, 2.0 ** -8, np.float32), np.zeros(32, np.float32)
    r = L.ref_conv_first(g.x, g.w0, s0, b0, None, 0.0, what=f"train first fwd {(B, n.H, n.W)}")
    x = L.poisoned(g.x, cuda)
    out = L.Guarded(r.ref16.shape, torch.float16, cuda)
    wp, sc, bi = E._dev(pack_first_weight(g.w0), cuda), E._dev(s0, cuda), E._dev(b0, cuda)
    _lib.check(tr.lib.od_conv_first_fwd(tr.ctx.handle, x.data_ptr(), wp.data_ptr(), sc.data_ptr(), bi.data_ptr(), out.t.data_ptr(),
                                        B, n.H, n.W, 32, _lib.OD_ACT_LINEAR, 0.0, E._stream()), "od_conv_first_fwd")
    torch.cuda.synchronize()
    L.assert_matches(out.numpy("z0"), r, f"train first fwd {(B, n.H, n.W)}")
    E.check_first_layer_weight_gradient(cuda, (B, n.H, n.W))


@pytest.mark.parametrize("shard", TRAIN_SHARDS, ids=str)
def test_every_distinct_layer_of_the_training_step(cuda, shard, monkeypatch):
    """Per distinct layer of the Trainer's node list, with the library's own selection (no size threshold lifted): the raw
    forward convolution (z rounded by the store), the same launch with bn_partials (every partial row exact, the rows added
    in float64 on the host -- lattice_ref.gen_bn, per_row), backward-data (the transposed form for stride 2; plain,
    accumulating and in place) and the slab weight gradient with its fixed-order reduce."""
    from object_detector_amd import weights as Wt
    from object_detector_amd.trainer import Trainer
    monkeypatch.delenv("OD_CONV_RDIRECT_MIN_PIXELS", raising=False)
    B, S = shard
    tr = Trainer(Wt.random_init(2), B, (S, S), device=cuda)
    seen = set()
    for n in tr.nodes:
        key = (n.H, n.W, n.Cin, n.Cout, n.k, n.stride, n.first, n.pred_off, n.need_dx)
        if key in seen:
            continue
        seen.add(key)
        if n.first:
            _verify_train_first(tr, n, cuda)
            continue
        case = (B, n.H, n.W, n.Cin, n.Cout, n.k, n.stride)
        _verify_train_forward(tr, n, cuda)
        if n.pred_off is None:
            E.check_bn_partial_rows(cuda, case)
        if n.need_dx:
            E.check_backward_data(cuda, case)
        E.check_weight_gradient(cuda, case, atomics=False)
    print(f"\n{shard}: {len(tr.nodes)} nodes, {len(seen)} distinct layers")
