"""The conv kernels compiled per epilogue policy (activation / residual mode / output type as template arguments), bit for
bit on exact-arithmetic inputs, and the kernel each launch resolved to.

od_conv_8ph and od_conv_igemm have one instantiation per policy the forward plans use and one that reads the policy at
run time.  Every case here runs as a ONE-OP PLAN, so the plan's kernel-name query tells which instantiation the library
selected: a launch that should take a compiled policy and silently runs the run-time one fails, and so does a combination
without an instantiation that does not end on the run-time one.  The name must still begin with what bench.py's roofline
parses (`od_conv_8ph<ksize, MF1` / `od_conv_igemm<BM, BN`).

Inputs, poisoned surroundings, guard bands and the comparison are those of test_gpu_conv_exact.py (imported): equality
with the once-rounded float64 reference; the one f16 neighbour on ELU's negative branch is lattice_ref's.  Shapes: B = 3,
10 x 10 maps -> M = 300 = one full tile plus a ragged one at every tile height; Cout = 208 / 200 put the channel bound
inside the last wave column / the last n-tile.  The CPU halves run in tests/test_lattice_epilogue_host.py.
"""
import ctypes as C
import pathlib
import re
import sys

import numpy as np
import pytest
import torch

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))

import lattice_ref as L  # noqa: E402
import test_gpu_conv_exact as E  # noqa: E402

pytestmark = pytest.mark.gpu

NE8 = E.tc.NE8
ACT_CODE = {None: 0, "leaky": 1, "elu": 2}
RES_CODE = {"none": 0, "same": 1, "up2": 2}
RT = -1  # the run-time instantiation


def epi(act, resm, out_f32=False):
    """The policy template argument (conv_common.h): act | res_mode << 2 | out_f32 << 4."""
    return ACT_CODE[act] | (RES_CODE[resm] << 2) | (int(out_f32) << 4)


# ---- the 8-wave kernel: every tile height (cfg NE8 .. NE8 + 3 = BM 256 .. 160), 3x3 and 1x1 --------------------------
# B, H, W, Cin, Cout, k, stride, act, res, cfg
E8_F16_CASES = [(3, 10, 10, 64, 256, k, 1, act, resm, cfg) for cfg in range(NE8, NE8 + 4) for k in (3, 1)
                for act, resm in (("leaky", "same"), ("elu", "up2"))]
E8_F32_CASES = [(3, 10, 10, 64, 208, k, 1, None, "none", cfg) for cfg in range(NE8, NE8 + 4) for k in (3, 1)]
# the fused pointwise layer (256 -> 128): B, H, W, Cin, Cout, k, stride, act, res, act2, cfg
E8_PW_CASES = [(3, 10, 10, 64, 256, k, 1, "leaky", resm, "leaky", cfg) for cfg in range(NE8, NE8 + 4) for k in (3, 1)
               for resm in ("none", "same")]
# one grouped launch, the only caller with per-segment output strides: B, [(H, W)], Cin, Cout, act, out_f32, cfg
E8_GROUPED_CASE = (3, [(10, 10), (6, 6), (4, 4)], 64, 256, "elu", False, NE8)
# ---- the table kernels: the configs the plans use (64 x 64: 3, 6; 64 x 128: 7; 128 x 128: 4, 5), 1x1 and 3x3 -------------
IGEMM_CASES = [(3, 10, 10, 64, cout, k, 1, act, resm, cfg) for cfg in (3, 6, 7, 4, 5) for k in (1, 3) for cout in (64, 200)
               for act, resm in (("leaky", "none"), ("leaky", "same"), ("elu", "up2"))]
IGEMM_TILE = {3: (64, 64), 6: (64, 64), 7: (64, 128), 4: (128, 128), 5: (128, 128)}  # cfg -> BM, BN
# ---- combinations without an instantiation of their own: f32 output with a residual; any f32 output on a table config
#      (the table kernels have the four f16 policies only) ---------------------------------------------------------------
UNSPECIALISED_CASES = [(3, 10, 10, 64, 256, 3, 1, "elu", "same", NE8), (3, 10, 10, 64, 200, 1, 1, "elu", "same", 7),
                       (3, 10, 10, 64, 200, 1, 1, None, "none", 7), (3, 10, 10, 64, 200, 3, 1, "leaky", "none", 5)]


def expected_name(case, out_f32=False, act2=False, off32=True):
    """The kernel a case must resolve to: (regex on the full name, the (BM, BN) / MF1 bench.py reads from its head).
    off32: whether every output offset of the launch fits 31 bits (conv_describe's p.off32); the compiled policies form
    them in 32 bits, so a launch beyond that runs the run-time instantiation (tests/test_gpu_large_offsets.py)."""
    k, act, resm, cfg = case[5], case[7], case[8], case[9]
    e = epi(act, resm, out_f32) if off32 else RT
    if cfg >= NE8:
        mf1 = 4 - (cfg - NE8)
        if act2 is not False:  # fused: 3x3 with leaky first epilogues has its instantiations, the 1x1 form runs the run-time one
            e, e2 = (e, epi(act2, "none")) if (k == 3 and e in (1, 5) and act2 == "leaky") else (RT, RT)
            return f"od_conv_8ph<{k}, {mf1}, {e}, {e2}, true, false>", str(mf1)
        have = {1: (1, 2, 10, 18), 3: (1, 5, 2, 10, 16, 17, 18)}[k]
        return f"od_conv_8ph<{k}, {mf1}, {e if e in have else RT}, -1, false, {'true' if k == 3 else 'false'}>", str(mf1)
    have = (1, 5, 2, 10) if not out_f32 else ()
    bm, bn = IGEMM_TILE[cfg]
    return rf"od_conv_igemm<{bm}, {bn}, 64, \d, \d, \d, {k}, \d, true, \d, false, {e if e in have else RT}>", None


def check_name(name, want, head):
    assert re.fullmatch(want if head is None else re.escape(want), name), f"resolved to {name}, expected {want}"
    m = re.match(r"od_conv_8ph<\d+, (\d+)", name) or re.match(r"od_conv_igemm<(\d+), (\d+)", name)
    assert m, f"{name}: bench.py's roofline cannot read the tile from the head of this name"
    if head is not None:
        assert m.group(1) == head


def run_plan(cuda, d, keep):
    """d as a plan of its own -> the kernel name the plan resolved it to (the launch has completed on return)."""
    from object_detector_amd import _lib
    ctx = E._ctx(cuda)
    op = _lib.PlanOp()
    op.kind = _lib.OD_OP_CONV
    op.conv = d
    arr = (_lib.PlanOp * 1)(op)
    h = C.c_void_p()
    _lib.check(ctx.lib.od_plan_create(ctx.handle, arr, 1, C.byref(h)), "od_plan_create (one op)")
    try:
        name = ctx.lib.od_plan_op_kernel_name(h, 0).decode()
        _lib.check(ctx.lib.od_plan_run(h, E._stream()), "od_plan_run (one op)")
        torch.cuda.synchronize()
    finally:
        ctx.lib.od_plan_destroy(h)
    del keep
    return name


def conv_desc(cuda, g, case, keep, out_f32=False):
    """The descriptor of a forward case on poisoned inputs (the output is the caller's)."""
    from object_detector_amd import _lib
    B, H, W, Cin, Cout, k, stride, act, resm, cfg = case[:10]
    keep += [L.poisoned(g.x, cuda), E._packed(g.w, g.scale, g.bias, cuda)]
    d = _lib.ConvDesc()
    d.x = keep[-2].data_ptr()
    d.w, d.scale, d.bias = (t.data_ptr() for t in keep[-1])
    if g.res is not None:
        keep.append(L.poisoned(g.res, cuda))
        d.res = keep[-1].data_ptr()
    d.B, d.H, d.W, d.Cin, d.Cout, d.ksize, d.stride = B, H, W, Cin, Cout, k, stride
    d.act, d.alpha = _lib.ACT_ENUM[act], float(E._alpha(act))
    d.res_mode = {"none": _lib.OD_RES_NONE, "same": _lib.OD_RES_SAME, "up2": _lib.OD_RES_UP2}[resm]
    d.out_dtype = _lib.OD_DT_F32 if out_f32 else _lib.OD_DT_F16
    d.tile_cfg, d.splitk = cfg, 1
    return d


@pytest.mark.parametrize("case", E8_F16_CASES + IGEMM_CASES, ids=str)
def test_compiled_policy_f16(cuda, case):
    g, r = E.build_fwd(case)
    keep = []
    d = conv_desc(cuda, g, case, keep)
    out = L.Guarded(r.ref16.shape, torch.float16, cuda)
    d.out = out.t.data_ptr()
    name = run_plan(cuda, d, keep)
    L.assert_matches(out.numpy(name), r, f"{name} {case}")
    check_name(name, *expected_name(case))


@pytest.mark.parametrize("case", E8_F32_CASES, ids=str)
def test_f32_logits_into_a_strided_slice(cuda, case):
    """linear / none / f32 through out_batch_stride / out_pix_stride into a slice of a larger [B, P, 26] buffer: equality,
    and everything around the slices untouched.  (The 1x1 form has no instantiation for this policy: run-time kernel.)"""
    B, H, W, Cin, Cout = case[:5]
    P_total, Cc, off = 1200, 26, 150
    g, r = E.build_fwd(case, out_f32=True)
    keep = []
    d = conv_desc(cuda, g, case, keep, out_f32=True)
    pred = L.Guarded((B, P_total, Cc), torch.float32, cuda, init=np.full((B, P_total, Cc), 7.0, np.float32))
    d.out = pred.t.data_ptr() + off * Cc * 4
    d.out_batch_stride, d.out_pix_stride = P_total * Cc, Cout
    name = run_plan(cuda, d, keep)
    got = pred.numpy(name)
    rows = H * W * Cout // Cc
    L.assert_equal(got[:, off:off + rows], r.ref32.reshape(B, rows, Cc), f"{name} {case}")
    assert (got[:, :off] == 7.0).all() and (got[:, off + rows:] == 7.0).all(), "written outside the slice"
    check_name(name, *expected_name(case, out_f32=True))


@pytest.mark.parametrize("case", E8_PW_CASES, ids=str)
def test_fused_pointwise_layer(cuda, case):
    """Both epilogues of the fused kernel: out AND out2 against the chained reference."""
    from object_detector_amd import _lib
    act2 = case[9]
    g, r1, r2 = E.build_pw(case)
    keep = []
    d = conv_desc(cuda, g, case[:9] + (case[10],), keep)
    keep.append(E._packed(g.w2, g.scale2, g.bias2, cuda))
    d.w2, d.scale2, d.bias2 = (t.data_ptr() for t in keep[-1])
    out = L.Guarded(r1.ref16.shape, torch.float16, cuda)
    out2 = L.Guarded(r2.ref16.shape, torch.float16, cuda)
    d.out, d.out2, d.Cout2 = out.t.data_ptr(), out2.t.data_ptr(), g.w2.shape[0]
    d.act2, d.alpha2 = _lib.ACT_ENUM[act2], float(E._alpha(act2))
    name = run_plan(cuda, d, keep)
    L.assert_matches(out.numpy(name), r1, f"{name} out {case}")
    L.assert_matches(out2.numpy(name), r2, f"{name} out2 {case}")
    check_name(name, *expected_name(case[:9] + (case[10],), act2=act2))


def test_grouped_launch(cuda):
    from object_detector_amd import _lib
    case = E8_GROUPED_CASE
    B, dims, Cin, Cout, act, out_f32, cfg = case
    g, xs, rs = E.build_grouped(case)
    keep = [E._packed(g.w, g.scale, g.bias, cuda)] + [L.poisoned(x, cuda) for x in xs]
    outs = [L.Guarded((B, h, w, Cout), torch.float16, cuda) for h, w in dims]
    d = _lib.ConvDesc()
    d.w, d.scale, d.bias = (t.data_ptr() for t in keep[0])
    d.B, d.Cin, d.Cout, d.ksize, d.stride = B, Cin, Cout, 3, 1
    d.act, d.alpha, d.out_dtype = _lib.ACT_ENUM[act], float(E._alpha(act)), _lib.OD_DT_F16
    d.tile_cfg, d.nseg, d.splitk = cfg, len(dims), 1
    for i, (x, o, (h, w)) in enumerate(zip(keep[1:], outs, dims)):
        d.seg_x[i], d.seg_out[i], d.seg_H[i], d.seg_W[i] = x.data_ptr(), o.t.data_ptr(), h, w
    name = run_plan(cuda, d, keep)
    for i, (o, r) in enumerate(zip(outs, rs)):
        L.assert_matches(o.numpy(f"segment {i}"), r, f"{name} segment {i}")
    check_name(name, *expected_name((B, 0, 0, Cin, Cout, 3, 1, act, "none", cfg)))


@pytest.mark.parametrize("case", UNSPECIALISED_CASES, ids=str)
def test_unspecialised_combination_runs_the_run_time_kernel(cuda, case):
    g, r = E.build_fwd(case, out_f32=True)
    keep = []
    d = conv_desc(cuda, g, case, keep, out_f32=True)
    out = L.Guarded(r.ref32.shape, torch.float32, cuda)
    d.out = out.t.data_ptr()
    name = run_plan(cuda, d, keep)
    L.assert_matches32(out.numpy(name), r, f"{name} {case}")
    want, head = expected_name(case, out_f32=True)
    assert "-1" in want
    check_name(name, want, head)
