"""Exact-lattice tests of the lane layouts of the training-side kernels (od_bn_stats, od_bn_bwd, od_scale_act).

train.hip is built without floating-point contraction, so every f32 expression in it is a sequence of correctly rounded IEEE
operations that numpy float32 reproduces.  The inputs sit on a lattice (z = k/4, dy = j/4 with |k|, |j| <= 8; scale = 2,
shift = 0.25, mean = 0.25, rstd = 2; LeakyReLU with alpha = 0.5 or linear) on which every term of every per-channel sum is a
multiple of 1/16 of magnitude <= 9, so every partial sum over up to 4104 rows is an integer multiple of 1/16 below 2^24 / 16:
exactly representable in f32 in ANY summation order.  The expected values therefore restate no reduction tree, and a row or
channel group that a layout slip drops or doubles changes them bit for bit.  ELU goes through the device expf and stays in
the tolerance test (test_gpu_train_kernels.py)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

f32 = np.float32
SCALE, SHIFT, MEAN, RSTD, ALPHA = f32(2), f32(0.25), f32(0.25), f32(2), f32(0.5)
OD_ERR_INVALID = -1  # include/odhip.h

# C -> B of the multi-row case; shapes are (B, 2, 2, C) so that the up2 residual is valid; M = 4 B gives three partial rows
# with a ragged last one
LAYOUTS = {
    8: 1026,    # G=1, 256 row lanes, butterfly over the whole wave
    24: 384,    # G=3 (not a power of two), 85 lanes, one idle thread
    32: 257,    # G=4, the network's narrowest layer
    208: 41,    # G=26, 9 lanes, 22 idle threads
    256: 33,    # G=32, butterfly to two half-waves
    512: 17,    # G=64, first width without the butterfly, 4 lanes
    2048: 5,    # G=256, lanes == 1
}
CASES = [(c, b) for c, b in LAYOUTS.items()] + [(c, 1) for c in LAYOUTS]  # B=1: fewer rows than row lanes, one workgroup
case_ids = [f"C{c}-B{b}" for c, b in CASES]


@functools.lru_cache(maxsize=None)
def lattice(Cn, B):
    """Seeded lattice tensors of one case (computed once, shared by the tests, never written)."""
    rng = np.random.default_rng(1000 * Cn + B)
    d = {"z": (rng.integers(-8, 9, (B, 2, 2, Cn)) / 4).astype(np.float16),
         "dy": (rng.integers(-8, 9, (B, 2, 2, Cn)) / 4).astype(np.float16),
         "res": (rng.integers(-8, 9, (B, 2, 2, Cn)) / 4).astype(np.float16),
         "res_up": (rng.integers(-8, 9, (B, 1, 1, Cn)) / 4).astype(np.float16)}
    for v in d.values():
        v.setflags(write=False)
    return d


def exact_sum(x):
    """Per-channel sum of an f32 [M, C] array whose partial sums are all exact in f32: the f64 sum, checked and cast."""
    s = x.astype(np.float64).sum(0)
    assert (s * 16 == np.round(s * 16)).all() and np.abs(x.astype(np.float64)).sum(0).max() * 16 < 2 ** 24
    return s.astype(f32)


def act_grad(zf, act):
    a = zf * SCALE + SHIFT
    assert (a != 0).all()
    return np.where(a > 0, f32(1), ALPHA).astype(f32) if act == "leaky" else np.ones_like(zf)


def dev(x, cuda):
    return torch.from_numpy(np.array(x)).to(cuda)  # a copy: the lattice arrays are read-only


def full(Cn, v, cuda):
    return torch.full((Cn,), float(v), dtype=torch.float32, device=cuda)


def ctx_of(cuda):
    from object_detector_amd.net import Context
    ctx = Context.get(cuda)
    return ctx.lib, ctx.handle, C.c_void_p(torch.cuda.current_stream().cuda_stream)


def assert_three_partial_rows(lib, M, Cn, B):
    if B > 1:  # a change of the rows-per-workgroup rule must not quietly turn these into single-workgroup cases
        assert lib.od_bn_workspace_bytes(M, Cn) // (8 * Cn) >= 3


@pytest.mark.parametrize("Cn,B", CASES, ids=case_ids)
def test_bn_stats_lattice(cuda, Cn, B):
    from object_detector_amd import train_ops as T
    lib, _h, _s = ctx_of(cuda)
    M = 4 * B
    assert_three_partial_rows(lib, M, Cn, B)
    z = lattice(Cn, B)["z"]
    zf = z.reshape(M, Cn).astype(f32)
    run_mean, run_var = full(Cn, 0, cuda), full(Cn, 0, cuda)
    mean, rstd, scale, shift = (t.cpu().numpy() for t in
                                T.bn_stats(dev(z, cuda), full(Cn, 1, cuda), full(Cn, 0, cuda), 1e-3, run_mean, run_var, 0.0))
    invM = f32(1) / f32(M)
    mu = exact_sum(zf) * invM
    var = np.maximum(exact_sum(zf * zf) * invM - mu * mu, f32(0))
    assert mu.dtype == f32 and var.dtype == f32
    assert np.array_equal(mean, mu)
    assert np.array_equal(run_mean.cpu().numpy(), mean)
    assert np.array_equal(run_var.cpu().numpy(), var)
    # rsqrtf of the device is not correctly rounded: these three against f64 at the tolerance of the parity test
    z64 = zf.astype(np.float64)
    rs64 = 1 / np.sqrt(z64.var(0) + 1e-3)
    np.testing.assert_allclose(rstd, rs64, rtol=1e-4)
    np.testing.assert_allclose(scale, rs64, rtol=1e-4)
    np.testing.assert_allclose(shift, -z64.mean(0) * rs64, rtol=1e-4)


@pytest.mark.parametrize("act", ["leaky", None], ids=["leaky", "linear"])
@pytest.mark.parametrize("Cn,B", CASES, ids=case_ids)
def test_bn_bwd_lattice(cuda, Cn, B, act):
    from object_detector_amd import train_ops as T
    lib, _h, _s = ctx_of(cuda)
    M = 4 * B
    assert_three_partial_rows(lib, M, Cn, B)
    L = lattice(Cn, B)
    zf, dyf = L["z"].reshape(M, Cn).astype(f32), L["dy"].reshape(M, Cn).astype(f32)
    dgamma, dbeta = full(Cn, 3, cuda), full(Cn, -2, cuda)  # pre-filled: the kernel accumulates
    dz, _, _ = T.bn_bwd(dev(L["z"], cuda), dev(L["dy"], cuda), full(Cn, SCALE, cuda), full(Cn, SHIFT, cuda),
                        full(Cn, MEAN, cuda), full(Cn, RSTD, cuda), act, float(ALPHA), bn=True, dgamma=dgamma, dbeta=dbeta)
    da = dyf * act_grad(zf, act)
    xh = (zf - MEAN) * RSTD
    s_da, s_dax = exact_sum(da), exact_sum(da * xh)
    assert np.array_equal(dgamma.cpu().numpy(), f32(3) + s_dax)
    assert np.array_equal(dbeta.cpu().numpy(), f32(-2) + s_da)
    invM = f32(1) / f32(M)
    want = SCALE * ((da - s_da * invM) - xh * (s_dax * invM))  # the operation order of od_bn_bwd_apply_k
    assert want.dtype == f32
    assert np.array_equal(dz.cpu().numpy().reshape(M, Cn), want.astype(np.float16))


BIAS_CASES = CASES + [(2056, 5)]  # G = 257: the second pass of the group loop has one group; the apply pass is the copy
bias_ids = case_ids + ["C2056-B5"]


@pytest.mark.parametrize("alias", [False, True], ids=["separate", "in-place"])
@pytest.mark.parametrize("Cn,B", BIAS_CASES, ids=bias_ids)
def test_bias_layer_bwd_lattice(cuda, Cn, B, alias):
    """bn = 0, linear (the prediction conv): dz = dy bit for bit, dbeta = sum dy; dz may alias dy."""
    from object_detector_amd import _lib
    lib, h, s = ctx_of(cuda)
    M = 4 * B
    assert_three_partial_rows(lib, M, Cn, B)
    L = lattice(Cn, B)
    z, dy = dev(L["z"], cuda), dev(L["dy"], cuda)
    dz = dy if alias else torch.full_like(dy, float("nan"))
    scale, shift = full(Cn, SCALE, cuda), full(Cn, SHIFT, cuda)
    dgamma, dbeta = full(Cn, 0, cuda), full(Cn, 0, cuda)
    wsb = lib.od_bn_workspace_bytes(M, Cn) + 2 * Cn * 4
    ws = torch.empty(wsb, dtype=torch.uint8, device=cuda)
    _lib.check(lib.od_bn_bwd(h, z.data_ptr(), dy.data_ptr(), scale.data_ptr(), shift.data_ptr(), None, None, M, Cn,
                             _lib.OD_ACT_LINEAR, 0.0, 0, dgamma.data_ptr(), dbeta.data_ptr(), dz.data_ptr(), ws.data_ptr(), wsb,
                             s), "od_bn_bwd")
    assert np.array_equal(dz.cpu().numpy().view(np.uint16), L["dy"].view(np.uint16))
    assert np.array_equal(dbeta.cpu().numpy(), exact_sum(L["dy"].reshape(M, Cn).astype(f32)))


@pytest.mark.parametrize("res_mode", ["none", "same", "up2"])
@pytest.mark.parametrize("act", ["leaky", None], ids=["leaky", "linear"])
@pytest.mark.parametrize("Cn,B", CASES, ids=case_ids)
def test_scale_act_lattice(cuda, Cn, B, act, res_mode):
    from object_detector_amd import train_ops as T
    L = lattice(Cn, B)
    res = {"none": None, "same": L["res"], "up2": L["res_up"]}[res_mode]
    y = T.scale_act(dev(L["z"], cuda), full(Cn, SCALE, cuda), full(Cn, SHIFT, cuda), act, float(ALPHA),
                    res=None if res is None else dev(res, cuda), res_mode=res_mode)
    a = L["z"].astype(f32) * SCALE + SHIFT
    want = np.where(a > 0, a, a * ALPHA).astype(f32) if act == "leaky" else a
    if res is not None:
        want = want + res.astype(f32)  # up2 on a 2 x 2 map: the one residual pixel of the image, broadcast
    assert want.dtype == f32
    assert np.array_equal(y.cpu().numpy(), want.astype(np.float16))


def test_pack_weights_backward_layout_needs_cout_multiple_of_8(cuda):
    """The backward-data pack is stored as groups of 8 output channels (od_conv2d_fwd, its only consumer, needs that anyway);
    the forward-only call (one partial 64 x 64 tile per tap) still takes any Cout and writes the f16 weights, nothing else."""
    from object_detector_amd import _lib
    lib, h, s = ctx_of(cuda)
    Cout, Cin, k = 12, 16, 3
    w = (np.random.default_rng(12).integers(-64, 65, (Cout, k * k * Cin)) / 8).astype(np.float32)  # exact in f16
    wd = torch.from_numpy(w).to(cuda)
    wf = torch.zeros(_lib.conv_weight_dims(Cout, Cin, k), dtype=torch.float16, device=cuda)
    wb = torch.zeros(_lib.conv_weight_dims(Cin, Cout, k), dtype=torch.float16, device=cuda)
    assert lib.od_pack_weights(h, wd.data_ptr(), wf.data_ptr(), wb.data_ptr(), Cout, Cin, k, s) == OD_ERR_INVALID
    assert not wf.any() and not wb.any()
    _lib.check(lib.od_pack_weights(h, wd.data_ptr(), wf.data_ptr(), None, Cout, Cin, k, s), "od_pack_weights")  # forward only
    want = np.zeros(tuple(wf.shape), np.float16)
    want[:Cout, :k * k * Cin] = w
    assert np.array_equal(wf.cpu().numpy(), want) and not wb.any()
