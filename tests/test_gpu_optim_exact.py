"""GPU: od_grad_stats, od_optim_prepare and od_optim_step_multi against tests/optim2_ref.py, bit for bit, through the C ABI.

As test_gpu_optimizer_exact.py: optim.hip is built with -ffp-contract=off, every f32 expression is a sequence of correctly
rounded operations (division and square root included) that numpy float32 reproduces, so results are compared as uint32
views with no tolerance.  Update inputs have magnitudes 10 ** uniform(-4, 2) with lr <= 0.1, so that no intermediate is
subnormal: the smallest is (1 - beta2) * gh**2 >= 1e-3 * (1e-4 * inv)**2 with inv = 1/8, about 1.6e-13.  The one f64 sum
that is compared bit for bit runs over g = k * 2**-10 with integer |k| <= 255, whose squares add exactly in any order.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import ema_ref as E
import optim2_ref as R2
import optim_ref as R

pytestmark = pytest.mark.gpu

OD_ERR_INVALID = -1
P32 = 0x4797e880  # 77777.0f: a finite poison, so that an update of a guard or gap element would change it
KINDS = ("sgd", "nesterov", "adamw")
# 256 x 256 threads per segment: one, two and three sweeps (4 elements per thread and sweep on the 16-byte path)
SEG_COUNTS = (1, 2, 3, 4, 5, 7, 255, 256, 257, 4100, 2 * 65536 + 5, 4 * 65536 + 9, 8 * 65536 + 13)
SEG_LR = (0.1, 0.05, 0.0, 0.02, 0.013, 0.07, 0.001, 0.09, 0.033, 0.1, 0.025, 0.06, 0.004)
SEG_WD = (1e-4, 2e-4, 5e-5, 0.0, 3e-4, 1e-3, 7e-5, 1e-5, 4e-4, 1e-4, 2e-3, 6e-4, 1e-4)
GUARD = 4096
MOM, BETAS, EPS, OMD, INV = 0.9, (0.9, 0.999), 1e-8, 0.01, 0.125


def _api(cuda):
    from object_detector_amd.net import Context
    ctx = Context.get(cuda)
    return ctx.lib, ctx.handle


def _s():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(got, want, what):
    got, want = np.asarray(got).reshape(-1), np.asarray(want).reshape(-1)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{what}: {bad.size} of {got.size} differ, first at {bad[0]}: got {got[bad[0]]:#x} want {want[bad[0]]:#x}"


def _cfg(kind, inv=INV, max_norm=0.0, omd=OMD, momentum=None, beta2=BETAS[1], eps=EPS):
    from object_detector_amd import _lib
    c = _lib.OptimCfg()
    c.kind = R2.KINDS[kind] if isinstance(kind, str) else kind
    c.momentum = (BETAS[0] if kind == "adamw" else MOM) if momentum is None else momentum
    c.beta2, c.eps, c.inv_loss_scale, c.max_grad_norm, c.ema_one_minus_decay = beta2, eps, inv, max_norm, omd
    return c


def _state_tensor(cuda, st):
    from object_detector_amd import _lib
    s = _lib.OptimState()
    for k, v in st.items():
        setattr(s, k, int(v) if k == "step" else float(v))
    return torch.frombuffer(bytearray(bytes(s)), dtype=torch.int32).to(cuda)


def _state_read(t):
    from object_detector_amd import _lib
    s = _lib.OptimState.from_buffer_copy(t.cpu().numpy().tobytes())
    return {k: (int(s.step) if k == "step" else np.float32(getattr(s, k))) for k, _ in _lib.OptimState._fields_}


def _state_same(got, want, what, keys=None):
    for k in keys or want:
        if k == "step":
            assert got[k] == want[k], (what, k, got[k], want[k])
        else:
            a, b = np.float32(got[k]).view(np.uint32), np.float32(want[k]).view(np.uint32)
            assert a == b, f"{what}: {k} got {got[k]!r} ({a:#x}) want {want[k]!r} ({b:#x})"


def _seg_table(cuda, offs, counts, lrs, wds):
    from object_detector_amd import _lib
    raw = b""
    for o, c, lr, wd in zip(offs, counts, lrs, wds):
        sg = _lib.SgdSeg()
        sg.offset, sg.count, sg.lr, sg.weight_decay = o, c, lr, wd
        raw += bytes(sg)
    return torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(cuda)


def _seg_layout():
    """Offsets of the segments in one flat buffer: segment i starts at phase i % 4 of a 16-byte line (all four phases, each
    more than once), 4 to 11 poisoned floats between neighbours, GUARD poisoned floats in front and behind."""
    offs, off = [], GUARD
    for i, c in enumerate(SEG_COUNTS):
        o = off + (i % 4 - off % 4) % 4
        offs.append(o)
        off = o + c + 4 + i % 5
    assert {o % 4 for o in offs} == {0, 1, 2, 3}
    return offs, off + GUARD


def _prepared(n_applied=3):
    """The state after `n_applied` clean od_optim_prepare calls without clipping (restated), so that bc1 / bc2 are not 0."""
    st = R2.new_state()
    for _ in range(n_applied):
        st = R2.prepare_ref(st, 1.0, 0, INV, 0.0, BETAS[0], BETAS[1])
    return st


def _ref_call(kind, ema_on, w, m, v, e, g, offs, st):
    w, m = w.copy(), m.copy()
    v = None if v is None else v.copy()
    e = None if e is None else e.copy()
    for o, c, lr, wd in zip(offs, SEG_COUNTS, SEG_LR, SEG_WD):
        sl = slice(o, o + c)
        nw, nm, nv = R2.step_ref(R2.KINDS[kind], w[sl], m[sl], None if v is None else v[sl], g[sl], np.float32(lr),
                                 BETAS[0] if kind == "adamw" else MOM, BETAS[1], EPS, np.float32(wd), st)
        w[sl], m[sl] = nw, nm
        if v is not None:
            v[sl] = nv
        if ema_on:
            e[sl] = E.ema_ref(e[sl], nw, OMD)
    return w, m, v, e


@pytest.fixture(scope="module")
def seg_case():
    """Host side of the segmented buffers, shared and read-only: poison everywhere but in the segments."""
    offs, total = _seg_layout()
    rng = np.random.default_rng(17)
    poison = np.array([P32], np.uint32).view(np.float32)[0]
    w0, m0, v0, e0, g1, g2 = (np.full(total, poison, np.float32) for _ in range(6))
    for o, c in zip(offs, SEG_COUNTS):
        w0[o:o + c], m0[o:o + c], e0[o:o + c] = R.values(rng, c, -3, 1), R.values(rng, c, -4, 0), R.values(rng, c, -3, 1)
        v0[o:o + c] = np.abs(R.values(rng, c, -4, 0))  # a second moment is not negative
        g1[o:o + c], g2[o:o + c] = R.values(rng, c, -4, 2), R.values(rng, c, -4, 2)
    for a in (w0, m0, v0, e0, g1, g2):
        a.setflags(write=False)
    return dict(offs=offs, total=total, w0=w0, m0=m0, v0=v0, e0=e0, g=(g1, g2), st=_prepared())


def _device_case(cuda, c, kind, ema_on, skew_v=0, skew_e=0):
    """Device copies; skew_*: that buffer sits `skew` floats off the others' 16-byte phase (a view into a longer tensor)."""
    def up(a, skew=0):
        t = torch.full((c["total"] + 4,), 0.0, dtype=torch.float32, device=cuda)
        t = t[skew:skew + c["total"]]
        t.copy_(torch.from_numpy(a.copy()))
        return t
    w, m = up(c["w0"]), up(c["m0"])
    v = up(c["v0"], skew_v) if kind == "adamw" else None
    e = up(c["e0"], skew_e) if ema_on else None
    return w, m, v, e


def _call(lib, h, cfg, w, m, v, g, e, tbl, nseg, st, skip=None):
    return lib.od_optim_step_multi(h, C.byref(cfg), w.data_ptr(), m.data_ptr(), None if v is None else v.data_ptr(),
                                   g.data_ptr(), None if e is None else e.data_ptr(), tbl.data_ptr(), nseg, st.data_ptr(),
                                   None if skip is None else skip.data_ptr(), _s())


def _run_two_calls(cuda, c, kind, ema_on, skew_v=0, skew_e=0):
    lib, h = _api(cuda)
    tbl = _seg_table(cuda, c["offs"], SEG_COUNTS, SEG_LR, SEG_WD)
    w, m, v, e = _device_case(cuda, c, kind, ema_on, skew_v, skew_e)
    st_d = _state_tensor(cuda, c["st"])
    rw, rm, rv, re = c["w0"], c["m0"], (c["v0"] if kind == "adamw" else None), (c["e0"] if ema_on else None)
    for call in range(2):
        g = torch.from_numpy(c["g"][call].copy()).to(cuda)
        assert _call(lib, h, _cfg(kind), w, m, v, g, e, tbl, len(SEG_COUNTS), st_d) == 0
        rw, rm, rv, re = _ref_call(kind, ema_on, rw, rm, rv, re, c["g"][call], c["offs"], c["st"])
        what = f"{kind} ema={ema_on} call {call}"
        _same(_u32(w.cpu().numpy()), _u32(rw), what + ": w")   # whole buffers: gaps and guards keep the poison
        _same(_u32(m.cpu().numpy()), _u32(rm), what + ": m")
        _same(_u32(g.cpu().numpy()), _u32(c["g"][call]), what + ": g")
        if rv is not None:
            _same(_u32(v.cpu().numpy()), _u32(rv), what + ": v")
        if re is not None:
            _same(_u32(e.cpu().numpy()), _u32(re), what + ": ema")
    _state_same(_state_read(st_d), c["st"], "the state is only read")
    return rw, rm


@pytest.mark.parametrize("ema_on", [False, True], ids=["plain", "ema"])
@pytest.mark.parametrize("kind", KINDS)
def test_step_multi_exact_two_calls(cuda, seg_case, kind, ema_on):
    """Every kind, without and with the average, two consecutive calls on 13 segments at all four 16-byte phases, one with
    lr = 0 and one with weight decay = 0; gaps, guards and g bit-identical afterwards."""
    rw, rm = _run_two_calls(cuda, seg_case, kind, ema_on)
    o, n = seg_case["offs"][2], SEG_COUNTS[2]  # lr = 0: the weights stay, the first moment moves
    assert np.array_equal(rw[o:o + n], seg_case["w0"][o:o + n]) and not np.array_equal(rm[o:o + n], seg_case["m0"][o:o + n])
    assert SEG_WD[3] == 0.0 and SEG_LR[2] == 0.0


@pytest.mark.parametrize("which", ["v", "ema"])
def test_step_multi_mixed_phase_goes_elementwise(cuda, seg_case, which):
    """v (or ema) one float off the phase of w: every segment takes the element-wise path, same bits."""
    _run_two_calls(cuda, seg_case, "adamw", True, skew_v=1 if which == "v" else 0, skew_e=3 if which == "ema" else 0)


@pytest.mark.parametrize("flag", [None, 0, 1, -1, 0x100], ids=str)
@pytest.mark.parametrize("kind", KINDS)
def test_step_multi_skip_flag(cuda, seg_case, kind, flag):
    lib, h = _api(cuda)
    c = seg_case
    tbl = _seg_table(cuda, c["offs"], SEG_COUNTS, SEG_LR, SEG_WD)
    w, m, v, e = _device_case(cuda, c, kind, True)
    g = torch.from_numpy(c["g"][0].copy()).to(cuda)
    fl = None if flag is None else torch.tensor([flag], dtype=torch.int32, device=cuda)
    assert _call(lib, h, _cfg(kind), w, m, v, g, e, tbl, len(SEG_COUNTS), _state_tensor(cuda, c["st"]), fl) == 0
    if flag:
        want = (c["w0"], c["m0"], c["v0"] if kind == "adamw" else None, c["e0"])
    else:
        want = _ref_call(kind, True, c["w0"], c["m0"], c["v0"] if kind == "adamw" else None, c["e0"], c["g"][0], c["offs"],
                         c["st"])
    for t, r, nm in zip((w, m, v, e), want, "w m v ema".split()):
        if r is not None:
            _same(_u32(t.cpu().numpy()), _u32(r), nm)
    if fl is not None:
        assert int(fl.item()) == flag  # only read


def test_step_multi_argument_checks(cuda, seg_case):
    """Each rejected call returns OD_ERR_INVALID and writes nothing."""
    lib, h = _api(cuda)
    c = seg_case
    n = len(SEG_COUNTS)
    tbl = _seg_table(cuda, c["offs"], SEG_COUNTS, SEG_LR, SEG_WD)
    w, m, v, e = _device_case(cuda, c, "adamw", True)
    g = torch.from_numpy(c["g"][0].copy()).to(cuda)
    st = _state_tensor(cuda, c["st"])
    nan = float("nan")
    bad = [
        (_cfg(3), w, m, v, g, e, n), (_cfg(-1), w, m, None, g, e, n),                    # unknown kind
        (_cfg("adamw"), w, m, v, g, e, 0), (_cfg("adamw"), w, m, v, g, e, 65536),        # nseg
        (_cfg("adamw"), w, m, None, g, e, n), (_cfg("sgd"), w, m, v, g, e, n),           # v against the kind
        (_cfg("nesterov"), w, m, v, g, e, n),
        (_cfg("adamw"), w, m, v, g, w, n), (_cfg("adamw"), w, m, v, g, m, n),            # ema aliases
        (_cfg("adamw"), w, m, v, g, v, n), (_cfg("adamw"), w, m, v, g, g, n),
        (_cfg("adamw", omd=-0.01), w, m, v, g, e, n), (_cfg("adamw", omd=1.01), w, m, v, g, e, n),
        (_cfg("adamw", omd=nan), w, m, v, g, e, n),
        (_cfg("adamw", momentum=1.0), w, m, v, g, e, n), (_cfg("adamw", momentum=-0.1), w, m, v, g, e, n),
        (_cfg("adamw", beta2=1.0), w, m, v, g, e, n), (_cfg("adamw", beta2=nan), w, m, v, g, e, n),
        (_cfg("sgd", momentum=1.0), w, m, None, g, e, n), (_cfg("nesterov", momentum=nan), w, m, None, g, e, n),
        (_cfg("adamw", eps=0.0), w, m, v, g, e, n), (_cfg("adamw", eps=-1e-8), w, m, v, g, e, n),
    ]
    for i, (cfg, *bufs, nseg) in enumerate(bad):
        assert _call(lib, h, cfg, *bufs[:5], tbl, nseg, st) == OD_ERR_INVALID, f"bad call {i} was accepted"
    torch.cuda.synchronize()
    for t, r, nm in zip((w, m, v, e, g), (c["w0"], c["m0"], c["v0"], c["e0"], c["g"][0]), "w m v ema g".split()):
        _same(_u32(t.cpu().numpy()), _u32(r), f"{nm} after rejected calls")
    # an SGD kind does not look at beta2 / eps
    assert _call(lib, h, _cfg("sgd", beta2=7.0, eps=-1.0), w, m, None, g, None, tbl, n, st) == 0


@pytest.mark.parametrize("ema_on", [False, True], ids=["plain", "ema"])
def test_sgd_kind_without_clipping_is_sgd_step_multi(cuda, seg_case, ema_on):
    """OD_OPT_SGD with clip_coef = 1 against od_sgd_step_multi[_ema] on the same buffers: bit-identical w and m."""
    lib, h = _api(cuda)
    c = seg_case
    n = len(SEG_COUNTS)
    tbl = _seg_table(cuda, c["offs"], SEG_COUNTS, SEG_LR, SEG_WD)
    st = _state_tensor(cuda, c["st"])
    assert np.float32(c["st"]["inv_scale_eff"]) == np.float32(INV) and np.float32(c["st"]["clip_coef"]) == 1.0
    w, m, _v, e = _device_case(cuda, c, "sgd", ema_on)
    w2, m2, _v2, e2 = _device_case(cuda, c, "sgd", ema_on)
    for call in range(2):
        g = torch.from_numpy(c["g"][call].copy()).to(cuda)
        assert _call(lib, h, _cfg("sgd"), w, m, None, g, e, tbl, n, st) == 0
        if ema_on:
            assert lib.od_sgd_step_multi_ema(h, w2.data_ptr(), m2.data_ptr(), g.data_ptr(), e2.data_ptr(), tbl.data_ptr(), n,
                                             MOM, INV, OMD, None, _s()) == 0
            _same(_u32(e.cpu().numpy()), _u32(e2.cpu().numpy()), f"ema call {call}")
        else:
            assert lib.od_sgd_step_multi(h, w2.data_ptr(), m2.data_ptr(), g.data_ptr(), tbl.data_ptr(), n, MOM, INV, None,
                                         _s()) == 0
        _same(_u32(w.cpu().numpy()), _u32(w2.cpu().numpy()), f"w call {call}")
        _same(_u32(m.cpu().numpy()), _u32(m2.cpu().numpy()), f"m call {call}")


# ---- od_grad_stats + od_optim_prepare -----------------------------------------------------------------------------------
def _groups(lib, n):
    """Workgroups of od_grad_stats's launch for n elements: one f64 partial each."""
    b = lib.od_grad_stats_workspace_bytes(n)
    assert b > 0 and b % 8 == 0
    return b // 8


def _stat_sizes(lib):
    """1 .. 1025, then n = 4 * 256 * G + 3 with G the launch's own workgroup count: the smallest such n (G = 1, three tail
    elements) and the one built from the largest G the code ever launches; and, so that the grid-stride loop wraps whatever
    a workgroup takes per sweep, a little more than twice the smallest n that launches that largest G."""
    gmax = _groups(lib, 1 << 40)
    fixed = [n for n in (4 * 256 * G + 3 for G in range(1, 8)) if 4 * 256 * _groups(lib, n) + 3 == n]
    assert fixed, "no n = 4 * 256 * G(n) + 3"
    lo, hi = 1, 1 << 40  # smallest n with G(n) == gmax: every workgroup has a full sweep there
    while lo < hi:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if _groups(lib, mid) == gmax else (mid + 1, hi)
    wraps = 2 * lo + 4 * 300 + 3
    assert _groups(lib, wraps) == gmax and wraps < 1 << 25
    return [1, 2, 3, 4, 5, 255, 1025, fixed[0], 4 * 256 * gmax + 3, wraps]


def _stats(lib, h, cuda, g_host, n, guard=64):
    """od_grad_stats on g_host inside poisoned guards.  -> (flag, partials f64 [G], device tensors to reuse)"""
    G = _groups(lib, n)
    buf = torch.full((n + 2 * guard,), float(np.array([P32], np.uint32).view(np.float32)[0]), dtype=torch.float32, device=cuda)
    buf[guard:guard + n] = torch.from_numpy(g_host)
    ws = torch.full((G + 2,), -1.0, dtype=torch.float64, device=cuda)
    flag = torch.tensor([7], dtype=torch.int32, device=cuda)  # stale: the call clears it
    assert lib.od_grad_stats(h, buf.data_ptr() + 4 * guard, n, flag.data_ptr(), ws.data_ptr() + 8, _s()) == 0
    wsh = ws.cpu().numpy()
    assert wsh[0] == -1.0 and wsh[-1] == -1.0, "a partial was written outside the workspace"
    _same(_u32(buf.cpu().numpy()[guard:guard + n]), _u32(g_host), "g is only read")
    return int(flag.item()), wsh[1:-1], (flag, ws)


def _exact_g(rng, n):
    return (rng.integers(-255, 256, n).astype(np.float32) * np.float32(2.0 ** -10)).astype(np.float32)


@pytest.mark.parametrize("max_norm", [0.0, "above", "below"], ids=str)
def test_grad_stats_prepare_exact(cuda, max_norm):
    """Exact-arithmetic inputs: grad_norm, clip_coef, inv_scale_eff and, after three calls, step / b1pow / b2pow / bc1 / bc2
    equal prepare_ref bit for bit, at every size; once without clipping, once with the norm above max_grad_norm and once
    with it below."""
    lib, h = _api(cuda)
    rng = np.random.default_rng(5)
    inv = 1.0 / 64.0
    for n in _stat_sizes(lib):
        st_ref = R2.new_state()
        st_d = _state_tensor(cuda, st_ref)
        for call in range(3):
            g = _exact_g(rng, n)
            if not g.any():
                g[0] = np.float32(2.0 ** -10)
            flag_ref, s_ref = R2.grad_stats_ref(g)
            true_norm = float(np.sqrt(s_ref)) * inv
            mx = {0.0: 0.0, "above": 0.5 * true_norm, "below": 3.0 * true_norm}[max_norm]
            flag, partials, (flag_d, ws) = _stats(lib, h, cuda, g, n)
            assert flag == flag_ref == 0
            assert float(partials.sum()) == float(s_ref), (n, partials.sum(), s_ref)  # exact in any order
            cfg = _cfg("adamw", inv=inv, max_norm=mx)
            assert lib.od_optim_prepare(h, C.byref(cfg), ws.data_ptr() + 8, n, flag_d.data_ptr(), st_d.data_ptr(), _s()) == 0
            st_ref = R2.prepare_ref(st_ref, s_ref, 0, inv, np.float32(mx), BETAS[0], BETAS[1])
            _state_same(_state_read(st_d), st_ref, f"n={n} call {call} max_norm={max_norm}")
            coef = float(st_ref["clip_coef"])
            assert {0.0: coef == 1.0, "above": 0.4 < coef < 0.6, "below": coef == 1.0}[max_norm], coef
        assert st_ref["step"] == 3


@pytest.mark.parametrize("bad", [np.inf, -np.inf, np.nan], ids=str)
def test_grad_stats_nonfinite_leaves_the_bias_correction(cuda, bad):
    """Inf / -Inf / NaN at the first element, the last vector element and in the tail: the flag is 1 and step, b1pow, b2pow,
    bc1, bc2 keep their values."""
    lib, h = _api(cuda)
    rng = np.random.default_rng(6)
    n = 4 * 700 + 3
    keep = ("step", "b1pow", "b2pow", "bc1", "bc2")
    st0 = _prepared(2)
    for where in (0, 4 * 700 - 1, n - 1, n - 3):
        g = _exact_g(rng, n)
        g[where] = bad
        st_d = _state_tensor(cuda, st0)
        flag, _partials, (flag_d, ws) = _stats(lib, h, cuda, g, n)
        assert flag == 1, where
        assert lib.od_optim_prepare(h, C.byref(_cfg("adamw", max_norm=1.0)), ws.data_ptr() + 8, n, flag_d.data_ptr(),
                                    st_d.data_ptr(), _s()) == 0
        _state_same(_state_read(st_d), st0, f"{bad} at {where}", keys=keep)
        assert int(flag_d.item()) == 1
    # and a clean call right behind counts one step
    g = _exact_g(rng, n)
    flag, _p, (flag_d, ws) = _stats(lib, h, cuda, g, n)
    assert flag == 0
    assert lib.od_optim_prepare(h, C.byref(_cfg("adamw")), ws.data_ptr() + 8, n, flag_d.data_ptr(), st_d.data_ptr(), _s()) == 0
    assert _state_read(st_d)["step"] == st0["step"] + 1


def test_grad_stats_gaussian_is_reproducible_and_accurate(cuda):
    """2**20 Gaussian elements: two runs give the same bits (a float atomic would not), and the f64 sum is within
    n * 2**-53 relative of numpy's: the bound n f64 additions of non-negative terms give."""
    lib, h = _api(cuda)
    n = 1 << 20
    g = np.random.default_rng(9).normal(0, 1, n).astype(np.float32)
    _f, p1, _ = _stats(lib, h, cuda, g, n)
    _f, p2, _ = _stats(lib, h, cuda, g, n)
    _same(p1.view(np.uint64), p2.view(np.uint64), "partials of two runs")
    s = 0.0
    for x in p1:  # ascending, as od_optim_prepare adds them
        s += float(x)
    _flag, want = R2.grad_stats_ref(g)
    rel = abs(s - float(want)) / float(want)
    print(f"sum of squares: device {s!r} numpy {float(want)!r} relative difference {rel:.3e} bound {n * 2.0 ** -53:.3e}")
    assert rel <= n * 2.0 ** -53


def test_grad_stats_argument_checks(cuda):
    lib, h = _api(cuda)
    g = torch.zeros(64, dtype=torch.float32, device=cuda)
    ws = torch.zeros(4, dtype=torch.float64, device=cuda)
    flag = torch.tensor([5], dtype=torch.int32, device=cuda)
    assert lib.od_grad_stats(h, g.data_ptr() + 4, 16, flag.data_ptr(), ws.data_ptr(), _s()) == OD_ERR_INVALID  # g alignment
    assert lib.od_grad_stats(h, g.data_ptr(), 0, flag.data_ptr(), ws.data_ptr(), _s()) == OD_ERR_INVALID
    assert lib.od_grad_stats(h, g.data_ptr(), 16, flag.data_ptr(), None, _s()) == OD_ERR_INVALID
    st = _state_tensor(cuda, R2.new_state())
    assert lib.od_optim_prepare(h, C.byref(_cfg(9)), ws.data_ptr(), 16, flag.data_ptr(), st.data_ptr(), _s()) == OD_ERR_INVALID
    assert lib.od_optim_prepare(h, C.byref(_cfg("adamw", beta2=1.0)), ws.data_ptr(), 16, flag.data_ptr(), st.data_ptr(),
                                _s()) == OD_ERR_INVALID
    torch.cuda.synchronize()
    assert int(flag.item()) == 5 and lib.od_grad_stats_workspace_bytes(0) == 0
    _state_same(_state_read(st), R2.new_state(), "state after rejected calls")
