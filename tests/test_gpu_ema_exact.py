"""GPU: od_sgd_step_multi_ema and od_ema_update against tests/optim_ref.py and tests/ema_ref.py, bit for bit, through the
C ABI.

w and m are sgd_ref of the inputs (and what od_sgd_step_multi writes from the same inputs); the average is
ema_ref(ema_before, w_new, omd): d = w_new - e; p = omd * d; e + p, three f32 roundings.  Comparisons are on uint32 views with
no tolerance; inputs are optim_ref.values (|x| in [1e-6, 1e3], lr <= 0.1), for which no intermediate is subnormal.  Every
buffer is compared WHOLE: the gaps between segments, the guards around them and the gradient buffer must keep their bits.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import ema_ref as E
import optim_ref as R

pytestmark = pytest.mark.gpu

OD_ERR_INVALID = -1
P32 = 0x4797e880  # 77777.0f: a finite poison, so that an update of a gap element would change it
POISON = np.array([P32], np.uint32).view(np.float32)[0]

SEG_COUNTS = (1, 3, 255, 256, 257, 4100, 65536, 65541, 2 * 65536 + 5)
SEG_LR = (0.1, 0.05, 0.0, 0.02, 0.013, 0.07, 0.001, 0.09, 0.033)
SEG_WD = (1e-4, 2e-4, 5e-5, 0.0, 3e-4, 1e-3, 7e-5, 1e-5, 4e-4)
GUARD = 4096
OMDS = (0.9, 2.0 ** -10, 1e-4, 0.0, 1.0)
MOMENTUM, INV = 0.9, 1.0 / 512.0


def _api(cuda):
    from object_detector_amd.net import Context
    ctx = Context.get(cuda)
    return ctx.lib, ctx.handle


def _s():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _u32(a):
    if isinstance(a, torch.Tensor):
        a = a.cpu().numpy()
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(got, want, what):
    got, want = _u32(got).reshape(-1), _u32(want).reshape(-1)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{what}: {bad.size} of {got.size} differ, first at {bad[0]}: got {got[bad[0]]:#x} want {want[bad[0]]:#x}"


def _flag(cuda, v):
    return torch.tensor([v], dtype=torch.int32, device=cuda)


def _table(cuda, offs, counts, lrs, wds):
    from object_detector_amd import _lib
    raw = b""
    for o, c, lr, wd in zip(offs, counts, lrs, wds):
        sg = _lib.SgdSeg()
        sg.offset, sg.count, sg.lr, sg.weight_decay = int(o), int(c), lr, wd
        raw += bytes(sg)
    return torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(cuda)


def _layout(counts, mod4=None, seed=4):
    """Offsets of the segments in one flat buffer with 4 to 40 poisoned floats between neighbours and GUARD in front and
    behind.  mod4 = None: multiples of 4 (the trainer's); else segment i starts at an offset = mod4[i % len(mod4)] (mod 4)."""
    rng = np.random.default_rng(seed)
    offs, off = [], GUARD
    for i, c in enumerate(counts):
        o = off + (0 if mod4 is None else mod4[i % len(mod4)])
        offs.append(o)
        end = o + c
        off = end + 4 + (-end) % 4 + 4 * int(rng.integers(0, 8))
        assert off % 4 == 0 and 4 <= off - end <= 40
    return offs, off + GUARD


def _case(counts, lrs, wds, mod4=None, seed=8, steps=2):
    """Host buffers (poison outside the segments) and the gradients of `steps` calls."""
    offs, total = _layout(counts, mod4)
    rng = np.random.default_rng(seed)
    w, m, e = (np.full(total, POISON, np.float32) for _ in range(3))
    gs = [np.full(total, POISON, np.float32) for _ in range(steps)]
    for o, c in zip(offs, counts):
        w[o:o + c], m[o:o + c] = R.values(rng, c, -3, 1), R.values(rng, c, -4, 0)
        e[o:o + c] = R.values(rng, c, -3, 1)
        for g in gs:
            g[o:o + c] = R.values(rng, c)
    # half of the last segment's average starts ON the weights, as the trainer's does; a segment with lr = 0 keeps its
    # weights, so an average that equals them is at the fixed point and must keep its bits
    o, c = offs[-1], counts[-1]
    e[o:o + c // 2] = w[o:o + c // 2]
    for o, c, lr in zip(offs, counts, lrs):
        if lr == 0.0:
            e[o:o + c] = w[o:o + c]
    return dict(offs=offs, total=total, counts=counts, lrs=lrs, wds=wds, w=w, m=m, e=e, g=gs)


def _ref_step(cs, w, m, e, g, omd):
    w, m, e = w.copy(), m.copy(), e.copy()
    for o, c, lr, wd in zip(cs["offs"], cs["counts"], cs["lrs"], cs["wds"]):
        w[o:o + c], m[o:o + c] = R.sgd_ref(w[o:o + c], m[o:o + c], g[o:o + c], lr, MOMENTUM, wd, INV)
        e[o:o + c] = E.ema_ref(e[o:o + c], w[o:o + c], omd)
    return w, m, e


@pytest.fixture(scope="module")
def nine():
    cs = _case(SEG_COUNTS, SEG_LR, SEG_WD)
    assert cs["total"] < 300_000 and all(o % 4 == 0 for o in cs["offs"])
    for a in (cs["w"], cs["m"], cs["e"], *cs["g"]):
        a.setflags(write=False)
    return cs


def _dev(cuda, a, skew=0):
    """The host buffer on the device; skew = 1: behind one extra float, so that the base pointer is 4 bytes off a 16-byte
    boundary."""
    t = torch.empty(a.size + skew, dtype=torch.float32, device=cuda)
    assert t.data_ptr() % 16 == 0
    t = t[skew:]
    t.copy_(torch.from_numpy(a.copy()))
    assert t.data_ptr() % 16 == 4 * skew
    return t


def _call(lib, h, w, m, g, e, tbl, nseg, omd, flag=None, momentum=MOMENTUM):
    return lib.od_sgd_step_multi_ema(h, w.data_ptr(), m.data_ptr(), g.data_ptr(), e.data_ptr(), tbl.data_ptr(), nseg,
                                     momentum, INV, omd, None if flag is None else flag.data_ptr(), _s())


def _run_and_check(cuda, cs, omd, skew=(0, 0, 0, 0), what=""):
    lib, h = _api(cuda)
    tbl = _table(cuda, cs["offs"], cs["counts"], cs["lrs"], cs["wds"])
    w, m, e = cs["w"], cs["m"], cs["e"]
    wd_, md_, ed_ = _dev(cuda, w, skew[0]), _dev(cuda, m, skew[1]), _dev(cuda, e, skew[3])
    for step, g in enumerate(cs["g"]):
        gd_ = _dev(cuda, g, skew[2])
        assert _call(lib, h, wd_, md_, gd_, ed_, tbl, len(cs["counts"]), omd) == 0
        e0 = e
        w, m, e = _ref_step(cs, w, m, e, g, omd)
        _same(wd_, w, f"{what} w after call {step}")
        _same(md_, m, f"{what} m after call {step}")
        _same(ed_, e, f"{what} ema after call {step}")
        _same(gd_, g, f"{what} g after call {step}")
        if omd == 0.0:
            _same(ed_, e0, f"{what} ema at omd = 0")
        for o, c, lr in zip(cs["offs"], cs["counts"], cs["lrs"]):
            if lr == 0.0:  # w == e before and after: the fixed point, for every omd
                assert np.array_equal(_u32(e[o:o + c]), _u32(cs["e"][o:o + c])) and np.array_equal(_u32(e[o:o + c]), _u32(w[o:o + c]))
    return w, m, e


@pytest.mark.parametrize("omd", OMDS, ids=str)
def test_fused_nine_segments_two_calls(cuda, nine, omd):
    """The segment counts of test_sgd_multi_exact_two_calls with per-segment lr / weight decay, offsets at multiples of 4 (the
    16-byte path): no body, a body without a tail, ragged tails, one and several trips of the vector loop.  At omd = 0 the
    average keeps its bits; at 1 it is e + (w - e), not always w."""
    w, _m, e = _run_and_check(cuda, nine, omd)
    o, c = nine["offs"][-1], SEG_COUNTS[-1]
    if omd == 1.0:
        assert (e[o:o + c] != w[o:o + c]).any(), "e + (w - e) == w everywhere: the inputs do not tell the two apart"
    if omd in (0.9, 1e-4):
        # the other form of the update, decay * e + omd * w, gives other bits: the test can tell the two apart
        w1, _m1, e1 = _ref_step(nine, nine["w"], nine["m"], nine["e"], nine["g"][0], omd)
        other = np.float32(1.0 - omd) * nine["e"][o:o + c] + np.float32(omd) * w1[o:o + c]
        assert (other.view(np.uint32) != e1[o:o + c].view(np.uint32)).mean() > 0.2


def test_fused_w_and_m_are_those_of_od_sgd_step_multi(cuda, nine):
    lib, h = _api(cuda)
    tbl = _table(cuda, nine["offs"], SEG_COUNTS, SEG_LR, SEG_WD)
    a = [_dev(cuda, nine[k]) for k in ("w", "m")] + [_dev(cuda, nine["g"][0])]
    b = [_dev(cuda, nine[k]) for k in ("w", "m")] + [_dev(cuda, nine["g"][0]), _dev(cuda, nine["e"])]
    assert lib.od_sgd_step_multi(h, a[0].data_ptr(), a[1].data_ptr(), a[2].data_ptr(), tbl.data_ptr(), len(SEG_COUNTS),
                                 MOMENTUM, INV, None, _s()) == 0
    assert _call(lib, h, b[0], b[1], b[2], b[3], tbl, len(SEG_COUNTS), 1e-3) == 0
    _same(b[0], a[0], "w: fused vs od_sgd_step_multi")
    _same(b[1], a[1], "m: fused vs od_sgd_step_multi")
    assert (_u32(b[0]) != _u32(nine["w"])).any()


@pytest.mark.parametrize("skew", [(1, 1, 1, 1), (0, 0, 0, 0), (0, 0, 0, 1), (1, 0, 1, 1)], ids=str)
def test_fused_misaligned_segments(cuda, skew):
    """Offsets = 1, 2, 3 (mod 4).  Base pointers all 4 bytes off a 16-byte boundary (a [1:] slice) or all on one: every
    segment has a scalar head, a 16-byte body and a scalar tail, and the seams are where an element would be lost or done
    twice.  One buffer skewed against the others: no common alignment, the whole segment goes one by one.  Same bits."""
    counts = (1, 2, 3, 4, 5, 6, 7, 8, 9, 255, 256, 257, 1023, 4100, 65541)
    lrs = tuple(0.1 / (1 + i % 5) for i in range(len(counts)))
    wds = tuple(1e-4 * (i % 3) for i in range(len(counts)))
    cs = _case(counts, lrs, wds, mod4=(1, 2, 3), seed=13)
    assert sorted({o % 4 for o in cs["offs"]}) == [1, 2, 3]
    _run_and_check(cuda, cs, 2.0 ** -10, skew=skew, what=f"skew {skew}")


def test_fused_many_small_segments(cuda):
    """3000 segments of 1 to 7 elements, at any offset: heads and tails only, or a body of one vector."""
    rng = np.random.default_rng(31)
    n = 3000
    counts = tuple(int(v) for v in rng.integers(1, 8, n))
    assert set(counts) == set(range(1, 8))
    lrs = tuple(float(v) for v in rng.uniform(1e-3, 0.1, n))
    wds = tuple(float(v) if i % 3 else 0.0 for i, v in enumerate(rng.uniform(1e-5, 1e-3, n)))
    cs = _case(counts, lrs, wds, mod4=(0, 1, 0, 2, 0, 3), seed=14, steps=1)
    _run_and_check(cuda, cs, 1e-4, what="3000 segments")


@pytest.mark.parametrize("flag", [None, 0, 1, -1, 0x100], ids=str)
def test_fused_skip_flag(cuda, nine, flag):
    lib, h = _api(cuda)
    tbl = _table(cuda, nine["offs"], SEG_COUNTS, SEG_LR, SEG_WD)
    w, m, g, e = _dev(cuda, nine["w"]), _dev(cuda, nine["m"]), _dev(cuda, nine["g"][0]), _dev(cuda, nine["e"])
    fl = None if flag is None else _flag(cuda, flag)
    assert _call(lib, h, w, m, g, e, tbl, len(SEG_COUNTS), 0.9, fl) == 0
    if flag:
        want = (nine["w"], nine["m"], nine["e"])
    else:
        want = _ref_step(nine, nine["w"], nine["m"], nine["e"], nine["g"][0], 0.9)
    for got, ref, name in zip((w, m, e), want, ("w", "m", "ema")):
        _same(got, ref, f"{name} flag {flag}")
    _same(g, nine["g"][0], "g")
    if fl is not None:
        assert int(fl.item()) == flag  # the kernel only reads it


def test_fused_argument_checks(cuda, nine):
    lib, h = _api(cuda)
    tbl = _table(cuda, nine["offs"], SEG_COUNTS, SEG_LR, SEG_WD)
    w, m, g, e = _dev(cuda, nine["w"]), _dev(cuda, nine["m"]), _dev(cuda, nine["g"][0]), _dev(cuda, nine["e"])
    n = len(SEG_COUNTS)
    P = lambda t: t.data_ptr()
    ok = dict(ctx=h, w=P(w), m=P(m), g=P(g), ema=P(e), segs=P(tbl), nseg=n, omd=0.5)
    bad = [dict(ctx=None), dict(w=None), dict(m=None), dict(g=None), dict(ema=None), dict(segs=None),
           dict(nseg=0), dict(nseg=-1), dict(nseg=65536),
           dict(omd=-1e-6), dict(omd=1.0 + 2.0 ** -20), dict(omd=float("nan")), dict(omd=float("inf")),
           dict(ema=P(w)), dict(ema=P(m)), dict(ema=P(g))]
    for change in bad:
        a = dict(ok, **change)
        rc = lib.od_sgd_step_multi_ema(a["ctx"], a["w"], a["m"], a["g"], a["ema"], a["segs"], a["nseg"], MOMENTUM, INV, a["omd"],
                                       None, _s())
        assert rc == OD_ERR_INVALID, change
    torch.cuda.synchronize()
    for got, name in ((w, "w"), (m, "m"), (g, "g"), (e, "e")):
        _same(got, nine["g"][0] if name == "g" else nine[name], f"{name} after rejected calls")
    for omd in (0.0, 1.0):  # the ends of the range are valid
        assert _call(lib, h, w, m, g, e, tbl, n, omd) == 0


# ---- od_ema_update -----------------------------------------------------------------------------------------------------
EMA_NS = (1, 3, 4, 5, 255, 256, 257, 1023, 65541, 2 ** 20 + 3)


def _flat_case(n, seed):
    rng = np.random.default_rng(seed)
    e = np.full(n + 2 * 64, POISON, np.float32)
    x = e.copy()
    e[64:64 + n], x[64:64 + n] = R.values(rng, n, -3, 1), R.values(rng, n, -3, 1)
    e[64:64 + n // 2] = x[64:64 + n // 2]  # the fixed point
    return e, x


@pytest.mark.parametrize("skew", [(0, 0), (1, 1), (0, 1)], ids=str)
@pytest.mark.parametrize("omd", [0.9, 2.0 ** -10, 0.0, 1.0], ids=str)
def test_ema_update_exact(cuda, omd, skew):
    """Inside guard bands of 64 poisoned floats; payload 16-byte aligned, 4 bytes off in both buffers (head + body + tail),
    and off in one only (one by one)."""
    lib, h = _api(cuda)
    for n in EMA_NS:
        e, x = _flat_case(n, n)
        ed_, xd_ = _dev(cuda, e, skew[0]), _dev(cuda, x, skew[1])
        assert lib.od_ema_update(h, ed_.data_ptr() + 256, xd_.data_ptr() + 256, n, omd, None, _s()) == 0
        want = e.copy()
        want[64:64 + n] = E.ema_ref(e[64:64 + n], x[64:64 + n], omd)
        _same(ed_, want, f"ema n={n}")
        _same(xd_, x, f"x n={n}")
        if omd == 0.0:
            _same(ed_, e, f"ema n={n} at omd = 0")


@pytest.mark.parametrize("flag", [None, 0, 1, -1, 0x100], ids=str)
def test_ema_update_skip_flag(cuda, flag):
    lib, h = _api(cuda)
    for n in (5, 65541):
        e, x = _flat_case(n, n + 1)
        ed_, xd_ = _dev(cuda, e), _dev(cuda, x)
        fl = None if flag is None else _flag(cuda, flag)
        assert lib.od_ema_update(h, ed_.data_ptr() + 256, xd_.data_ptr() + 256, n, 0.5, None if fl is None else fl.data_ptr(),
                                 _s()) == 0
        want = e.copy()
        if not flag:
            want[64:64 + n] = E.ema_ref(e[64:64 + n], x[64:64 + n], 0.5)
        _same(ed_, want, f"ema n={n} flag {flag}")
        _same(xd_, x, f"x n={n}")
        if fl is not None:
            assert int(fl.item()) == flag


def test_ema_update_argument_checks(cuda):
    lib, h = _api(cuda)
    n = 1023
    e, x = _flat_case(n, 3)
    ed_, xd_ = _dev(cuda, e), _dev(cuda, x)
    pe, px = ed_.data_ptr() + 256, xd_.data_ptr() + 256
    for args in ((None, pe, px, n, 0.5), (h, None, px, n, 0.5), (h, pe, None, n, 0.5), (h, pe, px, 0, 0.5), (h, pe, px, -4, 0.5),
                 (h, pe, px, n, -0.25), (h, pe, px, n, 1.5), (h, pe, px, n, float("nan")), (h, pe, pe, n, 0.5)):
        assert lib.od_ema_update(*args, None, _s()) == OD_ERR_INVALID, args
    torch.cuda.synchronize()
    _same(ed_, e, "ema after rejected calls")
    _same(xd_, x, "x after rejected calls")
