"""GPU: the kernels that turn a gradient buffer into the next step's weights, each against tests/optim_ref.py, bit for bit,
through the C ABI:

  od_sgd_step, od_sgd_step_multi, od_grad_nonfinite, od_copy_if_nonzero, od_cast_f32_bf16 / od_cast_bf16_f32, od_add_f16,
  od_down2_sum_add, od_pack_weights, od_pack_weights_multi

optim.hip and train.hip are built with -ffp-contract=off, so every f32 expression is a sequence of correctly rounded operations that
numpy float32 reproduces: results are compared as uint32 / uint16 views (signed zeros count), with no tolerance anywhere.
Input magnitudes are 10 ** uniform(-6, 3) with a random sign and lr <= 0.1, so that no input, intermediate or result of the
f32 arithmetic is subnormal.  Every output lies inside a larger buffer whose guards on both sides are compared too.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import optim_ref as R

pytestmark = pytest.mark.gpu

OD_ERR_INVALID = -1
P32 = 0x4797e880  # 77777.0f: a finite poison, so that an update of a guard element would change it
P16 = 0x7dad      # an f16 NaN no kernel here produces
_T = {4: (torch.int32, np.int32, np.uint32), 2: (torch.int16, np.int16, np.uint16)}


def _api(cuda):
    from object_detector_amd.net import Context
    ctx = Context.get(cuda)
    return ctx.lib, ctx.handle


def _s():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _same(got, want, what):
    got, want = np.asarray(got).reshape(-1), np.asarray(want).reshape(-1)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{what}: {bad.size} of {got.size} differ, first at {bad[0]}: got {got[bad[0]]:#x} want {want[bad[0]]:#x}"


class Guarded:
    """`n` elements of `size` bytes in the middle of a larger device buffer whose `g` elements on either side (and `skew`
    more in front, which moves the payload off its 16-byte alignment) hold `poison`.  Contents travel as unsigned bit patterns."""

    def __init__(self, cuda, n, size, poison, data=None, g=64, skew=0):
        self.tt, self.si, self.un = _T[size]
        self.n, self.lo, self.size, self.poison = n, g + skew, size, poison
        self.buf = torch.full((n + 2 * g + skew,), poison, dtype=self.tt, device=cuda)
        assert self.buf.data_ptr() % 16 == 0
        if data is not None:
            self.put(data)

    @property
    def ptr(self):
        return self.buf.data_ptr() + self.lo * self.size

    def put(self, data):
        a = np.ascontiguousarray(data).reshape(-1)
        assert a.size == self.n and a.itemsize == self.size
        self.buf[self.lo:self.lo + self.n] = torch.from_numpy(a.view(self.si)).to(self.buf.device)

    def bits(self):
        return self.buf.cpu().numpy().view(self.un)

    def check(self, payload_bits, what):
        """payload == payload_bits and both guards still hold the poison"""
        want = np.full(self.buf.numel(), self.poison, self.un)
        want[self.lo:self.lo + self.n] = np.ascontiguousarray(payload_bits).reshape(-1).view(self.un)
        _same(self.bits(), want, what)


def _u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _flag(cuda, v):
    return torch.tensor([v], dtype=torch.int32, device=cuda)


# ---- od_sgd_step -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("momentum,wd", [(0.0, 0.0), (0.0, 1e-4), (0.9, 0.0), (0.9, 1e-4)], ids=str)
def test_sgd_step_exact(cuda, momentum, wd):
    """n = 1 .. 10007 (one thread, a ragged workgroup, a second workgroup, a strided grid), two consecutive calls so that
    the second starts from a non-zero momentum."""
    lib, h = _api(cuda)
    rng = np.random.default_rng(21)
    inv = 1.0 / 128.0
    for n in (1, 255, 256, 257, 2049, 10007):
        w, m = R.values(rng, n, -3, 1), np.zeros(n, np.float32)
        wd_, md_ = Guarded(cuda, n, 4, P32, w), Guarded(cuda, n, 4, P32, m)
        for step, lr in enumerate((0.1, 0.03)):
            g = R.values(rng, n)
            gd_ = Guarded(cuda, n, 4, P32, g)
            assert lib.od_sgd_step(h, wd_.ptr, md_.ptr, gd_.ptr, n, lr, momentum, wd, inv, _s()) == 0
            w, m = R.sgd_ref(w, m, g, lr, momentum, wd, inv)
            wd_.check(_u32(w), f"w n={n} step {step}")
            md_.check(_u32(m), f"m n={n} step {step}")
            gd_.check(_u32(g), f"g n={n} step {step}")


@pytest.mark.parametrize("skew", [(0, 0, 0), (1, 1, 1), (3, 3, 3), (0, 1, 0), (2, 2, 1)], ids=str)
def test_sgd_step_phases(cuda, skew):
    """(w, m, g) each `skew` floats behind a 16-byte boundary.  A shared phase gives a head of 0, 3 or 1 elements, a 16-byte
    body that may be empty (n < 4 + head) and a tail of 0 .. 3; two buffers out of phase send the whole run one by one.  Two
    consecutive calls, same bits on every path, guards on both sides of all three buffers untouched."""
    lib, h = _api(cuda)
    rng = np.random.default_rng(23)
    inv = 1.0 / 128.0
    for n in (1, 2, 3, 4, 5, 7, 8, 9, 255, 257, 2051):
        w, m = R.values(rng, n, -3, 1), R.values(rng, n, -4, 0)
        wd_, md_ = Guarded(cuda, n, 4, P32, w, skew=skew[0]), Guarded(cuda, n, 4, P32, m, skew=skew[1])
        assert wd_.ptr % 16 == 4 * skew[0] and md_.ptr % 16 == 4 * skew[1]
        for step, lr in enumerate((0.1, 0.03)):
            g = R.values(rng, n)
            gd_ = Guarded(cuda, n, 4, P32, g, skew=skew[2])
            assert lib.od_sgd_step(h, wd_.ptr, md_.ptr, gd_.ptr, n, lr, 0.9, 1e-4, inv, _s()) == 0
            w, m = R.sgd_ref(w, m, g, lr, 0.9, 1e-4, inv)
            wd_.check(_u32(w), f"w n={n} skew {skew} step {step}")
            md_.check(_u32(m), f"m n={n} skew {skew} step {step}")
            gd_.check(_u32(g), f"g n={n} skew {skew} step {step}")


# ---- od_sgd_step_multi -------------------------------------------------------------------------------------------------
SEG_COUNTS = (1, 3, 255, 256, 257, 4100, 65536, 65541, 2 * 65536 + 5)  # 256 x 256 threads per segment: 1, 2 and 3 sweeps
SEG_LR = (0.1, 0.05, 0.0, 0.02, 0.013, 0.07, 0.001, 0.09, 0.033)
SEG_WD = (1e-4, 2e-4, 5e-5, 0.0, 3e-4, 1e-3, 7e-5, 1e-5, 4e-4)
SEG_GUARD = 65536


def _seg_layout():
    """offsets of the 9 segments in one flat buffer: multiples of 4 except segment 4's (odd), 4 to 40 poisoned floats between
    neighbours, SEG_GUARD poisoned floats in front and behind -> (offsets, total)"""
    rng = np.random.default_rng(4)
    offs, off = [], SEG_GUARD
    for i, c in enumerate(SEG_COUNTS):
        o = off + (1 if i == 4 else 0)
        offs.append(o)
        end = o + c
        gap = 4 + (-(end + 4)) % 4 + 4 * int(rng.integers(0, 8))
        off = end + gap
        assert off % 4 == 0 and 4 <= gap <= 40
    assert offs[4] % 2 == 1 and all(o % 4 == 0 for i, o in enumerate(offs) if i != 4)
    return offs, off + SEG_GUARD


def _seg_table(cuda, offs, counts, lrs, wds):
    from object_detector_amd import _lib
    raw = b""
    for o, c, lr, wd in zip(offs, counts, lrs, wds):
        sg = _lib.SgdSeg()
        sg.offset, sg.count, sg.lr, sg.weight_decay = o, c, lr, wd
        raw += bytes(sg)
    return torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(cuda)


def _multi_ref(w, m, g, offs, counts, lrs, wds, momentum, inv):
    w, m = w.copy(), m.copy()
    for o, c, lr, wd in zip(offs, counts, lrs, wds):
        w[o:o + c], m[o:o + c] = R.sgd_ref(w[o:o + c], m[o:o + c], g[o:o + c], lr, momentum, wd, inv)
    return w, m


@pytest.fixture(scope="module")
def seg_case():
    """Host side of the 9-segment buffer: poisoned everywhere but in the segments; the reference after one and two calls."""
    offs, total = _seg_layout()
    rng = np.random.default_rng(8)
    poison = np.array([P32], np.uint32).view(np.float32)[0]
    w0, m0, gs = (np.full(total, poison, np.float32) for _ in range(3))
    g2 = gs.copy()
    for o, c in zip(offs, SEG_COUNTS):
        w0[o:o + c], m0[o:o + c] = R.values(rng, c, -3, 1), R.values(rng, c, -4, 0)
        gs[o:o + c], g2[o:o + c] = R.values(rng, c), R.values(rng, c)
    inv = 1.0 / 512.0
    w1, m1 = _multi_ref(w0, m0, gs, offs, SEG_COUNTS, SEG_LR, SEG_WD, 0.9, inv)
    w2, m2 = _multi_ref(w1, m1, g2, offs, SEG_COUNTS, SEG_LR, SEG_WD, 0.9, inv)
    for a in (w0, m0, gs, g2, w1, m1, w2, m2):
        a.setflags(write=False)
    return dict(offs=offs, total=total, w0=w0, m0=m0, g=(gs, g2), w=(w1, w2), m=(m1, m2), inv=inv)


def test_sgd_multi_exact_two_calls(cuda, seg_case):
    """Per-segment lr / weight decay from the device table (one lr = 0, one decay = 0), tails of ragged sweeps, an odd
    offset; gaps, guards and the gradient buffer bit-identical afterwards."""
    lib, h = _api(cuda)
    c = seg_case
    assert 390_000 <= c["total"] <= 410_000
    tbl = _seg_table(cuda, c["offs"], SEG_COUNTS, SEG_LR, SEG_WD)
    w, m = torch.from_numpy(c["w0"].copy()).to(cuda), torch.from_numpy(c["m0"].copy()).to(cuda)
    for step in range(2):
        g = torch.from_numpy(c["g"][step].copy()).to(cuda)
        assert lib.od_sgd_step_multi(h, w.data_ptr(), m.data_ptr(), g.data_ptr(), tbl.data_ptr(), len(SEG_COUNTS), 0.9,
                                     c["inv"], None, _s()) == 0
        _same(_u32(w.cpu().numpy()), _u32(c["w"][step]), f"w after call {step}")
        _same(_u32(m.cpu().numpy()), _u32(c["m"][step]), f"m after call {step}")
        _same(_u32(g.cpu().numpy()), _u32(c["g"][step]), f"g after call {step}")
    # the lr = 0 segment kept its weights and still took the momentum; the decay = 0 one is not the decayed one
    o, n = c["offs"][2], SEG_COUNTS[2]
    assert np.array_equal(c["w"][1][o:o + n], c["w0"][o:o + n]) and not np.array_equal(c["m"][1][o:o + n], c["m0"][o:o + n])


def _skewed(cuda, a, skew):
    """The host buffer on the device behind `skew` extra floats: the base pointer is 4 * skew bytes off a 16-byte boundary."""
    t = torch.empty(a.size + skew, dtype=torch.float32, device=cuda)
    assert t.data_ptr() % 16 == 0
    t = t[skew:]
    t.copy_(torch.from_numpy(a.copy()))
    assert t.data_ptr() % 16 == 4 * skew
    return t


@pytest.mark.parametrize("skew", [(1, 1, 1), (0, 0, 1), (1, 0, 1)], ids=str)
def test_sgd_multi_misaligned_bases(cuda, seg_case, skew):
    """The nine segments with the base pointers of (w, m, g) advanced by `skew` floats.  All by one: every segment shares a
    phase that is not the boundary, so it has a scalar head, a 16-byte body and a scalar tail, and the seams are where an
    element would be lost or done twice.  One buffer against the others: no common phase, every segment goes one by one.
    Same bits; gaps, guards and the gradients bit-identical afterwards."""
    lib, h = _api(cuda)
    c = seg_case
    tbl = _seg_table(cuda, c["offs"], SEG_COUNTS, SEG_LR, SEG_WD)
    w, m = _skewed(cuda, c["w0"], skew[0]), _skewed(cuda, c["m0"], skew[1])
    for step in range(2):
        g = _skewed(cuda, c["g"][step], skew[2])
        assert lib.od_sgd_step_multi(h, w.data_ptr(), m.data_ptr(), g.data_ptr(), tbl.data_ptr(), len(SEG_COUNTS), 0.9,
                                     c["inv"], None, _s()) == 0
        _same(_u32(w.cpu().numpy()), _u32(c["w"][step]), f"skew {skew} w after call {step}")
        _same(_u32(m.cpu().numpy()), _u32(c["m"][step]), f"skew {skew} m after call {step}")
        _same(_u32(g.cpu().numpy()), _u32(c["g"][step]), f"skew {skew} g after call {step}")


@pytest.mark.parametrize("flag", [None, 0, 1, -1, 0x100], ids=str)
def test_sgd_multi_skip_flag(cuda, seg_case, flag):
    """skip_if_nonzero: NULL and a device 0 update; every non-zero value leaves w and m bit-identical."""
    lib, h = _api(cuda)
    c = seg_case
    tbl = _seg_table(cuda, c["offs"], SEG_COUNTS, SEG_LR, SEG_WD)
    w, m = torch.from_numpy(c["w0"].copy()).to(cuda), torch.from_numpy(c["m0"].copy()).to(cuda)
    g = torch.from_numpy(c["g"][0].copy()).to(cuda)
    fl = None if flag is None else _flag(cuda, flag)
    assert lib.od_sgd_step_multi(h, w.data_ptr(), m.data_ptr(), g.data_ptr(), tbl.data_ptr(), len(SEG_COUNTS), 0.9, c["inv"],
                                 None if fl is None else fl.data_ptr(), _s()) == 0
    skipped = bool(flag)
    _same(_u32(w.cpu().numpy()), _u32(c["w0"] if skipped else c["w"][0]), "w")
    _same(_u32(m.cpu().numpy()), _u32(c["m0"] if skipped else c["m"][0]), "m")
    if fl is not None:
        assert int(fl.item()) == flag  # the kernel only reads it


def test_sgd_multi_argument_checks(cuda, seg_case):
    lib, h = _api(cuda)
    c = seg_case
    tbl = _seg_table(cuda, c["offs"], SEG_COUNTS, SEG_LR, SEG_WD)
    w, m = torch.from_numpy(c["w0"].copy()).to(cuda), torch.from_numpy(c["m0"].copy()).to(cuda)
    g = torch.from_numpy(c["g"][0].copy()).to(cuda)
    for nseg in (0, 65536):
        assert lib.od_sgd_step_multi(h, w.data_ptr(), m.data_ptr(), g.data_ptr(), tbl.data_ptr(), nseg, 0.9, c["inv"], None,
                                     _s()) == OD_ERR_INVALID
    torch.cuda.synchronize()
    _same(_u32(w.cpu().numpy()), _u32(c["w0"]), "w after rejected calls")
    _same(_u32(m.cpu().numpy()), _u32(c["m0"]), "m after rejected calls")


def test_sgd_multi_many_small_segments(cuda):
    """The trainer's regime: 300 segments of 1 to 64 elements (gamma / beta / bias vectors), each at a 4-float boundary."""
    lib, h = _api(cuda)
    rng = np.random.default_rng(31)
    counts = [int(v) for v in rng.integers(1, 65, 300)]
    counts[:3] = [1, 64, 63]
    offs, off = [], 64
    for cnt in counts:
        offs.append(off)
        off += (cnt + 3) // 4 * 4
    total = off + 64
    lrs = [float(v) for v in rng.uniform(1e-3, 0.1, 300)]
    wds = [float(v) if i % 3 else 0.0 for i, v in enumerate(rng.uniform(1e-5, 1e-3, 300))]
    poison = np.array([P32], np.uint32).view(np.float32)[0]
    w, m, g = (np.full(total, poison, np.float32) for _ in range(3))
    for o, cnt in zip(offs, counts):
        w[o:o + cnt], m[o:o + cnt], g[o:o + cnt] = R.values(rng, cnt, -3, 1), R.values(rng, cnt, -4, 0), R.values(rng, cnt)
    inv = 1.0 / 256.0
    wr, mr = _multi_ref(w, m, g, offs, counts, lrs, wds, 0.9, inv)
    tbl = _seg_table(cuda, offs, counts, lrs, wds)
    wd_, md_, gd_ = (torch.from_numpy(a).to(cuda) for a in (w, m, g))
    assert lib.od_sgd_step_multi(h, wd_.data_ptr(), md_.data_ptr(), gd_.data_ptr(), tbl.data_ptr(), 300, 0.9, inv, None, _s()) == 0
    _same(_u32(wd_.cpu().numpy()), _u32(wr), "w")
    _same(_u32(md_.cpu().numpy()), _u32(mr), "m")
    _same(_u32(gd_.cpu().numpy()), _u32(g), "g")


# ---- od_grad_nonfinite -------------------------------------------------------------------------------------------------
BAD_BITS = (0x7f800000, 0xff800000, 0x7fc00000, 0x7f800001, 0xffc12345)  # +Inf, -Inf, quiet NaN, signalling NaN, negative NaN
FLAG_BEFORE = 0x55555555


def _nonfinite(lib, h, cuda, g_ptr, n):
    fl = _flag(cuda, FLAG_BEFORE)
    rc = lib.od_grad_nonfinite(h, g_ptr, n, fl.data_ptr(), _s())
    return rc, int(fl.item())


def _i32(bits):
    return int(np.array([bits], np.uint32).view(np.int32)[0])


def test_grad_nonfinite_small_sizes(cuda):
    """n = 1 .. 5 and 1003: the vector body, the scalar tail, or both; every position, every kind of bad value."""
    lib, h = _api(cuda)
    rng = np.random.default_rng(2)
    k = 0
    for n in (1, 2, 3, 4, 5, 1003):
        g = Guarded(cuda, n, 4, P32, R.values(rng, n))
        # the guards next to the buffer are non-finite: reading one element too many raises a false flag
        g.buf[:g.lo] = _i32(0x7fc00000)
        g.buf[g.lo + n:] = _i32(0x7fc00000)
        assert _nonfinite(lib, h, cuda, g.ptr, n) == (0, 0), n
        for pos in (range(n) if n <= 5 else (0, 3, 4, 511, 999, 1000, 1001, 1002)):
            keep = int(g.buf[g.lo + pos].item())
            g.buf[g.lo + pos] = _i32(BAD_BITS[k % 5])
            assert _nonfinite(lib, h, cuda, g.ptr, n) == (0, 1), (n, pos, hex(BAD_BITS[k % 5]))
            g.buf[g.lo + pos] = keep
            k += 1
        assert _nonfinite(lib, h, cuda, g.ptr, n) == (0, 0), n


def _tile_edge_positions(n):
    """Element 0, the first and last element of each 256-vector quarter of the last 1024-vector tile (ragged: a quarter may
    be short or absent), and every tail element behind the last whole vector."""
    n4 = n // 4
    pos = {0}
    t0 = (n4 - 1) // 1024 * 1024
    for q in range(4):
        a, b = t0 + 256 * q, min(t0 + 256 * (q + 1), n4)
        if a < b:
            pos |= {4 * a, 4 * b - 1}
    return sorted(pos | set(range(4 * n4, n)))


def test_grad_nonfinite_tile_edges(cuda):
    """Sizes around a scan tile of 1024 vectors (4096 floats), where a lane's four loads are in flight only if its fourth
    vector (base + 768) exists: 768 and 769 vectors, one vector short of a tile, exactly one, one tile and three quarters, two
    tiles and one vector; tails of 0, 1 and 3.  One bad value at a time at every edge; clean in between."""
    lib, h = _api(cuda)
    rng = np.random.default_rng(5)
    assert _tile_edge_positions(7175) == [0, 4096, 5119, 5120, 6143, 6144, 7167, 7168, 7171, 7172, 7173, 7174]
    k = 0
    for n in (3075, 3076, 3077, 4095, 4096, 4097, 7168, 7175, 8197):
        g = Guarded(cuda, n, 4, P32, R.values(rng, n))
        # the guards next to the buffer are non-finite: reading one element too many raises a false flag
        g.buf[:g.lo] = _i32(0x7fc00000)
        g.buf[g.lo + n:] = _i32(0x7fc00000)
        assert _nonfinite(lib, h, cuda, g.ptr, n) == (0, 0), n
        for pos in _tile_edge_positions(n):
            keep = int(g.buf[g.lo + pos].item())
            g.buf[g.lo + pos] = _i32(BAD_BITS[k % 5])
            assert _nonfinite(lib, h, cuda, g.ptr, n) == (0, 1), (n, pos, hex(BAD_BITS[k % 5]))
            g.buf[g.lo + pos] = keep
            k += 1
        assert _nonfinite(lib, h, cuda, g.ptr, n) == (0, 0), n


def test_grad_nonfinite_large_buffer(cuda):
    """n = 20 000 003 (80 MB): 5 000 000 vectors over a grid capped at 4096 x 256 threads, so every thread strides and the
    last sweep is ragged; 3 tail elements.  Exactly one bad element per call."""
    lib, h = _api(cuda)
    n = 20_000_003
    g = torch.full((n,), 1.5, dtype=torch.float32, device=cuda)
    gi = g.view(torch.int32)
    assert g.data_ptr() % 16 == 0
    assert _nonfinite(lib, h, cuda, g.data_ptr(), n) == (0, 0)
    for k, pos in enumerate((0, 3, 4, 1_048_575, 4_194_304, 16_777_216, n - 4, n - 3, n - 2, n - 1)):
        gi[pos] = _i32(BAD_BITS[k % 5])
        assert _nonfinite(lib, h, cuda, g.data_ptr(), n) == (0, 1), (pos, hex(BAD_BITS[k % 5]))
        g[pos] = 1.5
    assert _nonfinite(lib, h, cuda, g.data_ptr(), n) == (0, 0)
    # finite look-alikes raise nothing
    fmax = float(np.finfo(np.float32).max)
    g[0::2] = fmax
    g[1::2] = -fmax
    assert _nonfinite(lib, h, cuda, g.data_ptr(), n) == (0, 0), "+-FLT_MAX"
    g.fill_(-0.0)
    assert int(gi[n - 1].item()) == _i32(0x80000000)
    assert _nonfinite(lib, h, cuda, g.data_ptr(), n) == (0, 0), "-0.0"
    gi.fill_(0x7f000000)
    assert _nonfinite(lib, h, cuda, g.data_ptr(), n) == (0, 0), "0x7f000000"
    # a misaligned buffer is refused and the flag is left alone
    rc, fl = _nonfinite(lib, h, cuda, g.data_ptr() + 4, n - 1)
    assert rc == OD_ERR_INVALID and fl == FLAG_BEFORE


# ---- od_copy_if_nonzero ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flag", [0, 1, -1, 2])
def test_copy_if_nonzero(cuda, flag):
    lib, h = _api(cuda)
    rng = np.random.default_rng(6)
    for n in (1, 3, 4, 5, 1027, 2_100_001):
        src, old = R.values(rng, n), R.values(rng, n)
        sd, dd = Guarded(cuda, n, 4, P32, src), Guarded(cuda, n, 4, P32, old)
        fl = _flag(cuda, flag)
        assert lib.od_copy_if_nonzero(h, dd.ptr, sd.ptr, n, fl.data_ptr(), _s()) == 0
        dd.check(_u32(src if flag else old), f"dst n={n}")
        sd.check(_u32(src), f"src n={n}")
        assert int(fl.item()) == flag


# ---- od_cast_f32_bf16 / od_cast_bf16_f32 -----------------------------------------------------------------------------
def test_bf16_casts_exact(cuda):
    """Against optim_ref.bf16_ref on the CPU (itself checked against torch's CPU cast in test_optim_ref_host.py), NaN payloads
    included: the value list of test_bf16_casts_round_to_nearest_even, the ties around the largest finite value, and
    4 200 003 random floats (four sweeps of the capped grid, a ragged last one)."""
    lib, h = _api(cuda)
    rng = np.random.default_rng(0)
    special = np.concatenate([
        np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1.00390625, 1.01171875, 3.3895314e38], np.float32),
        np.array([0x7f7f8000, 0x7f7f7fff, 0xff7f8000, 0x7f7fffff, 0x7f800001, 0xffc00000, 0x7fffffff], np.uint32).view(np.float32)])
    big = np.concatenate([R.values(rng, 4_200_003 - 2000 - special.size, -30, 30), rng.normal(0, 1e-30, 1000).astype(np.float32),
                          rng.normal(0, 1, 1000).astype(np.float32), special])
    assert big.size == 4_200_003
    for v in (big, big[-1:], big[-2:], big[-3:], big[-5:], special):
        n = v.size
        src = Guarded(cuda, n, 4, P32, v)
        dst = Guarded(cuda, n, 2, P16)
        assert lib.od_cast_f32_bf16(h, src.ptr, dst.ptr, n, _s()) == 0
        want = R.bf16_ref(v)
        dst.check(want, f"f32 -> bf16 n={n}")
        back = Guarded(cuda, n, 4, P32)
        assert lib.od_cast_bf16_f32(h, dst.ptr, back.ptr, n, _s()) == 0
        back.check(_u32(R.bf16_widen_ref(want)), f"bf16 -> f32 n={n}")
        dst.check(want, f"bf16 source n={n}")


# ---- od_add_f16 --------------------------------------------------------------------------------------------------------
def _f16_vals(rng, n):
    return R.values(rng, n, -3, 3).astype(np.float16)


def test_add_f16_exact(cuda):
    """a += b in f32, one rounding to f16; overflow becomes Inf, Inf - Inf becomes NaN, NaN passes through -- the NaNs bit
    for bit as well: Inf - Inf gives the negative default NaN (0xfe00) on the device as in numpy on the host, and a quiet NaN
    operand keeps its payload on both."""
    lib, h = _api(cuda)
    rng = np.random.default_rng(12)
    sp_a = np.array([60000, 60000, -60000, np.inf, np.inf, np.nan, 1.0, -0.0], np.float16)
    sp_b = np.array([60000, 5504, -60000, -np.inf, 1.0, 1.0, np.nan, -0.0], np.float16)
    for n in (8, 16, 2056, 8 * 1_100_001):
        a, b = _f16_vals(rng, n), _f16_vals(rng, n)
        if n > 8:
            a[-8:], b[-8:] = sp_a[::-1], sp_b[::-1]
        a[:8], b[:8] = sp_a, sp_b
        want = R.add_f16_ref(a, b)
        assert np.isposinf(want[0]) and want[1] == 65504 and np.isneginf(want[2]) and np.isposinf(want[4])
        assert list(want.view(np.uint16)[[3, 5, 6, 7]]) == [0xfe00, 0x7e00, 0x7e00, 0x8000]
        ad, bd = Guarded(cuda, n, 2, P16, a), Guarded(cuda, n, 2, P16, b)
        assert lib.od_add_f16(h, ad.ptr, bd.ptr, n, _s()) == 0
        ad.check(want.view(np.uint16), f"a n={n}")
        bd.check(b.view(np.uint16), f"b n={n}")
    ad, bd = Guarded(cuda, 16, 2, P16, a[:16]), Guarded(cuda, 16, 2, P16, b[:16])
    for n in (0, 7, 12, -8):
        assert lib.od_add_f16(h, ad.ptr, bd.ptr, n, _s()) == OD_ERR_INVALID, n
    ad.check(a[:16].view(np.uint16), "a after rejected calls")


# ---- od_down2_sum_add ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1, 1, 8), (2, 3, 5, 8), (3, 4, 6, 64), (2, 5, 7, 208), (1, 20, 20, 1024)], ids=str)
@pytest.mark.parametrize("accumulate", [0, 1])
def test_down2_sum_add_exact(cuda, shape, accumulate):
    lib, h = _api(cuda)
    B, Hh, Wh, Cc = shape
    rng = np.random.default_rng(B * 100 + Cc)
    d = _f16_vals(rng, B * 2 * Hh * 2 * Wh * Cc).reshape(B, 2 * Hh, 2 * Wh, Cc)
    base = _f16_vals(rng, B * Hh * Wh * Cc).reshape(B, Hh, Wh, Cc)
    d[0, :2, :2, :] = 30000  # four addends that overflow f16 only in the sum
    base[0, 0, 0, :] = 0.5
    want = R.down2_ref(d, base if accumulate else None)
    assert np.isposinf(want[0, 0, 0]).all() and np.isfinite(want.reshape(-1)[Cc:]).all()
    dd = Guarded(cuda, d.size, 2, P16, d)
    ud = Guarded(cuda, base.size, 2, P16, base)  # accumulate = 0 must overwrite what is there
    assert lib.od_down2_sum_add(h, dd.ptr, ud.ptr, B, Hh, Wh, Cc, accumulate, _s()) == 0
    ud.check(want.view(np.uint16), f"dup {shape} accumulate={accumulate}")
    dd.check(d.view(np.uint16), "d")
    if shape == (2, 3, 5, 8):
        for bad_c in (4, 12, 0):
            assert lib.od_down2_sum_add(h, dd.ptr, ud.ptr, B, Hh, Wh, bad_c, accumulate, _s()) == OD_ERR_INVALID
        ud.check(want.view(np.uint16), "dup after rejected calls")


# ---- od_pack_weights / od_pack_weights_multi ---------------------------------------------------------------------------
PACK_CASES = [(64, 32, 3, 0), (128, 64, 1, 0), (208, 256, 3, 0), (256, 192, 3, 0), (16, 24, 3, 0), (1024, 512, 1, 0),
              (72, 1024, 1, 0),
              (16, 6, 3, 1), (24, 12, 1, 1)]  # the scalar branch: Cin % 4 != 0 / the master pointer advanced by one float


def _pack_case(cuda, Cout, Cin, k, skew, seed=0):
    rng = np.random.default_rng(Cout * 7 + Cin + k + seed)
    w = R.values(rng, Cout * k * k * Cin, -3, 1).reshape(Cout, k * k * Cin)
    dims = R.pack_dims(Cout, Cin, k)
    wf, wt = R.pack_ref(w, Cout, Cin, k, *dims, R.F16_NAN)
    return w, dims, wf, wt


@pytest.mark.parametrize("case", PACK_CASES, ids=str)
def test_pack_weights_exact(cuda, case):
    """Both destinations pre-filled with an f16 NaN: every in-range element is written at the restated place, no padding
    element is written at all (the packs' pads are zeroed once, at allocation)."""
    from object_detector_amd import _lib
    lib, h = _api(cuda)
    Cout, Cin, k, skew = case
    w, dims, wf, wt = _pack_case(cuda, Cout, Cin, k, skew)
    assert dims[:2] == _lib.conv_weight_dims(Cout, Cin, k) and dims[2:] == _lib.conv_weight_dims(Cin, Cout, k)
    wm = Guarded(cuda, w.size, 4, P32, w, skew=skew)
    assert (wm.ptr % 16 != 0) == bool(skew)
    fd = Guarded(cuda, wf.size, 2, R.F16_NAN)
    td = Guarded(cuda, wt.size, 2, R.F16_NAN)
    assert lib.od_pack_weights(h, wm.ptr, fd.ptr, td.ptr, Cout, Cin, k, _s()) == 0
    fd.check(wf, f"w_fwd {case}")
    td.check(wt, f"w_bwd {case}")
    # w_bwd = NULL writes only the forward pack
    fd2 = Guarded(cuda, wf.size, 2, R.F16_NAN)
    assert lib.od_pack_weights(h, wm.ptr, fd2.ptr, None, Cout, Cin, k, _s()) == 0
    fd2.check(wf, f"w_fwd alone {case}")
    wm.check(_u32(w), "masters")


def test_pack_weights_argument_checks(cuda):
    lib, h = _api(cuda)
    w, dims, wf, wt = _pack_case(cuda, 12, 8, 1, 0)
    wm = Guarded(cuda, w.size, 4, P32, w)
    fd, td = Guarded(cuda, wf.size, 2, R.F16_NAN), Guarded(cuda, wt.size, 2, R.F16_NAN)
    assert lib.od_pack_weights(h, wm.ptr, fd.ptr, td.ptr, 12, 8, 1, _s()) == OD_ERR_INVALID  # Cout % 8 != 0 with w_bwd
    assert lib.od_pack_weights(h, wm.ptr, fd.ptr + 2, None, 12, 8, 1, _s()) == OD_ERR_INVALID  # unaligned w_fwd
    assert lib.od_pack_weights(h, wm.ptr, fd.ptr, td.ptr + 8, 16, 8, 1, _s()) == OD_ERR_INVALID  # unaligned w_bwd
    assert lib.od_pack_weights(h, wm.ptr, fd.ptr, None, 12, 8, 2, _s()) == OD_ERR_INVALID  # ksize
    nothing = np.full(wf.size, R.F16_NAN, np.uint16)
    fd.check(nothing, "w_fwd after rejected calls")
    td.check(np.full(wt.size, R.F16_NAN, np.uint16), "w_bwd after rejected calls")
    assert lib.od_pack_weights(h, wm.ptr, fd.ptr, None, 12, 8, 1, _s()) == 0  # without w_bwd any Cout goes
    fd.check(wf, "w_fwd Cout = 12")


def test_pack_weights_multi_exact(cuda):
    """Three layers in one table over one flat master buffer: 288 workgroups per layer, of which the small layer (9 tiles)
    uses nine; equal to pack_ref, hence to the per-layer calls of test_pack_weights_exact."""
    from object_detector_amd import _lib
    lib, h = _api(cuda)
    cases = [(16, 24, 3), (208, 256, 3), (128, 64, 1)]
    refs, off, offs = [], 8, []
    for Cout, Cin, k in cases:
        refs.append(_pack_case(cuda, Cout, Cin, k, 0, seed=1))
        offs.append(off)
        off += refs[-1][0].size + 12
    flat = np.full(off, np.array([P32], np.uint32).view(np.float32)[0], np.float32)
    for o, (w, *_r) in zip(offs, refs):
        flat[o:o + w.size] = w.reshape(-1)
    fm = torch.from_numpy(flat).to(cuda)
    bufs, raw = [], b""
    for (Cout, Cin, k), o, (w, dims, wf, wt) in zip(cases, offs, refs):
        fd, td = Guarded(cuda, wf.size, 2, R.F16_NAN), Guarded(cuda, wt.size, 2, R.F16_NAN)
        bufs.append((fd, td))
        L = _lib.PackLayer()
        L.w_offset, L.w_fwd, L.w_bwd, L.Cout, L.Cin, L.ksize = o, fd.ptr, td.ptr, Cout, Cin, k
        raw += bytes(L)
    tbl = torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(cuda)
    assert lib.od_pack_weights_multi(h, fm.data_ptr(), tbl.data_ptr(), len(cases), _s()) == 0
    for case, (fd, td), (w, dims, wf, wt) in zip(cases, bufs, refs):
        fd.check(wf, f"multi w_fwd {case}")
        td.check(wt, f"multi w_bwd {case}")
        # the per-layer form on the same masters writes the same bits
        wm = Guarded(cuda, w.size, 4, P32, w)
        f1, t1 = Guarded(cuda, wf.size, 2, R.F16_NAN), Guarded(cuda, wt.size, 2, R.F16_NAN)
        assert lib.od_pack_weights(h, wm.ptr, f1.ptr, t1.ptr, *case, _s()) == 0
        _same(f1.bits(), fd.bits(), f"per-layer vs multi w_fwd {case}")
        _same(t1.bits(), td.bits(), f"per-layer vs multi w_bwd {case}")
    for nl in (0, 65536):
        assert lib.od_pack_weights_multi(h, fm.data_ptr(), tbl.data_ptr(), nl, _s()) == OD_ERR_INVALID
