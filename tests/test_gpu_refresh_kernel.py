"""GPU: od_net_refresh through the C ABI alone, on a hand-built table of small crafted layers, against
tests/refresh_ref.py bit for bit (uint16 / uint32 views, signed zeros count, no tolerance).

Layers: the image layer; Cout not a multiple of the pad at an offset that is 4-byte but not 16-byte aligned (the scalar
path); a cin_repeat = 2 pack with aligned runs of 8 and one with ragged runs (Cin = 12); a bias layer without BatchNorm;
one large enough that every workgroup makes more than one trip.  Inputs carry exact f16 ties in both directions, values
that round to f16 subnormals and to zero, +-65520 and beyond (Inf), -0.0, a tiny variance and a gamma of 0.  Every
destination is filled with a NaN pattern first, padding included, and sits between guard bands.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import refresh_ref as R
from object_detector_amd import _lib

pytestmark = pytest.mark.gpu

OD_ERR_INVALID = -1
P16, P32 = 0x7dad, 0x7fc12345  # NaN patterns the kernel never produces
GUARD = 64                      # elements on either side of every destination
EPS = 1e-3

# f32 values whose f16 conversion is decided by a tie, a subnormal, an overflow or a sign
SPECIALS = np.array([
    1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, -(1.0 + 2.0 ** -11), -(1.0 + 3 * 2.0 ** -11),  # ties: down to even, up to even
    2.0 ** -25, 3 * 2.0 ** -25, 1.5 * 2.0 ** -25, 2.0 ** -24, -(2.0 ** -25), 5 * 2.0 ** -26,  # subnormal results / ties / zero
    2.0 ** -14 * (1 - 2.0 ** -11), 2.0 ** -14 * (1 - 2.0 ** -12),  # largest subnormal, and the tie up to the smallest normal
    1e-9, -1e-9, 1e-30, 0.0, -0.0,
    65504.0, 65519.99, 65520.0, -65520.0, 65536.0, 1e6, -1e30, 3.0e38], np.float32)


def _s():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


class Dst:
    """A destination of n elements (2 or 4 bytes) inside a device buffer with GUARD poisoned elements on both sides."""

    def __init__(self, cuda, n, size):
        self.n, self.size = n, size
        self.tt, self.un, self.poison = (torch.int16, np.uint16, P16) if size == 2 else (torch.int32, np.uint32, P32)
        self.buf = torch.empty(n + 2 * GUARD, dtype=self.tt, device=cuda)
        self.fill()
        assert self.ptr % 16 == 0

    def fill(self):
        poison = np.full(self.buf.numel(), self.poison, self.un).view(np.int16 if self.size == 2 else np.int32)
        self.buf.copy_(torch.from_numpy(poison))

    @property
    def ptr(self):
        return self.buf.data_ptr() + GUARD * self.size

    def check(self, want, what):
        full = np.full(self.buf.numel(), self.poison, self.un)
        full[GUARD:GUARD + self.n] = np.ascontiguousarray(want).reshape(-1).view(self.un)
        got = self.buf.cpu().numpy().view(self.un)
        bad = np.flatnonzero(got != full)
        assert bad.size == 0, (f"{what}: {bad.size} of {got.size} elements differ, first at {bad[0] - GUARD} (payload index): "
                               f"got {got[bad[0]]:#x} want {full[bad[0]]:#x}")


def _case(cuda):
    """(entries, params_flat, stats_flat): six layers laid out in two flat buffers, sources separated by gaps."""
    rng = np.random.default_rng(7)
    shapes = [  # cout, cin, k, repeat, first, bn
        (32, 3, 3, 1, True, True),
        (24, 16, 1, 1, False, True),
        (64, 8, 3, 2, False, True),
        (208, 32, 1, 1, False, False),
        (16, 12, 3, 2, False, True),
        (512, 256, 3, 1, False, True),
    ]
    entries, off, soff = [], 0, 0
    for i, (cout, cin, k, rep, first, bn) in enumerate(shapes):
        n = cout * k * k * cin
        # layer 1: 4-byte aligned only (offset = 1 mod 4); layer 4: 8-byte aligned (2 mod 4); the others on the 16-byte grid
        w_off = off + {1: 1, 4: 2}.get(i, 0)
        off = (w_off + n + 3) // 4 * 4 + 8
        kw = {}
        for name in (("gamma", "beta") if bn else ("bias",)):
            kw[name] = off + (3 if i == 1 else 0)
            off += (cout + 3) // 4 * 4 + 4
        if bn:
            kw["mean"], kw["var"] = soff + (1 if i == 1 else 0), soff + (cout + 3) // 4 * 4 + 4
            soff += 2 * ((cout + 3) // 4 * 4 + 4)
        entries.append(R.entry(w_off, cout, cin, k, rep, first, **kw))
    flat = rng.normal(0.0, 1.0, off).astype(np.float32)
    stats = rng.normal(0.0, 0.5, soff).astype(np.float32)
    for e in entries:
        n = e["Cout"] * e["ksize"] ** 2 * e["Cin"]
        w = flat[e["w_offset"]:e["w_offset"] + n]
        w *= np.float32(0.05)
        # the special values at scattered places, and at the first and last weight of the layer
        pos = rng.choice(n, size=min(n, 4 * len(SPECIALS)), replace=False)
        w[pos] = np.resize(SPECIALS, pos.size)
        w[0], w[-1] = SPECIALS[0], SPECIALS[19]
        if e["has_bn"]:
            c = e["Cout"]
            var = stats[e["var_offset"]:e["var_offset"] + c]
            var[:] = rng.uniform(0.01, 2.0, c).astype(np.float32)
            var[0], var[1], var[2] = 0.0, 1e-30, 1e-40  # tiny variances (the last an f32 subnormal): scale = gamma / sqrt(eps)
            g = flat[e["gamma_offset"]:e["gamma_offset"] + c]
            g[3], g[4] = 0.0, -0.0  # scale 0 / -0: bias = beta - mean * (+-0)
    return entries, flat, stats


def _structs(entries, dsts):
    out = []
    for e, (wd, sd, bd) in zip(entries, dsts):
        L = _lib.RefreshLayer()
        for k, v in e.items():
            setattr(L, k, v)
        L.w_dst, L.scale_dst, L.bias_dst = wd.ptr, sd.ptr, bd.ptr
        out.append(L)
    return out


def _table(cuda, structs):
    return torch.frombuffer(bytearray(b"".join(bytes(s) for s in structs)), dtype=torch.uint8).to(cuda)


def _check_all(entries, dsts, flat, stats, tag):
    for i, (e, (wd, sd, bd)) in enumerate(zip(entries, dsts)):
        wp, sc, bi = R.layer_ref(flat, stats, e, EPS)
        wd.check(wp, f"{tag}: layer {i} pack")
        sd.check(sc, f"{tag}: layer {i} scale")
        bd.check(bi, f"{tag}: layer {i} bias")


def test_net_refresh_exact(cuda):
    from object_detector_amd.net import Context
    ctx = Context.get(cuda)
    lib, h = ctx.lib, ctx.handle
    entries, flat, stats = _case(cuda)
    dsts = [(Dst(cuda, e["Cout_pad"] * e["Kpad"], 2), Dst(cuda, e["Cout_pad"], 4), Dst(cuda, e["Cout_pad"], 4)) for e in entries]
    table = _table(cuda, _structs(entries, dsts))
    dflat, dstats = torch.from_numpy(flat).to(cuda), torch.from_numpy(stats).to(cuda)
    assert dflat.data_ptr() % 16 == 0 and entries[1]["w_offset"] % 4 == 1 and entries[4]["w_offset"] % 4 == 2
    assert lib.od_net_refresh(h, dflat.data_ptr(), dstats.data_ptr(), table.data_ptr(), len(entries), EPS, _s()) == 0
    torch.cuda.synchronize()
    _check_all(entries, dsts, flat, stats, "first call")
    # the crafted values did what they were put there for (in the reference, hence in the result)
    u = R.layer_ref(flat, stats, entries[5], EPS)[0][:512, :2304].view(np.uint16)
    assert (u == 0x7c00).any() and (u == 0xfc00).any() and (u == 0x8000).any()  # +Inf, -Inf, -0
    assert (((u & 0x7c00) == 0) & ((u & 0x03ff) != 0)).any()                      # f16 subnormals

    # second call: the sources of ONE layer change; only its destinations do
    e = entries[2]
    n = e["Cout"] * 9 * e["Cin"]
    before = [tuple(d.buf.clone() for d in t) for t in dsts]
    flat2, stats2 = flat.copy(), stats.copy()
    flat2[e["w_offset"]:e["w_offset"] + n] *= np.float32(-1.5)
    flat2[e["gamma_offset"]:e["gamma_offset"] + e["Cout"]] += np.float32(0.25)
    stats2[e["mean_offset"]:e["mean_offset"] + e["Cout"]] -= np.float32(0.125)
    dflat.copy_(torch.from_numpy(flat2))
    dstats.copy_(torch.from_numpy(stats2))
    assert lib.od_net_refresh(h, dflat.data_ptr(), dstats.data_ptr(), table.data_ptr(), len(entries), EPS, _s()) == 0
    torch.cuda.synchronize()
    _check_all(entries, dsts, flat2, stats2, "second call")
    for i, (t0, t1) in enumerate(zip(before, dsts)):
        same = [bool(torch.equal(a, d.buf)) for a, d in zip(t0, t1)]
        assert same == ([False] * 3 if i == 2 else [True] * 3), (i, same)


def test_integration_md_refresh_block(cuda):
    """INTEGRATION.md's three code blocks executed VERBATIM (only the library path is made absolute): the RefreshLayer
    mirror a foreign binding would add drives one refresh of a (pack, scale, bias) triple through the C ABI."""
    import pathlib
    import re
    md = (pathlib.Path(__file__).resolve().parent.parent / "INTEGRATION.md").read_text()
    blocks = re.findall(r"```python\n(.*?)```", md, flags=re.S)
    assert len(blocks) >= 3 and "od_net_refresh" in blocks[2]
    ns = {}
    exec(blocks[0].replace('C.CDLL("libodhip.so")', f'C.CDLL({str(_lib.LIB_PATH)!r})'), ns)
    exec(blocks[1], ns)
    exec(blocks[2], ns)
    assert [f[0] for f in ns["RefreshLayer"]._fields_] == [f[0] for f in _lib.RefreshLayer._fields_]
    entries, flat, stats = _case(cuda)
    e = entries[2]
    dst = (Dst(cuda, e["Cout_pad"] * e["Kpad"], 2), Dst(cuda, e["Cout_pad"], 4), Dst(cuda, e["Cout_pad"], 4))
    L = ns["RefreshLayer"]()
    for k, v in e.items():
        setattr(L, k, v)
    L.w_dst, L.scale_dst, L.bias_dst = (d.ptr for d in dst)
    table = _table(cuda, [L])
    dflat, dstats = torch.from_numpy(flat).to(cuda), torch.from_numpy(stats).to(cuda)
    ns["refresh_layers"](ns["ctx"], dflat.data_ptr(), dstats.data_ptr(), table.data_ptr(), 1,
                         stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    for d, want, what in zip(dst, R.layer_ref(flat, stats, e, EPS), ("pack", "scale", "bias")):
        d.check(want, f"INTEGRATION.md block: {what}")


def test_net_refresh_pack_only_entry_and_arguments(cuda):
    """scale_dst = bias_dst = NULL writes the pack alone; null pointers and a bad count are OD_ERR_INVALID and write nothing."""
    from object_detector_amd.net import Context
    ctx = Context.get(cuda)
    lib, h = ctx.lib, ctx.handle
    entries, flat, stats = _case(cuda)
    e = entries[2]
    wd = Dst(cuda, e["Cout_pad"] * e["Kpad"], 2)
    L = _lib.RefreshLayer()
    for k, v in e.items():
        setattr(L, k, v)
    L.w_dst = wd.ptr
    table = _table(cuda, [L])
    dflat, dstats = torch.from_numpy(flat).to(cuda), torch.from_numpy(stats).to(cuda)
    args = (dflat.data_ptr(), dstats.data_ptr(), table.data_ptr())
    for bad in ((None,) + args[1:], (args[0], None, args[2]), args[:2] + (None,)):
        assert lib.od_net_refresh(h, *bad, 1, EPS, _s()) == OD_ERR_INVALID
    assert lib.od_net_refresh(None, *args, 1, EPS, _s()) == OD_ERR_INVALID
    for n in (0, -1, 65536):
        assert lib.od_net_refresh(h, *args, n, EPS, _s()) == OD_ERR_INVALID
    torch.cuda.synchronize()
    wd.check(np.full(wd.n, P16, np.uint16), "rejected calls wrote nothing")
    assert lib.od_net_refresh(h, *args, 1, EPS, _s()) == 0
    torch.cuda.synchronize()
    wd.check(R.layer_ref(flat, stats, e, EPS)[0], "pack-only entry")
