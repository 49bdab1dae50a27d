"""Test support: a numpy / Python reference of the device JPEG decoder's three stages (entropy decode, libjpeg "islow"
IDCT, libjpeg-turbo fancy upsampling + jdcolor YCbCr->RGB).  It reads what object_detector_amd.jpeg.parse produces and
must equal PIL's decode byte for byte; that pins the libjpeg details the kernels of csrc/jpeg.hip reproduce.  `scan`
also reports what the entropy decode went through (block start bits, largest categories, ZRL runs), and `sync_rounds`
restates the round scheme of the parallel decode, so the device's round count can be pinned too.  Slow (a Python loop
per symbol): for small images only."""
from __future__ import annotations

import numpy as np

from object_detector_amd import jpeg

NATURAL = np.concatenate([jpeg.ZIGZAG, np.full(16, 63, np.int32)])  # libjpeg's jpeg_natural_order + safety entries


class _Bits:
    """Bit reader over stream bytes [start_byte, end_byte); bytes at or past the end read as zero (libjpeg inserts
    zeros at a marker).  `p` is the absolute bit position.  Holds the 16-bit window at every bit position."""

    def __init__(self, data, start_byte, end_byte):
        bits = np.unpackbits(np.asarray(data[start_byte:end_byte], np.uint8))
        pad = np.concatenate([bits, np.zeros(16, np.uint8)]).astype(np.int32)
        w = np.zeros(len(bits) + 1, np.int32)
        for i in range(16):
            w = (w << 1) | pad[i:i + len(w)]
        self.w, self.base, self.p = w.tolist(), start_byte * 8, start_byte * 8

    def peek(self, n):
        i = self.p - self.base
        return self.w[i] >> (16 - n) if i < len(self.w) else 0

    def get(self, n):
        v = self.peek(n)
        self.p += n
        return v


def _decode(t, br):
    e = int(t[br.peek(jpeg.LOOK_BITS)])
    if e >> 8:
        br.p += e >> 8
        return e & 255
    code = br.peek(16)
    for ln in range(jpeg.LOOK_BITS + 1, 17):
        c = code >> (16 - ln)
        if c <= t[512 + ln]:
            br.p += ln
            return int(t[548 + c + t[530 + ln]])
    br.p += 16
    return 0


def _extend(r, s):
    return r - (1 << s) + 1 if r < (1 << (s - 1)) else r


class Scan:
    """What the entropy decode of a file went through: `coef` int16 [n_blocks, 64] (natural order, MCU order),
    `starts` int64 [n_blocks] bit position in info.stream of each block's first symbol, `dc_cat` / `ac_cat` the largest
    DC-difference / AC magnitude category coded, `zrl_run` the longest run of consecutive ZRL symbols."""
    __slots__ = ("coef", "starts", "dc_cat", "ac_cat", "zrl_run")


def scan(info):
    sc = Scan()
    out = np.zeros((info.n_blocks, 64), np.int16)
    sc.coef, sc.starts = out, np.zeros(info.n_blocks, np.int64)
    sc.dc_cat = sc.ac_cat = sc.zrl_run = 0
    mcus = info.restart if info.restart else info.mcux * info.mcuy
    bounds = list(info.seg_start) + [len(info.stream)]
    for s in range(info.n_seg):
        br = _Bits(info.stream, bounds[s], bounds[s + 1])
        pred = [0, 0, 0]
        first = s * mcus * info.bpm
        last = min((s + 1) * mcus, info.mcux * info.mcuy) * info.bpm
        for g in range(first, last):
            ci = info.blocks[g % info.bpm][0]
            dc, ac = info.huff[2 * ci], info.huff[2 * ci + 1]
            sc.starts[g] = br.p
            n = _decode(dc, br)
            sc.dc_cat = max(sc.dc_cat, n)
            if n:
                pred[ci] += _extend(br.get(n), n)
            out[g, 0] = np.int16(np.int32(pred[ci]).astype(np.int16))
            k, zrl = 1, 0
            while k < 64:
                rs = _decode(ac, br)
                r, n = rs >> 4, rs & 15
                if n:
                    k += r
                    out[g, NATURAL[k]] = _extend(br.get(n), n)
                    sc.ac_cat = max(sc.ac_cat, n)
                    zrl = 0
                elif r != 15:
                    break
                else:
                    k += 15
                    zrl += 1
                    sc.zrl_run = max(sc.zrl_run, zrl)
                k += 1
    return sc


def coefficients(info):
    """-> int16 [n_blocks, 64] quantised coefficients in natural order, blocks in MCU order (stage 1)."""
    return scan(info).coef


def _run_sub(info, huff, br, end_bit, st):
    """The symbols of one subsequence that start before `end_bit`, from state (bit position, block of the MCU, zig-zag
    index) -> exit state.  Counting mode of the device decoder's run_sub."""
    br.p, c, k = st
    while br.p < end_bit:
        ci = info.blocks[c][0]
        if k == 0:
            n = _decode(huff[2 * ci], br)  # advances br.p past the code
            br.p += n
            k = 1
        else:
            rs = _decode(huff[2 * ci + 1], br)
            r, n = rs >> 4, rs & 15
            if n:
                k += r + 1
                br.p += n
            elif r == 15:
                k += 16
            else:
                k = 64
        if k >= 64:
            k = 0
            c = (c + 1) % info.bpm
    return br.p, c, k


def sync_states(info, sub_bits=jpeg.SUB_BITS):
    """Rounds the parallel decode described in the header of csrc/jpeg.hip needs for this file: round 0 runs every
    subsequence from the guessed state (its start bit, block 0 of the MCU, coefficient 0); each further round re-runs
    subsequence j from j-1's exit state if that exit moved in the round before, and the scheme stops after the first
    round in which no exit moved (at most n + 1 rounds are tried).  -> (the count the device reports, the final exit
    state (bit position, block of the MCU, zig-zag index) of every subsequence)."""
    subs = info.subsequences(sub_bits)
    n = len(subs)
    bounds = list(info.seg_start) + [len(info.stream)]
    readers = [_Bits(info.stream, bounds[s], bounds[s + 1]) for s in range(info.n_seg)]
    br = [readers[s] for s in np.cumsum(subs[:, 5]) - 1]
    huff = [t.tolist() for t in info.huff]  # plain lists: the loop below reads them a symbol at a time
    subs = subs.tolist()
    ex = [_run_sub(info, huff, br[j], subs[j][1], (subs[j][0], 0, 0)) for j in range(n)]
    moved = [True] * n
    rounds = 1
    while rounds <= n + 1:
        nex, nmoved = list(ex), [False] * n
        for j in range(n):
            if not subs[j][5] and moved[j - 1]:
                nex[j] = _run_sub(info, huff, br[j], subs[j][1], ex[j - 1])
                nmoved[j] = nex[j] != ex[j]
        ex, moved = nex, nmoved
        if not any(moved):
            break
        rounds += 1
    return rounds, ex


def sync_rounds(info, sub_bits=jpeg.SUB_BITS):
    """Synchronisation rounds of the parallel decode (see sync_states)."""
    return sync_states(info, sub_bits)[0]


C = dict(f0298=2446, f0390=3196, f0541=4433, f0765=6270, f0899=7373, f1175=9633, f1501=12299, f1847=15137,
         f1961=16069, f2053=16819, f2562=20995, f3072=25172)


def _idct_1d(x0, x1, x2, x3, x4, x5, x6, x7, shift):
    """jidctint's even / odd butterfly on int64 arrays; `shift` = the pass's descale."""
    z1 = (x2 + x6) * C["f0541"]
    t2 = z1 - x6 * C["f1847"]
    t3 = z1 + x2 * C["f0765"]
    t0 = (x0 + x4) << 13
    t1 = (x0 - x4) << 13
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    o0, o1, o2, o3 = x7, x5, x3, x1
    z1, z2, z3, z4 = o0 + o3, o1 + o2, o0 + o2, o1 + o3
    z5 = (z3 + z4) * C["f1175"]
    o0, o1, o2, o3 = o0 * C["f0298"], o1 * C["f2053"], o2 * C["f3072"], o3 * C["f1501"]
    z1, z2, z3, z4 = -z1 * C["f0899"], -z2 * C["f2562"], -z3 * C["f1961"] + z5, -z4 * C["f0390"] + z5
    o0, o1, o2, o3 = o0 + z1 + z3, o1 + z2 + z4, o2 + z2 + z3, o3 + z1 + z4
    r = 1 << (shift - 1)
    return [(t10 + o3 + r) >> shift, (t11 + o2 + r) >> shift, (t12 + o1 + r) >> shift, (t13 + o0 + r) >> shift,
            (t13 - o0 + r) >> shift, (t12 - o1 + r) >> shift, (t11 - o2 + r) >> shift, (t10 - o3 + r) >> shift]


def idct(coef, q):
    """int16 [N,64] natural-order coefficients, int32 [N,64] quantisation -> uint8 [N,8,8] (libjpeg jpeg_idct_islow,
    range limit included; the all-zero-AC shortcuts of jidctint give the same values as the full butterfly)."""
    x = (coef.astype(np.int64) * q).reshape(-1, 8, 8)
    cols = _idct_1d(*[x[:, r, :] for r in range(8)], 13 - 2)  # pass 1 over columns: rows of output index r
    ws = np.stack(cols, 1)  # [N, 8(row), 8(col)]
    rows = _idct_1d(*[ws[:, :, c] for c in range(8)], 13 + 2 + 3)
    v = np.stack(rows, 2) & 1023
    v = np.where(v < 512, v, v - 1024) + 128
    return np.clip(v, 0, 255).astype(np.uint8)


def planes(info, coef):
    """Stage 2: uint8 component planes padded to whole MCUs."""
    out = []
    pix = idct(coef, info.quant[[info.blocks[g % info.bpm][0] for g in range(info.n_blocks)]])
    for ci, (hs, vs) in enumerate(info.samp):
        p = np.zeros((info.mcuy * vs * 8, info.mcux * hs * 8), np.uint8)
        for g in range(info.n_blocks):
            c, bx, by = info.blocks[g % info.bpm]
            if c != ci:
                continue
            m = g // info.bpm
            X, Y = (m % info.mcux) * hs + bx, (m // info.mcux) * vs + by
            p[Y * 8:Y * 8 + 8, X * 8:X * 8 + 8] = pix[g]
        out.append(p)
    return out


def _upsample(p, cw, ch, hr, vr, W, H):
    """libjpeg-turbo's default upsampling of one chroma plane (real size cw x ch) by (hr, vr) to W x H."""
    v = p[:ch, :cw].astype(np.int64)
    if (hr, vr) == (1, 1):
        return v[:H, :W]
    if (hr, vr) == (1, 2):
        up = v[np.maximum(np.arange(ch) - 1, 0)]
        dn = v[np.minimum(np.arange(ch) + 1, ch - 1)]
        o = np.empty((2 * ch, cw), np.int64)
        o[0::2] = (3 * v + up + 1) >> 2
        o[1::2] = (3 * v + dn + 2) >> 2
        return o[:H, :W]
    if cw <= 2:  # narrow chroma: libjpeg-turbo replicates instead of the triangle filter
        return np.repeat(np.repeat(v, vr, 0), 2, 1)[:H, :W]
    if vr == 1:
        left = v[:, np.maximum(np.arange(cw) - 1, 0)]
        right = v[:, np.minimum(np.arange(cw) + 1, cw - 1)]
        o = np.empty((ch, 2 * cw), np.int64)
        o[:, 0::2] = (3 * v + left + 1) >> 2
        o[:, 1::2] = (3 * v + right + 2) >> 2
        o[:, 0] = v[:, 0]
        o[:, -1] = v[:, -1]
        return o[:H, :W]
    o = np.empty((2 * ch, 2 * cw), np.int64)
    for par, nb in ((0, np.maximum(np.arange(ch) - 1, 0)), (1, np.minimum(np.arange(ch) + 1, ch - 1))):
        cs = 3 * v + v[nb]
        left = cs[:, np.maximum(np.arange(cw) - 1, 0)]
        right = cs[:, np.minimum(np.arange(cw) + 1, cw - 1)]
        row = np.empty((ch, 2 * cw), np.int64)
        row[:, 0::2] = (3 * cs + left + 8) >> 4
        row[:, 1::2] = (3 * cs + right + 7) >> 4
        row[:, 0] = (cs[:, 0] * 4 + 8) >> 4
        row[:, -1] = (cs[:, -1] * 4 + 7) >> 4
        o[par::2] = row
    return o[:H, :W]


def decode(info):
    """Stages 1-3: JpegInfo -> uint8 [H,W,3], what PIL's Image.open(...).convert("RGB") gives."""
    W, H = info.width, info.height
    pl = planes(info, coefficients(info))
    y = pl[0][:H, :W].astype(np.int64)
    if info.ncomp == 1:
        return np.repeat(y[..., None].astype(np.uint8), 3, 2)
    hs, vs = info.samp[0]
    cw, ch = -(-W * 1 // hs), -(-H * 1 // vs)
    cb = _upsample(pl[1], cw, ch, hs, vs, W, H) - 128
    cr = _upsample(pl[2], cw, ch, hs, vs, W, H) - 128
    r = y + ((91881 * cr + 32768) >> 16)
    g = y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    return np.clip(np.stack([r, g, b], 2), 0, 255).astype(np.uint8)
