"""Host side of the device JPEG decoder (numpy + stdlib only: decode worker threads / processes import it).

`parse(data)` walks the markers of a JPEG file and either returns a `JpegInfo` with everything the device needs (frame
geometry, quantisation tables, Huffman decode tables, the unstuffed entropy-coded data and where each restart interval
starts in it) or the reason the file takes the host fallback route.  Supported: SOF0 / SOF1 Huffman, 8-bit samples,
one interleaved scan, 1 component or 3 YCbCr components with luma sampling (1,1) / (2,1) / (2,2) / (1,2) and chroma
(1,1).  Everything else (progressive, arithmetic, 12-bit, CMYK / Adobe transform, multi-scan, no EOI, a header that does
not parse, a Huffman table libjpeg refuses) is decoded by PIL on the host.  The contract of `parse`: it returns a
JpegInfo or raises Fallback, whatever the bytes are; no other exception escapes.

Huffman decode tables (HUFF_INTS int32 per table, libjpeg's jdhuff.c scheme):
    [0, 512)    lookahead on the next 9 bits: (code length << 8) | symbol, 0 when the code is longer than 9 bits
    [512, 530)  maxcode[l], l = 0..17: largest code of length l (-1: none); maxcode[17] is a sentinel
    [530, 548)  valoffset[l]: index into huffval of code c of length l is c + valoffset[l]
    [548, 804)  huffval
"""
from __future__ import annotations

import time

import numpy as np

LOOK_BITS = 9
HUFF_INTS = 804
SUB_BITS = 1024  # bits per subsequence of the parallel Huffman decode
SUB_INTS = 8     # int32 per subsequence record: start bit, end bit, segment end bit, first block, end block, first?, 0, 0

# zig-zag index -> natural (row-major) index
ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,
                   7, 14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31,
                   39, 46, 53, 60, 61, 54, 47, 55, 62, 63], np.int32)

_SOF_OTHER = {0xC2, 0xC3, 0xC5, 0xC6, 0xC7, 0xC9, 0xCA, 0xCB, 0xCD, 0xCE, 0xCF}
_LUMA = {(1, 1), (2, 1), (2, 2), (1, 2)}
_HUFF_CACHE: dict = {}


class Fallback(Exception):
    """The file is outside the supported subset (the message says why)."""


class JpegInfo:
    __slots__ = ("width", "height", "ncomp", "samp", "quant", "huff", "restart", "mcux", "mcuy", "bpm", "blocks",
                 "stream", "seg_start", "parse_us")

    @property
    def n_blocks(self):
        return self.mcux * self.mcuy * self.bpm

    @property
    def n_seg(self):
        return len(self.seg_start)

    def subsequences(self, sub_bits=SUB_BITS):
        """int32 [n_sub, SUB_INTS]: the parallel decode's subsequences.  None crosses a restart interval; each carries
        its interval's end bit and block range, which bound every read and write of the device decoder."""
        seg_bits = np.append(self.seg_start, len(self.stream)).astype(np.int64) * 8
        lo, hi = seg_bits[:-1], seg_bits[1:]
        n = np.maximum(1, -(-(hi - lo) // sub_bits))
        seg = np.repeat(np.arange(len(lo)), n)
        first = np.concatenate([[0], np.cumsum(n)[:-1]])
        j = np.arange(int(n.sum())) - np.repeat(first, n)
        start = lo[seg] + j * sub_bits
        mcus = self.restart if self.restart else self.mcux * self.mcuy
        fb = seg * mcus * self.bpm
        eb = np.minimum((seg + 1) * mcus, self.mcux * self.mcuy) * self.bpm
        rec = np.zeros((len(seg), SUB_INTS), np.int32)
        rec[:, 0] = start
        rec[:, 1] = np.minimum(start + sub_bits, hi[seg])
        rec[:, 2] = hi[seg]
        rec[:, 3] = fb
        rec[:, 4] = eb
        rec[:, 5] = j == 0
        return rec


def _u16(b, i):
    return (b[i] << 8) | b[i + 1]


def huff_table(counts: bytes, vals: bytes, is_dc: bool) -> np.ndarray:
    """DHT (16 code-length counts + symbols) -> int32 [HUFF_INTS] decode table (cached by content)."""
    key = (counts, vals, is_dc)
    t = _HUFF_CACHE.get(key)
    if t is not None:
        return t
    if len(vals) > 256 or (is_dc and any(v > 15 for v in vals)):
        raise Fallback("bad Huffman table")
    t = np.zeros(HUFF_INTS, np.int32)
    maxcode = t[512:530]
    valoff = t[530:548]
    maxcode[:] = -1
    maxcode[17] = 0x7FFFFFFF
    code, p = 0, 0
    for ln in range(1, 17):
        n = counts[ln - 1]
        if n:
            valoff[ln] = p - code
            for _ in range(n):
                if ln <= LOOK_BITS:
                    sh = LOOK_BITS - ln
                    t[code << sh:(code + 1) << sh] = (ln << 8) | vals[p]
                p += 1
                code += 1
            maxcode[ln] = code - 1
        if code >= (1 << ln):  # libjpeg's check (jdhuff.c): no code is all ones, so a complete length is refused too
            raise Fallback("bad Huffman table")
        code <<= 1
    t[548:548 + len(vals)] = np.frombuffer(vals, np.uint8)
    if len(_HUFF_CACHE) < 1024:
        _HUFF_CACHE[key] = t
    return t


def _entropy(buf: np.ndarray, pos: int):
    """Entropy-coded data from `pos` -> (unstuffed bytes, restart-marker numbers, segment starts, index of the marker
    that ends the scan).  Vectorised: FF 00 -> FF, fill FFs dropped, the stream cut at each RSTn."""
    d = buf[pos:]
    ff = np.flatnonzero(d[:-1] == 0xFF)
    nxt = d[ff + 1]
    fill = nxt == 0xFF
    rst = (nxt >= 0xD0) & (nxt <= 0xD7)
    ends = ff[~(fill | rst | (nxt == 0))]
    if len(ends) == 0:
        raise Fallback("no marker after the scan")
    end = int(ends[0])
    keep = ff < end
    ff, nxt, fill, rst = ff[keep], nxt[keep], fill[keep], rst[keep]
    mask = np.ones(end, bool)
    mask[ff[nxt == 0] + 1] = False  # the stuffed 00
    mask[ff[fill]] = False
    r = ff[rst]
    mask[r] = False
    mask[r + 1] = False
    stream = d[:end][mask]
    kept_before = np.cumsum(mask) - mask  # kept bytes before each position
    seg_start = np.concatenate([[0], kept_before[r]]).astype(np.int64) if len(r) else np.zeros(1, np.int64)
    return stream, (d[r + 1] - 0xD0).astype(np.int64), seg_start, pos + end


def parse(data) -> JpegInfo:
    """bytes of a JPEG file -> JpegInfo; raises Fallback for anything outside the supported subset."""
    t0 = time.perf_counter()
    b = bytes(data)
    buf = np.frombuffer(b, np.uint8)
    if len(b) < 4 or b[0] != 0xFF or b[1] != 0xD8:
        raise Fallback("not a JPEG")
    i = 2
    quant = {}
    dht = {}
    restart = 0
    frame = None
    scan = None
    jfif = adobe = False
    try:
        while True:
            if b[i] != 0xFF:
                raise Fallback("bad marker")
            while b[i] == 0xFF:
                i += 1
            m = b[i]
            i += 1
            if m == 0xD9:  # EOI
                break
            if m == 0x01 or 0xD0 <= m <= 0xD7:
                continue
            ln = _u16(b, i)
            seg = b[i + 2:i + ln]
            if len(seg) != ln - 2:
                raise Fallback("truncated")
            i += ln
            if m in (0xC0, 0xC1):
                if frame is not None:
                    raise Fallback("two frames")
                if seg[0] != 8:
                    raise Fallback("not 8-bit")
                h, w, nc = _u16(seg, 1), _u16(seg, 3), seg[5]
                comps = [(seg[6 + 3 * c], seg[7 + 3 * c] >> 4, seg[7 + 3 * c] & 15, seg[8 + 3 * c]) for c in range(nc)]
                frame = (h, w, comps)
            elif m in _SOF_OTHER:
                raise Fallback("progressive / arithmetic / lossless")
            elif m == 0xC4:
                k = 0
                while k < len(seg):
                    tc, th = seg[k] >> 4, seg[k] & 15
                    counts = seg[k + 1:k + 17]
                    n = sum(counts)
                    vals = seg[k + 17:k + 17 + n]
                    if tc > 1 or th > 3 or len(counts) != 16 or len(vals) != n:
                        raise Fallback("bad DHT")
                    dht[(tc, th)] = (counts, vals)
                    k += 17 + n
            elif m == 0xDB:
                k = 0
                while k < len(seg):
                    pq, tq = seg[k] >> 4, seg[k] & 15
                    nb = 128 if pq else 64
                    tab = seg[k + 1:k + 1 + nb]
                    if pq > 1 or tq > 3 or len(tab) != nb:
                        raise Fallback("bad DQT")
                    raw = np.frombuffer(tab, ">u2" if pq else np.uint8)
                    q = np.zeros(64, np.int32)
                    q[ZIGZAG] = raw
                    quant[tq] = q
                    k += 1 + nb
            elif m == 0xDD:
                restart = _u16(seg, 0)
            elif m == 0xE0 and seg[:5] == b"JFIF\0":
                jfif = True
            elif m == 0xEE and seg[:5] == b"Adobe":
                adobe = True
            elif m == 0xDA:
                if scan is not None:
                    raise Fallback("multi-scan")
                ns = seg[0]
                sc = [(seg[1 + 2 * c], seg[2 + 2 * c] >> 4, seg[2 + 2 * c] & 15) for c in range(ns)]
                ss, se, ahal = seg[1 + 2 * ns], seg[2 + 2 * ns], seg[3 + 2 * ns]
                if ss != 0 or se != 63 or ahal != 0:
                    raise Fallback("not a sequential scan")
                scan = (sc, {key: (v[0], v[1]) for key, v in dht.items()}, dict(quant), restart)
                stream, rst_no, seg_start, i = _entropy(buf, i)
            elif 0xC0 <= m <= 0xFE or m in (0xDC, 0xDE, 0xDF):
                pass  # APPn, COM, DNL/DHP/EXP: skipped
            else:
                raise Fallback("unknown marker")
    except IndexError:
        raise Fallback("truncated") from None
    if frame is None or scan is None:
        raise Fallback("no frame / scan")
    h, w, comps = frame
    sc, tabs, quant, restart = scan
    nc = len(comps)
    if adobe or nc not in (1, 3) or h == 0 or w == 0:
        raise Fallback("colour space")
    if nc == 3 and not jfif and [c[0] for c in comps] != [1, 2, 3]:
        raise Fallback("colour space")
    if [c[0] for c in sc] != [c[0] for c in comps]:
        raise Fallback("not one interleaved scan of all components")
    info = JpegInfo()
    info.width, info.height, info.ncomp = w, h, nc
    if nc == 1:
        samp = [(1, 1)]
        info.mcux, info.mcuy = -(-w // 8), -(-h // 8)
    else:
        samp = [(c[1], c[2]) for c in comps]
        if samp[0] not in _LUMA or samp[1] != (1, 1) or samp[2] != (1, 1):
            raise Fallback("sampling")
        info.mcux, info.mcuy = -(-w // (8 * samp[0][0])), -(-h // (8 * samp[0][1]))
    info.samp = samp
    blocks = []  # per block of an MCU: (component, x block, y block)
    for ci, (hs, vs) in enumerate(samp):
        blocks += [(ci, bx, by) for by in range(vs) for bx in range(hs)]
    info.blocks, info.bpm = blocks, len(blocks)
    try:
        info.quant = np.stack([quant[c[3]] for c in comps] + [quant[comps[0][3]]] * (3 - nc))
        huff = []
        for ci in range(3):
            _, td, ta = sc[min(ci, nc - 1)]
            huff.append(huff_table(*tabs[(0, td)], True))
            huff.append(huff_table(*tabs[(1, ta)], False))
    except KeyError:
        raise Fallback("missing table") from None
    info.huff = np.stack(huff)
    total = info.mcux * info.mcuy
    nseg = -(-total // restart) if restart else 1
    if len(seg_start) != nseg or (len(rst_no) and not np.array_equal(rst_no, np.arange(len(rst_no)) % 8)):
        raise Fallback("restart markers")
    info.restart, info.stream, info.seg_start = restart, stream, seg_start
    info.parse_us = (time.perf_counter() - t0) * 1e6
    return info


def parse_file(path):
    with open(path, "rb") as f:
        return parse(f.read())
