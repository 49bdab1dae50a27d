"""Test support: a baseline JPEG writer (numpy + stdlib) that can produce what Pillow's encoder never writes: any
Huffman table per slot, any selector per component, 8- or 16-bit quantisation tables in any slot, any component ids,
any restart interval, several tables per segment, tables after SOF, extra segments, fill bytes, luma sampling (1,2),
and a grey frame with any declared sampling byte.  Two entries: `encode_pixels` (float64 forward DCT, quantise) and
`encode_blocks` (quantised coefficients given directly).  Entropy data is byte-stuffed and padded with one-bits; no
table built here assigns the all-ones code."""
from __future__ import annotations

import struct

import numpy as np

# zig-zag index -> natural (row-major) index
ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,
                   7, 14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31,
                   39, 46, 53, 60, 61, 54, 47, 55, 62, 63])

AC_SYMBOLS = tuple(sorted([0x00, 0xF0] + [(r << 4) | s for r in range(16) for s in range(1, 11)]))
AC_UNUSED = (0x10, 0x20, 0x30, 0x40, 0x50, 0x60, 0x70)  # run / size 0 below ZRL: no encoder emits them


def _ac(counts, head):
    head = [int(x, 16) for x in head.split()]
    return bytes(counts), bytes(head + [s for s in AC_SYMBOLS if s not in head])


# the typical tables of ITU-T T.81 Annex K.3 (after the listed head, the AC symbols follow in ascending order)
STD_DC_LUMA = (bytes([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0]), bytes(range(12)))
STD_DC_CHROMA = (bytes([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0]), bytes(range(12)))
STD_AC_LUMA = _ac([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7D],
                  "01 02 03 00 04 11 05 12 21 31 41 06 13 51 61 07 22 71 14 32 81 91 a1 08 23 42 b1 c1 15 52 d1 f0 24 33 "
                  "62 72 82")
STD_AC_CHROMA = _ac([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77],
                    "00 01 02 03 11 04 05 21 31 06 12 41 51 07 61 71 13 22 32 81 08 14 42 91 a1 b1 c1 09 23 33 52 f0 15 "
                    "62 72 d1 0a 16 24 34 e1 25 f1")
STD_HUFF = {(0, 0): STD_DC_LUMA, (1, 0): STD_AC_LUMA, (0, 1): STD_DC_CHROMA, (1, 1): STD_AC_CHROMA}

# Annex K.1 quantisation tables, natural order
STD_Q_LUMA = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56,
                       14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
                       49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99])
STD_Q_CHROMA = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
                         47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32)


def long_table(symbols, unused=AC_UNUSED):
    """(counts, symbols) of a table whose codes of lengths 1..len(unused) go to symbols the data never uses and every
    symbol of `symbols` gets a 16-bit code: the longest codes the format allows for everything that is coded."""
    assert len(unused) <= 15 and not set(unused) & set(symbols)
    counts = [1] * len(unused) + [0] * (15 - len(unused)) + [len(symbols)]
    assert len(symbols) < (1 << (16 - len(unused)))  # the all-ones code stays free
    return bytes(counts), bytes(unused) + bytes(symbols)


LONG_AC = long_table(AC_SYMBOLS)
LONG_DC = long_table(tuple(range(12)), (12, 13, 14, 15))  # only 16 DC symbols are legal: four short codes


def code_map(counts, symbols, strict=True):
    """symbol -> (code, length), the canonical assignment of Annex C.  strict: refuse a table that assigns an all-ones
    code (the format reserves it, and libjpeg rejects such a table)."""
    out, code, p = {}, 0, 0
    for ln in range(1, 17):
        for _ in range(counts[ln - 1]):
            assert code < (1 << ln) - (1 if strict else 0), "the all-ones code is never assigned"
            out[symbols[p]] = (code, ln)
            p += 1
            code += 1
        code <<= 1
    assert p == len(symbols)
    return out


def _category(v):
    return int(abs(int(v))).bit_length()


def _bits(v, n):
    return v if v >= 0 else v + (1 << n) - 1


class _BitWriter:
    def __init__(self):
        self.parts = []

    def put(self, code, n):
        if n:
            self.parts.append(format(code, "0%db" % n))

    def flush(self):
        """-> the stuffed bytes of one entropy-coded segment, padded with one-bits."""
        s = "".join(self.parts)
        self.parts = []
        s += "1" * (-len(s) % 8)
        raw = int(s, 2).to_bytes(len(s) // 8, "big") if s else b""
        return raw.replace(b"\xff", b"\xff\x00")


def _segment(marker, payload):
    return bytes([0xFF, marker]) + struct.pack(">H", len(payload) + 2) + payload


def frame_geometry(width, height, samp):
    """samp: luma (h, v) of a colour frame, None for grey -> (mcux, mcuy, blocks of an MCU as (component, bx, by))."""
    if samp is None:
        return -(-width // 8), -(-height // 8), [(0, 0, 0)]
    hs, vs = samp
    blocks = [(0, bx, by) for by in range(vs) for bx in range(hs)] + [(1, 0, 0), (2, 0, 0)]
    return -(-width // (8 * hs)), -(-height // (8 * vs)), blocks


def encode_blocks(coef, width, height, samp=(2, 2), *, qtabs=None, qsel=None, q16=(), htabs=None, hsel=None, ids=None,
                  jfif=True, restart=None, grey_samp=0x11, one_segment=False, tables_after_sof=False, extras=False,
                  fill=False, sof=0xC0, strict=True):
    """Quantised coefficients int [n_blocks, 64] (natural order, blocks in MCU order) -> bytes of a baseline JPEG.
    samp        luma sampling of a 3-component frame, None for a grey one (`grey_samp` is its declared sampling byte)
    qtabs       {slot: int[64] natural order}; q16: slots written with 16-bit entries (Pq = 1); qsel: slot per component
    htabs       {(class, slot): (counts, symbols)}; hsel: (DC slot, AC slot) per component
    restart     None: no DRI segment; otherwise the DRI value (0 and values past the MCU count mean no markers)
    one_segment all tables in one DQT and one DHT segment; tables_after_sof: DQT / DHT between SOF and SOS
    extras      COM and APP5 segments between the others; fill: FF fill bytes in front of every RSTn and of EOI
    strict      False lets a Huffman table through that assigns an all-ones code (a file that decoders refuse)"""
    ncomp = 1 if samp is None else 3
    mcux, mcuy, blocks = frame_geometry(width, height, samp)
    bpm = len(blocks)
    coef = np.asarray(coef)
    assert coef.shape == (mcux * mcuy * bpm, 64)
    qtabs = {0: STD_Q_LUMA, 1: STD_Q_CHROMA} if qtabs is None else qtabs
    qsel = ([0, 1, 1] if qsel is None else list(qsel))[:ncomp]
    htabs = STD_HUFF if htabs is None else htabs
    hsel = ([(0, 0), (1, 1), (1, 1)] if hsel is None else list(hsel))[:ncomp]
    ids = ([1, 2, 3] if ids is None else list(ids))[:ncomp]
    codes = {key: code_map(*t, strict) for key, t in htabs.items()}

    dqt = []
    for slot in sorted(qtabs):
        q = np.asarray(qtabs[slot])[ZIGZAG]
        wide = slot in q16
        assert q.min() >= 1 and q.max() <= (65535 if wide else 255)
        dqt.append(bytes([(16 if wide else 0) | slot]) + q.astype(">u2" if wide else np.uint8).tobytes())
    dht = [bytes([(tc << 4) | slot]) + bytes(c) + bytes(v) for (tc, slot), (c, v) in sorted(htabs.items())]
    tables = []
    for marker, segs in ((0xDB, dqt), (0xC4, dht)):
        tables += [_segment(marker, b"".join(segs))] if one_segment else [_segment(marker, s) for s in segs]
    samp_bytes = [grey_samp] if samp is None else [(samp[0] << 4) | samp[1], 0x11, 0x11]
    frame = struct.pack(">BHHB", 8, height, width, ncomp)
    frame += b"".join(bytes([ids[c], samp_bytes[c], qsel[c]]) for c in range(ncomp))
    head = [_segment(0xE0, b"JFIF\0\x01\x01\0\0\x01\0\x01\0\0")] if jfif else []
    body = [_segment(sof, frame)] + tables if tables_after_sof else tables + [_segment(sof, frame)]
    if restart is not None:
        body.append(_segment(0xDD, struct.pack(">H", restart)))
    scan = bytes([ncomp]) + b"".join(bytes([ids[c], (hsel[c][0] << 4) | hsel[c][1]]) for c in range(ncomp))
    body.append(_segment(0xDA, scan + b"\0\x3f\0"))
    out = [b"\xff\xd8"] + head
    for k, s in enumerate(body):
        if extras:
            out.append(_segment(0xFE, b"comment %d" % k) if k % 2 else _segment(0xE5, b"\xff\xd8 app5 \xff\xda %d" % k))
        out.append(s)

    bw = _BitWriter()
    pred = [0] * ncomp
    rst = 0
    for m in range(mcux * mcuy):
        if restart and m and m % restart == 0:
            out += [bw.flush(), b"\xff" * (2 if fill else 0), bytes([0xFF, 0xD0 + rst])]
            rst = (rst + 1) & 7
            pred = [0] * ncomp
        for b in range(bpm):
            ci = blocks[b][0]
            blk = coef[m * bpm + b][ZIGZAG]
            dc, ac = codes[0, hsel[ci][0]], codes[1, hsel[ci][1]]
            diff = int(blk[0]) - pred[ci]
            pred[ci] = int(blk[0])
            n = _category(diff)
            assert n <= 11, "DC difference out of range"
            bw.put(*dc[n])
            bw.put(_bits(diff, n), n)
            run = 0
            for k in range(1, 64):
                v = int(blk[k])
                if v == 0:
                    run += 1
                    continue
                while run > 15:
                    bw.put(*ac[0xF0])
                    run -= 16
                n = _category(v)
                assert n <= 10, "AC coefficient out of range"
                bw.put(*ac[(run << 4) | n])
                bw.put(_bits(v, n), n)
                run = 0
            if run:
                bw.put(*ac[0x00])
    out += [bw.flush(), b"\xff" * (2 if fill else 0), b"\xff\xd9"]
    return b"".join(out)


_T = np.arange(8)
_DCT = np.cos((2 * _T[None, :] + 1) * _T[:, None] * np.pi / 16) * np.where(_T == 0, np.sqrt(1 / 8), 0.5)[:, None]


def quantise(planes, width, height, samp, qtabs, qsel, pad="edge"):
    """Component planes (float, any size >= the component's) -> int [n_blocks, 64] in MCU order: padding to whole MCUs
    (`pad`: "edge" replication as encoders do, or "constant" zeros, which a decoder must keep out of the picture),
    level shift, float64 forward DCT, round(coefficient / q)."""
    mcux, mcuy, blocks = frame_geometry(width, height, samp)
    out = np.zeros((mcux * mcuy, len(blocks), 64), np.int64)
    for ci, p in enumerate(planes):
        hs, vs = samp if (ci == 0 and samp is not None) else (1, 1)
        ph, pw = mcuy * vs * 8, mcux * hs * 8
        p = np.asarray(p, np.float64)
        p = np.pad(p, ((0, max(0, ph - p.shape[0])), (0, max(0, pw - p.shape[1]))), mode=pad)[:ph, :pw] - 128.0
        b = p.reshape(mcuy, vs, 8, mcux, hs, 8).transpose(0, 3, 1, 4, 2, 5)  # [mcuy, mcux, by, bx, 8, 8]
        c = np.einsum("ui,...ij,vj->...uv", _DCT, b, _DCT).reshape(mcuy * mcux, vs * hs, 64)
        q = np.rint(c / np.asarray(qtabs[qsel[ci]], np.float64)).astype(np.int64)
        q[..., 0] = np.clip(q[..., 0], -1024, 1023)
        q[..., 1:] = np.clip(q[..., 1:], -1023, 1023)
        idx = [k for k, blk in enumerate(blocks) if blk[0] == ci]
        out[:, idx] = q
    return out.reshape(-1, 64)


def encode_pixels(img, samp=(2, 2), pad="edge", **kw):
    """uint8 [H,W,3] RGB (samp = luma sampling) or [H,W] grey (samp ignored) -> JPEG bytes (see encode_blocks).  Chroma
    is the box average of its luma footprint."""
    a = np.asarray(img, np.float64)
    height, width = a.shape[:2]
    qtabs = kw.get("qtabs") or {0: STD_Q_LUMA, 1: STD_Q_CHROMA}
    if a.ndim == 2:
        samp, planes = None, [a]
    else:
        hs, vs = samp
        r, g, b = a[..., 0], a[..., 1], a[..., 2]
        y = 0.299 * r + 0.587 * g + 0.114 * b
        planes = [y]
        for c in (128 - 0.168736 * r - 0.331264 * g + 0.5 * b, 128 + 0.5 * r - 0.418688 * g - 0.081312 * b):
            c = np.pad(c, ((0, -height % vs), (0, -width % hs)), mode="edge")
            planes.append(c.reshape(c.shape[0] // vs, vs, c.shape[1] // hs, hs).mean((1, 3)))
    qsel = list(kw.get("qsel") or [0, 1, 1])
    coef = quantise(planes, width, height, samp, qtabs, qsel, pad)
    return encode_blocks(coef, width, height, samp, **kw)
