"""Test support: the crafted JPEG files of tests/test_jpeg_crafted_host.py and tests/test_gpu_jpeg_crafted.py, built by
jpeg_write from fixed seeds.  Every file is a valid baseline stream that PIL decodes; each group reaches one regime
Pillow's own encoder never writes.  `group(name)` -> {case name: bytes} (built once per process)."""
from __future__ import annotations

import functools

import numpy as np

import jpeg_write as jw

ONES = np.ones(64, np.int64)
FLAT4_DC = (bytes([0, 0, 0, 12] + [0] * 12), bytes(range(12)))  # every DC category at 4 bits
MIXED_AC = (jw.STD_AC_LUMA[0], jw.STD_AC_CHROMA[1])  # a third AC table: luma code lengths over the chroma symbol order
LONG = {(0, 0): jw.LONG_DC, (1, 0): jw.LONG_AC}
SHARED = dict(htabs=LONG, hsel=[(0, 0)] * 3)
Q1 = dict(qtabs={0: ONES}, qsel=[0, 0, 0])


def noise01(h, w, seed, channels=None):
    """0 / 255 noise: with quantisation 1 almost every coefficient is large."""
    shape = (h, w) if channels is None else (h, w, channels)
    return (np.random.default_rng(seed).integers(0, 2, shape) * 255).astype(np.uint8)


def picture(w, h, seed):
    """Ordinary content: 8-pixel patches of random colour plus noise."""
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, (h // 8 + 1, w // 8 + 1, 3))
    a = np.kron(base, np.ones((8, 8, 1), np.int64))[:h, :w]
    return np.clip(a + rng.integers(-40, 41, a.shape), 0, 255).astype(np.uint8)


def extreme(seed=11):
    """48 x 32 grey: black, white, one-pixel checkerboard and binary-noise blocks side by side."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:8, 0:8]
    kinds = [np.zeros((8, 8)), np.full((8, 8), 255), ((yy + xx) & 1) * 255, 255 - ((yy + xx) & 1) * 255]
    a = np.zeros((32, 48), np.uint8)
    for by in range(4):
        for bx in range(6):
            k = (by * 6 + bx) % 6
            a[by * 8:by * 8 + 8, bx * 8:bx * 8 + 8] = kinds[k] if k < 4 else rng.integers(0, 2, (8, 8)) * 255
    return a


def _long():
    g = noise01(24, 40, 1)
    c = noise01(24, 40, 2, 3)
    return {
        "long_grey": jw.encode_pixels(g, **Q1, htabs=LONG),
        "long_grey_declares_2x2": jw.encode_pixels(g, **Q1, htabs=LONG, grey_samp=0x22),
        "long_444": jw.encode_pixels(c, (1, 1), **Q1, **SHARED),
        "long_444_restart1": jw.encode_pixels(c, (1, 1), **Q1, **SHARED, restart=1),
    }


FLAT_HUFF = dict(htabs={(0, 0): FLAT4_DC, (1, 0): jw.LONG_AC}, hsel=[(0, 0)] * 3)  # DC 4 bits + EOB 16 bits per block
FLAT_SIZE = (400, 304)


def _flat():
    w, h = FLAT_SIZE
    a = np.full((h, w, 3), 128, np.uint8)
    return {
        "flat_420": jw.encode_pixels(a, (2, 2), **FLAT_HUFF),
        "flat_422": jw.encode_pixels(a, (2, 1), **FLAT_HUFF),
        "flat_grey": jw.encode_pixels(a[..., 0], **FLAT_HUFF),
    }


def _tables():
    htabs = {(0, 0): jw.STD_DC_LUMA, (0, 1): jw.STD_DC_CHROMA, (0, 3): FLAT4_DC,
             (1, 0): jw.STD_AC_LUMA, (1, 1): jw.STD_AC_CHROMA, (1, 2): MIXED_AC}
    kw = dict(htabs=htabs, hsel=[(0, 0), (1, 1), (3, 2)], qtabs={0: jw.STD_Q_LUMA // 4 + 1, 2: jw.STD_Q_CHROMA // 4 + 1,
                                                                   3: np.full(64, 7)}, qsel=[0, 2, 3])
    a = picture(37, 19, 3)
    return {
        "tables_422": jw.encode_pixels(a, (2, 1), **kw, ids=[7, 9, 200], restart=3),
        "tables_420": jw.encode_pixels(a, (2, 2), **kw, ids=[7, 9, 200], restart=3),
        "tables_444": jw.encode_pixels(a, (1, 1), **kw, ids=[200, 1, 0], restart=3),
    }


def _extreme():
    g = extreme()
    c = np.repeat(g[..., None], 3, 2)
    out = {}
    for q in (1, 2):
        kw = dict(qtabs={0: ONES * q}, qsel=[0, 0, 0])
        out[f"extreme_grey_q{q}"] = jw.encode_pixels(g, **kw)
        out[f"extreme_420_q{q}"] = jw.encode_pixels(c, (2, 2), **kw)
    return out


def coef_blocks(kind, n, seed):
    """int [n, 64] natural-order coefficient blocks of the coefficient-domain cases (magnitudes 1..3)."""
    rng = np.random.default_rng(seed)
    c = np.zeros((n, 64), np.int64)
    c[:, 0] = rng.integers(-3, 4, n)
    sign = rng.integers(0, 2, (n, 64)) * 2 - 1
    if kind in ("only63", "only49"):
        k = jw.ZIGZAG[int(kind[4:])]
        c[:, k] = sign[:, k] * rng.integers(1, 4, n)
    elif kind == "full":
        c[:, 1:] = sign[:, 1:]
    elif kind == "alternating":
        c[1::2, 1:] = sign[1::2, 1:]  # even blocks: a DC symbol and EOB
    return c


def _coef():
    out = {}
    for s, kind in enumerate(("only63", "only49", "full", "alternating")):
        kw = dict(qtabs={0: np.full(64, 8), 1: np.full(64, 5)})
        out[f"{kind}_grey"] = jw.encode_blocks(coef_blocks(kind, 12, s), 32, 24, None, **kw)
        out[f"{kind}_420"] = jw.encode_blocks(coef_blocks(kind, 24, 10 + s), 32, 32, (2, 2), **kw)
    return out


def _headers():
    a = picture(53, 37, 5)
    enc = functools.partial(jw.encode_pixels, a, (2, 2))
    q = {0: np.minimum(jw.STD_Q_LUMA, 255), 1: np.minimum(jw.STD_Q_CHROMA, 255)}
    return {
        "dqt16": enc(qtabs=q, q16=(0, 1), sof=0xC1),
        "one_segment": enc(one_segment=True),
        "tables_after_sof": enc(tables_after_sof=True),
        "extras": enc(extras=True),
        "fill": enc(fill=True, restart=2),
        "everything": enc(one_segment=True, tables_after_sof=True, extras=True, fill=True, restart=5, jfif=False),
        "dri_past_end": enc(restart=1000),
        "dri_zero": enc(restart=0),
    }


def _geometry():
    # MCUs are padded with zeros, not by edge replication: padded samples that reach the upsampling filter would show
    out = {}
    sizes = [(w, h) for w in (4, 5, 6) for h in (1, 2, 5)] + [(2000, 1), (1, 1)]
    for name, samp in (("420", (2, 2)), ("422", (2, 1))):
        for tn, kw in (("std", {}), ("long", SHARED)):
            for w, h in sizes:
                out[f"{name}_{tn}_{w}x{h}"] = jw.encode_pixels(picture(w, h, w * 7 + h), samp, "constant", **kw)
    for tn, kw in (("std", {}), ("long", dict(htabs=LONG))):
        out[f"grey_{tn}_8x1500"] = jw.encode_pixels(picture(8, 1500, 9)[..., 1], pad="constant", **kw)
    return out


H1V2_SIZES = [(13, 21), (16, 16), (1, 2), (3, 5), (9, 10)]  # 9 x 10: the last chroma row is not the plane's last


def _h1v2():
    return {f"h1v2_{w}x{h}": jw.encode_pixels(picture(w, h, 40 + w), (1, 2), "constant") for w, h in H1V2_SIZES}


_GROUPS = dict(long=_long, flat=_flat, tables=_tables, extreme=_extreme, coef=_coef, headers=_headers,
               geometry=_geometry, h1v2=_h1v2)
GROUPS = tuple(_GROUPS)


@functools.lru_cache(maxsize=None)
def group(name):
    return _GROUPS[name]()


@functools.lru_cache(maxsize=None)
def model_rounds(name, case):
    """jpeg_ref.sync_rounds of one file (computed once per process: a deep file costs seconds)."""
    import jpeg_ref
    from object_detector_amd import jpeg
    return jpeg_ref.sync_rounds(jpeg.parse(group(name)[case]))
