"""Reference for od_augment_warp (csrc/augment.hip, K14b): numpy f32, op for op.  TEST INFRASTRUCTURE ONLY.

`sample` is a POINT sampler: aug_sample of the kernel at arbitrary normalised positions (u, v) -- crop -> clamp -> bilinear
-> saturation / contrast / brightness -> round half up -> clamp -- where oracle.augment.augment evaluates the same sequence
on the regular grid of an output image (tests/test_warp_host.py ties the two together byte for byte).  `warp` puts the
frozen per-pixel semantics of include/odhip.h on top, in that operation order:
  1. px = x + 0.5, py = y + 0.5
  2. fx = (a0*px + a1*py) + a2, fy = (a3*px + a4*py) + a5
  3. outside [0, W) x [0, H): fill_rgb, no colour matrix
  4. tile by fx >= split_x, fy >= split_y; u = (fx - X0) / Wt, v = (fy - Y0) / Ht; c = sample(tile, u, v);
     t = ((k0*c0 + k1*c1) + k2*c2) + k3, round half up, clamp
  5. two frames: t = A*mix_a + B*mix_b, round half up, clamp
  6. erase list on normalised output coordinates
Every product and sum below is one f32 operation on f32 operands (numpy does not contract)."""
from __future__ import annotations

import numpy as np

f = np.float32


def _get(p, k):
    return p[k] if isinstance(p, dict) else getattr(p, k)


def _round_u8(t):
    return np.minimum(np.maximum(np.floor(t + f(0.5)), f(0)), f(255))


def sample(img, p, u, v):
    """img uint8 [h,w,3]; p: dict / object with crop, flip, brightness, contrast, saturation; u, v: f32 arrays of one shape
    -> f32 [..., 3] of whole numbers in [0, 255]."""
    u, v = np.asarray(u, f), np.asarray(v, f)
    sh, sw = img.shape[:2]
    if _get(p, "flip"):
        u = f(1.0) - u
    x1, y1, x2, y2 = (f(c) for c in _get(p, "crop"))
    sx = (x1 + u * (x2 - x1)) * f(sw) - f(0.5)
    sy = (y1 + v * (y2 - y1)) * f(sh) - f(0.5)
    sx = np.minimum(np.maximum(sx, f(0)), f(sw - 1))
    sy = np.minimum(np.maximum(sy, f(0)), f(sh - 1))
    x0 = np.floor(sx).astype(np.int64)
    y0 = np.floor(sy).astype(np.int64)
    x1i = np.minimum(x0 + 1, sw - 1)
    y1i = np.minimum(y0 + 1, sh - 1)
    fx = (sx - x0.astype(f))[..., None]
    fy = (sy - y0.astype(f))[..., None]
    im = img[..., :3].astype(f)
    p00, p01, p10, p11 = im[y0, x0], im[y0, x1i], im[y1i, x0], im[y1i, x1i]
    top = p00 + (p01 - p00) * fx
    bot = p10 + (p11 - p10) * fx
    c = top + (bot - top) * fy
    gray = (c[..., 0] * f(0.299) + c[..., 1] * f(0.587)) + c[..., 2] * f(0.114)
    t = gray[..., None] + (c - gray[..., None]) * f(_get(p, "saturation"))
    t = (t - f(127.5)) * f(_get(p, "contrast")) + f(127.5)
    t = t + f(_get(p, "brightness"))
    return _round_u8(t)


def frame_colour(images4, out_hw, split, tiles, a, k, fill):
    """One frame's finished colour at every output pixel (steps 1-4) -> f32 [H,W,3]."""
    H, W = out_hw
    a = np.asarray(a, f).reshape(6)
    k = np.asarray(k, f).reshape(3, 4)
    px = (np.arange(W, dtype=f) + f(0.5))[None, :]
    py = (np.arange(H, dtype=f) + f(0.5))[:, None]
    fx = (a[0] * px + a[1] * py) + a[2]
    fy = (a[3] * px + a[4] * py) + a[5]
    outside = (fx < f(0)) | (fx >= f(W)) | (fy < f(0)) | (fy >= f(H))
    sx, sy = split
    right, low = fx >= f(sx), fy >= f(sy)
    out = np.empty((H, W, 3), f)
    out[...] = np.asarray(fill[:3], np.uint8).astype(f)
    rects = [(0, 0, sx, sy), (sx, 0, W - sx, sy), (0, sy, sx, H - sy), (sx, sy, W - sx, H - sy)]  # TL, TR, BL, BR
    for t, (X0, Y0, Wt, Ht) in enumerate(rects):
        m = ~outside & (right == bool(t & 1)) & (low == bool(t & 2))
        if not m.any():
            continue
        assert Wt > 0 and Ht > 0
        u = (fx[m] - f(X0)) / f(Wt)
        v = (fy[m] - f(Y0)) / f(Ht)
        c = sample(images4[t], tiles[t], u, v)
        for ch in range(3):
            out[..., ch][m] = _round_u8(((k[ch, 0] * c[:, 0] + k[ch, 1] * c[:, 1]) + k[ch, 2] * c[:, 2]) + k[ch, 3])
    return out


def warp(frames, out_hw, mix=(1.0, 0.0), fill=(114, 114, 114), erase=()):
    """frames: one or two dicts with images4 (four uint8 arrays, None where unused), split, tiles, a (6), k (3x4);
    erase: [((x1,y1,x2,y2), (r,g,b))] -> uint8 [H,W,3]."""
    H, W = out_hw
    assert len(frames) in (1, 2)
    cols = [frame_colour(fr["images4"], out_hw, fr["split"], fr["tiles"], fr["a"], fr["k"], fill) for fr in frames]
    c = cols[0]
    if len(frames) == 2:
        c = _round_u8(c * f(mix[0]) + cols[1] * f(mix[1]))
    out = c.astype(np.uint8)
    cu = (np.arange(W, dtype=f) + f(0.5)) / f(W)
    cv = (np.arange(H, dtype=f) + f(0.5)) / f(H)
    for (ex1, ey1, ex2, ey2), rgb in list(erase)[:3]:
        mx = (cu >= f(ex1)) & (cu < f(ex2))
        my = (cv >= f(ey1)) & (cv < f(ey2))
        out[np.ix_(my, mx)] = np.asarray(rgb, np.uint8)
    return out


def from_params(wp, images, out_hw):
    """od_gen.WarpParams + its sources (one 4-tuple of uint8 arrays per frame) -> uint8 [H,W,3]."""
    frames = [{"images4": q, "split": mp.split, "tiles": mp.tiles, "a": a, "k": k}
              for q, mp, a, k in zip(images, wp.frames, wp.inv, wp.colour)]
    return warp(frames, out_hw, wp.mix, wp.fill, wp.erase)
