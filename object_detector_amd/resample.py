"""Pillow's BILINEAR resize as fixed-point coefficient tables (numpy + stdlib only: decode worker processes import it).

`Image.resize(size, Image.BILINEAR)` on 8-bit RGB is two separable passes, horizontal first, each with per-output-pixel
integer weights of 22 fraction bits: out = clip8((2^21 + sum(in * w)) >> 22).  A pass is skipped when its dimension does
not change.  Image.resize runs the vertical pass first when the image is more than 100 times as tall as wide and
shrinks vertically; each pass rounds to 8 bits, so the order shows in the result (`vertical_first`).  The tables are
computed here in double precision exactly as Pillow computes them (Resample.c, precompute_coeffs /
normalize_coeffs_8bpc) and cached per (source, destination) length; `resize` applies them with numpy and is
byte-identical to PIL.  The device resample kernels (csrc/jpeg.hip) read the same tables and follow the same order.
"""
from __future__ import annotations

import functools
import math

import numpy as np

PRECISION_BITS = 22


@functools.lru_cache(maxsize=256)
def coeffs(in_size: int, out_size: int):
    """-> (bounds int32 [out, 2] = (first source index, tap count), weights int32 [out, ksize]).  Read-only (cached)."""
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = 1.0 * fs  # bilinear support 1
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / fs
    bounds = np.zeros((out_size, 2), np.int32)
    kk = np.zeros((out_size, ksize), np.int32)
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        w = []
        for x in range(xmax):
            t = abs((x + xmin - center + 0.5) * ss)
            w.append(1.0 - t if t < 1.0 else 0.0)
        ww = sum(w) if w else 0.0
        for x in range(xmax):
            k = w[x] / ww if ww != 0.0 else w[x]
            kk[xx, x] = int(-0.5 + k * (1 << PRECISION_BITS)) if k < 0 else int(0.5 + k * (1 << PRECISION_BITS))
        bounds[xx] = (xmin, xmax)
    bounds.setflags(write=False)
    kk.setflags(write=False)
    return bounds, kk


def table(in_size: int, out_size: int) -> np.ndarray:
    """The device layout of one pass: int32 [out, 2 + ksize] rows of (first index, tap count, weights...)."""
    b, k = coeffs(in_size, out_size)
    return np.ascontiguousarray(np.concatenate([b, k], 1), np.int32)


def _pass(a: np.ndarray, axis: int, out_size: int) -> np.ndarray:
    b, k = coeffs(a.shape[axis], out_size)
    ksize = k.shape[1]
    idx = np.minimum(b[:, :1] + np.arange(ksize)[None, :], a.shape[axis] - 1)  # taps past xmax have weight 0
    g = np.take(a.astype(np.int64), idx, axis=axis)  # axis -> (out, ksize)
    shape = [1] * g.ndim
    shape[axis], shape[axis + 1] = out_size, ksize
    acc = (g * k.reshape(shape)).sum(axis + 1) + (1 << (PRECISION_BITS - 1))
    return np.clip(acc >> PRECISION_BITS, 0, 255).astype(np.uint8)


def resize(img: np.ndarray, size_wh) -> np.ndarray:
    """uint8 [H,W,C] -> uint8 [h,w,C]; equals np.asarray(Image.fromarray(img).resize(size_wh, Image.BILINEAR))."""
    w, h = size_wh
    out = np.asarray(img, np.uint8)
    if vertical_first(out.shape[:2], h):
        out = _pass(out, 0, h)
    if out.shape[1] != w:
        out = _pass(out, 1, w)
    if out.shape[0] != h:
        out = _pass(out, 0, h)
    return out


def vertical_first(src_hw, out_h) -> bool:
    """Image.resize's pass order: vertical first for a very tall, narrow image that shrinks vertically."""
    return src_hw[0] > 100 * src_hw[1] and out_h < src_hw[0]


def letterbox_size(src_hw, size_hw, keep_aspect):
    """(nw, nh) of the resized image inside the [H,W] canvas, and the (sx, sy) scale load_image returns."""
    H, Wd = size_hw
    if not keep_aspect:
        return (Wd, H), (1.0, 1.0)
    h, w = src_hw
    s = min(Wd / w, H / h)
    nw, nh = max(1, round(w * s)), max(1, round(h * s))
    return (nw, nh), (nw / Wd, nh / H)
