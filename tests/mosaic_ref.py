"""Reference for od_augment_mosaic (csrc/augment.hip): numpy f32, built on oracle/augment.py.  TEST INFRASTRUCTURE ONLY.

A tile of the frame with origin (X0, Y0) and extent Wt x Ht samples its source at u = ((x - X0) + 0.5) / Wt,
v = ((y - Y0) + 0.5) / Ht -- exactly the coordinates oracle.augment.augment uses for an output of Ht x Wt pixels -- so a
tile IS oracle.augment.augment(src, (Ht, Wt), tile parameters, no erasing).  The erase list then acts on the whole frame in
normalised output coordinates, with the oracle's comparison."""
from __future__ import annotations

import numpy as np

from oracle import augment as oaug


def tile_rects(split, out_hw):
    H, W = out_hw
    sx, sy = split
    return [(0, 0, sx, sy), (sx, 0, W - sx, sy), (0, sy, sx, H - sy), (sx, sy, W - sx, H - sy)]  # TL, TR, BL, BR


def mosaic(images4, out_hw, split, tiles, erase=()):
    """images4: four uint8 [h,w,3] arrays (None where the tile is empty); tiles: four dicts / objects with crop, flip,
    brightness, contrast, saturation; erase: [((x1,y1,x2,y2), (r,g,b))] -> uint8 [H,W,3]."""
    f = np.float32
    H, W = out_hw
    assert 1 <= split[0] <= W and 1 <= split[1] <= H
    out = np.zeros((H, W, 3), np.uint8)
    for img, p, (X0, Y0, Wt, Ht) in zip(images4, tiles, tile_rects(split, out_hw)):
        if Wt <= 0 or Ht <= 0:
            continue
        g = (lambda k: p[k]) if isinstance(p, dict) else (lambda k: getattr(p, k))
        out[Y0:Y0 + Ht, X0:X0 + Wt] = oaug.augment(img, (Ht, Wt), g("crop"), g("flip"), g("brightness"), g("contrast"),
                                                   g("saturation"), ())
    cu = (np.arange(W, dtype=f) + f(0.5)) / f(W)
    cv = (np.arange(H, dtype=f) + f(0.5)) / f(H)
    for (ex1, ey1, ex2, ey2), rgb in list(erase)[:3]:
        mx = (cu >= f(ex1)) & (cu < f(ex2))
        my = (cv >= f(ey1)) & (cv < f(ey2))
        out[np.ix_(my, mx)] = np.asarray(rgb, np.uint8)
    return out
