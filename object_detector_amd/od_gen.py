"""`tk.dl.od.od_gen`: training data generator (reference check_generator.py:17-18, check_assign.py:21-22).

    gen = create_generator((512, 512), preprocess_input=lambda x: x, encode_truth=od.pb.encode_truth)
    g, steps = gen.flow(X, y, data_augmentation=True)      # infinite iterator of (X_batch, y_batch)

Augmentation list is [BUILD-DEFINED] (docs/MODEL.md:60-64 names Random Erasing "and anything else at hand", erasing
constrained so that boxes are not hidden too much): horizontal flip, random crop/zoom that keeps every box centre,
brightness / contrast / saturation jitter, Random Erasing limited to <= 40 % of any box.  Augmentation PARAMETERS are
sampled on the host (numpy Generator, seeded); the pixel work runs on the device through od_augment_batch when a GPU
is present (`device=`), prior-box encoding always runs on the device (encode_truth = od.pb.encode_truth).

Mosaic [BUILD-DEFINED, opt-in: `create_generator(..., mosaic=P, device=...)`]: with probability P an output image is
composed of four images (the batch's own + three drawn from the whole dataset) around a split point; the pixel work is one
od_augment_mosaic launch that gathers from the four sources where they live (device_cache: in HBM).  The numbers, all named
arguments of `sample_mosaic` with these defaults:
  split_range = (0.3, 0.7)  the split point is uniform over this part of the frame, per axis, in whole output pixels
  max_aspect  = 1.5         a tile's crop is narrowed about its centre (widened on the other axis only where it would
                            get thinner than a source pixel) until x-scale / y-scale of the tile lies in [1/1.5, 1.5]
  drop_frac   = 0.1         a box of which less than this share stays inside its tile is dropped
  ignore_frac = 0.4         below this share (and >= drop_frac) the box is a sliver: kept as an ignore region
                            (difficults = True) if ignore_regions=True, dropped otherwise -- never trained as a positive
  min_px      = 2.0         a clipped box thinner than this many output pixels is dropped
Each tile gets its own `sample_params` draw (crop / flip / colour, no erasing); Random Erasing acts once on the whole frame.
More than pb.GMAX boxes after merging: ignore regions go first, smallest area first, then ordinary boxes, smallest first.
`Generator.stats` counts mosaics, boxes_dropped, boxes_ignored, boxes_over_gmax.

Warp / HSV / MixUp [BUILD-DEFINED, opt-in, need `device=`]: `create_generator(..., affine=dict(degrees=0, translate=0.1,
scale=0.5, shear=0), hsv=(h, s, v), mixup=P, mixup_beta=8.0, fill=(114, 114, 114))`.  Any of the three switched on sends
every augmented batch through ONE od_augment_warp launch (csrc/augment.hip, K14b; the per-pixel semantics are frozen in
include/odhip.h): each output image is one or two FRAMES -- a frame is a mosaic or, as the degenerate mosaic, a single image --
seen through an inverse affine matrix and a 3x4 colour matrix, blended with the MixUp weights, `fill` where a frame does not
reach, one erase list at the end.  An image that takes none of the options rides along as identity.  Draw order per output
image (all from the generator's one rng):
  1. the frame: the mosaic decision (only if mosaic > 0) and sample_mosaic, or sample_params -- as without these options, but
     with erasing OFF
  2. the affine (sample_affine: theta, zoom, shear x, shear y, tx, ty) if `affine` is given; boxes follow through warp_boxes
  3. the HSV jitter (sample_hsv: hue, sat, val) if `hsv` is given
  4. the MixUp decision (only if mixup > 0)
  5. if taken: the partner's index over the whole dataset, the partner's whole frame (steps 1-3; it may be a mosaic), then
     r ~ Beta(mixup_beta, mixup_beta); mix_a = f32(r), mix_b = f32(1) - mix_a; the annotations are concatenated and cut to
     pb.GMAX by mosaic_boxes' rule
  6. one erase list for the final image, against the final boxes (if random_erasing: a uniform draw < 0.5, then _sample_erase)
warp_boxes: a box's four corners go through the forward matrix, the enclosing box is clipped to the frame, and
visible = clipped / enclosing area decides with mosaic's drop_frac / ignore_frac / min_px; a clipped box with sides in a ratio
above max_aspect = 20 is dropped too.  `Generator.stats` gains "warps" (output images of this path) and "mixups" (those made of
two frames) only when an option is on; with the options at their defaults nothing changes: not a draw, not a key.
"""
from __future__ import annotations

import math

import numpy as np

from .pb import GMAX, ObjectsAnnotation


class AugParams:
    """Per-image augmentation parameters (sampled on the host, consumed by the pixel kernel / host path)."""
    __slots__ = ("crop", "flip", "brightness", "contrast", "saturation", "erase")

    def __init__(self):
        self.crop = (0.0, 0.0, 1.0, 1.0)  # x1,y1,x2,y2 in normalised source coordinates
        self.flip = False
        self.brightness = 0.0   # additive, in [0,255] units
        self.contrast = 1.0
        self.saturation = 1.0
        self.erase = []         # [(x1,y1,x2,y2 in normalised OUTPUT coords, (r,g,b))]


def sample_params(rng: np.random.Generator, ann: ObjectsAnnotation, random_erasing=True) -> AugParams:
    p = AugParams()
    b = ann.bboxes
    if rng.random() < 0.5 and len(b):  # crop/zoom keeping all box centres inside
        cx = (b[:, 0] + b[:, 2]) / 2
        cy = (b[:, 1] + b[:, 3]) / 2
        x1 = rng.uniform(0, max(1e-6, min(cx.min(), 0.3)))
        y1 = rng.uniform(0, max(1e-6, min(cy.min(), 0.3)))
        x2 = rng.uniform(min(1 - 1e-6, max(cx.max(), 0.7)), 1)
        y2 = rng.uniform(min(1 - 1e-6, max(cy.max(), 0.7)), 1)
        p.crop = (float(x1), float(y1), float(x2), float(y2))
    p.flip = bool(rng.random() < 0.5)
    p.brightness = float(rng.uniform(-32, 32)) if rng.random() < 0.5 else 0.0
    p.contrast = float(rng.uniform(0.6, 1.4)) if rng.random() < 0.5 else 1.0
    p.saturation = float(rng.uniform(0.6, 1.4)) if rng.random() < 0.5 else 1.0
    if random_erasing and rng.random() < 0.5:
        p.erase = _sample_erase(rng, transform_boxes(b, p))
    return p


def _sample_erase(rng, nb):
    """1-3 Random-Erasing rectangles in normalised output coordinates, none hiding more than 40 % of a box of `nb`."""
    erase = []
    for _ in range(int(rng.integers(1, 4))):
        for _try in range(10):
            area = rng.uniform(0.02, 0.2)
            ar = math.exp(rng.uniform(math.log(0.3), math.log(1 / 0.3)))
            w, h = min(1.0, math.sqrt(area * ar)), min(1.0, math.sqrt(area / ar))
            x1, y1 = rng.uniform(0, 1 - w), rng.uniform(0, 1 - h)
            r = np.array([x1, y1, x1 + w, y1 + h], np.float32)
            if _hidden_fraction(r, nb) <= 0.4:  # box-aware constraint
                erase.append((tuple(float(v) for v in r), tuple(int(v) for v in rng.integers(0, 256, 3))))
                break
    return erase


def _hidden_fraction(rect, boxes):
    if not len(boxes):
        return 0.0
    iw = np.clip(np.minimum(rect[2], boxes[:, 2]) - np.maximum(rect[0], boxes[:, 0]), 0, None)
    ih = np.clip(np.minimum(rect[3], boxes[:, 3]) - np.maximum(rect[1], boxes[:, 1]), 0, None)
    area = np.maximum((boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1]), 1e-12)
    return float((iw * ih / area).max())


def transform_boxes(bboxes, p: AugParams, clip=True):
    """Boxes follow the crop then the flip; clipped to the frame (clip=False: as they fall, for the visible share)."""
    b = np.asarray(bboxes, np.float32).reshape(-1, 4).copy()
    x1, y1, x2, y2 = p.crop
    b[:, [0, 2]] = (b[:, [0, 2]] - x1) / (x2 - x1)
    b[:, [1, 3]] = (b[:, [1, 3]] - y1) / (y2 - y1)
    if p.flip:
        b[:, [0, 2]] = 1.0 - b[:, [2, 0]]
    return np.clip(b, 0.0, 1.0) if clip else b


class MosaicParams:
    """One mosaic output image: the split point in output pixels, the four tiles' parameters (TL, TR, BL, BR; no erasing
    of their own) and the whole-frame erase list."""
    __slots__ = ("split", "tiles", "erase")

    def __init__(self, split, tiles, erase=()):
        self.split = (int(split[0]), int(split[1]))  # (split_x, split_y)
        self.tiles = list(tiles)
        self.erase = list(erase)

    @classmethod
    def single(cls, p: AugParams, input_size):
        """The degenerate mosaic of one image: split = (W, H), p in the TL tile, p's erase list on the frame -- the output
        of od_augment_mosaic equals od_augment_batch(p) byte for byte."""
        q = AugParams()
        q.crop, q.flip, q.brightness, q.contrast, q.saturation = p.crop, p.flip, p.brightness, p.contrast, p.saturation
        return cls((input_size[1], input_size[0]), [q, AugParams(), AugParams(), AugParams()], p.erase)


def tile_rects(split, input_size):
    """-> the four tiles' (X0, Y0, Wt, Ht) in output pixels: TL, TR, BL, BR."""
    H, W = input_size
    sx, sy = split
    return [(0, 0, sx, sy), (sx, 0, W - sx, sy), (0, sy, sx, H - sy), (sx, sy, W - sx, H - sy)]


def _span(a, b, new_len):
    """[a, b] resized to new_len (<= 1) about its centre, shifted back into [0, 1]."""
    new_len = min(float(new_len), 1.0)
    c = 0.5 * (a + b)
    a, b = c - 0.5 * new_len, c + 0.5 * new_len
    if a < 0.0:
        a, b = 0.0, new_len
    if b > 1.0:
        a, b = 1.0 - new_len, 1.0
    return a, b


def fit_tile_aspect(crop, src_wh, tile_wh, max_aspect=1.5):
    """Crop (normalised source coordinates) whose picture, stretched over a tile of tile_wh pixels, is distorted by at most
    max_aspect: d = x-scale / y-scale in [1/max_aspect, max_aspect].  The crop is NARROWED about its centre on the axis that
    is squeezed -- a mosaic tile is a cut-out of its image, and what the cut leaves of an object is what mosaic_boxes
    weighs -- and only a crop that would become thinner than one source pixel is widened on the other axis instead."""
    x1, y1, x2, y2 = (float(v) for v in crop)
    sw, sh = max(1.0, float(src_wh[0])), max(1.0, float(src_wh[1]))
    tw, th = float(tile_wh[0]), float(tile_wh[1])
    if tw <= 0 or th <= 0:
        return (x1, y1, x2, y2)
    d = (tw / ((x2 - x1) * sw)) / (th / ((y2 - y1) * sh))
    if d > max_aspect:      # stretched in x: show less of the source's height
        want = (y2 - y1) * max_aspect / d
        if want * sh >= 1.0:
            y1, y2 = _span(y1, y2, want)
        else:
            x1, x2 = _span(x1, x2, (x2 - x1) * d / max_aspect)
    elif d < 1.0 / max_aspect:
        want = (x2 - x1) * d * max_aspect
        if want * sw >= 1.0:
            x1, x2 = _span(x1, x2, want)
        else:
            y1, y2 = _span(y1, y2, (y2 - y1) / (d * max_aspect))
    return (x1, y1, x2, y2)


def mosaic_boxes(anns4, tiles, split, input_size, drop_frac=0.1, ignore_frac=0.4, min_px=2.0, ignore_regions=False,
                 gmax=GMAX, stats=None):
    """The merged annotation of a mosaic: every box follows its tile (transform_boxes into tile coordinates, through the
    tile rectangle into output coordinates, clipped to the tile), then visible = clipped area / unclipped area decides:
    < drop_frac or thinner than min_px output pixels -> dropped; < ignore_frac -> an ignore region (difficults = True) with
    ignore_regions, dropped without; else kept.  Input difficults are carried through.  More than gmax boxes: flagged
    boxes go first, smallest area first, then unflagged ones, smallest first (ties: lowest index)."""
    H, W = input_size
    st = stats if stats is not None else {}
    rows = []  # the tiles that show objects: (annotation, per-box row of tile numbers)
    for a, p, (X0, Y0, Wt, Ht) in zip(anns4, tiles, tile_rects(split, input_size)):
        if a.num_objects == 0:
            continue
        if Wt <= 0 or Ht <= 0:  # an empty tile shows nothing
            st["boxes_dropped"] = st.get("boxes_dropped", 0) + a.num_objects
            continue
        x1, y1, x2, y2 = p.crop
        rows.append((a, (x1, y1, x2 - x1, y2 - y1, float(p.flip), X0, Y0, Wt, Ht)))
    if not rows:
        return ObjectsAnnotation(anns4[0].path, W, H)
    # all tiles' boxes in one pass (float64; the arithmetic of transform_boxes, unclipped and clipped)
    t = np.repeat(np.array([r[1] for r in rows], np.float64), [r[0].num_objects for r in rows], axis=0)
    b = np.concatenate([r[0].bboxes for r in rows]).astype(np.float64)
    rx = (b[:, [0, 2]] - t[:, 0:1]) / t[:, 2:3]
    ry = (b[:, [1, 3]] - t[:, 1:2]) / t[:, 3:4]
    rx = np.where(t[:, 4:5] > 0, 1.0 - rx[:, ::-1], rx)
    cx, cy = np.clip(rx, 0.0, 1.0), np.clip(ry, 0.0, 1.0)
    area_raw = (rx[:, 1] - rx[:, 0]) * (ry[:, 1] - ry[:, 0])
    area_cl = (cx[:, 1] - cx[:, 0]) * (cy[:, 1] - cy[:, 0])
    visible = np.where(area_raw > 0, area_cl / np.where(area_raw > 0, area_raw, 1.0), 0.0)
    thin = ((cx[:, 1] - cx[:, 0]) * t[:, 7] < min_px) | ((cy[:, 1] - cy[:, 0]) * t[:, 8] < min_px)
    drop = thin | (visible < drop_frac)
    sliver = ~drop & (visible < ignore_frac)
    if not ignore_regions:
        drop, sliver = drop | sliver, np.zeros(len(b), bool)
    st["boxes_dropped"] = st.get("boxes_dropped", 0) + int(drop.sum())
    st["boxes_ignored"] = st.get("boxes_ignored", 0) + int(sliver.sum())
    out = np.stack([(t[:, 5] + cx[:, 0] * t[:, 7]) / W, (t[:, 6] + cy[:, 0] * t[:, 8]) / H,
                    (t[:, 5] + cx[:, 1] * t[:, 7]) / W, (t[:, 6] + cy[:, 1] * t[:, 8]) / H], 1)
    merged = ObjectsAnnotation(anns4[0].path, W, H, np.concatenate([r[0].classes for r in rows]), np.clip(out, 0.0, 1.0),
                               np.concatenate([r[0].difficults for r in rows]) | sliver).select(~drop)
    return _limit_gmax(merged, gmax, st)


def _limit_gmax(merged, gmax, st):
    """At most gmax boxes: flagged boxes go first, smallest area first, then unflagged ones, smallest first (ties: lowest
    index); the number removed is counted into st["boxes_over_gmax"]."""
    over = merged.num_objects - gmax
    if over > 0:
        b = merged.bboxes.astype(np.float64)
        area = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
        order = np.lexsort((np.arange(len(area)), area, ~merged.difficults))  # flagged first, then area, then index
        keep = np.ones(len(area), bool)
        keep[order[:over]] = False
        merged = merged.select(keep)
        st["boxes_over_gmax"] = st.get("boxes_over_gmax", 0) + int(over)
    return merged


def sample_mosaic(rng: np.random.Generator, anns4, input_size, random_erasing=True, split_range=(0.3, 0.7), max_aspect=1.5,
                  drop_frac=0.1, ignore_frac=0.4, min_px=2.0, ignore_regions=False, gmax=GMAX, stats=None):
    """Four annotations (TL, TR, BL, BR) -> (MosaicParams, merged ObjectsAnnotation in output coordinates).  Draws, in this
    order: split_x, split_y, the four tiles' sample_params (erasing off), then the whole-frame erase list."""
    H, W = input_size
    assert len(anns4) == 4
    sx = int(rng.integers(max(1, int(round(split_range[0] * W))), min(W, int(round(split_range[1] * W))) + 1))
    sy = int(rng.integers(max(1, int(round(split_range[0] * H))), min(H, int(round(split_range[1] * H))) + 1))
    tiles = []
    for a, (_x0, _y0, Wt, Ht) in zip(anns4, tile_rects((sx, sy), input_size)):
        p = sample_params(rng, a, random_erasing=False)
        p.crop = fit_tile_aspect(p.crop, (a.width or 1, a.height or 1), (Wt, Ht), max_aspect)
        tiles.append(p)
    merged = mosaic_boxes(anns4, tiles, (sx, sy), input_size, drop_frac, ignore_frac, min_px, ignore_regions, gmax, stats)
    erase = _sample_erase(rng, merged.bboxes) if random_erasing and rng.random() < 0.5 else []
    if stats is not None:
        stats["mosaics"] = stats.get("mosaics", 0) + 1
    return MosaicParams((sx, sy), tiles, erase), merged


IDENTITY_AFFINE = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0)
IDENTITY_COLOUR = ((1.0, 0.0, 0.0, 0.0), (0.0, 1.0, 0.0, 0.0), (0.0, 0.0, 1.0, 0.0))
AFFINE_DEFAULTS = {"degrees": 0.0, "translate": 0.1, "scale": 0.5, "shear": 0.0}
# RGB -> YIQ (NTSC); hsv_matrix inverts it numerically in f64
TYIQ = ((0.299, 0.587, 0.114), (0.596, -0.274, -0.322), (0.211, -0.523, 0.312))


_TYIQ = np.array(TYIQ, np.float64)
_TYIQ_INV = np.linalg.inv(_TYIQ)
_EYE3 = np.eye(3)


class WarpParams:
    """One output image of od_augment_warp: one or two frames (MosaicParams without erase lists; a single image is
    MosaicParams.single), per frame the INVERSE affine matrix (six f32: output pixel centre -> frame position, both in
    output pixels) and the 3x4 colour matrix, the MixUp weights (mix_a, mix_b), the fill colour and the final image's erase
    list."""
    __slots__ = ("frames", "inv", "colour", "mix", "fill", "erase")

    def __init__(self, frames, inv=None, colour=None, mix=(1.0, 0.0), fill=(114, 114, 114), erase=()):
        self.frames = list(frames)
        self.inv = [np.asarray(m, np.float32).reshape(6) for m in (inv if inv is not None else [IDENTITY_AFFINE] * len(self.frames))]
        self.colour = [np.asarray(k, np.float32).reshape(3, 4)
                       for k in (colour if colour is not None else [IDENTITY_COLOUR] * len(self.frames))]
        self.mix = (float(np.float32(mix[0])), float(np.float32(mix[1])))
        self.fill = tuple(int(v) for v in fill)
        self.erase = list(erase)


def sample_affine(rng: np.random.Generator, input_size, degrees=0.0, translate=0.1, scale=0.5, shear=0.0):
    """-> the forward matrix M (3x3, f64), frame position -> output position, both in output pixels:
    M = T . Sh . R . S . C with C moving the frame centre to the origin, S the zoom ~ U(1-scale, 1+scale), R the rotation by
    theta ~ U(-degrees, degrees), Sh the shear by tan of ~ U(-shear, shear) degrees per axis and T the translation to
    ~ U(0.5-translate, 0.5+translate) . (W, H).  Six draws, in this order: theta, zoom, shear x, shear y, tx, ty."""
    H, W = input_size
    th = math.radians(rng.uniform(-degrees, degrees))
    z = rng.uniform(1.0 - scale, 1.0 + scale)
    shx = math.tan(math.radians(rng.uniform(-shear, shear)))
    shy = math.tan(math.radians(rng.uniform(-shear, shear)))
    tx = rng.uniform(0.5 - translate, 0.5 + translate) * W
    ty = rng.uniform(0.5 - translate, 0.5 + translate) * H
    # the product written out in python floats (f64): this runs per frame on the generator's thread, where five small numpy
    # matrices and their four products cost several times the six draws
    c, s = z * math.cos(th), z * math.sin(th)  # R . S = [[c, -s], [s, c]]
    a00, a01, a10, a11 = c + shx * s, shx * c - s, shy * c + s, c - shy * s  # Sh . R . S
    return np.array([[a00, a01, tx - (a00 * W + a01 * H) / 2], [a10, a11, ty - (a10 * W + a11 * H) / 2], [0.0, 0.0, 1.0]],
                    np.float64)


def affine_inverse(M):
    """The six numbers od_augment_warp takes: the top two rows of inv(M), inverted in f64, then cast to f32."""
    (a, b, tx), (c, d, ty) = ((float(v) for v in row) for row in np.asarray(M, np.float64)[:2])
    det = a * d - b * c
    if det == 0.0 or not math.isfinite(det):
        raise ValueError(f"affine matrix is singular: {M!r}")
    ia, ib, ic, id_ = d / det, -b / det, -c / det, a / det  # [A | t]^-1 = [A^-1 | -A^-1 t]
    return np.array([ia, ib, -(ia * tx + ib * ty), ic, id_, -(ic * tx + id_ * ty)], np.float64).astype(np.float32)


def hsv_matrix(hue, sat, val):
    """-> the 3x4 f32 colour matrix val . Tyiq^-1 . diag(1, sat, sat) . Rot(hue) . Tyiq, offset column 0: hue in turns
    (Rot turns the I/Q plane by 2 pi hue), sat and val as factors.  Computed in f64, then cast.
        Tyiq = [[0.299,  0.587,  0.114],
                [0.596, -0.274, -0.322],
                [0.211, -0.523,  0.312]]        (RGB -> YIQ, NTSC; Tyiq^-1 = numpy.linalg.inv of it)
    Evaluated as val . (I + Tyiq^-1 . (diag . Rot - I) . Tyiq), the same matrix, so that hsv_matrix(0, 1, 1) is the identity
    to the last bit."""
    a, sat = 2.0 * math.pi * float(hue), float(sat)
    c, s = sat * math.cos(a), sat * math.sin(a)
    d = np.array([[0.0, 0.0, 0.0], [0.0, c - 1.0, -s], [0.0, s, c - 1.0]], np.float64)  # diag(1, sat, sat) . Rot(hue) - I
    out = np.zeros((3, 4), np.float64)
    out[:, :3] = float(val) * (_EYE3 + _TYIQ_INV @ d @ _TYIQ)
    return out.astype(np.float32)


def sample_hsv(rng: np.random.Generator, hsv):
    """hsv = (h, s, v): hue ~ U(-h, h) turns, sat ~ U(1-s, 1+s), val ~ U(1-v, 1+v), drawn in this order -> hsv_matrix."""
    h, s, v = hsv
    hue = rng.uniform(-h, h)
    sat = rng.uniform(1.0 - s, 1.0 + s)
    val = rng.uniform(1.0 - v, 1.0 + v)
    return hsv_matrix(hue, sat, val)


def warp_boxes(ann, M, input_size, drop_frac=0.1, ignore_frac=0.4, min_px=2.0, max_aspect=20, ignore_regions=False,
               stats=None):
    """The annotation of a frame (boxes in frame coordinates, as mosaic_boxes / transform_boxes leave them) after the affine
    M (forward, 3x3, output pixels): every box's four corners go through M in f64, their enclosing box is clipped to the
    frame, and visible = clipped area / enclosing area decides as in mosaic_boxes: thinner than min_px output pixels or
    < drop_frac -> dropped; < ignore_frac -> an ignore region (difficults = True) with ignore_regions, dropped without; then
    a box whose clipped sides are in a ratio above max_aspect is dropped as well.  Input difficults are carried through;
    stats counts boxes_dropped and boxes_ignored."""
    H, W = input_size
    st = stats if stats is not None else {}
    n = ann.num_objects
    if n == 0:
        return ObjectsAnnotation(ann.path, W, H)
    M = np.asarray(M, np.float64)
    b = ann.bboxes.astype(np.float64)
    cx = b[:, (0, 2, 2, 0)] * W  # corners: TL, TR, BR, BL
    cy = b[:, (1, 1, 3, 3)] * H
    wx = M[0, 0] * cx + M[0, 1] * cy + M[0, 2]
    wy = M[1, 0] * cx + M[1, 1] * cy + M[1, 2]
    ex0, ex1, ey0, ey1 = wx.min(1), wx.max(1), wy.min(1), wy.max(1)  # the enclosing box ...
    out = np.empty((n, 4), np.float64)                                # ... clipped to the frame
    np.clip(ex0, 0.0, W, out=out[:, 0]), np.clip(ey0, 0.0, H, out=out[:, 1])
    np.clip(ex1, 0.0, W, out=out[:, 2]), np.clip(ey1, 0.0, H, out=out[:, 3])
    cw, chh = out[:, 2] - out[:, 0], out[:, 3] - out[:, 1]
    area_raw = (ex1 - ex0) * (ey1 - ey0)
    seen = area_raw > 0
    visible = np.where(seen, cw * chh / np.where(seen, area_raw, 1.0), 0.0)
    thin = (cw < min_px) | (chh < min_px)
    drop = thin | (visible < drop_frac)
    sliver = ~drop & (visible < ignore_frac)
    if not ignore_regions:
        drop, sliver = drop | sliver, np.zeros(n, bool)
    far = ~drop & (np.maximum(cw, chh) > max_aspect * np.minimum(cw, chh))
    drop, sliver = drop | far, sliver & ~far
    st["boxes_dropped"] = st.get("boxes_dropped", 0) + int(drop.sum())
    st["boxes_ignored"] = st.get("boxes_ignored", 0) + int(sliver.sum())
    out /= (W, H, W, H)
    keep = ~drop
    return ObjectsAnnotation(ann.path, W, H, ann.classes[keep], out[keep], (ann.difficults | sliver)[keep])


def mixup_annotations(anns, gmax=GMAX, stats=None):
    """The annotation of a MixUp: the frames' (already warped) boxes one after the other, cut to gmax by mosaic_boxes'
    rule."""
    a0 = anns[0]
    merged = ObjectsAnnotation(a0.path, a0.width, a0.height, np.concatenate([a.classes for a in anns]),
                               np.concatenate([a.bboxes for a in anns]), np.concatenate([a.difficults for a in anns]))
    return _limit_gmax(merged, gmax, stats if stats is not None else {})


def apply_pixels_host(img_u8: np.ndarray, p: AugParams, out_hw) -> np.ndarray:
    """Host pixel path (PIL resize): used when no device is given."""
    from PIL import Image
    H, W = out_hw
    h0, w0 = img_u8.shape[:2]
    x1, y1, x2, y2 = p.crop
    box = (int(round(x1 * w0)), int(round(y1 * h0)), max(int(round(x2 * w0)), int(round(x1 * w0)) + 1),
           max(int(round(y2 * h0)), int(round(y1 * h0)) + 1))
    im = Image.fromarray(img_u8).crop(box).resize((W, H), Image.BILINEAR)
    a = np.asarray(im, np.float32)
    if p.flip:
        a = a[:, ::-1]
    if p.saturation != 1.0:
        g = a @ np.array([0.299, 0.587, 0.114], np.float32)
        a = g[..., None] + (a - g[..., None]) * p.saturation
    if p.contrast != 1.0:
        a = (a - 127.5) * p.contrast + 127.5
    a = a + p.brightness
    a = np.clip(np.rint(a), 0, 255).astype(np.uint8)
    for (ex1, ey1, ex2, ey2), col in p.erase:
        a[int(ey1 * H):int(math.ceil(ey2 * H)), int(ex1 * W):int(math.ceil(ex2 * W))] = col
    return a


def _fill_aug(q, p: AugParams, offset, src_h, src_w):
    q.src_offset, q.src_h, q.src_w = offset, src_h, src_w
    q.crop_x1, q.crop_y1, q.crop_x2, q.crop_y2 = p.crop
    q.flip, q.brightness, q.contrast, q.saturation = int(p.flip), p.brightness, p.contrast, p.saturation


def _fill_erase(q, erase):
    q.n_erase = min(3, len(erase))
    for e, (rect, col) in enumerate(erase[:3]):
        for k in range(4):
            q.erase[e][k] = rect[k]
        for k in range(3):
            q.erase_rgb[e][k] = col[k]


class _Sources:
    """Where a launch finds its source images.  Device tensors are read where they are: one base pointer (the first
    tensor's) and a SIGNED 64-bit offset per image.  Host arrays are packed, each once however often it is shown, into one
    upload at 16-byte aligned offsets."""

    def __init__(self, flat, who):
        import torch
        self.resident = len(flat) > 0 and all(isinstance(im, torch.Tensor) for im in flat)
        if not flat or (not self.resident and any(isinstance(im, torch.Tensor) for im in flat)):
            raise ValueError(f"{who}: sources must be all host arrays or all device tensors, at least one")
        self.flat = flat
        self.base = flat[0].data_ptr() if self.resident else 0
        self.off, self.chunks, self.packed_at = 0, [], {}

    def locate(self, img):
        """-> (src_offset, src_h, src_w)"""
        if self.resident:
            import torch
            assert img.is_cuda and img.dtype == torch.uint8 and img.is_contiguous() and img.shape[-1] == 3
            return img.data_ptr() - self.base, img.shape[0], img.shape[1]
        if id(img) not in self.packed_at:
            a = np.ascontiguousarray(img[..., :3], np.uint8)
            self.packed_at[id(img)] = (self.off, a.shape[0], a.shape[1])
            self.chunks.append((self.off, a.reshape(-1)))
            self.off += (a.size + 15) // 16 * 16
        return self.packed_at[id(img)]

    def upload(self, dev):
        """-> (base pointer, what must stay alive until the launch is enqueued)"""
        if self.resident:
            return self.base, self.flat
        import torch
        src = torch.from_numpy(self.packed()).to(dev)
        return src.data_ptr(), src

    def packed(self):
        """The host arrays located so far, in one uint8 array."""
        packed = np.zeros(self.off, np.uint8)
        for o, c in self.chunks:
            packed[o:o + c.size] = c
        return packed


def _fill_mosaic(q, quad, mp, out_hw, i, sources):
    """One od_mosaic_params (without its erase list) from the four sources and MosaicParams of output image i."""
    H, Wd = out_hw
    sx, sy = mp.split
    if not (1 <= sx <= Wd and 1 <= sy <= H):
        raise ValueError(f"mosaic split {mp.split} outside [1, {Wd}] x [1, {H}]")
    q.split_x, q.split_y = sx, sy
    first = None
    for t, (X0, Y0, Wt, Ht) in enumerate(tile_rects((sx, sy), out_hw)):
        img, p = quad[t], mp.tiles[t]
        if Wt > 0 and Ht > 0:
            if img is None:
                raise ValueError(f"image {i}: tile {t} is {Wt}x{Ht} pixels but has no source")
            if p.erase:
                raise ValueError("a mosaic tile carries no erase list of its own (MosaicParams.erase acts on the frame)")
        if img is None:  # never sampled: any valid source will do
            img = first if first is not None else next(im for im in quad if im is not None)
        first = img if first is None else first
        _fill_aug(q.tile[t], p, *sources.locate(img))
        q.tile[t].n_erase = 0


def apply_mosaic_device(images, params, out_hw, device):
    """K14, four sources per output image: images = list of B 4-tuples (TL, TR, BL, BR) of uint8 [h,w,3] host arrays or
    uint8 DEVICE tensors (None for a tile that is empty or unused: it is never sampled) + list[MosaicParams] -> uint8
    torch tensor [B,H,W,3] on `device` through od_augment_mosaic.  Device tensors are read where they are: one base pointer
    and a SIGNED 64-bit offset per tile, so the sources may lie anywhere in the device's address space."""
    import torch

    from . import _lib
    from .net import Context, _stream_ptr
    ctx = Context.get(device)
    H, Wd = out_hw
    B = len(images)
    arr = (_lib.MosaicParams * B)()
    sources = _Sources([im for quad in images for im in quad if im is not None], "apply_mosaic_device")
    for i, (quad, mp) in enumerate(zip(images, params)):
        _fill_mosaic(arr[i], quad, mp, out_hw, i, sources)
        _fill_erase(arr[i], mp.erase)
    dev = torch.device(device)
    src_ptr, src = sources.upload(dev)
    prm = torch.from_numpy(np.frombuffer(bytes(arr), np.uint8).copy()).to(dev)
    out = torch.empty((B, H, Wd, 3), dtype=torch.uint8, device=dev)
    _lib.check(ctx.lib.od_augment_mosaic(ctx.handle, src_ptr, prm.data_ptr(), out.data_ptr(), B, H, Wd, _stream_ptr()),
               "od_augment_mosaic")
    del src
    return out


def apply_warp_device(images, params, out_hw, device, out=None):
    """K14b: images = list of B lists, one 4-tuple of sources (as apply_mosaic_device takes them) per frame of the output
    image, + list[WarpParams] -> uint8 torch tensor [B,H,W,3] on `device` through one od_augment_warp launch (written into
    `out`, a contiguous uint8 [B,H,W,3] tensor on the device, where one is given).  Everything the kernel trusts is checked
    here, before the launch: ValueError for n_frames outside {1, 2}, a split out of range, an erase list on a tile or on a
    frame, and mixed host / device sources."""
    import torch

    from . import _lib
    from .net import Context, _stream_ptr
    H, Wd = out_hw
    B = len(images)
    arr, sources = _pack_warp(images, params, out_hw)
    ctx = Context.get(device)
    dev = torch.device(device)
    src_ptr, src = sources.upload(dev)
    prm = torch.from_numpy(np.frombuffer(bytes(arr), np.uint8).copy()).to(dev)
    if out is None:
        out = torch.empty((B, H, Wd, 3), dtype=torch.uint8, device=dev)
    elif not (out.is_cuda and out.dtype == torch.uint8 and out.is_contiguous() and tuple(out.shape) == (B, H, Wd, 3)):
        raise ValueError(f"out must be a contiguous uint8 device tensor of shape {(B, H, Wd, 3)}")
    _lib.check(ctx.lib.od_augment_warp(ctx.handle, src_ptr, prm.data_ptr(), out.data_ptr(), B, H, Wd, _stream_ptr()),
               "od_augment_warp")
    del src
    return out


def _pack_warp(images, params, out_hw):
    """apply_warp_device's checks and packing -> (ctypes array of od_warp_params, _Sources)."""
    from . import _lib
    B = len(images)
    for i, (frames, wp) in enumerate(zip(images, params)):
        n = len(wp.frames)
        if n not in (1, 2) or not (len(frames) == len(wp.inv) == len(wp.colour) == n):
            raise ValueError(f"image {i}: n_frames must be 1 or 2 with one source quad, matrix and colour matrix each, got "
                             f"{n} frames, {len(frames)} quads, {len(wp.inv)} matrices, {len(wp.colour)} colour matrices")
        if any(mp.erase for mp in wp.frames):
            raise ValueError("a frame of a warp carries no erase list of its own (WarpParams.erase acts on the final image)")
    sources = _Sources([im for frames in images for quad in frames for im in quad if im is not None], "apply_warp_device")
    arr = (_lib.WarpParams * B)()
    for i, (frames, wp) in enumerate(zip(images, params)):
        q = arr[i]
        q.n_frames = len(wp.frames)
        q.mix_a, q.mix_b = wp.mix
        for ch in range(3):
            q.fill_rgb[ch] = int(wp.fill[ch])
        for f, (quad, mp) in enumerate(zip(frames, wp.frames)):
            _fill_mosaic(q.frame[f], quad, mp, out_hw, i, sources)
            q.frame[f].n_erase = 0
            q.a[f][:] = wp.inv[f].tolist()
            for ch, row in enumerate(wp.colour[f].tolist()):
                q.k[f][ch][:] = row
        _fill_erase(q, wp.erase)
    return arr, sources


def apply_pixels_device(images, params, out_hw, device):
    """K14: list of uint8 [h,w,3] arrays (host) or uint8 [h,w,3] DEVICE tensors + list[AugParams] -> uint8 torch tensor
    [B,H,W,3] on `device`.  Device tensors (the generator's device-resident image cache) are read where they are: the
    kernel takes one base pointer and a 64-bit offset per image, so the images need not share an allocation."""
    import ctypes as C

    import torch

    from . import _lib
    from .net import Context, _stream_ptr
    ctx = Context.get(device)
    H, Wd = out_hw
    B = len(images)
    arr = (_lib.AugParams * B)()
    resident = B > 0 and all(isinstance(im, torch.Tensor) for im in images)
    off = 0
    chunks = []
    for i, (img, p) in enumerate(zip(images, params)):
        if resident:
            assert img.is_cuda and img.dtype == torch.uint8 and img.is_contiguous() and img.shape[-1] == 3
            a = img
            this_off = img.data_ptr() - images[0].data_ptr()
        else:
            a = np.ascontiguousarray(img[..., :3], np.uint8)
            chunks.append(a.reshape(-1))
            this_off = off
        _fill_aug(arr[i], p, this_off, a.shape[0], a.shape[1])
        _fill_erase(arr[i], p.erase)
        if not resident:
            off += (a.size + 15) // 16 * 16
    dev = torch.device(device)
    if resident:
        src = images[0]
    else:
        packed = np.zeros(off, np.uint8)
        o = 0
        for c in chunks:
            packed[o:o + c.size] = c
            o += (c.size + 15) // 16 * 16
        src = torch.from_numpy(packed).to(dev)
    prm = torch.from_numpy(np.frombuffer(bytes(arr), np.uint8).copy()).to(dev)
    out = torch.empty((B, H, Wd, 3), dtype=torch.uint8, device=dev)
    _lib.check(ctx.lib.od_augment_batch(ctx.handle, src.data_ptr(), prm.data_ptr(), out.data_ptr(), B, H, Wd,
                                        _stream_ptr()), "od_augment_batch")
    return out


class Generator:
    def __init__(self, input_size, preprocess_input=None, encode_truth=None, random_erasing=True, device=None, workers=None,
                 on_device=False, device_cache=False, mosaic=0.0, ignore_regions=False, mosaic_args=None, affine=None, hsv=None,
                 mixup=0.0, mixup_beta=8.0, fill=(114, 114, 114)):
        # device_cache (needs device=): every image is decoded and uploaded ONCE and stays in HBM as a uint8 tensor; from the
        # second epoch on a batch costs the host only its augmentation parameters.  VOC07+12 trainval decoded is ~9 GB --
        # a few per cent of one MI355X's 288 GB -- so the dataset lives where the augmentation kernel reads it.
        self.device_cache = bool(device_cache)
        if self.device_cache and device is None:
            raise ValueError("device_cache=True needs device=")
        # on_device (needs device=): X_batch stays a uint8 DEVICE tensor [B,H,W,3] -- what Trainer.step consumes -- instead of
        # coming back to the host as numpy (the reference's generator feeds Keras from the host; the visual checkers
        # check_generator.py / check_assign.py keep on_device=False and get numpy, as they index pixels on the host).
        # With encode_truth = od.pb.encode_truth_device the targets stay on the device as well: no host round trip per step.
        self.on_device = bool(on_device)
        if self.on_device and device is None:
            raise ValueError("on_device=True needs device=")
        # mosaic (needs device=): the probability that an output image of flow(data_augmentation=True) is composed of four
        # images (module docstring); ignore_regions: what becomes of a sliver a tile border leaves of an object -- an ignore
        # region (difficults = True; the PriorBoxes must be built with ignore_regions=True as well) or nothing.
        # mosaic_args: sample_mosaic's named numbers (split_range, max_aspect, drop_frac, ignore_frac, min_px, gmax).
        self.mosaic = float(mosaic)
        if not 0.0 <= self.mosaic <= 1.0:
            raise ValueError(f"mosaic is a probability, got {mosaic!r}")
        if self.mosaic > 0.0 and device is None:
            raise ValueError("mosaic > 0 needs device= (the composition is od_augment_mosaic; there is no host path)")
        self.ignore_regions = bool(ignore_regions)
        self.mosaic_args = dict(mosaic_args or {})
        self.stats = {"mosaics": 0, "boxes_dropped": 0, "boxes_ignored": 0, "boxes_over_gmax": 0}
        # affine / hsv / mixup (need device=; module docstring): the random affine warp's ranges (a dict over
        # AFFINE_DEFAULTS), the HSV jitter's half-widths (h, s, v), the probability that an output image is a MixUp of two
        # frames with ratio ~ Beta(mixup_beta, mixup_beta), and the colour where a warped frame does not reach.
        self.affine = None
        if affine is not None:
            if not isinstance(affine, dict) or set(affine) - set(AFFINE_DEFAULTS):
                raise ValueError(f"affine is a dict over {sorted(AFFINE_DEFAULTS)}, got {affine!r}")
            self.affine = {k: float(v) for k, v in {**AFFINE_DEFAULTS, **affine}.items()}
            if any(not v >= 0.0 for v in self.affine.values()):
                raise ValueError(f"affine ranges must be >= 0, got {affine!r}")
            if self.affine["scale"] >= 1.0:
                raise ValueError(f"affine scale must be < 1 (the zoom is U(1-scale, 1+scale)), got {affine['scale']!r}")
        self.hsv = None
        if hsv is not None:
            try:
                self.hsv = tuple(float(v) for v in hsv)
            except (TypeError, ValueError):
                self.hsv = ()
            if len(self.hsv) != 3 or any(not v >= 0.0 for v in self.hsv):
                raise ValueError(f"hsv is three non-negative numbers (h, s, v), got {hsv!r}")
        self.mixup, self.mixup_beta = float(mixup), float(mixup_beta)
        if not 0.0 <= self.mixup <= 1.0:
            raise ValueError(f"mixup is a probability, got {mixup!r}")
        if not self.mixup_beta > 0.0:
            raise ValueError(f"mixup_beta must be > 0, got {mixup_beta!r}")
        self.fill = tuple(int(v) for v in fill)
        if len(self.fill) != 3 or any(not 0 <= v <= 255 for v in self.fill):
            raise ValueError(f"fill is an (r, g, b) of bytes, got {fill!r}")
        self.warp = self.affine is not None or self.hsv is not None or self.mixup > 0.0
        if self.warp and device is None:
            raise ValueError("affine / hsv / mixup need device= (the pixel work is od_augment_warp; there is no host path)")
        if self.warp:  # a default generator's dict stays as it was
            self.stats.update(warps=0, mixups=0)
        # the most recent batch of the warp path, for checkers: [(per frame the four source indices, WarpParams)] per image
        self.last_warp = None
        self.input_size = tuple(int(v) for v in input_size)
        self.preprocess_input = preprocess_input
        self.encode_truth = encode_truth
        self.random_erasing = random_erasing
        self.device = device  # e.g. "cuda:0": pixel work runs in od_augment_batch (K14); None: host path (PIL)
        # image decode (and the host augmentation) of a batch runs on a thread pool, the NEXT batch's decode is already in
        # flight while this one is consumed; augmentation parameters are still drawn in index order on the calling thread,
        # so the stream of batches is identical for any worker count
        import os
        self.workers = int(workers if workers is not None else os.environ.get("OD_GEN_WORKERS", min(8, os.cpu_count() or 1)))

    def _load(self, x):
        if isinstance(x, np.ndarray):
            return x[..., :3].astype(np.uint8)
        from .tk.ndimage import load
        return load(x)

    def generate(self, x, ann: ObjectsAnnotation, rng, data_augmentation):
        img = self._load(x)
        p = sample_params(rng, ann, self.random_erasing) if data_augmentation else AugParams()
        out = apply_pixels_host(img, p, self.input_size)
        new_ann = ObjectsAnnotation(ann.path, self.input_size[1], self.input_size[0], ann.classes,
                                    transform_boxes(ann.bboxes, p), ann.difficults)
        return out, new_ann

    def flow(self, X, y, batch_size=16, data_augmentation=False, shuffle=False, seed=0, prefetch=0):
        """-> (infinite iterator of (X_batch [B,H,W,3], y_batch), steps_per_epoch)   (check_generator.py:18)
        prefetch = N > 0 (needs on_device=True): the batches are produced by a background thread, N ahead, on a HIP stream of
        its own -- parameter sampling, packing, the upload, od_augment_batch and encode_truth overlap the training step that
        consumes the previous batch (13.7 -> 10.9 ms per step of scripts/train.py at 32 x 320^2); the stream of batches is the
        same as without prefetch."""
        n = len(X)
        steps = max(1, math.ceil(n / batch_size))
        if prefetch and not self.on_device:
            raise ValueError("prefetch needs on_device=True (device batches on the generator's own stream)")

        def it():
            from concurrent.futures import ThreadPoolExecutor
            rng = np.random.default_rng(seed)
            pool = ThreadPoolExecutor(max_workers=self.workers) if self.workers > 1 else None
            resident = {} if self.device_cache else None  # image index -> uint8 device tensor [h,w,3]

            class _Done:  # a cached image needs no decode: stands in for the pool's future
                def __init__(self, v):
                    self.v = v

                def result(self):
                    return self.v

            def fetch(i):
                i = int(i)
                if resident is not None and i in resident:
                    return _Done(resident[i])
                return pool.submit(self._load, X[i]) if pool is not None else _Done(self._load(X[i]))

            def load_batch(idx):
                return [fetch(i) for i in idx] if (pool is not None or resident is not None) else None

            def to_resident(idx, raw):
                import torch
                out = []
                for i, im in zip(idx, raw):
                    if not isinstance(im, torch.Tensor):
                        im = torch.from_numpy(np.ascontiguousarray(im[..., :3], np.uint8)).to(torch.device(self.device))
                        resident[int(i)] = im
                    out.append(im)
                return out

            def plain_annotation(i, p):
                return ObjectsAnnotation(y[i].path, self.input_size[1], self.input_size[0], y[i].classes,
                                         transform_boxes(y[i].bboxes, p), y[i].difficults)

            def draw_with_mosaic(idx):
                """Per output image, in index order: one uniform draw decides; a mosaic then draws its three partners from
                the whole dataset and its parameters (sample_mosaic), any other image its sample_params as always."""
                prm, mos = [], []
                for i in idx:
                    if rng.random() < self.mosaic:
                        four = [int(i)] + [int(j) for j in rng.integers(0, n, 3)]
                        mp, ann = sample_mosaic(rng, [y[j] for j in four], self.input_size, self.random_erasing,
                                                ignore_regions=self.ignore_regions, stats=self.stats, **self.mosaic_args)
                        prm.append(None), mos.append((four, mp, ann))
                    else:
                        prm.append(sample_params(rng, y[i], self.random_erasing)), mos.append(None)
                return prm, mos

            def compose(idx, raw, prm, mos):
                """One od_augment_mosaic launch for the whole batch; an image that is no mosaic rides along as the
                degenerate one (byte-identical to od_augment_batch).  Partner images come through fetch / to_resident."""
                partners = [j for m in mos if m is not None for j in m[0][1:]]
                got = [f.result() for f in [fetch(j) for j in partners]]
                if resident is not None:
                    got = to_resident(partners, got)
                got = iter(got)
                quads, mps, anns = [], [], []
                for i, im, p, m in zip(idx, raw, prm, mos):
                    if m is None:
                        quads.append((im, None, None, None))
                        mps.append(MosaicParams.single(p, self.input_size))
                        anns.append(plain_annotation(i, p))
                    else:
                        quads.append((im, next(got), next(got), next(got)))
                        mps.append(m[1]), anns.append(m[2])
                return apply_mosaic_device(quads, mps, self.input_size, self.device), anns

            def draw_frame(i):
                """Steps 1-3 of the warp path's draw order for one frame: the mosaic decision and its parameters (erasing
                off), the affine, the HSV -> (four source indices, MosaicParams, inverse matrix, colour matrix, annotation)."""
                if self.mosaic > 0.0 and rng.random() < self.mosaic:
                    four = [int(i)] + [int(j) for j in rng.integers(0, n, 3)]
                    mp, ann = sample_mosaic(rng, [y[j] for j in four], self.input_size, False,
                                            ignore_regions=self.ignore_regions, stats=self.stats, **self.mosaic_args)
                else:
                    p = sample_params(rng, y[i], False)
                    four, mp, ann = [int(i), None, None, None], MosaicParams.single(p, self.input_size), plain_annotation(i, p)
                inv, colour = IDENTITY_AFFINE, IDENTITY_COLOUR
                if self.affine is not None:
                    M = sample_affine(rng, self.input_size, **self.affine)
                    inv = affine_inverse(M)
                    ann = warp_boxes(ann, M, self.input_size, ignore_regions=self.ignore_regions, stats=self.stats,
                                     **{k: v for k, v in self.mosaic_args.items() if k in ("drop_frac", "ignore_frac", "min_px")})
                if self.hsv is not None:
                    colour = sample_hsv(rng, self.hsv)
                return four, mp, inv, colour, ann

            def warped(idx, raw):
                """The batch through od_augment_warp (module docstring, 'Warp / HSV / MixUp'): per output image the frame, the
                MixUp decision, the partner's frame and the ratio, then the final image's erase list; one launch."""
                recs, anns = [], []
                for i in idx:
                    frames = [draw_frame(i)]
                    mix = (1.0, 0.0)
                    if self.mixup > 0.0 and rng.random() < self.mixup:
                        frames.append(draw_frame(int(rng.integers(0, n))))
                        r = np.float32(rng.beta(self.mixup_beta, self.mixup_beta))
                        mix = (r, np.float32(1.0) - r)
                        self.stats["mixups"] += 1
                    self.stats["warps"] += 1
                    ann = mixup_annotations([f[4] for f in frames], self.mosaic_args.get("gmax", GMAX), self.stats)
                    erase = _sample_erase(rng, ann.bboxes) if self.random_erasing and rng.random() < 0.5 else []
                    recs.append(([f[0] for f in frames],
                                 WarpParams([f[1] for f in frames], [f[2] for f in frames], [f[3] for f in frames], mix,
                                            self.fill, erase)))
                    anns.append(ann)
                own = {int(i): im for i, im in zip(idx, raw)}
                others = sorted({j for fours, _wp in recs for four in fours for j in four if j is not None and j not in own})
                got = [f.result() for f in [fetch(j) for j in others]]
                if resident is not None:
                    got = to_resident(others, got)
                own.update(zip(others, got))
                images = [[tuple(own[j] if j is not None else None for j in four) for four in fours] for fours, _wp in recs]
                self.last_warp = recs
                return apply_warp_device(images, [wp for _f, wp in recs], self.input_size, self.device), anns

            while True:
                order = rng.permutation(n) if shuffle else np.arange(n)
                batches = [order[s:s + batch_size] for s in range(0, n, batch_size)]
                nxt = load_batch(batches[0])
                for bi, idx in enumerate(batches):
                    futs, nxt = nxt, (load_batch(batches[bi + 1]) if bi + 1 < len(batches) else None)
                    raw = [f.result() for f in futs] if futs is not None else [self._load(X[i]) for i in idx]
                    if resident is not None:
                        raw = to_resident(idx, raw)
                    mos = anns = None
                    if self.warp and data_augmentation:
                        prm = None
                    elif self.mosaic > 0.0 and data_augmentation:
                        prm, mos = draw_with_mosaic(idx)
                        if not any(m is not None for m in mos):
                            mos = None
                    else:  # not one draw more than before mosaic existed: the stream of batches is unchanged
                        prm = [sample_params(rng, y[i], self.random_erasing) if data_augmentation else AugParams() for i in idx]
                    if prm is None or mos is not None:
                        xb, anns = warped(idx, raw) if prm is None else compose(idx, raw, prm, mos)
                        if not self.on_device:
                            xb = xb.cpu().numpy()
                    elif self.device is not None:
                        xb = apply_pixels_device(raw, prm, self.input_size, self.device)
                        if not self.on_device:
                            xb = xb.cpu().numpy()
                    elif pool is not None:
                        xb = np.stack(list(pool.map(lambda ip: apply_pixels_host(ip[0], ip[1], self.input_size), zip(raw, prm))))
                    else:
                        xb = np.stack([apply_pixels_host(img, p, self.input_size) for img, p in zip(raw, prm)])
                    if anns is None:
                        anns = [plain_annotation(i, p) for i, p in zip(idx, prm)]
                    if self.preprocess_input is not None:
                        xb = self.preprocess_input(xb)
                    yb = self.encode_truth(list(anns)) if self.encode_truth is not None else list(anns)
                    yield xb, yb
        if prefetch:
            return _prefetched(it(), int(prefetch), self.device), steps
        return it(), steps


def _prefetched(iterator, depth, device):
    """Run `iterator` in a daemon thread on its own HIP stream, `depth` batches ahead.  Every batch travels with an event
    recorded behind its last kernel; the consumer's current stream waits for it (no host wait), and the tensors are
    registered with that stream so that the caching allocator does not hand their memory back while they are in use."""
    import queue
    import threading

    import torch
    dev = torch.device(device)
    q = queue.Queue(maxsize=depth)
    stream = torch.cuda.Stream(device=dev)
    stop = threading.Event()

    def work():
        try:
            with torch.cuda.device(dev), torch.cuda.stream(stream):
                for item in iterator:
                    ev = torch.cuda.Event()
                    ev.record(stream)
                    while not stop.is_set():
                        try:
                            q.put((item, ev), timeout=0.2)
                            break
                        except queue.Full:
                            continue
                    if stop.is_set():
                        return
        except BaseException as e:  # noqa: BLE001 -- hand the failure to the consumer
            q.put((e, None))

    t = threading.Thread(target=work, daemon=True, name="od_gen-prefetch")
    t.start()

    def gen():
        try:
            while True:
                item, ev = q.get()
                if ev is None:
                    raise item
                cur = torch.cuda.current_stream(dev)
                cur.wait_event(ev)
                for v in item:
                    if isinstance(v, torch.Tensor) and v.is_cuda:
                        v.record_stream(cur)
                yield item
        finally:  # consumer closed / garbage-collected the iterator: stop the thread BEFORE the interpreter can tear down
            stop.set()
            try:
                while True:
                    q.get_nowait()
            except queue.Empty:
                pass
            t.join(timeout=10.0)
    return gen()


def create_generator(input_size, preprocess_input=None, encode_truth=None, **kw):
    return Generator(input_size, preprocess_input, encode_truth, **kw)
