"""Sliced inference: a large image is cut into overlapping tiles (+ the whole image as the last tile), every tile is one row
of the network batch, and the candidate lists of an image's tiles are merged in ONE NMS + box voting on the device.

[BUILD-DEFINED] (the reference has no slicing; DESIGN.md "Sliced inference" freezes the semantics).  This module is the single
definition of the geometry: both image routes of `ObjectDetector.predict` and the tests call it.  SlicePostprocessor is the
device side, beside the pipeline's Postprocessor as TtaPostprocessor is.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import torch

from . import _lib
from .net import _stream_ptr
from .postprocess import records_host

MAX_TILES = 16
VOTE_IOU = 0.5  # [BUILD-DEFINED] box-voting overlap (tta.VOTE_IOU)
LEFT, TOP, RIGHT, BOTTOM = 1, 2, 4, 8  # bits of edges(): that side of the tile is interior (not on the image border)


def axis_tiles(L, n, overlap):
    """n tiles of equal length along an axis of L pixels -> [(start, end)].  tl = min(L, ceil(L / (n - (n-1)*overlap))),
    starts j*(L - tl) // (n-1): the first tile starts at 0, the last ends at L, neighbours overlap or touch."""
    L, n = int(L), int(n)
    tl = min(L, int(math.ceil(L / (n - (n - 1) * float(overlap)))))
    starts = [j * (L - tl) // (n - 1) if n > 1 else 0 for j in range(n)]
    return [(s, s + tl) for s in starts]


class SliceGrid:
    """ny x nx tiles (+ the full view, last) per image."""

    def __init__(self, ny, nx, overlap=0.2, full_view=True, edge=0.01):
        self.ny, self.nx, self.overlap, self.full_view, self.edge = int(ny), int(nx), float(overlap), bool(full_view), float(edge)
        self.T = self.ny * self.nx + int(self.full_view)

    @property
    def edge_lo_hi(self):
        """The (edge_lo, edge_hi) od_slice_merge takes: f32(slice_edge), f32(1 - slice_edge); edge < 0 disables the rule."""
        return float(np.float32(self.edge)), float(np.float32(1 - self.edge))

    def rects(self, w, h):
        """int32 [T,4] pixel rectangles (x0, y0, x1, y1) of a w x h image, row-major over the grid, the full view last."""
        xs, ys = axis_tiles(w, self.nx, self.overlap), axis_tiles(h, self.ny, self.overlap)
        out = [(x0, y0, x1, y1) for (y0, y1) in ys for (x0, x1) in xs]
        if self.full_view:
            out.append((0, 0, int(w), int(h)))
        return np.array(out, np.int32).reshape(self.T, 4)

    def __repr__(self):
        return f"SliceGrid({self.ny}, {self.nx}, overlap={self.overlap}, full_view={self.full_view}, edge={self.edge})"


def edges(rects, w, h):
    """int32 [T]: one bitmask per tile, LEFT / TOP / RIGHT / BOTTOM set where that side does not lie on the image border."""
    r = np.asarray(rects, np.int64).reshape(-1, 4)
    return (LEFT * (r[:, 0] != 0) + TOP * (r[:, 1] != 0) + RIGHT * (r[:, 2] != w) + BOTTOM * (r[:, 3] != h)).astype(np.int32)


def affine(rects, w, h):
    """f32 [T,4] (ox, oy, sx, sy): tile origin and size as fractions of the image, each ONE f32 division."""
    r = np.asarray(rects, np.int64).reshape(-1, 4)
    F = np.float32
    fw, fh = F(w), F(h)
    return np.stack([r[:, 0].astype(F) / fw, r[:, 1].astype(F) / fh, (r[:, 2] - r[:, 0]).astype(F) / fw,
                     (r[:, 3] - r[:, 1]).astype(F) / fh], 1).astype(F)


def normalize(slices, slice_overlap=0.2, slice_full_view=True, slice_edge=0.01, batch_size=None, tta=None, keep_aspect=False):
    """The slice arguments of ObjectDetector -> None (slicing off) or a SliceGrid.  Raises ValueError for anything the
    sliced route does not define; called before anything touches the GPU."""
    if slices is None:
        return None
    if isinstance(slices, (str, bytes)) or not isinstance(slices, (tuple, list)) or len(slices) != 2:
        raise ValueError(f"slices must be None or (ny, nx), got {slices!r}")
    ny, nx = slices
    for v in (ny, nx):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 1:
            raise ValueError(f"slices must be two integers >= 1, got {slices!r}")
    ov = float(slice_overlap)
    if not 0.0 <= ov <= 0.5:  # also refuses NaN
        raise ValueError(f"slice_overlap must lie in [0, 0.5], got {slice_overlap!r}")
    edge = float(slice_edge)
    if not edge < 0.5:
        raise ValueError(f"slice_edge must be below 0.5 (negative disables the rule), got {slice_edge!r}")
    grid = SliceGrid(int(ny), int(nx), ov, slice_full_view, edge)
    if grid.T > MAX_TILES:
        raise ValueError(f"slices={slices!r} gives {grid.T} tiles per image; at most {MAX_TILES}")
    if batch_size is not None and grid.T > int(batch_size):
        raise ValueError(f"slices={slices!r} gives {grid.T} tiles per image, more than batch_size={batch_size}: an image's "
                         f"tiles share one network batch")
    if tta is not None:
        raise ValueError("slices and tta cannot be combined")
    if keep_aspect:
        raise ValueError("slices stretch every tile to the input size; keep_aspect=True is not available with slices")
    return grid


def host_tiles(img, grid, size_hw, out):
    """The host route: out[t] (uint8 [H,W,3] each) = PIL crop + resize(BILINEAR) of tile t of the uint8 [h,w,3] image.
    -> (w, h) of the image."""
    from PIL import Image
    H, Wd = size_hw
    h, w = img.shape[:2]
    pil = Image.fromarray(img)
    for t, (x0, y0, x1, y1) in enumerate(grid.rects(w, h).tolist()):
        np.copyto(out[t], np.asarray(pil.crop((x0, y0, x1, y1)).resize((Wd, H), Image.BILINEAR), np.uint8))
    return w, h


def load_native(x):
    """path / ndarray -> (uint8 [h,w,3] at the image's own size, came from a file)."""
    import os
    if isinstance(x, (str, os.PathLike)):
        from PIL import Image
        return np.asarray(Image.open(x).convert("RGB"), np.uint8), True
    a = np.asarray(x)
    if a.dtype != np.uint8:
        a = np.clip(a, 0, 255).astype(np.uint8)
    if a.ndim != 3 or a.shape[2] < 3:
        raise ValueError(f"sliced predict() takes RGB images [h,w,3], got an array of shape {a.shape}")
    return np.ascontiguousarray(a[..., :3]), False


class SlicePostprocessor:
    """Beside the Postprocessor `post` of one pipeline: candidate buffers of the whole batch, the per-row affine / edge
    arrays, the merge workspace, and the record block of the G = B // T images of a batch with its pinned mirror."""

    def __init__(self, post, grid, vote_iou=VOTE_IOU):
        self.post, self.lib, self.ctx, self.grid = post, post.lib, post.ctx, grid
        self.vote_iou = float(vote_iou)
        B, P, K = post.B, post.P, post.K
        self.T = grid.T
        if not 1 <= self.T <= MAX_TILES or self.T > B:
            raise ValueError(f"SlicePostprocessor: {self.T} tiles per image with a batch of {B}")
        self.G = G = B // self.T
        dev = post.priors.device
        self.boxes = torch.empty((B, P, 4), dtype=torch.float32, device=dev)
        self.keys = torch.empty((B, K), dtype=torch.int64, device=dev)  # u64 payload, sorted descending
        self.counts = torch.empty((B,), dtype=torch.int32, device=dev)
        # rows of (ox, oy, sx, sy) as f32 bits, then the edge masks: one upload per batch
        n = G * self.T
        self.geom = torch.zeros((n * 5,), dtype=torch.int32, device=dev)
        self.geom_host = torch.zeros((n * 5,), dtype=torch.int32).pin_memory()
        self.tiles = self.geom[:n * 4].view(torch.float32).view(n, 4)
        self.edges = self.geom[n * 4:]
        self._geom_copied = None
        self._geom_sizes = None  # the image sizes the device arrays were last made for
        self.src = torch.empty((G, post.max_det, 2), dtype=torch.int32, device=dev)
        self.keep_count = torch.empty((G,), dtype=torch.int32, device=dev)
        self.det = torch.empty((G, 1 + 6 * post.max_det), dtype=torch.float32, device=dev)
        self.det_host = torch.empty((G, 1 + 6 * post.max_det), dtype=torch.float32).pin_memory()
        self.ws_bytes = self.lib.od_slice_merge_workspace_bytes(G, self.T, K)
        self.ws = torch.empty((self.ws_bytes,), dtype=torch.uint8, device=dev)

    def set_geometry(self, sizes):
        """(w, h) of the batch's images (at most G) -> the tiles / edges device arrays, queued on the current stream."""
        sizes = [(int(w), int(h)) for w, h in sizes]
        assert len(sizes) <= self.G
        if sizes == self._geom_sizes:  # frames of one size: the arrays on the device are already these
            return
        self._geom_sizes = sizes
        if self._geom_copied is not None:
            self._geom_copied.synchronize()  # the previous upload out of the pinned block
        host = self.geom_host.numpy()
        host[:] = 0
        n, T = self.G * self.T, self.T
        for g, (w, h) in enumerate(sizes):
            r = self.grid.rects(w, h)
            host[g * T * 4:(g + 1) * T * 4] = affine(r, w, h).reshape(-1).view(np.int32)
            host[n * 4 + g * T:n * 4 + (g + 1) * T] = edges(r, w, h)
        self.geom.copy_(self.geom_host, non_blocking=True)
        self._geom_copied = torch.cuda.Event()
        self._geom_copied.record()

    def candidates(self, pred, conf_threshold):
        """pred of the whole batch -> boxes / sorted keys / counts of every row (Postprocessor.candidates)."""
        self.post.candidates(pred, conf_threshold, self.boxes, self.keys, self.counts)

    def merge(self):
        """The rows' candidates -> self.det (record block of G images, word 0 of a row = class), self.src, self.keep_count;
        queues the single device->host copy of the block.  Rows from G*T on are never read."""
        p = self.post
        lo, hi = self.grid.edge_lo_hi
        # the soft scan in place of the greedy one (the report carries the rescored confidences): the two ABIs differ in
        # this argument group alone
        entry, nms = ("od_slice_merge_soft", (C.byref(p.soft_cfg()),)) if p.soft else \
            ("od_slice_merge", (p.iou_threshold, p.strict, p.max_det))
        _lib.check(getattr(self.lib, entry)(self.ctx.handle, self.keys.data_ptr(), self.counts.data_ptr(), self.boxes.data_ptr(),
                                            self.tiles.data_ptr(), self.edges.data_ptr(), self.G, self.T, p.P, p.NC, p.K, lo, hi,
                                            *nms, self.vote_iou, self.det.data_ptr(), self.src.data_ptr(),
                                            self.keep_count.data_ptr(), self.ws.data_ptr(), self.ws_bytes, _stream_ptr()), entry)
        self.det_host.copy_(self.det, non_blocking=True)
        return self.det, self.keep_count

    def run(self, net, x_u8, sizes, conf_threshold):
        """The whole sliced step of one batch on the current stream: x_u8 uint8 [B,H,W,3] holds the tiles (None = they are
        in net.input already), sizes the (w, h) of the batch's images."""
        self.set_geometry(sizes)
        self.candidates(net.forward(x_u8), conf_threshold)
        return self.merge()

    def detections_host(self, n_valid):
        """-> [(class i32 [n], conf f32 [n], boxes f32 [n,4])] for the first n_valid images, from the pinned block."""
        return records_host(self.det_host, n_valid)
