"""Test-time augmentation on the device: views of a batch -> per-view top-K candidates -> ONE merged NMS + box voting.

[BUILD-DEFINED] (the reference has no TTA; DESIGN.md "Flip test-time augmentation" freezes the semantics).  A pipeline with
TTA keeps its Postprocessor (priors, workspaces, the record block `det` and its pinned mirror) and adds this class beside
it: one set of candidate buffers per view, one mirrored image buffer, the merge workspace.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib
from .net import _stream_ptr

VIEW_NAMES = ("flip",)
VOTE_IOU = 0.5  # [BUILD-DEFINED] box-voting overlap
MAX_VIEWS = 8


def normalize_views(tta):
    """The `tta=` argument of ObjectDetector -> None (TTA off) or the tuple of EXTRA views beside the identity view:
    () = the identity view alone (box voting only), ("flip",) = identity + mirror."""
    if tta is None:
        return None
    if isinstance(tta, (str, bytes)) or not isinstance(tta, (tuple, list)):
        raise ValueError(f"tta must be None, () or a tuple of view names out of {VIEW_NAMES}, got {tta!r}")
    views = tuple(tta)
    for v in views:
        if v not in VIEW_NAMES:
            raise ValueError(f"tta: unknown view {v!r}; the views defined are {VIEW_NAMES}")
    if len(set(views)) != len(views):
        raise ValueError(f"tta: a view is named twice in {views!r}")
    return views


class TtaPostprocessor:
    """Candidate buffers of 1 + len(views) views and the merge, beside the Postprocessor `post` of the same pipeline.
    View 0 is the identity; view i + 1 is views[i]."""

    def __init__(self, post, input_shape, views=("flip",), vote_iou=VOTE_IOU):
        self.post, self.lib, self.ctx = post, post.lib, post.ctx
        self.views = normalize_views(views)
        if self.views is None:
            raise ValueError("TtaPostprocessor needs a tuple of views; tta=None is the plain Postprocessor path")
        self.flips = (0,) + tuple(int(v == "flip") for v in self.views)
        self.V = len(self.flips)
        self.vote_iou = float(vote_iou)
        dev = post.priors.device
        B, P, K = post.B, post.P, post.K
        self.boxes = torch.empty((self.V, B, P, 4), dtype=torch.float32, device=dev)
        self.keys = torch.empty((self.V, B, K), dtype=torch.int64, device=dev)  # u64 payload, sorted descending
        self.counts = torch.empty((self.V, B), dtype=torch.int32, device=dev)
        self.src = torch.empty((B, post.max_det, 2), dtype=torch.int32, device=dev)
        self.mirrored = torch.empty(tuple(input_shape), dtype=torch.uint8, device=dev) if any(self.flips) else None
        self.ws_bytes = self.lib.od_tta_merge_workspace_bytes(B, self.V, K)
        self.ws = torch.empty((self.ws_bytes,), dtype=torch.uint8, device=dev)
        self._desc = (_lib.TtaView * self.V)()
        for v in range(self.V):
            self._desc[v] = _lib.TtaView(self.keys[v].data_ptr(), self.counts[v].data_ptr(), self.boxes[v].data_ptr(), P,
                                         self.flips[v])

    def flip(self, x_u8: torch.Tensor) -> torch.Tensor:
        """Mirror uint8 [B,H,W,3] left-to-right into this pipeline's image buffer (od_hflip_u8)."""
        assert x_u8.dtype == torch.uint8 and x_u8.is_contiguous() and x_u8.shape == self.mirrored.shape
        B, H, W, _ = x_u8.shape
        _lib.check(self.lib.od_hflip_u8(self.ctx.handle, x_u8.data_ptr(), self.mirrored.data_ptr(), B, H, W, _stream_ptr()),
                   "od_hflip_u8")
        return self.mirrored

    def candidates(self, view: int, pred: torch.Tensor, conf_threshold: float):
        """pred of view `view` -> its boxes / sorted keys / counts (Postprocessor.candidates)."""
        self.post.candidates(pred, conf_threshold, self.boxes[view], self.keys[view], self.counts[view])

    def merge(self):
        """All views' candidates -> post.det (record block, word 0 of a row = class), self.src, post.keep_count; queues
        the single device->host copy of the block."""
        p = self.post
        # the soft scan in place of the greedy one (the report carries the rescored confidences): the two ABIs differ in
        # this argument group alone
        entry, nms = ("od_tta_merge_soft", (C.byref(p.soft_cfg()),)) if p.soft else \
            ("od_tta_merge", (p.iou_threshold, p.strict, p.max_det))
        _lib.check(getattr(self.lib, entry)(self.ctx.handle, self._desc, self.V, p.B, p.NC, p.K, *nms, self.vote_iou,
                                            p.det.data_ptr(), self.src.data_ptr(), p.keep_count.data_ptr(),
                                            self.ws.data_ptr(), self.ws_bytes, _stream_ptr()), entry)
        p.det_host.copy_(p.det, non_blocking=True)
        return p.det, p.keep_count

    def run(self, net, x_u8, conf_threshold: float):
        """The whole TTA step of one batch on the current stream: x_u8 (or net.input when None) through every view."""
        pred = net.forward(x_u8)
        self.candidates(0, pred, conf_threshold)
        for v in range(1, self.V):  # only "flip" is defined
            pred = net.forward(self.flip(net.input))
            self.candidates(v, pred, conf_threshold)
        return self.merge()
