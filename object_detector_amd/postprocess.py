"""Device post-processing of the prediction tensor: confidence + decode (K5/K6), exact top-K (K7), NMS (K8).

Replaces the in-graph decode + NMS of reference `ObjectDetector.predict` (voc_validate.py:27;
docs/MODEL.md:54-58 confidence = objectness x class probability, :78-82 same-class NMS).
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib
from .net import Context, _stream_ptr

# [BUILD-DEFINED] defaults (the reference does not pin them)
IOU_THRESHOLD = 0.45
PRE_NMS_TOPK = 1024
MAX_DETECTIONS = 200
LOC_SCALE = 0.1
MAX_CLASSES = 1024  # od_detect / od_head_postprocess / od_loss_fwd_bwd: 1 <= NC <= 1024
# the suppression stage: greedy NMS, or Soft-NMS with linear / Gaussian score decay (DESIGN.md "Soft-NMS")
NMS_METHODS = {"hard": _lib.OD_NMS_HARD, "soft-linear": _lib.OD_NMS_SOFT_LINEAR, "soft-gaussian": _lib.OD_NMS_SOFT_GAUSSIAN}
SOFT_SIGMA = 0.5
SOFT_MIN_CONF_FLOOR = 1e-6  # od_soft_nms_cfg.min_conf >= 1e-6


def check_nms_args(nms="hard", soft_sigma=SOFT_SIGMA, soft_min_conf=None):
    """The `nms=` / `soft_sigma=` / `soft_min_conf=` arguments of Postprocessor and ObjectDetector -> (nms, sigma, min_conf
    or None), or ValueError.  Touches no device."""
    if nms not in NMS_METHODS:
        raise ValueError(f"nms must be one of {tuple(NMS_METHODS)}, got {nms!r}")
    sigma = float(soft_sigma)
    if not sigma > 0:
        raise ValueError(f"soft_sigma must be > 0, got {soft_sigma!r}")
    if soft_min_conf is not None:
        soft_min_conf = float(soft_min_conf)
        if not soft_min_conf >= SOFT_MIN_CONF_FLOOR:
            raise ValueError(f"soft_min_conf must be >= {SOFT_MIN_CONF_FLOOR}, got {soft_min_conf!r}")
    return nms, sigma, soft_min_conf


def records_host(block, n_valid):
    """A pinned record block [B, 1 + 6*max_det] (word 0 = the keep count, row r = {word0 (int bits), conf, x1, y1, x2, y2})
    -> [(word0 i32 [n], conf f32 [n], boxes f32 [n,4])] for its first n_valid images."""
    a = block.numpy()
    out = []
    for b in range(n_valid):
        n = int(a[b, :1].view(np.int32)[0])
        rows = a[b, 1:1 + 6 * n].reshape(n, 6)
        out.append((rows[:, 0].copy().view(np.int32), rows[:, 1].copy(), rows[:, 2:6].copy()))
    return out


class Postprocessor:
    def __init__(self, batch_size, num_priors, num_classes, priors, device="cuda:0", topk=PRE_NMS_TOPK,
                 max_det=MAX_DETECTIONS, iou_threshold=IOU_THRESHOLD, strict_nms=False, loc_scale=LOC_SCALE, nms="hard",
                 soft_sigma=SOFT_SIGMA, soft_min_conf=None):
        # nms="hard" (default): the greedy scan, exactly the calls below.  "soft-linear" / "soft-gaussian": the soft scan
        # (od_detect_soft / od_soft_nms / the _soft merges); soft_min_conf=None means the call's conf_threshold.
        self.nms_method, self.soft_sigma, self.soft_min_conf = check_nms_args(nms, soft_sigma, soft_min_conf)
        self.soft = self.nms_method != "hard"
        self._conf_threshold = None  # of the last run() / candidates call: the soft scan's min_conf when none is given
        self.ctx = Context.get(device)
        self.lib = self.ctx.lib
        dev = torch.device(device)
        self.B, self.P, self.NC = int(batch_size), int(num_priors), int(num_classes)
        if not 1 <= self.NC <= MAX_CLASSES:
            raise _lib.OdError(f"Postprocessor: num_classes = {self.NC} outside the supported class counts 1..{MAX_CLASSES}")
        self.K, self.max_det = int(topk), int(max_det)
        self.iou_threshold, self.strict, self.loc_scale = float(iou_threshold), int(bool(strict_nms)), float(loc_scale)
        self.priors = torch.as_tensor(priors, dtype=torch.float32).contiguous().to(dev)
        assert self.priors.shape == (self.P, 4)
        B, P, NC, K = self.B, self.P, self.NC, self.K
        # the product path (run -> od_detect) never materialises the confidence tensor; `conf` is filled on demand from the
        # last pred (same kernel code, same bits) for callers that want the dense [B,P,NC] view (tests, head())
        self._conf = None
        self._pred = None
        self._conf_valid = False
        self.fused = P % 2 == 0  # NC > 76 runs od_detect's streamed kernels (same entry point, same results)
        self.boxes = torch.empty((B, P, 4), dtype=torch.float32, device=dev)
        self.keys = torch.empty((B, K), dtype=torch.int64, device=dev)  # u64 payload
        self.counts = torch.empty((B,), dtype=torch.int32, device=dev)
        self.keep_flat = torch.empty((B, self.max_det), dtype=torch.int32, device=dev)
        self.keep_count = torch.empty((B,), dtype=torch.int32, device=dev)
        self.keep_conf = torch.empty((B, self.max_det), dtype=torch.float32, device=dev) if self.soft else None
        self.ws_topk_bytes = self.lib.od_topk_workspace_bytes(B, P * NC, K)
        self.ws_nms_bytes = self.lib.od_nms_workspace_bytes(B, K)
        # kept detections of the batch as one record block + its pinned host mirror: ONE device->host copy per batch
        self.det = torch.empty((B, 1 + 6 * self.max_det), dtype=torch.float32, device=dev)
        self.det_host = torch.empty((B, 1 + 6 * self.max_det), dtype=torch.float32).pin_memory()
        self._ws_topk = None  # only the three-call path (head / topk / nms separately) needs it
        self.ws_nms = torch.empty((self.ws_nms_bytes,), dtype=torch.uint8, device=dev)
        self.ws_det_bytes = self.lib.od_detect_workspace_bytes(B, P, NC, K)
        self.ws_det = torch.empty((self.ws_det_bytes,), dtype=torch.uint8, device=dev)
        _lib.check(self.lib.od_detect_workspace_init(self.ctx.handle, self.ws_det.data_ptr(), self.ws_det_bytes, B, P, NC,
                                                     _stream_ptr()), "od_detect_workspace_init")
        torch.cuda.current_stream(dev).synchronize()  # the pipelines use this workspace on their own streams

    @property
    def ws_topk(self):
        if self._ws_topk is None:
            self._ws_topk = torch.empty((self.ws_topk_bytes,), dtype=torch.uint8, device=self.priors.device)
        return self._ws_topk

    @property
    def conf(self):
        """Dense confidences f32 [B,P,NC] of the last batch: written by head(), or computed on demand from the pred that
        run() saw (od_head_postprocess: the same confidence code as the fused path, bit-identical values)."""
        if self._conf is None:
            self._conf = torch.empty((self.B, self.P, self.NC), dtype=torch.float32, device=self.priors.device)
        if not self._conf_valid:
            if self._pred is None:
                raise _lib.OdError("Postprocessor.conf: nothing has been processed yet")
            self.head(self._pred)
        return self._conf

    def head(self, pred: torch.Tensor, clip=True):
        assert pred.dtype == torch.float32 and pred.is_contiguous() and tuple(pred.shape) == (self.B, self.P, self.NC + 6)
        if self._conf is None:
            self._conf = torch.empty((self.B, self.P, self.NC), dtype=torch.float32, device=self.priors.device)
        _lib.check(self.lib.od_head_postprocess(self.ctx.handle, pred.data_ptr(), self.priors.data_ptr(),
                                                self._conf.data_ptr(), self.boxes.data_ptr(), self.B, self.P, self.NC,
                                                self.loc_scale, int(clip), _stream_ptr()), "od_head_postprocess")
        self._pred, self._conf_valid = pred, True
        return self._conf, self.boxes

    def topk(self, conf: torch.Tensor, conf_threshold: float):
        assert conf.dtype == torch.float32 and conf.is_contiguous()
        self._conf_threshold = float(conf_threshold)
        _lib.check(self.lib.od_topk_scores(self.ctx.handle, conf.data_ptr(), self.B, self.P * self.NC, self.K,
                                           float(conf_threshold), self.keys.data_ptr(), self.counts.data_ptr(),
                                           self.ws_topk.data_ptr(), self.ws_topk_bytes, _stream_ptr()), "od_topk_scores")
        return self.keys, self.counts

    def soft_cfg(self, conf_threshold=None):
        """The od_soft_nms_cfg of this post-processor; min_conf = soft_min_conf, or the given / last conf_threshold."""
        if conf_threshold is None:
            conf_threshold = self._conf_threshold
        mc = self.soft_min_conf
        if mc is None:
            if conf_threshold is None:
                raise _lib.OdError("Postprocessor.soft_cfg: no conf_threshold yet and no soft_min_conf")
            mc = max(float(conf_threshold), SOFT_MIN_CONF_FLOOR)
        return _lib.SoftNmsCfg(NMS_METHODS[self.nms_method], self.strict, self.max_det, self.iou_threshold, self.soft_sigma, mc)

    def nms(self, boxes: torch.Tensor, keys: torch.Tensor, counts: torch.Tensor):
        if self.soft:
            cfg = self.soft_cfg()
            _lib.check(self.lib.od_soft_nms(self.ctx.handle, boxes.data_ptr(), keys.data_ptr(), counts.data_ptr(), self.B,
                                            self.P, self.NC, self.K, C.byref(cfg), self.keep_flat.data_ptr(),
                                            self.keep_conf.data_ptr(), self.keep_count.data_ptr(), self.det.data_ptr(),
                                            self.ws_nms.data_ptr(), self.ws_nms_bytes, _stream_ptr()), "od_soft_nms")
            return self.keep_flat, self.keep_count
        _lib.check(self.lib.od_nms(self.ctx.handle, boxes.data_ptr(), keys.data_ptr(), counts.data_ptr(), self.B,
                                   self.P, self.NC, self.K, self.iou_threshold, self.strict, self.max_det,
                                   self.keep_flat.data_ptr(), self.keep_count.data_ptr(), self.ws_nms.data_ptr(),
                                   self.ws_nms_bytes, _stream_ptr()), "od_nms")
        return self.keep_flat, self.keep_count

    def gather(self):
        """Queue the gather of this batch's kept detections (od_gather_detections) and its copy into the pinned host block
        on the current stream; read with detections_host() after the stream / event has been waited for.  A soft
        post-processor's scan has written the record block already, with the rescored confidences: only the copy is queued."""
        if self.soft:
            self.det_host.copy_(self.det, non_blocking=True)
            return
        _lib.check(self.lib.od_gather_detections_pred(self.ctx.handle, self._pred.data_ptr(), self.boxes.data_ptr(),
                                                      self.keep_flat.data_ptr(), self.keep_count.data_ptr(), self.B, self.P,
                                                      self.NC, self.max_det, self.det.data_ptr(), _stream_ptr()),
                   "od_gather_detections_pred")
        self.det_host.copy_(self.det, non_blocking=True)

    def detections_host(self, n_valid):
        """-> [(flat i32 [n], conf f32 [n], boxes f32 [n,4])] for the first n_valid images, from the pinned block."""
        return records_host(self.det_host, n_valid)

    def candidates(self, pred: torch.Tensor, conf_threshold: float, boxes, keys, counts):
        """pred [B,P,C] -> boxes [B,P,4] / sorted keys [B,K] / counts [B] in the caller's buffers (od_detect_candidates:
        od_detect without the NMS, clip = 1): what the merges of tta.py and slicing.py take one list per view / row from."""
        assert pred.dtype == torch.float32 and pred.is_contiguous() and tuple(pred.shape) == (self.B, self.P, self.NC + 6)
        self._conf_threshold = float(conf_threshold)
        _lib.check(self.lib.od_detect_candidates(self.ctx.handle, pred.data_ptr(), self.priors.data_ptr(), self.B, self.P,
                                                 self.NC, self.loc_scale, 1, float(conf_threshold), self.K, boxes.data_ptr(),
                                                 None, keys.data_ptr(), counts.data_ptr(), self.ws_det.data_ptr(),
                                                 self.ws_det_bytes, self.ws_nms.data_ptr(), self.ws_nms_bytes, _stream_ptr()),
                   "od_detect_candidates")

    def run(self, pred: torch.Tensor, conf_threshold: float):
        """pred [B,P,C] -> (keep_flat i32 [B,max_det] (-1 padded), keep_count i32 [B]); boxes / keys stay on device.
        ONE C-ABI call (od_detect, three launches); run_unfused() is the same result through head -> topk -> nms."""
        if not self.fused:
            return self.run_unfused(pred, conf_threshold)
        assert pred.dtype == torch.float32 and pred.is_contiguous() and tuple(pred.shape) == (self.B, self.P, self.NC + 6)
        self._conf_threshold = float(conf_threshold)
        if self.soft:
            cfg = self.soft_cfg()
            _lib.check(self.lib.od_detect_soft(self.ctx.handle, pred.data_ptr(), self.priors.data_ptr(), self.B, self.P, self.NC,
                                               self.loc_scale, 1, float(conf_threshold), self.K, C.byref(cfg),
                                               self.boxes.data_ptr(), None, self.keys.data_ptr(), self.counts.data_ptr(),
                                               self.keep_flat.data_ptr(), self.keep_conf.data_ptr(),
                                               self.keep_count.data_ptr(), self.det.data_ptr(), self.ws_det.data_ptr(),
                                               self.ws_det_bytes, self.ws_nms.data_ptr(), self.ws_nms_bytes, _stream_ptr()),
                       "od_detect_soft")
            self._pred, self._conf_valid = pred, False
            return self.keep_flat, self.keep_count
        _lib.check(self.lib.od_detect(self.ctx.handle, pred.data_ptr(), self.priors.data_ptr(), self.B, self.P, self.NC,
                                      self.loc_scale, 1, float(conf_threshold), self.K, self.iou_threshold, self.strict,
                                      self.max_det, self.boxes.data_ptr(), None, self.keys.data_ptr(), self.counts.data_ptr(),
                                      self.keep_flat.data_ptr(), self.keep_count.data_ptr(), self.ws_det.data_ptr(),
                                      self.ws_det_bytes, self.ws_nms.data_ptr(), self.ws_nms_bytes, _stream_ptr()), "od_detect")
        self._pred, self._conf_valid = pred, False
        return self.keep_flat, self.keep_count

    def run_unfused(self, pred: torch.Tensor, conf_threshold: float):
        """The three-call path (od_head_postprocess -> od_topk_scores -> od_nms): materialises conf, same kept indices."""
        conf, boxes = self.head(pred)
        keys, counts = self.topk(conf, conf_threshold)
        return self.nms(boxes, keys, counts)
