"""`od.pb`: prior boxes with device-side encode_truth / decode_locs (reference check_assign.py:21,25-27).

`decode_locs(locs, xp=np)` and `encode_truth(y)` keep the reference call shapes; both run the HIP kernels
(od_decode_locs / od_assign_anchors) and hand numpy arrays back, exactly what check_assign.py consumes.

`PriorBoxes(..., ignore_regions=True)` [BUILD-DEFINED, opt-in]: `ObjectsAnnotation.difficults` (COCO iscrowd, VOC difficult,
a sliver a mosaic tile border left of an object) marks ignore regions, as both evaluators treat them.  Such a box owns no
prior, and a prior that would be background is not trained on (all-zero target row) when at least `ign_thr` of ITS area lies
inside a region (od_assign_anchors_ign).  IGN_THR = 0.5 is a policy value of this build, not a tolerance.

`PriorBoxes(..., assigner="atss", atss_topk=9)` [BUILD-DEFINED, opt-in]: Adaptive Training Sample Selection (Zhang et al.,
CVPR 2020) decides which priors learn which object instead of the fixed IoU thresholds: the priors of the `atss_topk` cells
nearest to the object's centre on every level are candidates, and the IoU threshold is the candidates' own mean + standard
deviation (od_assign_atss; the frozen rule is the header comment of csrc/assign_atss.hip).  `pos_thr` / `neg_thr` are unused
there; `ignore_regions` works as above.  The default "max-iou" is the rule of od_assign_anchors.

`PriorBoxes(..., assigner="tal", tal_topk=13, tal_alpha=1.0, tal_beta=6.0)` [BUILD-DEFINED, opt-in]: task-aligned assignment
(TOOD, Feng et al., ICCV 2021).  The only assigner that reads the network's output: `encode_batch(annotations, pred=...)`
takes this step's raw predictions (device f32 [B,P,NC+6]), and an object's positives are the `tal_topk` priors, among those
whose cell centre lies inside it, with the largest P(object) * P(class) ^ alpha * IoU(predicted box, object) ^ beta
(od_assign_tal; the frozen rule is the header comment of csrc/assign_tal.hip).  There is nothing to encode before the forward
pass, so `encode_truth` / `encode_truth_device` refuse it: pass the annotations to `Trainer.step`.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib, priors as PR
from .net import Context, _stream_ptr

POS_THR, NEG_THR, LOC_SCALE = 0.5, 0.4, 0.1
IGN_THR = 0.5
GMAX = 128
ASSIGNERS = ("max-iou", "atss", "tal")
ATSS_TOPK, ATSS_MAX_TOPK = 9, 32
TAL_TOPK, TAL_MAX_TOPK, TAL_ALPHA, TAL_BETA = 13, 32, 1.0, 6.0  # TOOD's defaults


def check_assigner(assigner, atss_topk):
    """ValueError for an assigner or a top-k that od_assign_atss would refuse (host-only: no library is loaded)."""
    if assigner not in ASSIGNERS:
        raise ValueError(f"assigner must be one of {ASSIGNERS}, got {assigner!r}")
    if isinstance(atss_topk, bool) or int(atss_topk) != atss_topk or not 1 <= int(atss_topk) <= ATSS_MAX_TOPK:
        raise ValueError(f"atss_topk must be an integer in 1..{ATSS_MAX_TOPK}, got {atss_topk!r}")
    return assigner, int(atss_topk)


def check_tal(tal_topk, tal_alpha, tal_beta):
    """ValueError for what od_assign_tal would refuse: a top-k outside 1..32, a non-positive or non-finite alpha / beta
    (host-only: no library is loaded)."""
    if isinstance(tal_topk, bool) or int(tal_topk) != tal_topk or not 1 <= int(tal_topk) <= TAL_MAX_TOPK:
        raise ValueError(f"tal_topk must be an integer in 1..{TAL_MAX_TOPK}, got {tal_topk!r}")
    for name, v in (("tal_alpha", tal_alpha), ("tal_beta", tal_beta)):
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not (np.isfinite(v) and v > 0):
            raise ValueError(f"{name} must be a finite number > 0, got {v!r}")
    return int(tal_topk), float(tal_alpha), float(tal_beta)


class ObjectsAnnotation:
    """Ground truth of one image (what the generator yields when encode_truth is None: `.classes`, `.bboxes`,
    reference check_generator.py:21).  bboxes are corner form, normalised [0,1]."""

    def __init__(self, path=None, width=0, height=0, classes=(), bboxes=(), difficults=None):
        self.path = path
        self.width, self.height = int(width), int(height)
        self.classes = np.asarray(classes, np.int32).reshape(-1)
        self.bboxes = np.asarray(bboxes, np.float32).reshape(-1, 4)
        self.difficults = (np.zeros(len(self.classes), bool) if difficults is None
                           else np.asarray(difficults, bool).reshape(-1))

    @property
    def num_objects(self):
        return len(self.classes)

    def select(self, keep, bboxes=None, difficults=None, width=None, height=None):
        """The objects `keep` (bool mask or indices) names: classes, boxes and difficult flags are filtered TOGETHER, so a
        dropped box never shifts another box's flag.  bboxes / difficults (full length) replace the stored ones first."""
        b = self.bboxes if bboxes is None else np.asarray(bboxes, np.float32).reshape(-1, 4)
        d = self.difficults if difficults is None else np.asarray(difficults, bool).reshape(-1)
        assert len(b) == len(d) == len(self.classes)
        return ObjectsAnnotation(self.path, self.width if width is None else width, self.height if height is None else height,
                                 self.classes[keep], b[keep], d[keep])


class PriorBoxes:
    def __init__(self, input_size=(320, 320), num_classes=20, prior_wh=PR.DEFAULT_PRIOR_WH, device="cuda:0",
                 pos_thr=POS_THR, neg_thr=NEG_THR, loc_scale=LOC_SCALE, ignore_regions=False, ign_thr=IGN_THR,
                 assigner="max-iou", atss_topk=ATSS_TOPK, tal_topk=TAL_TOPK, tal_alpha=TAL_ALPHA, tal_beta=TAL_BETA):
        self.assigner, self.atss_topk = check_assigner(assigner, atss_topk)
        self.tal_topk, self.tal_alpha, self.tal_beta = check_tal(tal_topk, tal_alpha, tal_beta)
        self.input_size = tuple(int(v) for v in input_size)
        self.num_classes = int(num_classes)
        self.prior_wh = np.asarray(prior_wh, np.float64)
        self.pb_locs = PR.make_priors(self.input_size, self.prior_wh)  # f32 [P,4]
        self.pos_thr, self.neg_thr, self.loc_scale = float(pos_thr), float(neg_thr), float(loc_scale)
        self.ignore_regions, self.ign_thr = bool(ignore_regions), float(ign_thr)
        if self.ignore_regions and not self.ign_thr > 0.0:
            raise ValueError(f"ign_thr must be > 0, got {ign_thr!r}")
        self.device = torch.device(device)
        self._ctx = None
        self._priors_dev = None
        self.last_metric = None  # assigner="tal": the metric [B,P] of the last encode_batch (device)

    def __len__(self):
        return len(self.pb_locs)

    # -- device plumbing ------------------------------------------------------------------------------------
    def _ensure(self):
        if self._ctx is None:
            self._ctx = Context.get(self.device)
            self._priors_dev = torch.from_numpy(self.pb_locs).to(self.device)
        return self._ctx

    @property
    def priors_device(self):
        self._ensure()
        return self._priors_dev

    def decode_locs(self, locs, xp=np):
        """corner-form offsets [P,4] / [N,P,4] -> boxes; zeros decode to the prior boxes (check_assign.py:27)."""
        from . import ops
        self._ensure()
        if isinstance(locs, torch.Tensor):
            t = locs.to(self.device, torch.float32)
        else:
            t = torch.from_numpy(np.ascontiguousarray(np.asarray(locs, np.float32))).to(self.device)
        out = ops.decode_locs(t, self._priors_dev, self.loc_scale, clip=False)
        if xp is np:
            return out.cpu().numpy()
        return out

    def encode_batch(self, annotations, return_device=False, pred=None):
        """list[ObjectsAnnotation] -> y f32 [B,P,2+NC+4] (+ npos [B], assigned [B,P]) through od_assign_anchors, or, with
        ignore_regions=True, through od_assign_anchors_ign with `difficults` as the region flags (assigned -3 = ignored by a
        region).  assigner="atss": through od_assign_atss, with the same flags.  assigner="tal": through od_assign_tal on
        `pred`, the network's raw output of this step (device f32 [B,P,NC+6]; the static assigners ignore it); the metric
        of the call stays in `self.last_metric` (device f32 [B,P])."""
        self._check_pred(len(annotations), pred)
        return self.encode_uploaded(self.upload_batch(annotations), return_device=return_device, pred=pred)

    def _check_pred(self, B, pred):
        P, NC = len(self.pb_locs), self.num_classes
        if self.assigner == "tal":
            if not isinstance(pred, torch.Tensor) or not pred.is_cuda or pred.dtype != torch.float32 \
                    or tuple(pred.shape) != (B, P, NC + 6):
                raise ValueError(f'assigner "tal" needs pred: a device f32 tensor [{B}, {P}, {NC + 6}], got '
                                 + ("None" if pred is None else f"{type(pred).__name__} {tuple(getattr(pred, 'shape', ()))} "
                                    f"{getattr(pred, 'dtype', '')} on {getattr(pred, 'device', '?')}"))

    def upload_batch(self, annotations):
        """The host half of encode_batch: boxes, classes, counts and region flags of a batch, packed and copied to the
        device -> what encode_uploaded takes.  Trainer.step with assigner="tal" does this BEFORE its forward pass, so that
        no host-to-device copy sits between the forward pass and the assignment."""
        self._ensure()
        B = len(annotations)
        gmax = max(1, max((a.num_objects for a in annotations), default=1))
        if gmax > GMAX:
            raise ValueError(f"more than {GMAX} objects in one image")
        gb = np.zeros((B, gmax, 4), np.float32)
        gc = np.zeros((B, gmax), np.int32)
        gn = np.zeros((B,), np.int32)
        gf = np.zeros((B, gmax), np.int32) if self.ignore_regions else None
        for i, a in enumerate(annotations):
            n = a.num_objects
            gb[i, :n], gc[i, :n], gn[i] = a.bboxes, a.classes, n
            if gf is not None:
                gf[i, :n] = a.difficults
        dev = self.device
        gb_t, gc_t, gn_t = (torch.from_numpy(v).to(dev) for v in (gb, gc, gn))
        gf_t = torch.from_numpy(gf).to(dev) if gf is not None else None
        return B, gmax, gb_t, gc_t, gn_t, gf_t

    def encode_uploaded(self, uploaded, return_device=False, pred=None):
        """The device half of encode_batch, on the current stream: the assigner's launches on an upload_batch result."""
        B, gmax, gb_t, gc_t, gn_t, gf_t = uploaded
        self._check_pred(B, pred)
        ctx, dev = self._ensure(), self.device
        P, NC = len(self.pb_locs), self.num_classes
        y = torch.empty((B, P, NC + 6), dtype=torch.float32, device=dev)
        npos = torch.empty((B,), dtype=torch.int32, device=dev)
        assigned = torch.empty((B, P), dtype=torch.int32, device=dev)
        if self.assigner == "tal":
            levels = PR.level_shapes(self.input_size)
            grid_hw = (C.c_int32 * (2 * len(levels)))(*[v for hw in levels for v in hw])
            wsb = ctx.lib.od_assign_tal_workspace_bytes(B, P, gmax)
            ws = torch.empty((wsb,), dtype=torch.uint8, device=dev)
            pred = pred.contiguous()
            self.last_metric = torch.empty((B, P), dtype=torch.float32, device=dev)
            _lib.check(ctx.lib.od_assign_tal(ctx.handle, self._priors_dev.data_ptr(), grid_hw, len(levels), PR.NUM_PRIORS,
                                             pred.data_ptr(), gb_t.data_ptr(), gc_t.data_ptr(), gn_t.data_ptr(),
                                             None if gf_t is None else gf_t.data_ptr(), self.ign_thr, self.tal_alpha,
                                             self.tal_beta, self.tal_topk, B, P, gmax, NC, self.loc_scale, y.data_ptr(),
                                             assigned.data_ptr(), npos.data_ptr(), self.last_metric.data_ptr(),
                                             ws.data_ptr(), wsb, _stream_ptr()), "od_assign_tal")
        elif self.assigner == "atss":
            levels = PR.level_shapes(self.input_size)
            grid_hw = (C.c_int32 * (2 * len(levels)))(*[v for hw in levels for v in hw])
            wsb = ctx.lib.od_assign_atss_workspace_bytes(B, P, gmax)
            ws = torch.empty((wsb,), dtype=torch.uint8, device=dev)
            _lib.check(ctx.lib.od_assign_atss(ctx.handle, self._priors_dev.data_ptr(), grid_hw, len(levels), PR.NUM_PRIORS,
                                              gb_t.data_ptr(), gc_t.data_ptr(), gn_t.data_ptr(),
                                              None if gf_t is None else gf_t.data_ptr(), self.ign_thr, self.atss_topk,
                                              B, P, gmax, NC, self.loc_scale, y.data_ptr(), assigned.data_ptr(),
                                              npos.data_ptr(), ws.data_ptr(), wsb, _stream_ptr()), "od_assign_atss")
        else:
            wsb = ctx.lib.od_assign_workspace_bytes(B, P, gmax)
            ws = torch.empty((wsb,), dtype=torch.uint8, device=dev)
            if gf_t is not None:
                _lib.check(ctx.lib.od_assign_anchors_ign(ctx.handle, self._priors_dev.data_ptr(), gb_t.data_ptr(),
                                                         gc_t.data_ptr(), gn_t.data_ptr(), gf_t.data_ptr(), self.ign_thr, B, P,
                                                         gmax, NC, self.pos_thr, self.neg_thr, self.loc_scale, y.data_ptr(),
                                                         assigned.data_ptr(), npos.data_ptr(), ws.data_ptr(), wsb,
                                                         _stream_ptr()), "od_assign_anchors_ign")
            else:
                _lib.check(ctx.lib.od_assign_anchors(ctx.handle, self._priors_dev.data_ptr(), gb_t.data_ptr(), gc_t.data_ptr(),
                                                     gn_t.data_ptr(), B, P, gmax, NC, self.pos_thr, self.neg_thr,
                                                     self.loc_scale, y.data_ptr(), assigned.data_ptr(), npos.data_ptr(),
                                                     ws.data_ptr(), wsb, _stream_ptr()), "od_assign_anchors")
        if return_device:
            return y, npos, assigned
        return y.cpu().numpy(), npos.cpu().numpy(), assigned.cpu().numpy()

    def _no_truth_without_pred(self):
        if self.assigner == "tal":
            raise ValueError('assigner "tal" assigns from the predictions of the step, so there is no target before the '
                             'forward pass: hand the annotations to Trainer.step(x, annotations=...) (a generator with '
                             'encode_truth=None yields them), or call encode_batch(annotations, pred=...)')

    def encode_truth_device(self, y):
        """encode_truth whose result stays on the device: list of annotations -> f32 DEVICE tensor [B,P,C] (the generator
        callback for training loops: `Trainer.step(x, y_target=...)` takes it as is)."""
        self._no_truth_without_pred()
        if isinstance(y, ObjectsAnnotation):
            y = [y]
        return self.encode_batch(list(y), return_device=True)[0]

    def encode_truth(self, y):
        """Generator callback (check_assign.py:21): list of annotations -> array [B,P,C]; one annotation -> [P,C]."""
        self._no_truth_without_pred()
        if isinstance(y, ObjectsAnnotation):
            return self.encode_batch([y])[0][0]
        return self.encode_batch(list(y))[0]
