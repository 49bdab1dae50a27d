"""Validation during Trainer.fit: a detector whose weights are refreshed on the device from the live trainer
(ObjectDetector.refresh_from: one od_net_refresh launch, no host round trip), run over a held-out set and scored.

    od = ObjectDetector.from_trainer(tr, batch_size=16)
    v = Validator(od, X_val, y_val, keep_best="results/best.npz")
    tr.fit(batches, steps, validate_every=500, validator=v)     # v.history: one record per validation

The validator reads the trainer's buffers and writes none of them: a run with it ends with the weights, statistics and
losses of the run without it.  Under a multi-rank launch predict() shards the images over the ranks as it always does
(every rank ends with all predictions); only the main process writes the keep_best file.
"""
from __future__ import annotations

import os
import pathlib

import numpy as np

from . import weights as W

COCO_STAT_NAMES = ("AP", "AP50", "AP75", "AP_small", "AP_medium", "AP_large", "AR1", "AR10", "AR100", "AR_small", "AR_medium",
                   "AR_large")
METRICS = ("mAP", "mAP_VOC") + tuple("coco_" + n for n in COCO_STAT_NAMES)


def coco_ground_truth(y, num_classes, class_names=None):
    """ObjectsAnnotation list -> tk.data.coco's CocoGroundTruth (image ids 0..n-1 in order, category ids = class indices
    0..num_classes-1, pixel xywh boxes from the normalised corners, `difficults` as crowd flags) for tk.data.coco.evaluate.
    num_classes is the DETECTOR's class count, not what the annotations happen to contain: every class it can predict must
    be a category (a class without ground truth scores -1 and is left out of the means, as in pycocotools).  ValueError for
    class_names of another length or an annotated class outside 0..num_classes-1."""
    from .cocoeval import CocoGroundTruth
    y = list(y)
    nc = int(num_classes)
    if class_names is not None and len(class_names) != nc:
        raise ValueError(f"{len(class_names)} class names for {nc} classes")
    top = max([int(np.max(a.classes)) for a in y if len(a.classes)], default=-1)
    low = min([int(np.min(a.classes)) for a in y if len(a.classes)], default=0)
    if top >= nc or low < 0:
        raise ValueError(f"annotated classes {low}..{top} are not all inside the detector's 0..{nc - 1}")
    img, cls, box, crowd = [], [], [], []
    for i, a in enumerate(y):
        w, h = float(a.width), float(a.height)
        for c, b, d in zip(a.classes, np.asarray(a.bboxes, np.float64).reshape(-1, 4), a.difficults):
            img.append(i)
            cls.append(int(c))
            box.append([b[0] * w, b[1] * h, (b[2] - b[0]) * w, (b[3] - b[1]) * h])
            crowd.append(bool(d))
    boxes = np.asarray(box, np.float64).reshape(-1, 4)
    return CocoGroundTruth(
        image_ids=np.arange(len(y), dtype=np.int64), widths=np.array([float(a.width) for a in y], np.float64),
        heights=np.array([float(a.height) for a in y], np.float64), file_names=[str(getattr(a, "path", "")) for a in y],
        category_ids=np.arange(nc, dtype=np.int64),
        category_names=[str(n) for n in (class_names if class_names is not None else range(nc))],
        ann_image_ids=np.asarray(img, np.int64), ann_classes=np.asarray(cls, np.int64), ann_bboxes=boxes,
        ann_areas=boxes[:, 2] * boxes[:, 3], ann_crowd=np.asarray(crowd, bool))


def write_params_atomically(path, params, meta=None):
    """weights.save to a temporary file beside `path`, then one rename: a run killed while writing leaves the previous
    file whole (how scripts/train.py writes state.npz)."""
    path = pathlib.Path(path)
    path.parent.mkdir(parents=True, exist_ok=True)
    tmp = path.with_name(path.name + ".tmp.npz")  # np.savez keeps a name that already ends in .npz
    W.save(tmp, params, meta)
    os.replace(tmp, path)


class Validator:
    """validator(trainer, step) -> the record it appended to validator.history:

      1. od.refresh_from(trainer, ema): ema=None takes the averaged model when the trainer keeps one, the raw weights
         otherwise; True / False choose
      2. od.predict(X, conf_threshold): whatever route the detector was built with (tta, slices, nms=, image_decode)
      3. tk.data.voc.evaluate -> {"step", "mAP", "mAP_VOC", "ema"}; coco=True adds the twelve COCO statistics as "coco_AP",
         "coco_AP50", ... "coco_AR_large" (tk.data.coco.evaluate on ground truth converted once, in the constructor)
      4. keep_best=path: when record[metric] is above every earlier one, trainer.export_params(ema) is written to `path`
         (temporary file, then rename) by the main process; best_step / best_value remember it

    od: an ObjectDetector of the trainer's architecture on its device (ObjectDetector.from_trainer); X, y: images (paths
    or arrays) and their ObjectsAnnotation.  ValueError for an unknown metric, a COCO metric without coco=True, or
    len(X) != len(y)."""

    def __init__(self, od, X, y, conf_threshold=0.01, metric="mAP_VOC", ema=None, coco=False, keep_best=None,
                 class_names=None):
        if metric not in METRICS:
            raise ValueError(f"metric must be one of {METRICS}, got {metric!r}")
        if metric.startswith("coco_") and not coco:
            raise ValueError(f"metric {metric!r} needs coco=True")
        self.X, self.y = list(X), list(y)
        if len(self.X) != len(self.y):
            raise ValueError(f"{len(self.X)} images for {len(self.y)} annotations")
        self.od, self.conf_threshold, self.metric = od, float(conf_threshold), metric
        self.ema, self.coco = ema, bool(coco)
        self.keep_best = None if keep_best is None else pathlib.Path(keep_best)
        self.history, self.best_step, self.best_value = [], None, None
        self.last_predictions = None  # the ObjectsPrediction list of the latest call (plots, per-class scores)
        self._coco_gt = coco_ground_truth(self.y, od.num_classes, class_names) if self.coco else None

    def resume_best(self):
        """A continued run: take best_step / best_value from the meta of an existing keep_best file (written with this
        metric), so that a first validation that scores worse does not replace it.  -> True when it did.  A fresh run does
        not call this: its first validation starts a new file."""
        if self.keep_best is None or not self.keep_best.exists():
            return False
        with np.load(self.keep_best, allow_pickle=False) as z:
            if "__meta__." + self.metric not in z.files or "__meta__.step" not in z.files:
                return False
            self.best_value, self.best_step = float(z["__meta__." + self.metric]), int(z["__meta__.step"])
        return True

    def __call__(self, trainer, step):
        from .tk.data import voc
        from .tk.dl import is_main_process
        ema = (trainer.ema_decay is not None) if self.ema is None else bool(self.ema)
        self.od.refresh_from(trainer, ema=ema)
        pred = self.last_predictions = self.od.predict(self.X, conf_threshold=self.conf_threshold)
        rec = {"step": int(step)}
        rec.update(voc.evaluate(self.y, pred, num_classes=self.od.num_classes))
        rec["ema"] = ema
        if self.coco:
            from .tk.data import coco
            stats = coco.evaluate(self._coco_gt, pred, device=self.od.device).stats
            rec.update({"coco_" + n: float(v) for n, v in zip(COCO_STAT_NAMES, stats)})
        self.history.append(rec)
        if self.best_value is None or rec[self.metric] > self.best_value:
            self.best_step, self.best_value = int(step), rec[self.metric]
            if self.keep_best is not None and is_main_process():
                write_params_atomically(self.keep_best, trainer.export_params(ema=ema),
                                        {"prior_wh": np.asarray(trainer.pb.prior_wh), "step": np.int64(step),
                                         self.metric: np.float64(rec[self.metric])})
        return rec
