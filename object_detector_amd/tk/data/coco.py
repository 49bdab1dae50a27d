"""tk.data.coco: detection data in COCO's annotation format (one instances JSON + an image directory), for datasets with
more classes than VOC's 20.  Host-side only, standard library json.

load_od(annotation_json, image_dir) -> (X, y, class_names):
  X            object array of image paths (image_dir / file_name), in the JSON's image order
  y            object array of ObjectsAnnotation: corner-form boxes normalised by the image's width / height
               (COCO bbox = [x, y, w, h] in pixels), classes 0..NC-1
  class_names  the category names, in ascending category id (class i = the i-th smallest id)
Crowd regions (iscrowd = 1) are kept as `difficults`, which tk.data.voc.evaluate neither counts nor penalises.  Images
without annotations are kept with zero objects.  An image with more than pb.GMAX objects raises ValueError naming it (the
anchor assignment takes at most GMAX ground-truth boxes per image; nothing is truncated).

COCO bbox evaluation (object_detector_amd/cocoeval.py; the matching and accumulation run on the GPU):
  load_gt(annotation_json) -> CocoGroundTruth         the raw boxes, areas, crowd flags and ids load_od normalises away
  to_results(gt, y_pred, image_ids=None) -> [dict]    ObjectsPrediction lists as COCO result dicts; save_results(path, r)
  evaluate(gt, predictions, image_ids=None) -> CocoEvaluation   stats (12,), precision / recall / scores, summary(),
                                                      ap_per_class()"""
from __future__ import annotations

import json
import pathlib

import numpy as np

from ...cocoeval import CocoEvaluation, CocoGroundTruth, evaluate, load_gt, save_results, to_results  # noqa: F401
from ...pb import GMAX, ObjectsAnnotation


def load_od(annotation_json, image_dir):
    doc = json.loads(pathlib.Path(annotation_json).read_text())
    cats = sorted(doc.get("categories", []), key=lambda c: int(c["id"]))
    cat_to_class = {int(c["id"]): i for i, c in enumerate(cats)}
    class_names = [str(c["name"]) for c in cats]
    objs = {}
    for a in doc.get("annotations", []):
        objs.setdefault(int(a["image_id"]), []).append(a)
    X, y = [], []
    for im in doc.get("images", []):
        w, h = float(im["width"]), float(im["height"])
        path = pathlib.Path(image_dir) / im["file_name"]
        anns = objs.get(int(im["id"]), [])
        if len(anns) > GMAX:
            raise ValueError(f"{path}: {len(anns)} objects, more than the {GMAX} per image the anchor assignment takes")
        classes, bboxes, crowd = [], [], []
        for a in anns:
            cid = int(a["category_id"])
            if cid not in cat_to_class:
                raise ValueError(f"{path}: category id {cid} is not among the JSON's categories")
            bx, by, bw, bh = (float(v) for v in a["bbox"])
            classes.append(cat_to_class[cid])
            bboxes.append([bx / w, by / h, (bx + bw) / w, (by + bh) / h])
            crowd.append(bool(a.get("iscrowd", 0)))
        X.append(path)
        y.append(ObjectsAnnotation(path, w, h, classes, bboxes, crowd))
    Xa = np.empty(len(X), dtype=object)
    Xa[:] = X
    ya = np.empty(len(y), dtype=object)
    ya[:] = y
    return Xa, ya, class_names
