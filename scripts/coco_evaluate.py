#!/usr/bin/env python3
"""COCO bbox evaluation of the detector on a COCO-format dataset (instances JSON + image directory): the twelve
AP / AR statistics of pycocotools' COCOeval and a per-class AP table, computed by tk.data.coco.evaluate on the GPU.
--results-json evaluates an existing results file without a detector."""
import argparse
import pathlib

import numpy as np

import _common  # noqa: F401
import pytoolkit as tk


def _main():
    tk.better_exceptions()
    p = argparse.ArgumentParser()
    p.add_argument("--coco-json", required=True, type=pathlib.Path, help="COCO instances JSON (the ground truth)")
    p.add_argument("--coco-image-dir", default=None, type=pathlib.Path)
    p.add_argument("--weights", default=None, type=pathlib.Path)
    p.add_argument("--input-size", default=(320, 320), type=int, nargs=2)
    p.add_argument("--batch-size", default=16, type=int)
    p.add_argument("--precision", default=None, choices=("f16", "mixed"),
                   help="mixed = every logit within 1e-3 x scale of an fp32 run (ObjectDetector(precision=...)); default f16")
    p.add_argument("--device-decode", action="store_true",
                   help="decode JPEGs and resize every input on the GPU (ObjectDetector(image_decode='device'))")
    _common.add_tta_arguments(p)
    _common.add_nms_arguments(p)
    _common.add_slice_arguments(p)
    p.add_argument("--conf-threshold", default=None, type=float,
                   help="detections below this confidence are dropped (default: the detector's DEFAULT_CONF_THRESHOLD)")
    p.add_argument("--limit", default=0, type=int, help="evaluate the first N images of the JSON only")
    p.add_argument("--save-results", default=None, type=pathlib.Path, help="write the detections as a COCO results JSON")
    p.add_argument("--results-json", default=None, type=pathlib.Path,
                   help="evaluate this COCO results JSON instead of running the detector")
    p.set_defaults(synthetic=0)
    args = p.parse_args()
    with tk.dl.session():
        tk.log.init()
        _run(args)


@tk.log.trace()
def _run(args):
    from object_detector_amd import detector, weights
    log = tk.log.get(__name__)
    gt = tk.data.coco.load_gt(args.coco_json)
    image_ids = list(gt.image_ids[:args.limit]) if args.limit else None
    if args.results_json is not None:
        predictions = args.results_json
    else:
        if args.coco_image_dir is None or args.weights is None:
            raise SystemExit("--coco-image-dir and --weights are needed unless --results-json is given")
        params, meta = weights.load(args.weights)
        nc = weights.infer_arch(params)[0]
        if nc != len(gt.category_ids):
            raise SystemExit(f"{args.weights}: {nc} classes, but {args.coco_json} has {len(gt.category_ids)} categories")
        if "class_names" in meta and [str(v) for v in meta["class_names"]] != gt.category_names:
            raise SystemExit(f"{args.weights}: its class names differ from the category names of {args.coco_json}")
        X, _, _ = tk.data.coco.load_od(args.coco_json, args.coco_image_dir)
        if args.limit:
            X = X[:args.limit]
        od = _common.make_detector(tk, args, args.batch_size, tuple(args.input_size), keep_aspect=False,
                                   strict_nms=False, use_multi_gpu=True, precision=args.precision,
                                   device_decode=args.device_decode)
        conf = detector.DEFAULT_CONF_THRESHOLD if args.conf_threshold is None else args.conf_threshold
        predictions = od.predict(X, conf_threshold=conf)
    if not tk.dl.is_main_process():
        return
    if args.save_results is not None and args.results_json is None:
        tk.data.coco.save_results(args.save_results, tk.data.coco.to_results(gt, predictions, image_ids))
    ev = tk.data.coco.evaluate(gt, predictions, image_ids=image_ids)
    for line in ev.summary():
        log.info(line)
    ap = ev.ap_per_class()
    w = max(len(n) for n in gt.category_names)
    log.info(f"{'category':<{w}}     id  AP@[.50:.95]")
    for cid, name, v in zip(gt.category_ids, gt.category_names, ap):
        log.info(f"{name:<{w}} {int(cid):>6}  {'-' if v < 0 else f'{v:.3f}':>12}")
    log.info(f"mean over {int(np.sum(ap > -1))} categories with GT: {ev.stats[0]:.3f}")


if __name__ == "__main__":
    _main()
