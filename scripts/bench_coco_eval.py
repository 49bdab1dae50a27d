#!/usr/bin/env python3
"""COCO bbox evaluation at COCO val2017 scale (5000 images, 80 categories, ~7 GTs and 100 detections per image), generated
from a seed: host packing, od_coco_match / od_coco_accumulate device time (hipEvents), end-to-end tk.data.coco.evaluate()
from ObjectsPrediction lists (median of 5 after a warm-up), and the numpy reference of the tests on a subset of the images
(checked bit-identical there).  Prints one JSON line."""
import argparse
import json
import pathlib
import statistics
import sys
import tempfile
import time

import numpy as np

import _common  # noqa: F401
import pytoolkit as tk
from object_detector_amd import cocoeval as CE
from object_detector_amd.detector import ObjectsPrediction

sys.path.insert(0, str(_common.ROOT / "tests"))
import cocoeval_ref as ref  # noqa: E402


def make_val2017_like(seed, n_images=5000, n_cats=80, gt_per_image=7.0, dets_per_image=100, crowd_frac=0.01):
    """-> (gt_doc, y_pred list[ObjectsPrediction]).  GT boxes span small / medium / large; detections are jittered copies
    of GTs (60 %, 85 % of them with the GT's class) plus random boxes; scores quantised to 1e-3 (ties)."""
    rng = np.random.default_rng(seed)
    ids = rng.choice(np.arange(1, 20 * n_images), n_images, replace=False)
    cat_ids = np.sort(rng.choice(np.arange(1, 91), n_cats, replace=False))
    p_cat = 1.0 / np.arange(1, n_cats + 1) ** 0.8
    p_cat /= p_cat.sum()
    images, anns, y = [], [], []

    def boxes(n, W, H):
        area = np.exp(rng.uniform(np.log(40.0), np.log(0.6 * W * H), n))
        ar = np.exp(rng.uniform(-1, 1, n))
        w = np.minimum(W - 1.0, np.sqrt(area * ar))
        h = np.minimum(H - 1.0, area / w)
        x, yy = rng.uniform(0, 1, n) * (W - w), rng.uniform(0, 1, n) * (H - h)
        return np.round(np.stack([x, yy, w, h], 1), 2)

    for iid in ids:
        W, H = int(rng.integers(200, 641)), int(rng.integers(200, 641))
        images.append(dict(id=int(iid), file_name=f"{int(iid):012d}.jpg", width=W, height=H))
        n = int(rng.poisson(gt_per_image))
        gb, gc = boxes(n, W, H), rng.choice(n_cats, n, p=p_cat)
        crowd = rng.uniform(0, 1, n) < crowd_frac
        for b, c, cr in zip(gb, gc, crowd):
            anns.append(dict(id=len(anns) + 1, image_id=int(iid), category_id=int(cat_ids[c]), bbox=b.tolist(),
                             area=float(round(b[2] * b[3] * 0.9, 3)), iscrowd=int(cr)))
        nj = int(round(0.6 * dets_per_image)) if n else 0
        src = rng.integers(0, max(n, 1), nj)
        jb = gb[src] + rng.normal(0, 0.08, (nj, 4)) * np.concatenate([gb[src, 2:], gb[src, 2:]], 1) if n else np.zeros((0, 4))
        jc = np.where(rng.uniform(0, 1, nj) < 0.85, gc[src] if n else 0, rng.integers(0, n_cats, nj))
        rb = boxes(dets_per_image - nj, W, H)
        db = np.concatenate([jb, rb])
        dc = np.concatenate([jc, rng.integers(0, n_cats, dets_per_image - nj)])
        xyxy = np.clip(np.stack([db[:, 0] / W, db[:, 1] / H, (db[:, 0] + db[:, 2]) / W, (db[:, 1] + db[:, 3]) / H], 1), 0, 1)
        score = np.round(rng.uniform(0.001, 1.0, dets_per_image), 3)
        y.append(ObjectsPrediction(dc, score.astype(np.float32), xyxy.astype(np.float32)))
    cats = [dict(id=int(c), name=f"category{int(c)}") for c in cat_ids]
    return dict(images=images, annotations=anns, categories=cats), y


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--seed", default=0, type=int)
    p.add_argument("--images", default=5000, type=int)
    p.add_argument("--ref-images", default=500, type=int, help="images of the subset the numpy reference evaluates")
    p.add_argument("--repeats", default=5, type=int)
    args = p.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_coco_eval.py measures the GPU kernels; no GPU is visible")
    doc, y = make_val2017_like(args.seed, args.images)
    with tempfile.TemporaryDirectory() as d:
        path = pathlib.Path(d) / "instances.json"
        path.write_text(json.dumps(doc))
        gt = tk.data.coco.load_gt(path)
    t0 = time.perf_counter()
    dets = CE._as_dets(gt, y, None)
    t1 = time.perf_counter()
    packed = CE.pack(gt, dets)
    t2 = time.perf_counter()
    timings = {}
    tk.data.coco.evaluate(gt, y, timings=timings)  # warm-up (code objects, allocator)
    walls = []
    for _ in range(args.repeats):
        torch.cuda.synchronize()
        s = time.perf_counter()
        ev = tk.data.coco.evaluate(gt, y, timings=timings)
        walls.append((time.perf_counter() - s) * 1e3)
    dev = [dict(timings)]
    for _ in range(2):
        CE.run_device(packed, timings=timings)
        dev.append(dict(timings))
    # the reference on the first --ref-images images (sorted id order), and the device on the same subset
    sub = sorted(int(v) for v in gt.image_ids)[:args.ref_images]
    pos = {int(v): i for i, v in enumerate(gt.image_ids)}
    y_sub = [y[pos[i]] for i in sub]
    res_sub = tk.data.coco.to_results(gt, y_sub, image_ids=sub)
    s = time.perf_counter()
    r = ref.evaluate(doc, res_sub, image_ids=sub)
    ref_s = time.perf_counter() - s
    ev_sub = tk.data.coco.evaluate(gt, y_sub, image_ids=sub)
    same = all(np.array_equal(getattr(ev_sub, k), r[k]) for k in ("precision", "recall", "scores", "stats"))
    print(json.dumps({
        "bench": "coco_eval", "images": len(gt.image_ids), "categories": len(gt.category_ids),
        "gts": int(len(gt.ann_areas)), "dets": int(len(dets.scores)), "groups": int(packed.n_groups),
        "dets_kept": int(len(packed.det_out)), "max_category_dets": int(np.diff(packed.cat_off).max()),
        "results_to_arrays_ms": round((t1 - t0) * 1e3, 2), "pack_ms": round((t2 - t1) * 1e3, 2),
        "match_ms": round(statistics.median(d["match_ms"] for d in dev), 3),
        "accumulate_ms": round(statistics.median(d["accumulate_ms"] for d in dev), 3),
        "evaluate_ms_median": round(statistics.median(walls), 2), "evaluate_ms": [round(v, 2) for v in walls],
        "stats": [round(float(v), 6) for v in ev.stats],
        "ref_images": len(sub), "ref_s": round(ref_s, 2), "ref_bit_identical": bool(same)}))


if __name__ == "__main__":
    main()
