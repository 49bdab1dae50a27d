"""Plain numpy / Python restatement of the COCO bbox protocol of object_detector_amd/cocoeval.py (pycocotools' COCOeval
with default parameters; the two stated differences included), one loop per group as the rules read.  It is the oracle
of the GPU tests and never imported by the product package.  Also: a seeded problem generator with the protocol's edge
cases (tests, scripts/bench_coco_eval.py)."""
from __future__ import annotations

import math

import numpy as np

IOU_THRS = np.linspace(.5, 0.95, 10)
REC_THRS = np.linspace(.0, 1.00, 101)
MAX_DETS = [1, 10, 100]
AREA_RNG = [[0 ** 2, 1e5 ** 2], [0 ** 2, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]]
AREA_LBL = ["all", "small", "medium", "large"]


def bb_iou(d, g, crowd):
    """pycocotools maskApi.c bbIou for one pair, in Python floats (f64, no contraction)."""
    da = d[2] * d[3]
    ga = g[2] * g[3]
    w = min(d[0] + d[2], g[0] + g[2]) - max(d[0], g[0])
    if w <= 0:
        return 0.0
    h = min(d[1] + d[3], g[1] + g[3]) - max(d[1], g[1])
    if h <= 0:
        return 0.0
    i = w * h
    u = da if crowd else (da + ga) - i
    return i / u


def evaluate(gt_doc, results, image_ids=None):
    """-> dict(precision [T,R,K,A,M], recall [T,K,A,M], scores [T,R,K,A,M], stats (12,), lines)."""
    all_imgs = {int(im["id"]) for im in gt_doc["images"]}
    scope = sorted(all_imgs if image_ids is None else {int(i) for i in image_ids})
    assert set(scope) <= all_imgs
    in_scope = set(scope)
    cat_ids = sorted(int(c["id"]) for c in gt_doc["categories"])
    K, T, R, A, M = len(cat_ids), len(IOU_THRS), len(REC_THRS), len(AREA_RNG), len(MAX_DETS)
    gts, dts = {}, {}
    for a in gt_doc["annotations"]:
        if int(a["image_id"]) not in all_imgs or int(a["category_id"]) not in cat_ids:
            raise ValueError("annotation of an undeclared image or category")
        bb = [float(v) for v in a["bbox"]]
        g = dict(bbox=bb, area=float(a["area"]) if "area" in a else bb[2] * bb[3], crowd=bool(a.get("iscrowd", 0)))
        gts.setdefault((int(a["image_id"]), int(a["category_id"])), []).append(g)
    for r in results:
        bb = [float(v) for v in r["bbox"]]
        if not all(math.isfinite(v) for v in bb + [float(r["score"])]):
            raise ValueError("non-finite result")
        if int(r["image_id"]) not in all_imgs:
            raise ValueError("result for an image outside the ground truth")
        if int(r["image_id"]) not in in_scope or int(r["category_id"]) not in cat_ids:
            continue
        dts.setdefault((int(r["image_id"]), int(r["category_id"])), []).append(
            dict(bbox=bb, area=bb[2] * bb[3], score=float(r["score"])))

    # evaluateImg: per (category, area range) the list over images in sorted-id order (None = no GT and no detection)
    E = {}
    for k, cid in enumerate(cat_ids):
        for img in scope:
            gt = gts.get((img, cid), [])
            dt = dts.get((img, cid), [])
            if not gt and not dt:
                for a in range(A):
                    E.setdefault((k, a), []).append(None)
                continue
            order = np.argsort([-d["score"] for d in dt], kind="mergesort")
            dt = [dt[i] for i in order[:MAX_DETS[-1]]]
            ious = [[bb_iou(d["bbox"], g["bbox"], g["crowd"]) for g in gt] for d in dt]
            for a, (lo, hi) in enumerate(AREA_RNG):
                g_ig = [1 if (g["crowd"] or g["area"] < lo or g["area"] > hi) else 0 for g in gt]
                gind = np.argsort(g_ig, kind="mergesort")  # non-ignored first, file order within each
                gtm = np.zeros((T, len(gt)), bool)
                dtm = np.zeros((T, len(dt)), bool)
                dt_ig = np.zeros((T, len(dt)), bool)
                if gt and dt:
                    for t, thr in enumerate(IOU_THRS):
                        for di in range(len(dt)):
                            best = min([thr, 1 - 1e-10])
                            m = -1
                            for gi in gind:
                                if gtm[t, gi] and not gt[gi]["crowd"]:
                                    continue
                                if m > -1 and g_ig[m] == 0 and g_ig[gi] == 1:
                                    break
                                if ious[di][gi] < best:
                                    continue
                                best = ious[di][gi]
                                m = gi
                            if m == -1:
                                continue
                            dt_ig[t, di] = g_ig[m]
                            dtm[t, di] = True
                            gtm[t, m] = True
                out = np.array([d["area"] < lo or d["area"] > hi for d in dt], bool).reshape(1, len(dt))
                dt_ig = np.logical_or(dt_ig, np.logical_and(~dtm, out))
                E.setdefault((k, a), []).append(dict(scores=np.array([d["score"] for d in dt]), dtm=dtm, dt_ig=dt_ig,
                                                     g_ig=np.array(g_ig, int)))

    # accumulate
    precision = -np.ones((T, R, K, A, M))
    recall = -np.ones((T, K, A, M))
    scores = -np.ones((T, R, K, A, M))
    for k in range(K):
        for a in range(A):
            Es = [e for e in E[(k, a)] if e is not None]
            if not Es:
                continue
            for m, max_det in enumerate(MAX_DETS):
                dt_scores = np.concatenate([e["scores"][:max_det] for e in Es])
                inds = np.argsort(-dt_scores, kind="mergesort")
                dt_scores_sorted = dt_scores[inds]
                dtm = np.concatenate([e["dtm"][:, :max_det] for e in Es], axis=1)[:, inds]
                dt_ig = np.concatenate([e["dt_ig"][:, :max_det] for e in Es], axis=1)[:, inds]
                g_ig = np.concatenate([e["g_ig"] for e in Es])
                npig = np.count_nonzero(g_ig == 0)
                if npig == 0:
                    continue
                tps = np.logical_and(dtm, np.logical_not(dt_ig))
                fps = np.logical_and(np.logical_not(dtm), np.logical_not(dt_ig))
                tp_sum = np.cumsum(tps, axis=1).astype(dtype=float)
                fp_sum = np.cumsum(fps, axis=1).astype(dtype=float)
                for t, (tp, fp) in enumerate(zip(tp_sum, fp_sum)):
                    tp, fp = np.array(tp), np.array(fp)
                    nd = len(tp)
                    rc = tp / npig
                    pr = tp / (fp + tp + np.spacing(1))
                    q = np.zeros((R,))
                    ss = np.zeros((R,))
                    recall[t, k, a, m] = rc[-1] if nd else 0
                    pr = np.maximum.accumulate(pr[::-1])[::-1] if nd else pr
                    ri = np.searchsorted(rc, REC_THRS, side="left")
                    for r, pi in enumerate(ri):
                        if pi >= nd:
                            break
                        q[r] = pr[pi]
                        ss[r] = dt_scores_sorted[pi]
                    precision[t, :, k, a, m] = q
                    scores[t, :, k, a, m] = ss
    stats, lines = summarize(precision, recall)
    return dict(precision=precision, recall=recall, scores=scores, stats=stats, lines=lines)


def summarize(precision, recall):
    def one(ap=1, iou_thr=None, area="all", max_dets=100):
        i_str = " {:<18} {} @[ IoU={:<9} | area={:>6s} | maxDets={:>3d} ] = {:0.3f}"
        title = "Average Precision" if ap == 1 else "Average Recall"
        typ = "(AP)" if ap == 1 else "(AR)"
        iou = f"{IOU_THRS[0]:0.2f}:{IOU_THRS[-1]:0.2f}" if iou_thr is None else f"{iou_thr:0.2f}"
        aind = [i for i, a in enumerate(AREA_LBL) if a == area]
        mind = [i for i, m in enumerate(MAX_DETS) if m == max_dets]
        if ap == 1:
            s = precision
            if iou_thr is not None:
                s = s[np.where(iou_thr == IOU_THRS)[0]]
            s = s[:, :, :, aind, mind]
        else:
            s = recall
            if iou_thr is not None:
                s = s[np.where(iou_thr == IOU_THRS)[0]]
            s = s[:, :, aind, mind]
        mean_s = -1 if len(s[s > -1]) == 0 else np.mean(s[s > -1])
        return mean_s, i_str.format(title, typ, iou, area, max_dets, mean_s)

    spec = [(1, None, "all", 100), (1, .5, "all", 100), (1, .75, "all", 100), (1, None, "small", 100),
            (1, None, "medium", 100), (1, None, "large", 100), (0, None, "all", 1), (0, None, "all", 10),
            (0, None, "all", 100), (0, None, "small", 100), (0, None, "medium", 100), (0, None, "large", 100)]
    out = [one(*s) for s in spec]
    return np.array([o[0] for o in out]), [o[1] for o in out]


# ---- generated problems ----------------------------------------------------------------------------------------------
def make_problem(seed, n_images=120, n_cats=10, gt_per_image=7.0, dets_per_image=40, crowd_frac=0.03, edge_cases=True,
                 big_category_dets=0):
    """-> (gt_doc, results): COCO instances dict and result dicts.  Scores are quantised to 1e-3 (ties within and across
    images).  edge_cases adds: categories without GT, empty images, GT-only and detection-only groups, areas exactly 32^2
    and 96^2, an IoU exactly at a threshold, zero-width boxes, unknown category ids, a group with more than 100
    detections, one with 300 GTs, annotations without `area` / `iscrowd`.  big_category_dets: that many extra detections
    of the first category spread over the images (multi-chunk accumulation)."""
    rng = np.random.default_rng(seed)
    ids = rng.choice(np.arange(1, 50 * n_images), n_images, replace=False)  # JSON order != sorted order
    cat_ids = np.sort(rng.choice(np.arange(1, 10 * n_cats + 10), n_cats, replace=False))
    images = []
    for i in ids:
        images.append(dict(id=int(i), file_name=f"{int(i):08d}.jpg", width=int(rng.integers(200, 641)),
                           height=int(rng.integers(200, 641))))
    cats = [dict(id=int(c), name=f"c{int(c)}") for c in rng.permutation(cat_ids)]
    with_gt = cat_ids[:-2] if edge_cases else cat_ids  # the last two categories never get a GT
    p_cat = 1.0 / np.arange(1, len(with_gt) + 1)
    p_cat /= p_cat.sum()
    anns, results = [], []

    def box(W, H):
        area = np.exp(rng.uniform(np.log(40.0), np.log(0.6 * W * H)))  # small, medium and large
        ar = np.exp(rng.uniform(-1, 1))
        w = min(W - 1.0, np.sqrt(area * ar))
        h = min(H - 1.0, area / w)
        x, y = rng.uniform(0, W - w), rng.uniform(0, H - h)
        return [round(float(x), 2), round(float(y), 2), round(float(w), 2), round(float(h), 2)]

    empty = set(int(v) for v in ids[:3]) if edge_cases else set()
    for im in images:
        if im["id"] in empty:
            continue
        W, H = im["width"], im["height"]
        n = int(rng.poisson(gt_per_image))
        mine = []
        for _ in range(n):
            c = int(rng.choice(with_gt, p=p_cat))
            b = box(W, H)
            a = dict(id=len(anns) + 1, image_id=im["id"], category_id=c, bbox=b, area=round(b[2] * b[3] * 0.9, 3),
                     iscrowd=int(rng.uniform() < crowd_frac))
            if edge_cases and rng.uniform() < 0.05:
                del a["area"]
            if edge_cases and rng.uniform() < 0.05:
                del a["iscrowd"]
            anns.append(a)
            mine.append(a)
        nd = int(rng.integers(dets_per_image // 2, dets_per_image + 1))
        for _ in range(nd):
            if mine and rng.uniform() < 0.6:
                g = mine[int(rng.integers(len(mine)))]
                j = rng.normal(0, 0.08, 4) * np.array([g["bbox"][2], g["bbox"][3]] * 2)
                b = [g["bbox"][0] + j[0], g["bbox"][1] + j[1], max(0.0, g["bbox"][2] + j[2]), max(0.0, g["bbox"][3] + j[3])]
                c = g["category_id"] if rng.uniform() < 0.85 else int(rng.choice(cat_ids))
            else:
                b, c = box(W, H), int(rng.choice(cat_ids))
            results.append(dict(image_id=im["id"], category_id=c, bbox=[float(v) for v in b],
                                score=round(float(rng.uniform(0.001, 1.0)), 3)))
    if edge_cases:
        im0, im1, im2 = images[3]["id"], images[4]["id"], images[5]["id"]
        c0, c1 = int(with_gt[0]), int(with_gt[1])

        def gt(img, c, b, **kw):
            anns.append(dict(id=len(anns) + 1, image_id=img, category_id=c, bbox=b, **kw))

        def det(img, c, b, s):
            results.append(dict(image_id=img, category_id=c, bbox=b, score=s))
        # IoU exactly 0.5 against [0,0,10,10]; areas exactly at 32^2 and 96^2 (field and box); zero-width boxes
        gt(im0, c0, [0, 0, 10, 10], area=100.0, iscrowd=0)
        det(im0, c0, [0, 0, 10, 5], 0.5)
        gt(im0, c0, [100, 100, 32, 32], area=1024.0, iscrowd=0)
        det(im0, c0, [100, 100, 32, 32], 0.5)
        gt(im0, c0, [50, 20, 96, 96], iscrowd=0)
        det(im0, c0, [52, 20, 94, 96], 0.7)
        gt(im0, c0, [10, 150, 0, 20], iscrowd=0)
        det(im0, c0, [10, 150, 0, 20], 0.9)
        det(im0, c0, [12, 20, 0, 0], 0.4)
        # crowd GT swallowing several detections
        gt(im1, c1, [0, 0, 150, 150], area=20000.0, iscrowd=1)
        for s in (0.3, 0.3, 0.2):
            det(im1, c1, [10, 10, 20, 20], s)
        # unknown category ids
        det(im1, int(cat_ids.max()) + 7, [0, 0, 10, 10], 0.99)
        # a group with more than 100 detections
        for _ in range(130):
            det(im2, c1, box(images[5]["width"], images[5]["height"]), round(float(rng.uniform(0, 1)), 3))
        # a group with 300 GTs (small boxes on a grid) and 100+ detections on them
        im3 = images[6]
        for r in range(15):
            for q in range(20):
                gt(im3["id"], c0, [q * 10.0, r * 10.0, 8.0, 8.0], iscrowd=0)
        for _ in range(120):
            q, r = int(rng.integers(20)), int(rng.integers(15))
            det(im3["id"], c0, [q * 10.0 + rng.uniform(-2, 2), r * 10.0 + rng.uniform(-2, 2), 8.0, 8.0],
                round(float(rng.uniform(0, 1)), 3))
    for _ in range(big_category_dets):
        im = images[int(rng.integers(len(images)))]
        results.append(dict(image_id=im["id"], category_id=int(cat_ids[0]), bbox=box(im["width"], im["height"]),
                            score=round(float(rng.uniform(0, 1)), 3)))
    return dict(images=images, annotations=anns, categories=cats), results
