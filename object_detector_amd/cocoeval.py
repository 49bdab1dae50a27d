"""COCO bbox evaluation (the twelve AP / AR statistics of pycocotools' COCOeval, default parameters) with the matching and
the accumulation on the GPU (csrc/cocoeval.hip).  Public entry points are re-exported by tk.data.coco.

The protocol, which the kernels and the numpy restatement in the tests both follow bit for bit in f64:

1. Scope: the GT JSON's image ids (or the `image_ids` subset) sorted ascending; the category ids sorted ascending, class i
   of the detector = the i-th smallest.  A GT's area is its `area` field (default w*h), iscrowd defaults to 0; a
   detection's area is w*h.
2. Groups (image, category) with a GT or a detection.  GTs keep file order; detections are stable-sorted by descending
   score (ties in input order) and cut to the first 100: the position is the detection's rank.
3. IoU = pycocotools' bbIou in f64 without contraction; u = da for a crowd GT, else (da + ga) - i, da / ga box areas.
4. Matching per group, IoU threshold t and area range a: a GT is ignored when crowd or its area lies outside a; the
   non-ignored GTs are visited first, then the ignored ones, each in file order.  Per detection in rank order: best =
   min(t, 1 - 1e-10); skip GTs matched before (unless crowd); stop at the first ignored GT once a non-ignored one is held;
   skip iou < best; else take it (an equal IoU replaces the earlier GT).  A matched detection is ignored when its GT is;
   an unmatched one when its area lies outside a.
5. Accumulation per category k, area range a, maxDet m, threshold t: npig = GTs of k not ignored under a (0: precision,
   recall and scores stay -1).  The sequence = detections of k with rank < maxDet, stable-sorted by descending score
   (ties: image position, then rank), ignored ones included.  tp / fp = running counts of non-ignored matched /
   unmatched detections; rc = tp / npig; pr = tp / ((fp + tp) + 2^-52), then its suffix maximum; recall = rc[-1] (0 for
   an empty sequence); i_r = searchsorted(rc, rec_thrs[r], 'left'); precision = pr[i_r], scores = score[i_r], 0 past
   the end.
6. Summary (numpy): the mean of the selected entries > -1, or -1.

Deliberate differences from pycocotools: a match is a boolean (a GT with id 0 counts as matched), and a missing `area` /
`iscrowd` gets a default instead of a KeyError.
"""
from __future__ import annotations

import ctypes as C
import json
import pathlib
from dataclasses import dataclass

import numpy as np

IOU_THRS = np.linspace(.5, 0.95, 10)
REC_THRS = np.linspace(.0, 1.00, 101)
MAX_DETS = (1, 10, 100)
AREA_NAMES = ("all", "small", "medium", "large")
AREA_RNG = np.array([[0, 1e5 ** 2], [0, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]], np.float64)
T, R, A, M = len(IOU_THRS), len(REC_THRS), len(AREA_RNG), len(MAX_DETS)


@dataclass
class CocoGroundTruth:
    """The raw values of a COCO instances JSON that evaluation needs.  Images are in JSON order (load_od's X order);
    annotations are flat arrays in file order."""
    image_ids: np.ndarray        # int64 [I], JSON order
    widths: np.ndarray           # float64 [I]
    heights: np.ndarray          # float64 [I]
    file_names: list
    category_ids: np.ndarray     # int64 [K], ascending (class i = category_ids[i])
    category_names: list
    ann_image_ids: np.ndarray    # int64 [N]
    ann_classes: np.ndarray      # int64 [N], index into category_ids
    ann_bboxes: np.ndarray       # float64 [N, 4], pixel xywh
    ann_areas: np.ndarray        # float64 [N]
    ann_crowd: np.ndarray        # bool [N]


def load_gt(annotation_json) -> CocoGroundTruth:
    doc = json.loads(pathlib.Path(annotation_json).read_text())
    cats = sorted(doc.get("categories", []), key=lambda c: int(c["id"]))
    cat_ids = np.array([int(c["id"]) for c in cats], np.int64)
    images = doc.get("images", [])
    image_ids = np.array([int(im["id"]) for im in images], np.int64)
    anns = doc.get("annotations", [])
    n = len(anns)
    a_img = np.array([int(a["image_id"]) for a in anns], np.int64)
    a_cat = np.array([int(a["category_id"]) for a in anns], np.int64)
    boxes = np.array([[float(v) for v in a["bbox"]] for a in anns], np.float64).reshape(n, 4)
    areas = np.array([float(a["area"]) if "area" in a else np.nan for a in anns], np.float64)
    no_area = np.isnan(areas)
    areas[no_area] = boxes[no_area, 2] * boxes[no_area, 3]
    crowd = np.array([bool(a.get("iscrowd", 0)) for a in anns], bool)
    bad_img = ~np.isin(a_img, image_ids)
    if bad_img.any():
        raise ValueError(f"annotation image id {int(a_img[bad_img][0])} is not among the JSON's images")
    cls = np.searchsorted(cat_ids, a_cat)
    bad_cat = (cls >= len(cat_ids)) | (cat_ids[np.minimum(cls, max(len(cat_ids) - 1, 0))] != a_cat) if len(cat_ids) \
        else np.ones(n, bool)
    if bad_cat.any():
        raise ValueError(f"annotation category id {int(a_cat[bad_cat][0])} is not among the JSON's categories")
    return CocoGroundTruth(
        image_ids=image_ids, widths=np.array([float(im["width"]) for im in images], np.float64),
        heights=np.array([float(im["height"]) for im in images], np.float64),
        file_names=[str(im.get("file_name", "")) for im in images], category_ids=cat_ids,
        category_names=[str(c["name"]) for c in cats], ann_image_ids=a_img, ann_classes=cls.astype(np.int64),
        ann_bboxes=boxes, ann_areas=areas, ann_crowd=crowd)


# ---- results ---------------------------------------------------------------------------------------------------------
@dataclass
class _Dets:
    image_ids: np.ndarray  # int64 [N]
    category_ids: np.ndarray  # int64 [N]
    bboxes: np.ndarray  # float64 [N, 4] pixel xywh
    scores: np.ndarray  # float64 [N]


def _dets_from_predictions(gt, y_pred, image_ids):
    ids = np.asarray(gt.image_ids if image_ids is None else image_ids, np.int64)
    y_pred = list(y_pred)
    if len(y_pred) != len(ids):
        raise ValueError(f"{len(y_pred)} predictions for {len(ids)} images")
    pos = {int(v): i for i, v in enumerate(gt.image_ids)}
    missing = [int(v) for v in ids if int(v) not in pos]
    if missing:
        raise ValueError(f"image id {missing[0]} is not among the ground truth's images")
    ip = np.array([pos[int(v)] for v in ids], np.int64)
    counts = np.array([len(p.classes) for p in y_pred], np.int64)
    if counts.sum() == 0:
        z = np.zeros(0, np.int64)
        return _Dets(z, z, np.zeros((0, 4)), np.zeros(0))
    cls = np.concatenate([np.asarray(p.classes, np.int64).reshape(-1) for p in y_pred])
    if cls.min() < 0 or cls.max() >= len(gt.category_ids):
        raise ValueError(f"class index outside 0..{len(gt.category_ids) - 1}")
    b = np.concatenate([np.asarray(p.bboxes, np.float32).reshape(-1, 4) for p in y_pred]).astype(np.float64)
    conf = np.concatenate([np.asarray(p.confs, np.float32).reshape(-1) for p in y_pred]).astype(np.float64)
    W = np.repeat(gt.widths[ip], counts)
    H = np.repeat(gt.heights[ip], counts)
    xywh = np.stack([b[:, 0] * W, b[:, 1] * H, (b[:, 2] - b[:, 0]) * W, (b[:, 3] - b[:, 1]) * H], 1)
    return _Dets(np.repeat(ids, counts), gt.category_ids[cls], xywh, conf)


def to_results(gt, y_pred, image_ids=None) -> list:
    """COCO result dicts of `y_pred` (ObjectsPrediction per image, aligned with image_ids, default gt.image_ids), in image
    order and prediction order within an image: bbox = [x1*W, y1*H, (x2-x1)*W, (y2-y1)*H] in f64 from the f32 corners,
    score = float(conf), category_id = gt.category_ids[class]."""
    d = _dets_from_predictions(gt, y_pred, image_ids)
    return [{"image_id": int(i), "category_id": int(c), "bbox": [float(v) for v in b], "score": float(s)}
            for i, c, b, s in zip(d.image_ids.tolist(), d.category_ids.tolist(), d.bboxes, d.scores.tolist())]


def save_results(path, results):
    pathlib.Path(path).write_text(json.dumps(results))


def _dets_from_dicts(results):
    n = len(results)
    return _Dets(np.array([int(r["image_id"]) for r in results], np.int64).reshape(n),
                 np.array([int(r["category_id"]) for r in results], np.int64).reshape(n),
                 np.array([[float(v) for v in r["bbox"]] for r in results], np.float64).reshape(n, 4),
                 np.array([float(r["score"]) for r in results], np.float64).reshape(n))


def _as_dets(gt, predictions, image_ids):
    if isinstance(predictions, (str, pathlib.Path)):
        return _dets_from_dicts(json.loads(pathlib.Path(predictions).read_text()))
    predictions = list(predictions)
    if not predictions or isinstance(predictions[0], dict):
        return _dets_from_dicts(predictions)
    return _dets_from_predictions(gt, predictions, image_ids)


# ---- host packing ----------------------------------------------------------------------------------------------------
@dataclass
class Packed:
    """Flat, sorted arrays the two kernels read (every order decided here, with numpy's stable sorts)."""
    K: int
    n_groups: int
    gt_off: np.ndarray     # int32 [G+1]
    det_off: np.ndarray    # int32 [G+1]
    gt_box: np.ndarray     # float64 [Ng, 4], grouped, file order within a group
    gt_area: np.ndarray    # float64 [Ng]
    gt_crowd: np.ndarray   # int32 [Ng]
    det_box: np.ndarray    # float64 [Nd, 4], grouped, rank order within a group
    det_out: np.ndarray    # int32 [Nd]: slot in accumulation order
    cat_off: np.ndarray    # int32 [K+1]
    acc_rank: np.ndarray   # int32 [Nd], accumulation order
    acc_score: np.ndarray  # float64 [Nd], accumulation order
    npig: np.ndarray       # int32 [K, A]


def pack(gt, dets, image_ids=None) -> Packed:
    K = len(gt.category_ids)
    if K == 0:
        raise ValueError("the ground truth declares no categories")
    scope = np.unique(np.asarray(gt.image_ids if image_ids is None else image_ids, np.int64))
    if not np.isin(scope, gt.image_ids).all():
        raise ValueError(f"image id {int(scope[~np.isin(scope, gt.image_ids)][0])} is not among the ground truth's images")
    if not (np.isfinite(dets.bboxes).all() and np.isfinite(dets.scores).all()):
        raise ValueError("non-finite box or score in the results")
    if not np.isin(dets.image_ids, gt.image_ids).all():
        bad = dets.image_ids[~np.isin(dets.image_ids, gt.image_ids)][0]
        raise ValueError(f"result image id {int(bad)} is not among the ground truth's images")
    # detections: in scope, known category
    dcls = np.searchsorted(gt.category_ids, dets.category_ids)
    known = (dcls < K) & (gt.category_ids[np.minimum(dcls, K - 1)] == dets.category_ids)
    keep = known & np.isin(dets.image_ids, scope)
    d_idx = np.flatnonzero(keep)
    d_pos = np.searchsorted(scope, dets.image_ids[d_idx])
    d_key = d_pos * K + dcls[d_idx]
    d_score = dets.scores[d_idx]
    # GTs in scope
    g_idx = np.flatnonzero(np.isin(gt.ann_image_ids, scope))
    g_key = np.searchsorted(scope, gt.ann_image_ids[g_idx]) * K + gt.ann_classes[g_idx]
    keys = np.unique(np.concatenate([g_key, d_key]))
    G = len(keys)
    g_grp = np.searchsorted(keys, g_key)
    d_grp = np.searchsorted(keys, d_key)
    # GTs: by group, file order within it
    go = np.argsort(g_grp, kind="stable")
    gt_off = np.zeros(G + 1, np.int64)
    np.cumsum(np.bincount(g_grp, minlength=G), out=gt_off[1:])
    # detections: by group, descending score, input order; rank = position in the group; keep rank < 100
    do = np.lexsort((np.arange(len(d_idx)), -d_score, d_grp))
    starts = np.zeros(G + 1, np.int64)
    np.cumsum(np.bincount(d_grp, minlength=G), out=starts[1:])
    rank = np.arange(len(do)) - starts[d_grp[do]]
    do, rank = do[rank < MAX_DETS[-1]], rank[rank < MAX_DETS[-1]]
    det_off = np.zeros(G + 1, np.int64)
    np.cumsum(np.bincount(d_grp[do], minlength=G), out=det_off[1:])
    # accumulation order: category, descending score, image position, rank
    cat = d_key[do] % K
    pos = d_key[do] // K
    sc = d_score[do]
    ao = np.lexsort((rank, pos, -sc, cat))
    det_out = np.empty(len(do), np.int64)
    det_out[ao] = np.arange(len(do))
    cat_off = np.zeros(K + 1, np.int64)
    np.cumsum(np.bincount(cat, minlength=K), out=cat_off[1:])
    # npig[k, a]: GTs of k not ignored under a
    ga, gc, gk = gt.ann_areas[g_idx], gt.ann_crowd[g_idx], gt.ann_classes[g_idx]
    npig = np.stack([np.bincount(gk[~gc & (ga >= lo) & (ga <= hi)], minlength=K) for lo, hi in AREA_RNG], 1)
    gsel = g_idx[go]
    return Packed(
        K=K, n_groups=G, gt_off=gt_off.astype(np.int32), det_off=det_off.astype(np.int32),
        gt_box=gt.ann_bboxes[gsel], gt_area=gt.ann_areas[gsel], gt_crowd=gt.ann_crowd[gsel].astype(np.int32),
        det_box=dets.bboxes[d_idx[do]], det_out=det_out.astype(np.int32), cat_off=cat_off.astype(np.int32),
        acc_rank=rank[ao].astype(np.int32), acc_score=sc[ao], npig=npig.astype(np.int32))


# ---- device ----------------------------------------------------------------------------------------------------------
def _align(v, a=256):
    return (v + a - 1) // a * a


def run_device(p: Packed, device=None, timings=None):
    """Upload `p` (one copy), launch od_coco_match and od_coco_accumulate, copy the results back (one copy) ->
    (precision [T,R,K,A,M], recall [T,K,A,M], scores [T,R,K,A,M]).  timings: a dict that receives the device time of
    each kernel in ms (hipEvents)."""
    import torch

    from . import _lib
    if not torch.cuda.is_available():
        raise _lib.OdError("COCO evaluation runs on the MI355X (no GPU visible); there is no CPU path")
    from .net import Context
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    ctx = Context.get(dev)
    lib = _lib.load()
    arrays = {"gt_off": p.gt_off, "det_off": p.det_off, "gt_box": p.gt_box, "gt_area": p.gt_area, "gt_crowd": p.gt_crowd,
              "det_box": p.det_box, "det_out": p.det_out, "cat_off": p.cat_off, "rank": p.acc_rank,
              "score": p.acc_score, "npig": p.npig, "iou_thrs": IOU_THRS, "area_rng": AREA_RNG, "rec_thrs": REC_THRS,
              "max_dets": np.array(MAX_DETS, np.int32)}
    off, total = {}, 0
    for k, a in arrays.items():
        off[k] = total
        total = _align(total + a.nbytes)
    host = np.zeros(max(total, 256), np.uint8)
    for k, a in arrays.items():
        host[off[k]:off[k] + a.nbytes] = np.ascontiguousarray(a).reshape(-1).view(np.uint8)
    nd, ng, K = len(p.det_out), len(p.gt_area), p.K
    n_prec, n_rec = T * R * K * A * M, T * K * A * M
    ws_bytes = int(lib.od_coco_match_workspace_bytes(ng))
    o_mt = 0
    o_ig = _align(o_mt + 8 * nd)
    o_prec = _align(o_ig + 8 * nd)
    o_rec = o_prec + 8 * n_prec
    o_sc = o_rec + 8 * n_rec
    o_ws = _align(o_sc + 8 * n_prec)
    with torch.cuda.device(dev):
        blob = torch.from_numpy(host).to(dev, non_blocking=False)
        work = torch.empty(max(o_ws + ws_bytes, 256), dtype=torch.uint8, device=dev)
        b, w = blob.data_ptr(), work.data_ptr()
        P = {k: C.c_void_p(b + o) for k, o in off.items()}
        st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)] if timings is not None else None
        if ev:
            ev[0].record()
        _lib.check(lib.od_coco_match(ctx.handle, P["gt_off"], P["det_off"], p.n_groups, P["gt_box"], P["gt_area"],
                                     P["gt_crowd"], ng, P["det_box"], P["det_out"], P["iou_thrs"], P["area_rng"],
                                     C.c_void_p(w + o_mt), C.c_void_p(w + o_ig), C.c_void_p(w + o_ws), ws_bytes, st),
                   "od_coco_match")
        if ev:
            ev[1].record()
        _lib.check(lib.od_coco_accumulate(ctx.handle, P["cat_off"], K, P["rank"], P["score"], C.c_void_p(w + o_mt),
                                          C.c_void_p(w + o_ig), P["npig"], P["rec_thrs"], P["max_dets"],
                                          C.c_void_p(w + o_prec), C.c_void_p(w + o_rec), C.c_void_p(w + o_sc), st),
                   "od_coco_accumulate")
        if ev:
            ev[2].record()
        out = work[o_prec:o_sc + 8 * n_prec].cpu().numpy().view(np.float64)
        if ev:
            timings["match_ms"] = ev[0].elapsed_time(ev[1])
            timings["accumulate_ms"] = ev[1].elapsed_time(ev[2])
    precision = out[:n_prec].reshape(T, R, K, A, M).copy()
    recall = out[n_prec:n_prec + n_rec].reshape(T, K, A, M).copy()
    scores = out[n_prec + n_rec:].reshape(T, R, K, A, M).copy()
    return precision, recall, scores


# ---- summary ---------------------------------------------------------------------------------------------------------
_STATS = ((1, None, "all", 100), (1, .5, "all", 100), (1, .75, "all", 100), (1, None, "small", 100),
          (1, None, "medium", 100), (1, None, "large", 100), (0, None, "all", 1), (0, None, "all", 10),
          (0, None, "all", 100), (0, None, "small", 100), (0, None, "medium", 100), (0, None, "large", 100))


def summarize(precision, recall):
    """-> (stats (12,), the 12 pycocotools summary lines)."""
    stats, lines = np.zeros(12), []
    for i, (ap, iou, area, md) in enumerate(_STATS):
        aind, mind = AREA_NAMES.index(area), MAX_DETS.index(md)
        s = precision[:, :, :, aind, mind] if ap else recall[:, :, aind, mind]
        if iou is not None:
            s = s[np.where(iou == IOU_THRS)[0]]
        stats[i] = -1 if len(s[s > -1]) == 0 else np.mean(s[s > -1])
        iou_str = f"{IOU_THRS[0]:0.2f}:{IOU_THRS[-1]:0.2f}" if iou is None else f"{iou:0.2f}"
        lines.append(" {:<18} {} @[ IoU={:<9} | area={:>6s} | maxDets={:>3d} ] = {:0.3f}".format(
            "Average Precision" if ap else "Average Recall", "(AP)" if ap else "(AR)", iou_str, area, md, stats[i]))
    return stats, lines


@dataclass
class CocoEvaluation:
    precision: np.ndarray  # [T, R, K, A, M]
    recall: np.ndarray     # [T, K, A, M]
    scores: np.ndarray     # [T, R, K, A, M]
    stats: np.ndarray      # (12,)
    category_ids: np.ndarray
    category_names: list

    def summary(self):
        return summarize(self.precision, self.recall)[1]

    def ap_per_class(self):
        """(K,) AP@[.50:.95] for area all and 100 detections; -1 for a class without GT."""
        s = self.precision[:, :, :, 0, M - 1]
        out = np.full(s.shape[2], -1.0)
        for k in range(s.shape[2]):
            v = s[:, :, k]
            if (v > -1).any():
                out[k] = np.mean(v[v > -1])
        return out


def evaluate(gt, predictions, image_ids=None, device=None, timings=None) -> CocoEvaluation:
    """COCO bbox evaluation of `predictions` against `gt` (a CocoGroundTruth).  predictions: a sequence of
    ObjectsPrediction aligned with image_ids (default gt.image_ids), a list of COCO result dicts, or the path of a results
    JSON -- the three give identical arrays.  image_ids restricts the evaluation to those images.  Runs on the GPU;
    raises _lib.OdError without one."""
    p = pack(gt, _as_dets(gt, predictions, image_ids), image_ids)
    precision, recall, scores = run_device(p, device, timings)
    stats, _ = summarize(precision, recall)
    return CocoEvaluation(precision, recall, scores, stats, gt.category_ids, list(gt.category_names))
