"""Numpy restatement of sliced inference (DESIGN.md "Sliced inference"): the tile pixels of od_tiles_resize and the merge of
od_slice_merge, one image at a time, as plain loops in np.float32 (one rounding per operation, no contraction).  The merged
order, the NMS and the box voting are tta_ref's; the geometry is object_detector_amd.slicing's (the single definition).

A tile list is a dict: keys u64 [K] (sorted descending, the first `count` valid), count, boxes f32 [P,4] in tile coordinates.
"""
from __future__ import annotations

import numpy as np

import tta_ref
from object_detector_amd import resample, slicing

F = np.float32
LOW = np.uint64(0xFFFFFFFF)


def tile_pixels(img, rects, size_wh):
    """uint8 [h,w,3], rects int [T,4] -> uint8 [T,H,W,3]: resample.resize of every crop (= PIL crop + resize(BILINEAR))."""
    return np.stack([resample.resize(img[y0:y1, x0:x1], size_wh) for x0, y0, x1, y1 in np.asarray(rects).tolist()])


def cut_at_seam(box, edge, edge_lo, edge_hi):
    """The interior-edge rule on a tile-normalised box; edge_lo < 0 disables it."""
    if not F(edge_lo) >= 0:
        return False
    lo, hi = F(edge_lo), F(edge_hi)
    return bool((edge & slicing.LEFT and box[0] <= lo) or (edge & slicing.TOP and box[1] <= lo) or
                (edge & slicing.RIGHT and box[2] >= hi) or (edge & slicing.BOTTOM and box[3] >= hi))


def to_image(box, aff):
    """(x1, y1, x2, y2) in tile coordinates -> image coordinates: min(max(o + s * v, 0), 1), multiply and add rounded separately."""
    ox, oy, sx, sy = (F(v) for v in aff)
    out = []
    for v, o, s in ((box[0], ox, sx), (box[1], oy, sy), (box[2], ox, sx), (box[3], oy, sy)):
        out.append(min(max(F(o + F(s * F(v))), F(0)), F(1)))
    return np.array(out, F)


def candidates(tiles, NC, edges, aff, edge_lo, edge_hi):
    """Steps 1-2: the surviving candidates as (conf_bits, tile, flat, cls, box in image coordinates), in tile / list order,
    and the number the rule dropped."""
    out, dropped = [], 0
    for t, tl in enumerate(tiles):
        n = int(tl["count"])
        keys = np.asarray(tl["keys"][:n], np.uint64)
        bits = (keys >> np.uint64(32)).astype(np.int64)
        flat = (LOW - (keys & LOW)).astype(np.int64)
        p, c = flat // NC, flat % NC
        boxes = np.asarray(tl["boxes"], F)[p].reshape(n, 4)
        # the same two steps on whole columns: numpy float32 arrays round every multiply and every add on its own
        o = np.asarray(aff[t], F)[[0, 1, 0, 1]]
        s = np.asarray(aff[t], F)[[2, 3, 2, 3]]
        mapped = np.minimum(np.maximum(o + s * boxes, F(0)), F(1)).astype(F)
        for r in range(n):
            if cut_at_seam(boxes[r], int(edges[t]), edge_lo, edge_hi):
                dropped += 1
                continue
            out.append((int(bits[r]), t, int(flat[r]), int(c[r]), mapped[r]))
    return out, dropped


def merge_image(tiles, NC, K, edges, aff, edge_lo, edge_hi, iou_threshold=0.45, strict=False, max_det=200, vote_iou=0.5,
                cands=None):
    """-> dict(src i32 [n,2] (tile, flat), cls i32 [n], conf_bits u32 [n], boxes f32 [n,4], dropped, merged) of one image.
    cands: candidates(...) of the same arguments, when the caller already has them."""
    cands, dropped = cands if cands is not None else candidates(tiles, NC, edges, aff, edge_lo, edge_hi)
    merged = tta_ref.merged_order(cands, K)
    keep = tta_ref.nms(merged, iou_threshold, strict, max_det)
    table = tta_ref._table(merged)
    n = len(keep)
    return {
        "src": np.array([[merged[i][1], merged[i][2]] for i in keep], np.int32).reshape(n, 2),
        "cls": np.array([merged[i][3] for i in keep], np.int32),
        "conf_bits": np.array([merged[i][0] for i in keep], np.uint32),
        "boxes": np.array([tta_ref.vote(merged, i, vote_iou, table) for i in keep], F).reshape(n, 4),
        "dropped": dropped,
        "merged": len(merged),
    }


# ---- generated cases (shared by tests/test_slicing_host.py, which checks the conditions on the reference, and
#      tests/test_gpu_slice_merge.py, which runs the device on the same arrays) ------------------------------------------------
def make_row(rng, K, P, NC, n, quantise):
    """Generated candidates of one batch row in the style of test_gpu_tta._make_view: keys u64 [K] sorted descending (unused
    slots 0) and clustered boxes [P,4]; centres over (0.02, 0.98), so that clipped boxes reach the tile's sides."""
    centers = rng.uniform(0.02, 0.98, (24, 2))
    which = rng.integers(0, 24, P)
    c = centers[which] + rng.normal(0, 0.012, (P, 2))
    wh = rng.uniform(0.08, 0.3, (24, 2))[which] * rng.uniform(0.9, 1.1, (P, 2))
    boxes = np.clip(np.concatenate([c - wh / 2, c + wh / 2], 1), 0, 1).astype(F)
    pri = rng.choice(P, min(P, 400), replace=False)
    flat = rng.choice(len(pri) * 3, n, replace=False)
    flat = pri[flat // 3].astype(np.int64) * NC + (flat % 3) * 5
    conf = rng.uniform(0.011, 1.0, n).astype(F)
    if quantise:  # confidences on a coarse grid: ties inside a list and across tiles
        conf = (np.ceil(conf * 32) / 32).astype(F)
    k = (conf.view(np.uint32).astype(np.uint64) << np.uint64(32)) | (LOW - flat.astype(np.uint64))
    keys = np.zeros(K, np.uint64)
    keys[:n] = np.sort(k)[::-1]
    return keys, boxes


SCENARIOS = {  # name: (G, grid arguments (ny, nx, full view), K, how the lists are filled)
    "t1": (1, (1, 1, False), 1024, "full"),
    "g2_t5": (2, (2, 2, True), 1024, "rand"),
    "t16_full": (1, (3, 5, True), 1024, "full"),
    "t10_ties": (1, (3, 3, True), 1024, "ties"),
    "tile_emptied_by_rule": (1, (2, 2, True), 1024, "emptied"),
    "one_empty_tile": (1, (2, 2, True), 1024, "one_empty"),
    "all_empty": (2, (2, 2, True), 1024, "empty"),
    "rule_disabled": (1, (2, 2, True), 1024, "disabled"),
    "g6_t5_k256": (6, (2, 2, True), 256, "rand"),
}


def scenario(name):
    """-> dict of the arrays od_slice_merge takes for scenario `name` (numpy), with the SliceGrid and the image sizes."""
    import lattice_ref as L
    G, (ny, nx, full), K, how = SCENARIOS[name]
    rng = np.random.default_rng(L.seed_of("slice_merge", name))
    NC, P = 20, 4200
    grid = slicing.SliceGrid(ny, nx, 0.2, full, -1.0 if how == "disabled" else 0.01)
    T = grid.T
    keys = np.zeros((G * T, K), np.uint64)
    counts = np.zeros(G * T, np.int32)
    boxes = np.zeros((G * T, P, 4), F)
    tiles = np.zeros((G * T, 4), F)
    edge = np.zeros(G * T, np.int32)
    sizes = [(640 + 37 * g, 480 + 11 * g) for g in range(G)]
    for g, (w, h) in enumerate(sizes):
        r = grid.rects(w, h)
        tiles[g * T:(g + 1) * T] = slicing.affine(r, w, h)
        edge[g * T:(g + 1) * T] = slicing.edges(r, w, h)
        for t in range(T):
            row = g * T + t
            n = {"full": K, "empty": 0, "ties": K - 7 * t}.get(how, int(rng.integers(1, K + 1)))
            if how == "one_empty" and t == 2:
                n = 0
            if how == "rand" and t == 0:
                n = K // 2 + g
            counts[row] = n
            keys[row], boxes[row] = make_row(rng, K, P, NC, n, quantise=(how == "ties" or t % 2 == 0))
            if how == "emptied" and t == 1:  # the top-right tile: its left side is interior, and every box starts on it
                assert edge[row] & slicing.LEFT
                boxes[row, :, 0] = 0
    lo, hi = grid.edge_lo_hi
    return {"G": G, "T": T, "K": K, "NC": NC, "P": P, "keys": keys, "counts": counts, "boxes": boxes, "tiles": tiles,
            "edges": edge, "edge_lo": lo, "edge_hi": hi, "grid": grid, "sizes": sizes}


def image_lists(sc, g):
    """The tile lists, edges and affine rows of image g of a scenario, as merge_image takes them."""
    T = sc["T"]
    rows = range(g * T, (g + 1) * T)
    lists = [{"keys": sc["keys"][r], "count": int(sc["counts"][r]), "boxes": sc["boxes"][r]} for r in rows]
    return lists, sc["edges"][g * T:(g + 1) * T], sc["tiles"][g * T:(g + 1) * T]
