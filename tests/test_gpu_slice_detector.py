"""GPU: ObjectDetector(slices=...) end to end -- the network input of predict() against the reference tiles, the candidates
against the plain detector's on those rows, the record block against tests/slice_ref.py on the device's own candidates, the
host and the device image route against each other.  Bit for bit; nothing here has a tolerance."""
import numpy as np
import pytest
import torch

import slice_ref
from object_detector_amd import slicing

pytestmark = pytest.mark.gpu

F = np.float32
THR = 0.01
_REFS = {}  # candidates of one image (bytes) -> slice_ref.merge_image of them


def _images(sizes_wh, seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for w, h in sizes_wh]


def _check_pipeline(od, p, imgs, what):
    """One pipeline after a sliced batch of `imgs`: input rows, record block, sources.  -> (tiles kept from, predictions)"""
    grid, slc, post = od.slices, p.slc, p.post
    T, H, W = grid.T, od.input_size[0], od.input_size[1]
    n = len(imgs)
    x = p.net.input.cpu().numpy()
    want = np.concatenate([slice_ref.tile_pixels(im, grid.rects(im.shape[1], im.shape[0]), (W, H)) for im in imgs])
    assert np.array_equal(x[:n * T], want), f"{what}: network input rows differ from the reference tiles"
    assert not x[slc.G * T:].any(), f"{what}: the unused rows are not zero"
    keys = slc.keys.cpu().numpy().view(np.uint64)
    counts, boxes = slc.counts.cpu().numpy(), slc.boxes.cpu().numpy()
    det, src, kc = slc.det.cpu().numpy(), slc.src.cpu().numpy(), slc.keep_count.cpu().numpy()
    lo, hi = grid.edge_lo_hi
    tiles_seen, preds = [], []
    for g, im in enumerate(imgs):
        h, w = im.shape[:2]
        r = grid.rects(w, h)
        rows = range(g * T, (g + 1) * T)
        assert np.array_equal(slc.tiles.cpu().numpy()[g * T:(g + 1) * T].view(np.uint32), slicing.affine(r, w, h).view(np.uint32))
        assert np.array_equal(slc.edges.cpu().numpy()[g * T:(g + 1) * T], slicing.edges(r, w, h))
        lists = [{"keys": keys[q], "count": int(counts[q]), "boxes": boxes[q]} for q in rows]
        # the reference of one set of candidates is computed once: the two image routes give the same network input
        ck = (w, h, keys[list(rows)].tobytes(), counts[list(rows)].tobytes(), boxes[list(rows)].tobytes())
        if ck not in _REFS:
            _REFS[ck] = slice_ref.merge_image(lists, od.num_classes, post.K, slicing.edges(r, w, h), slicing.affine(r, w, h),
                                              lo, hi, post.iou_threshold, bool(post.strict), post.max_det, od.slice_vote_iou)
        ref = _REFS[ck]
        k = len(ref["cls"])
        assert int(kc[g]) == k and int(det[g, :1].view(np.int32)[0]) == k, (what, g)
        rec = det[g, 1:].reshape(post.max_det, 6).view(np.uint32)
        assert np.array_equal(src[g, :k], ref["src"]), (what, g)
        assert np.array_equal(rec[:k, 0].view(np.int32), ref["cls"]) and np.array_equal(rec[:k, 1], ref["conf_bits"]), (what, g)
        assert np.array_equal(rec[:k, 2:6], ref["boxes"].view(np.uint32)), (what, g)
        assert (rec[k:, 0].view(np.int32) == -1).all() and (rec[k:, 1:] == 0).all() and (src[g, k:] == -1).all(), (what, g)
        tiles_seen += src[g, :k, 0].tolist()
        preds.append((ref["cls"], ref["conf_bits"], ref["boxes"]))
    return tiles_seen, preds


def _same(pred, ref):
    cls, bits, boxes = ref
    assert pred.flat_indices is None
    assert np.array_equal(pred.classes, cls) and np.array_equal(pred.confs.view(np.uint32), bits)
    assert np.array_equal(pred.bboxes.view(np.uint32), boxes.view(np.uint32))
    assert len(boxes) == 0 or (boxes.min() >= 0 and boxes.max() <= 1)


def _run_both_routes(od, imgs):
    """predict() on both image routes; every batch's pipeline is checked after each.  -> tiles the kept detections came from"""
    G = od.slices and od.batch_size // od.slices.T
    od.predict(imgs[:1], conf_threshold=THR)  # the first submit measures the stream set and restarts the pipeline rotation
    tiles_seen, results = [], {}
    for route in ("host", "device"):
        first = od._next
        results[route] = od.predict(imgs, conf_threshold=THR, image_decode=route)
        assert len(results[route]) == len(imgs)
        for bi, s in enumerate(range(0, len(imgs), G)):
            p = od._pipes[(first + bi) % len(od._pipes)]
            seen, refs = _check_pipeline(od, p, imgs[s:s + G], f"{route} batch {bi}")
            tiles_seen += seen
            for pr, ref in zip(results[route][s:s + G], refs):
                _same(pr, ref)
    for a, d in zip(results["host"], results["device"]):
        assert np.array_equal(a.classes, d.classes) and np.array_equal(a.confs.view(np.uint32), d.confs.view(np.uint32))
        assert np.array_equal(a.bboxes.view(np.uint32), d.bboxes.view(np.uint32))
    return tiles_seen


def test_sliced_detector_end_to_end(cuda):
    from object_detector_amd.detector import ObjectDetector
    od = ObjectDetector.synthetic(10, (96, 96), seed=2, device=cuda, slices=(2, 2))
    plain = ObjectDetector.synthetic(10, (96, 96), seed=2, device=cuda)
    assert od.slices.T == 5 and all(p.slc.G == 2 and p.slc.det.shape[0] == 2 for p in od._pipes)
    imgs = _images([(200, 150), (333, 97), (180, 240)], seed=7)  # two batches, the second partial
    tiles_seen = _run_both_routes(od, imgs)
    assert any(t < 4 for t in tiles_seen), "no kept detection came from a tile"
    assert any(t == 4 for t in tiles_seen), "no kept detection came from the full view"
    assert od.decode_stats == {"jpeg": 0, "fallback": 0, "array": 3}

    # the candidates of every row are the plain detector's on the same network input
    p = od._pipes[0]
    x = p.net.input.clone()
    od.synchronize()
    p.slc.run(p.net, x, [(im.shape[1], im.shape[0]) for im in imgs[:2]], THR)
    plain.predict_batch_device(x, conf_threshold=THR)
    torch.cuda.synchronize()
    assert int(plain.post.counts.sum()) > 0
    assert torch.equal(plain.post.counts, p.slc.counts) and torch.equal(plain.post.keys, p.slc.keys)
    assert torch.equal(plain.post.boxes.view(torch.int32), p.slc.boxes.view(torch.int32))

    # the entries that take a ready-made batch are refused, graph replay too
    for call in (lambda: od.predict_batch_device(x), lambda: od.submit(x), lambda: od.collect(0)):
        with pytest.raises(ValueError, match="predict\\(\\) is the public route"):
            call()
    for call in (lambda: od.predict_batch_device(x, graph=True), lambda: od.submit(x, graph=True)):
        with pytest.raises(ValueError, match="graph"):
            call()
    for kw, msg in (({"slices": (4, 4)}, "at most 16"), ({"slices": (2, 2), "tta": ()}, "tta"),
                    ({"slices": (2, 2), "keep_aspect": True}, "keep_aspect"), ({"slices": (3, 3)}, "batch_size")):
        with pytest.raises(ValueError, match=msg):
            ObjectDetector.synthetic(8, (96, 96), seed=2, device=cuda, **kw)


def test_a_file_is_decoded_once_on_the_host(cuda, tmp_path):
    """Image files: both routes decode them with PIL at their own size (decode_stats counts them as "fallback" on the device
    route) and agree bit for bit."""
    from PIL import Image
    from object_detector_amd.detector import ObjectDetector
    od = ObjectDetector.synthetic(5, (96, 96), seed=2, device=cuda, slices=(2, 2), n_inflight=1)
    paths = []
    for i, im in enumerate(_images([(160, 120), (131, 77)], seed=9)):
        paths.append(str(tmp_path / f"im{i}.png"))
        Image.fromarray(im).save(paths[-1])
    host = od.predict(paths, conf_threshold=THR, image_decode="host")
    devr = od.predict(paths, conf_threshold=THR, image_decode="device")
    assert od.decode_stats == {"jpeg": 0, "fallback": 2, "array": 0}
    assert sum(len(a) for a in host) > 0
    for a, d in zip(host, devr):
        assert np.array_equal(a.classes, d.classes) and np.array_equal(a.confs.view(np.uint32), d.confs.view(np.uint32))
        assert np.array_equal(a.bboxes.view(np.uint32), d.bboxes.view(np.uint32))


def test_slices_none_is_the_plain_detector(cuda):
    from object_detector_amd.detector import ObjectDetector
    from oracle import network as onet
    B, S = 2, 96
    xt = torch.from_numpy(onet.synthetic_images(B, S, seed=0)).to(cuda)
    plain = ObjectDetector.synthetic(B, (S, S), seed=2, device=cuda)
    none = ObjectDetector.synthetic(B, (S, S), seed=2, device=cuda, slices=None, slice_overlap=0.3, slice_full_view=False)
    assert none.slices is None and all(p.slc is None for p in none._pipes) and not hasattr(none.post, "tiles")
    kf, kc = plain.predict_batch_device(xt, conf_threshold=THR)
    kf2, kc2 = none.predict_batch_device(xt, conf_threshold=THR)
    torch.cuda.synchronize()
    assert torch.equal(kf, kf2) and torch.equal(kc, kc2) and int(kc.sum()) > 0
    a, b = plain.collect(plain.submit(xt, conf_threshold=THR)), none.collect(none.submit(xt, conf_threshold=THR))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[0], kf)
    imgs = _images([(120, 90), (96, 96)], seed=1)
    for pa, pb in zip(plain.predict(imgs, conf_threshold=THR), none.predict(imgs, conf_threshold=THR)):
        assert np.array_equal(pa.flat_indices, pb.flat_indices) and np.array_equal(pa.confs.view(np.uint32), pb.confs.view(np.uint32))
        assert np.array_equal(pa.bboxes.view(np.uint32), pb.bboxes.view(np.uint32))


def test_sliced_detector_32x320_with_unused_rows(cuda):
    """32 x 320^2, T = 5: six images per batch, rows 30 and 31 unused."""
    from object_detector_amd.detector import ObjectDetector
    od = ObjectDetector.synthetic(32, (320, 320), seed=2, device=cuda, slices=(2, 2), n_inflight=2)
    assert all(p.slc.G == 6 and p.slc.T == 5 for p in od._pipes)
    imgs = _images([(640, 480), (500, 700), (321, 320), (1000, 600), (320, 320), (777, 333)], seed=4)
    tiles_seen = _run_both_routes(od, imgs)
    assert len(tiles_seen) > 0
