"""GPU: flip test-time augmentation, bit for bit.  (a) od_hflip_u8 against torch.flip, (b) od_detect_candidates against
od_detect, (c) od_tta_merge against the numpy restatement tests/tta_ref.py, (d) ObjectDetector(tta=("flip",)) end to end.
Every output of (a)-(c) is a view inside a sentinel-filled allocation whose guards must stay untouched; nothing here has a
tolerance."""
import ctypes as C

import numpy as np
import pytest
import torch

import lattice_ref as L
import tta_ref
from oracle import network as onet
from oracle import postprocess as opp

pytestmark = pytest.mark.gpu

F = np.float32


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ctx(cuda):
    from object_detector_amd import _lib
    from object_detector_amd.net import Context
    ctx = Context.get(cuda)
    return _lib, ctx.lib, ctx.handle


# ---- (a) od_hflip_u8 -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 32])
@pytest.mark.parametrize("H,W", [(96, 96), (320, 320), (640, 640), (33, 50)], ids=["96", "320", "640", "33x50"])
def test_hflip_equals_torch_flip(cuda, B, H, W):
    """The three network sizes (16 pixels per thread) and one width that takes the pixel-per-thread kernel."""
    _lib, lib, h = _ctx(cuda)
    rng = np.random.default_rng(L.seed_of("hflip", B, H, W))
    x = rng.integers(0, 255, (B, H, W, 3), dtype=np.uint8)  # 255 is the poison around the input
    src = L.poisoned(x, cuda)
    dst = L.Guarded((B, H, W, 3), torch.uint8, cuda)
    for _rep in range(2):
        _lib.check(lib.od_hflip_u8(h, src.data_ptr(), dst.t.data_ptr(), B, H, W, _stream()), "od_hflip_u8")
        torch.cuda.synchronize()
        got = dst.numpy("od_hflip_u8")
        assert np.array_equal(got, torch.flip(torch.from_numpy(x), dims=[2]).numpy())
        assert np.array_equal(src.cpu().numpy(), x)
    with pytest.raises(_lib.OdError, match="overlap"):
        _lib.check(lib.od_hflip_u8(h, src.data_ptr(), src.data_ptr(), B, H, W, _stream()), "od_hflip_u8")


# ---- (b) od_detect_candidates ----------------------------------------------------------------------------------------------
def _regime_pred(mode, rng, B, P, NC):
    """The regimes of tests/test_gpu_postprocess.py::test_fused_detect_equals_the_three_call_path, for any class count."""
    pred = rng.normal(0, 2, (B, P, NC + 6)).astype(F)
    thr = 0.01
    if mode == "trained_like":
        pred[..., 0], pred[..., 1] = 4.0 + rng.normal(0, 0.3, (B, P)), -4.0 + rng.normal(0, 0.3, (B, P))
        hot = rng.integers(0, P, (B, 40))
        for b in range(B):
            pred[b, hot[b], 0], pred[b, hot[b], 1] = -3.0, 3.0
            pred[b, hot[b], 2 + rng.integers(0, NC, 40)] += 6.0
    elif mode == "ties":
        pred[..., :2 + NC] = np.round(pred[..., :2 + NC])
    elif mode == "few":
        pred[..., 0], pred[..., 1] = 9.0, -9.0
        pred[:, :17, 0], pred[:, :17, 1] = -2.0, 2.0  # 17 live priors
    elif mode == "none":
        pred[..., 0], pred[..., 1] = 20.0, -20.0
    elif mode == "all_equal":
        pred[...] = 0.0  # every conf = 0.5 / NC
        thr = 0.4 / NC
    else:
        assert mode == "random"
    return pred, thr


@pytest.mark.parametrize("NC", [20, 80])
@pytest.mark.parametrize("mode", ["random", "trained_like", "ties", "few", "none", "all_equal"])
def test_detect_candidates_equals_detect(cuda, mode, NC):
    """keys / counts / boxes of od_detect_candidates == od_detect's on the same pred and the same workspace, three calls in a
    row, both dispatches (NC = 20: whole rows in LDS; NC = 80: streamed), and the calls alternate with od_detect to show that
    either leaves the workspace ready for the other.  The suppression mask of the NMS workspace is never written."""
    from object_detector_amd.postprocess import Postprocessor
    _lib, lib, h = _ctx(cuda)
    B, K = 3, 1024
    priors = opp.make_priors((320, 320))
    P = len(priors)
    pp = Postprocessor(B, P, NC, priors, device=cuda, topk=K)
    pred, thr = _regime_pred(mode, np.random.default_rng(L.seed_of("cand", mode, NC)), B, P, NC)
    pt = torch.from_numpy(pred).to(cuda)
    boxes = L.Guarded((B, P, 4), torch.float32, cuda)
    keys = L.Guarded((B, K), torch.int64, cuda)
    counts = L.Guarded((B,), torch.int32, cuda)
    mask_off = B * 1024 * (8 + 16 + 4)  # nms.hip's layout: sorted keys, boxes, classes, then the mask
    for thr_i in (thr, 0.3):
        pp.run(pt, thr_i)
        torch.cuda.synchronize()
        ref_boxes, ref_keys, ref_counts = pp.boxes.clone(), pp.keys.clone(), pp.counts.clone()
        ref_kf, ref_kc = pp.keep_flat.clone(), pp.keep_count.clone()
        if thr_i == thr:
            n = ref_counts.cpu().numpy()
            if mode == "none":
                assert (n == 0).all()
            elif mode in ("few", "trained_like"):
                assert (n > 0).all() and (n < K).all(), (mode, n)
            else:
                assert (n == K).all(), (mode, n)
        for _rep in range(3):
            boxes.t.zero_(), keys.t.zero_(), counts.t.fill_(-7)
            pp.ws_nms[mask_off:].fill_(0x5A)
            _lib.check(lib.od_detect_candidates(h, pt.data_ptr(), pp.priors.data_ptr(), B, P, NC, pp.loc_scale, 1, float(thr_i),
                                                K, boxes.t.data_ptr(), None, keys.t.data_ptr(), counts.t.data_ptr(),
                                                pp.ws_det.data_ptr(), pp.ws_det_bytes, pp.ws_nms.data_ptr(), pp.ws_nms_bytes,
                                                _stream()), "od_detect_candidates")
            torch.cuda.synchronize()
            assert bool((pp.ws_nms[mask_off:] == 0x5A).all()), "od_detect_candidates ran an NMS launch"
            assert np.array_equal(counts.numpy("counts"), ref_counts.cpu().numpy())
            assert np.array_equal(keys.numpy("keys"), ref_keys.cpu().numpy()), mode
            assert np.array_equal(boxes.numpy("boxes").view(np.uint32), ref_boxes.cpu().numpy().view(np.uint32))
            pp.run(pt, thr_i)  # od_detect on the workspace od_detect_candidates left behind
            torch.cuda.synchronize()
            assert torch.equal(pp.keys, ref_keys) and torch.equal(pp.counts, ref_counts) and torch.equal(pp.boxes, ref_boxes)
            assert torch.equal(pp.keep_flat, ref_kf) and torch.equal(pp.keep_count, ref_kc)


# ---- (c) od_tta_merge --------------------------------------------------------------------------------------------------------
def _make_view(rng, B, K, P, NC, counts, quantise):
    """Generated candidates of one view: keys u64 [B,K] sorted descending (unused slots 0), counts, clustered boxes."""
    keys = np.zeros((B, K), np.uint64)
    boxes = np.zeros((B, P, 4), F)
    for b in range(B):
        n = counts[b]
        centers = rng.uniform(0.15, 0.85, (24, 2))
        which = rng.integers(0, 24, P)
        c = centers[which] + rng.normal(0, 0.012, (P, 2))
        wh = rng.uniform(0.08, 0.3, (24, 2))[which] * rng.uniform(0.9, 1.1, (P, 2))
        boxes[b] = np.clip(np.concatenate([c - wh / 2, c + wh / 2], 1), 0, 1).astype(F)
        # candidates sit on few priors and few classes, so that same-class overlaps (suppression, votes) are common
        pri = rng.choice(P, min(P, 400), replace=False)
        flat = rng.choice(len(pri) * 3, n, replace=False)
        flat = pri[flat // 3].astype(np.int64) * NC + (flat % 3) * 5
        conf = rng.uniform(0.011, 1.0, n).astype(F)
        if quantise:  # confidences on a coarse grid: ties inside a view and across views
            conf = (np.ceil(conf * 32) / 32).astype(F)
        k = (conf.view(np.uint32).astype(np.uint64) << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - flat.astype(np.uint64))
        keys[b, :n] = np.sort(k)[::-1]
    return keys, np.asarray(counts, np.int32), boxes


def _scenario(name, rng):
    """-> (B, K, NC, [(keys, counts, boxes, P, flip)])"""
    NC = 20
    if name == "v1":
        B, K, spec = 1, 1024, [(16800, 0, "full")]
    elif name == "v2_flip":
        B, K, spec = 2, 1024, [(16800, 0, "rand"), (16800, 1, "rand")]
    elif name == "v2_two_sizes":
        B, K, spec = 2, 1024, [(16800, 0, "rand"), (67200, 1, "full")]
    elif name == "v4":
        B, K, spec = 2, 512, [(16800, 0, "rand"), (67200, 1, "rand"), (4200, 0, "rand"), (16800, 1, "full")]
    elif name == "identical_views":
        B, K, spec = 2, 1024, [(16800, 0, "rand"), None]
    elif name == "one_empty_view":
        B, K, spec = 2, 1024, [(16800, 0, "rand"), (16800, 1, "empty")]
    elif name == "all_views_empty":
        B, K, spec = 2, 1024, [(16800, 0, "empty"), (16800, 1, "empty")]
    elif name == "sum_below_K":
        B, K, spec = 2, 1024, [(16800, 0, "small"), (16800, 1, "small")]
    elif name == "sum_is_VK":
        B, K, spec = 2, 1024, [(16800, 0, "full"), (16800, 1, "full"), (16800, 0, "full")]
    elif name == "B32":
        B, K, spec = 32, 256, [(16800, 0, "rand"), (16800, 1, "rand")]
    elif name == "v8":  # the view capacity: P and flip alternate, and the quantised even views tie across views
        B, K, spec = 1, 1024, [((16800, 4200)[v % 2], v % 2, how)
                               for v, how in enumerate(("full", "rand", "rand", "small", "empty", "rand", "full", "rand"))]
    else:
        raise AssertionError(name)
    views = []
    for v, sp in enumerate(spec):
        if sp is None:  # the same lists and boxes again: every confidence is tied across the two views
            keys, counts, boxes, P, _ = views[0]
            views.append((keys.copy(), counts.copy(), boxes.copy(), P, 0))
            continue
        P, flip, how = sp
        counts = {"full": [K] * B, "empty": [0] * B, "small": [int(rng.integers(1, K // 4)) for _ in range(B)],
                  "rand": [int(rng.integers(0, K + 1)) for _ in range(B)]}[how]
        if how == "rand":
            counts[0] = K // 2 + v
        keys, counts, boxes = _make_view(rng, B, K, P, NC, counts, quantise=(v % 2 == 0))
        views.append((keys, counts, boxes, P, flip))
    return B, K, NC, views


SCENARIOS = ["v1", "v2_flip", "v2_two_sizes", "v4", "identical_views", "one_empty_view", "all_views_empty", "sum_below_K",
             "sum_is_VK", "B32", "v8"]


def _check_merge(out, src, kc, views_np, b, NC, K, thr, strict, max_det, vote_iou, what):
    ref = tta_ref.merge_image(views_np, NC, K, thr, strict, max_det, vote_iou)
    n = len(ref["cls"])
    assert int(kc[b]) == n, (what, b, int(kc[b]), n)
    row = out[b]
    assert int(row[:1].view(np.int32)[0]) == n, (what, b)
    rec = row[1:].reshape(max_det, 6).view(np.uint32)
    assert np.array_equal(src[b, :n], ref["src"]), (what, b)
    assert np.array_equal(rec[:n, 0].view(np.int32), ref["cls"]), (what, b)
    assert np.array_equal(rec[:n, 1], ref["conf_bits"]), (what, b)
    assert np.array_equal(rec[:n, 2:6], ref["boxes"].view(np.uint32)), (what, b)
    assert (rec[n:, 0].view(np.int32) == -1).all() and (rec[n:, 1:] == 0).all() and (src[b, n:] == -1).all(), (what, b)
    return n


@pytest.mark.parametrize("vote_iou", [0.0, 0.5, 0.9])
@pytest.mark.parametrize("strict", [0, 1])
@pytest.mark.parametrize("name", SCENARIOS)
def test_tta_merge_equals_reference(cuda, name, strict, vote_iou):
    """Kept (view, flat), class, confidence bits, box bits, counts and the padding of od_tta_merge against tta_ref on generated
    keys and boxes; three consecutive calls on one workspace that is filled with a different byte before each."""
    kept, total, B, K = _run_merge_case(cuda, name, strict, vote_iou, 0.45, 200)
    assert (sum(kept) == 0) == (total == 0)
    if total:
        assert sum(kept) < min(total, B * K), "the case never suppressed anything"


@pytest.mark.parametrize("vote_iou", [0.0, 0.5])
def test_tta_merge_more_kept_than_one_round(cuda, vote_iou):
    """max_det = 300 with a suppression threshold that removes little: more than 256 kept detections in an image, which the
    voting kernel takes in a second round, and the max_det cut."""
    kept, total, B, K = _run_merge_case(cuda, "v2_flip", 0, vote_iou, 0.9, 300)
    assert max(kept) == 300 and sum(kept) < total


def _run_merge_case(cuda, name, strict, vote_iou, thr, max_det):
    _lib, lib, h = _ctx(cuda)
    B, K, NC, views = _scenario(name, np.random.default_rng(L.seed_of("merge", name)))
    V = len(views)
    dev = [(torch.from_numpy(k.view(np.int64)).to(cuda), torch.from_numpy(c).to(cuda), torch.from_numpy(bx).to(cuda))
           for k, c, bx, _, _ in views]
    desc = (_lib.TtaView * V)()
    for v, (k, c, bx) in enumerate(dev):
        desc[v] = _lib.TtaView(k.data_ptr(), c.data_ptr(), bx.data_ptr(), views[v][3], views[v][4])
    ws_bytes = lib.od_tta_merge_workspace_bytes(B, V, K)
    assert ws_bytes > 0
    ws = L.Guarded((ws_bytes,), torch.uint8, cuda)
    out = L.Guarded((B, 1 + 6 * max_det), torch.float32, cuda)
    src = L.Guarded((B, max_det, 2), torch.int32, cuda)
    kc = L.Guarded((B,), torch.int32, cuda)
    results = []
    for rep in range(3):
        ws.t.fill_((0x00, 0xFF, 0x5A)[rep])  # nothing may carry over from call to call, or depend on what was there
        out.t.fill_(float("nan")), src.t.fill_(12345), kc.t.fill_(-9)
        _lib.check(lib.od_tta_merge(h, desc, V, B, NC, K, thr, strict, max_det, float(vote_iou), out.t.data_ptr(),
                                    src.t.data_ptr(), kc.t.data_ptr(), ws.t.data_ptr(), ws_bytes, _stream()), "od_tta_merge")
        torch.cuda.synchronize()
        ws.check("workspace")
        results.append((out.numpy("out").copy(), src.numpy("src").copy(), kc.numpy("keep_count").copy()))
    for r in results[1:]:
        assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(r, results[0])), "calls differ"
    o, s, n = results[0]
    kept = []
    for b in range(B):
        views_np = [{"keys": k[b], "count": int(c[b]), "boxes": bx[b], "flip": bool(fl)} for k, c, bx, _, fl in views]
        kept.append(_check_merge(o, s, n, views_np, b, NC, K, thr, bool(strict), max_det, vote_iou, name))
    total = sum(int(c.sum()) for _, c, _, _, _ in views)
    # src NULL: the same record block
    out.t.fill_(float("nan"))
    _lib.check(lib.od_tta_merge(h, desc, V, B, NC, K, thr, strict, max_det, float(vote_iou), out.t.data_ptr(), None,
                                kc.t.data_ptr(), ws.t.data_ptr(), ws_bytes, _stream()), "od_tta_merge")
    torch.cuda.synchronize()
    assert np.array_equal(out.numpy("out").view(np.uint32), o.view(np.uint32))
    return kept, total, B, K


def test_tta_merge_rejects_bad_arguments(cuda):
    _lib, lib, h = _ctx(cuda)
    t = torch.zeros(64, dtype=torch.int64, device=cuda)
    desc = (_lib.TtaView * 9)()
    for v in range(9):
        desc[v] = _lib.TtaView(t.data_ptr(), t.data_ptr(), t.data_ptr(), 8, 0)
    assert lib.od_tta_merge_workspace_bytes(1, 9, 4) == 0 and lib.od_tta_merge_workspace_bytes(1, 1, 2048) == 0
    n = lib.od_tta_merge_workspace_bytes(1, 2, 4)
    ws = torch.zeros(n, dtype=torch.uint8, device=cuda)
    for V, K, nbytes, msg in ((9, 4, n, "outside 1..8"), (0, 4, n, "outside 1..8"), (2, 2048, n, "K <= 1024"),
                              (2, 4, n - 1, "workspace")):
        with pytest.raises(_lib.OdError, match=msg):
            _lib.check(lib.od_tta_merge(h, desc, V, 1, 20, K, 0.45, 0, 4, 0.5, t.data_ptr(), None, t.data_ptr(),
                                        ws.data_ptr(), nbytes, _stream()), "od_tta_merge")


# ---- (d) end to end ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,S", [(2, 96), (32, 320)], ids=["2x96", "32x320"])
def test_detector_with_flip_tta(cuda, B, S):
    from object_detector_amd.detector import ObjectDetector
    thr = 0.01
    x = onet.synthetic_images(B, S, seed=0)
    xt = torch.from_numpy(x).to(cuda)
    od = ObjectDetector.synthetic(B, (S, S), seed=2, device=cuda, tta=("flip",))
    plain = ObjectDetector.synthetic(B, (S, S), seed=2, device=cuda)
    det, kcount = od.predict_batch_device(xt, conf_threshold=thr)
    torch.cuda.synchronize()
    tta = od._pipes[0].tta
    det, kcount = det.cpu().numpy(), kcount.cpu().numpy()
    src = tta.src.cpu().numpy()
    cand = [(tta.keys[v].cpu().numpy().view(np.uint64), tta.counts[v].cpu().numpy(), tta.boxes[v].cpu().numpy())
            for v in range(2)]
    assert int(cand[0][1].sum()) > 0 and int(cand[1][1].sum()) > 0

    # every view's candidates are the plain detector's od_detect keys / boxes on that view's image
    for v, xin in enumerate((xt, torch.flip(xt, dims=[2]).contiguous())):
        plain.predict_batch_device(xin, conf_threshold=thr)
        torch.cuda.synchronize()
        assert np.array_equal(plain.post.counts.cpu().numpy(), cand[v][1]), v
        assert np.array_equal(plain.post.keys.cpu().numpy().view(np.uint64), cand[v][0]), v
        assert np.array_equal(plain.post.boxes.cpu().numpy().view(np.uint32), cand[v][2].view(np.uint32)), v

    # the merged result is the reference's on the device's own candidates
    post = od.post
    for b in range(B):
        views_np = [{"keys": cand[v][0][b], "count": int(cand[v][1][b]), "boxes": cand[v][2][b], "flip": v == 1}
                    for v in range(2)]
        _check_merge(det, src, kcount, views_np, b, od.num_classes, post.K, post.iou_threshold, bool(post.strict),
                     post.max_det, od.tta_vote_iou, f"{B}x{S}")
    assert (src[:, :, 0] == 1).any() and (src[:, :, 0] == 0).any(), "one view never contributed a detection"

    # submit / collect returns the same block; graph replay is refused
    d2, k2 = od.collect(od.submit(xt, conf_threshold=thr))
    assert np.array_equal(d2.cpu().numpy().view(np.uint32), det.view(np.uint32)) and np.array_equal(k2.cpu().numpy(), kcount)
    with pytest.raises(ValueError, match="graph"):
        od.predict_batch_device(xt, graph=True)
    with pytest.raises(ValueError, match="graph"):
        od.submit(xt, graph=True)

    # predict() on the same arrays: host and device decode routes agree with each other and with the block
    imgs = [x[b] for b in range(B)] + [x[0]]  # a second, partial batch
    host = od.predict(imgs, conf_threshold=thr, image_decode="host")
    devr = od.predict(imgs, conf_threshold=thr, image_decode="device")
    assert len(host) == len(devr) == B + 1
    for i, (a, d) in enumerate(zip(host, devr)):
        b = i % B
        n = int(kcount[b])
        rec = det[b, 1:1 + 6 * n].reshape(n, 6)
        assert a.flat_indices is None and d.flat_indices is None
        for pr in (a, d):
            assert np.array_equal(pr.classes, rec[:, 0].copy().view(np.int32)), i
            assert np.array_equal(pr.confs.view(np.uint32), rec[:, 1].copy().view(np.uint32)), i
            assert np.array_equal(pr.bboxes.view(np.uint32), np.ascontiguousarray(rec[:, 2:6]).view(np.uint32)), i
    od.close_decode_pool()


def test_voting_only_and_tta_none(cuda):
    """tta=() is one identity view: the kept set of the plain detector with voted boxes.  tta=None is the plain detector:
    bit-identical keep_flat / keep_count, and no TTA buffers."""
    from object_detector_amd.detector import ObjectDetector
    B, S, thr = 2, 96, 0.01
    x = onet.synthetic_images(B, S, seed=0)
    xt = torch.from_numpy(x).to(cuda)
    plain = ObjectDetector.synthetic(B, (S, S), seed=2, device=cuda)
    none = ObjectDetector.synthetic(B, (S, S), seed=2, device=cuda, tta=None)
    assert all(p.tta is None for p in none._pipes)
    kf, kc = plain.predict_batch_device(xt, conf_threshold=thr)
    kf2, kc2 = none.predict_batch_device(xt, conf_threshold=thr)
    torch.cuda.synchronize()
    assert torch.equal(kf, kf2) and torch.equal(kc, kc2) and int(kc.sum()) > 0
    a, b = plain.collect(plain.submit(xt, conf_threshold=thr)), none.collect(none.submit(xt, conf_threshold=thr))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[0], kf)

    vote = ObjectDetector.synthetic(B, (S, S), seed=2, device=cuda, tta=(), tta_vote_iou=0.5)
    det, kc3 = vote.predict_batch_device(xt, conf_threshold=thr)
    torch.cuda.synchronize()
    assert vote._pipes[0].tta.V == 1 and vote._pipes[0].tta.mirrored is None
    assert torch.equal(kc3, kc)
    src = vote._pipes[0].tta.src.cpu().numpy()
    kfn, det = kf.cpu().numpy(), det.cpu().numpy()
    cand = vote._pipes[0].tta
    for i in range(B):
        n = int(kc[i])
        assert np.array_equal(src[i, :n, 1], kfn[i, :n]) and (src[i, :n, 0] == 0).all()
        views_np = [{"keys": cand.keys[0][i].cpu().numpy().view(np.uint64), "count": int(cand.counts[0][i]),
                     "boxes": cand.boxes[0][i].cpu().numpy(), "flip": False}]
        _check_merge(det, src, kc3.cpu().numpy(), views_np, i, vote.num_classes, vote.post.K, vote.post.iou_threshold,
                     bool(vote.post.strict), vote.post.max_det, 0.5, "vote only")


def test_keep_aspect_mirrors_the_canvas(cuda):
    """keep_aspect letterboxes an image onto the canvas; TTA mirrors the whole canvas and un-mirrors the boxes in canvas
    coordinates, so predict() is the record block of the canvas batch with the existing scale division applied -- on the host
    and on the device decode route alike."""
    from object_detector_amd.detector import ObjectDetector
    from object_detector_amd.imageio import load_image
    B, S, thr = 2, 96, 0.01
    rng = np.random.default_rng(3)
    imgs = [rng.integers(0, 256, (60, 96, 3), dtype=np.uint8), rng.integers(0, 256, (96, 48, 3), dtype=np.uint8)]
    od = ObjectDetector.synthetic(B, (S, S), seed=2, device=cuda, keep_aspect=True, tta=("flip",))
    canvas, scales = zip(*(load_image(im, (S, S), True, True) for im in imgs))
    assert any(sc != (1.0, 1.0) for sc in scales)
    det, kc = od.predict_batch_device(torch.from_numpy(np.stack(canvas)).to(cuda), conf_threshold=thr)
    torch.cuda.synchronize()
    det, kc = det.cpu().numpy(), kc.cpu().numpy()
    assert int(kc.sum()) > 0
    host = od.predict(imgs, conf_threshold=thr, image_decode="host")
    devr = od.predict(imgs, conf_threshold=thr, image_decode="device")
    for b in range(B):
        n = int(kc[b])
        rec = det[b, 1:1 + 6 * n].reshape(n, 6)
        sx, sy = scales[b]
        want = np.clip(rec[:, 2:6] / np.array([sx, sy, sx, sy], F), 0.0, 1.0).astype(F)
        for pr in (host[b], devr[b]):
            assert np.array_equal(pr.classes, rec[:, 0].copy().view(np.int32))
            assert np.array_equal(pr.confs.view(np.uint32), rec[:, 1].copy().view(np.uint32))
            assert np.array_equal(pr.bboxes.view(np.uint32), want.view(np.uint32))
