"""GPU: Soft-NMS, bit for bit.  (a) od_soft_nms against the numpy restatement tests/soft_nms_ref.py, (b) its hard mode against
od_nms, (c) od_detect_soft against od_detect_candidates + od_soft_nms, (d) od_tta_merge_soft / od_slice_merge_soft against the
reference and, in hard mode, against od_tta_merge / od_slice_merge, (e) ObjectDetector(nms=...) end to end on every route.
Inputs sit in poisoned memory, outputs in guarded allocations, every call runs twice on the same buffers; nothing here has a
tolerance."""
import ctypes as C

import numpy as np
import pytest
import torch

import lattice_ref as L
import slice_ref
import soft_nms_ref as R
import tta_ref
from oracle import network as onet
from oracle import postprocess as opp
from test_gpu_tta import _make_view, _regime_pred

pytestmark = pytest.mark.gpu

F = np.float32
THR, SIGMA, MIN_CONF = R.GEN_THR, R.GEN_SIGMA, R.GEN_MIN_CONF
_TD = {np.dtype(np.uint64): torch.int64, np.dtype(np.int64): torch.int64, np.dtype(np.int32): torch.int32,
       np.dtype(np.float32): torch.float32}


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ctx(cuda):
    from object_detector_amd import _lib
    from object_detector_amd.net import Context
    ctx = Context.get(cuda)
    return _lib, ctx.lib, ctx.handle


def _poisoned(arr, cuda):
    """L.poisoned for any dtype: the bytes in the middle of a poisoned allocation, viewed as the array's type."""
    a = np.ascontiguousarray(arr)
    return L.poisoned(a.reshape(-1).view(np.uint8), cuda).view(_TD[a.dtype]).view(a.shape)


def _cfg(_lib, method, strict, max_det, thr=THR, sigma=SIGMA, min_conf=MIN_CONF):
    return _lib.SoftNmsCfg(R.METHODS[method], int(strict), int(max_det), float(thr), float(sigma), float(min_conf))


class _Outs:
    def __init__(self, B, max_det, cuda):
        self.kf = L.Guarded((B, max_det), torch.int32, cuda)
        self.kconf = L.Guarded((B, max_det), torch.float32, cuda)
        self.kc = L.Guarded((B,), torch.int32, cuda)
        self.det = L.Guarded((B, 1 + 6 * max_det), torch.float32, cuda)

    def poison(self):
        self.kf.t.fill_(12345), self.kconf.t.fill_(float("nan")), self.kc.t.fill_(-9), self.det.t.fill_(float("nan"))

    def read(self):
        return (self.kf.numpy("keep_flat"), self.kconf.numpy("keep_conf").view(np.uint32), self.kc.numpy("keep_count"),
                self.det.numpy("det").view(np.uint32))


def _lists(key, B, K, P, NC, counts):
    """B generated images (soft_nms_ref.crowded_image) -> boxes f32 [B,P,4], keys u64 [B,K] (unused slots 0), counts i32 [B]."""
    boxes = np.zeros((B, P, 4), F)
    keys = np.zeros((B, K), np.uint64)
    for b, n in enumerate(counts):
        boxes[b], k = R.crowded_image(L.seed_of("soft", key, b), n=max(n, 1), NC=NC, P=P)
        keys[b, :n] = k[:n]
    return boxes, keys, np.asarray(counts, np.int32)


def _expect(boxes, keys, counts, NC, method, strict, max_det, thr=THR, sigma=SIGMA, min_conf=MIN_CONF):
    """The reference's four outputs for a batch, as the device lays them out."""
    B = len(counts)
    kf = np.full((B, max_det), -1, np.int32)
    kconf = np.zeros((B, max_det), F)
    kc = np.zeros(B, np.int32)
    det = np.zeros((B, 1 + 6 * max_det), np.uint32)
    for b in range(B):
        f, s, bx = R.soft_nms_image(boxes[b], keys[b, :counts[b]], NC, R.METHODS[method], thr, bool(strict), max_det, sigma,
                                    min_conf)
        kf[b, :len(f)], kconf[b, :len(f)], kc[b] = f, s, len(f)
        det[b] = R.det_rows(f, s, bx, max_det)
    return kf, kconf.view(np.uint32), kc, det


def _run_soft_nms(cuda, boxes, keys, counts, NC, K, cfgs, min_conf=MIN_CONF):
    """od_soft_nms on one set of inputs for every (method, strict, max_det) of cfgs, twice each -> {cfg: outputs}."""
    _lib, lib, h = _ctx(cuda)
    B, P = boxes.shape[:2]
    bt, kt, ct = _poisoned(boxes, cuda), _poisoned(keys, cuda), _poisoned(counts, cuda)
    ws_bytes = lib.od_nms_workspace_bytes(B, K)
    ws = L.Guarded((ws_bytes,), torch.uint8, cuda)
    got = {}
    for method, strict, max_det in cfgs:
        cfg = _cfg(_lib, method, strict, max_det, min_conf=min_conf)
        o = _Outs(B, max_det, cuda)
        reps = []
        for rep in range(2):
            o.poison()
            ws.t.fill_((0xFF, 0x5A)[rep])
            _lib.check(lib.od_soft_nms(h, bt.data_ptr(), kt.data_ptr(), ct.data_ptr(), B, P, NC, K, C.byref(cfg),
                                       o.kf.t.data_ptr(), o.kconf.t.data_ptr(), o.kc.t.data_ptr(), o.det.t.data_ptr(),
                                       ws.t.data_ptr(), ws_bytes, _stream()), "od_soft_nms")
            torch.cuda.synchronize()
            ws.check("workspace")
            reps.append(o.read())
        assert all(np.array_equal(a, b) for a, b in zip(*reps)), (method, strict, max_det, "two calls differ")
        got[(method, strict, max_det)] = reps[0]
    assert np.array_equal(bt.cpu().numpy(), boxes) and np.array_equal(kt.cpu().numpy().view(np.uint64), keys)
    return got


# ---- (a) od_soft_nms against the reference ----------------------------------------------------------------------------------
SIZES = [(0, 128), (1, 128), (63, 128), (64, 128), (65, 128), (100, 100), (1000, 1024), (1024, 1024)]


@pytest.mark.parametrize("NC", [1, 3])
@pytest.mark.parametrize("n,K", SIZES, ids=[f"n{n}_K{K}" for n, K in SIZES])
def test_soft_nms_equals_reference(cuda, n, K, NC):
    """keep_flat, keep_conf bits, keep_count and the record block for every method x strict x max_det in (1, 7, 200); three
    images with different counts (n, n // 2, n - 3).  The large lists draw their flat indices with repetition (P * NC < n):
    candidates on one prior and class are exact duplicates."""
    counts = [n, n // 2, max(n - 3, 0)]
    boxes, keys, counts = _lists((n, K, NC), 3, K, 256, NC, counts)
    cfgs = [(m, s, md) for m in R.METHODS for s in (0, 1) for md in (1, 7, 200)]
    got = _run_soft_nms(cuda, boxes, keys, counts, NC, K, cfgs)
    for cfg in cfgs:
        want = _expect(boxes, keys, counts, NC, *cfg)
        for g, w, what in zip(got[cfg], want, ("keep_flat", "keep_conf", "keep_count", "det")):
            assert np.array_equal(g, w), (cfg, what)
    if n >= 63:  # the case means something: soft keeps what hard drops, 7 cuts the list, 200 does not
        kc = {c: got[c][2] for c in cfgs}
        assert (kc[("linear", 0, 7)] == 7).any() and (kc[("hard", 0, 200)] < 200).all()
        assert (kc[("gaussian", 0, 200)] > kc[("hard", 0, 200)]).all()


@pytest.mark.parametrize("name", list(R.CRAFTED))
def test_soft_nms_crafted_lists(cuda, name):
    """Duplicates (linear weight 0: dropped), zero-area boxes (inter == 0: untouched), a rescored tie (the lower rank wins), a
    chain decayed by three kept boxes -- tests/test_soft_nms_host.py states what the reference must show on each."""
    boxes, keys, NC = R.crafted(name)
    n, K = len(keys), 128
    kb = np.zeros((3, K), np.uint64)
    kb[:, :n] = keys
    counts = np.array([n, n - 1, 1], np.int32)
    bb = np.stack([boxes] * 3)
    cfgs = [(m, s, 200) for m in R.METHODS for s in (0, 1)]
    got = _run_soft_nms(cuda, bb, kb, counts, NC, K, cfgs, min_conf=0.01)
    for cfg in cfgs:
        m, s, md = cfg
        want = _expect(bb, kb, counts, NC, m, s, md, thr=0.3, sigma=0.5, min_conf=0.01)
        for g, w, what in zip(got[cfg], want, ("keep_flat", "keep_conf", "keep_count", "det")):
            assert np.array_equal(g, w), (name, cfg, what)
    kc = {c: int(got[c][2][0]) for c in cfgs}
    if name == "duplicates":
        assert kc[("linear", 0, 200)] == 1 and kc[("gaussian", 0, 200)] == n
    elif name == "zero_area":
        assert all(v == n for v in kc.values())
    elif name == "tie":
        kf, kconf = got[("linear", 0, 200)][:2]
        assert kconf[0, 1] == kconf[0, 2] and kf[0, 1] < kf[0, 2]
    else:
        assert kc[("hard", 0, 200)] == 3 and kc[("linear", 0, 200)] == 4 and kc[("gaussian", 0, 200)] == 4


# ---- (b) hard mode against od_nms -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,K", [(65, 128), (100, 100), (1024, 1024)], ids=["n65", "n100", "n1024"])
@pytest.mark.parametrize("strict", [0, 1])
def test_hard_mode_equals_od_nms(cuda, n, K, strict):
    _lib, lib, h = _ctx(cuda)
    B, P, NC = 3, 256, 3
    boxes, keys, counts = _lists(("hard", n, K), B, K, P, NC, [n, n // 2, max(n - 3, 0)])
    bt, kt, ct = _poisoned(boxes, cuda), _poisoned(keys, cuda), _poisoned(counts, cuda)
    ws_bytes = lib.od_nms_workspace_bytes(B, K)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=cuda)
    for max_det in (7, 200):
        kf = L.Guarded((B, max_det), torch.int32, cuda)
        kc = L.Guarded((B,), torch.int32, cuda)
        _lib.check(lib.od_nms(h, bt.data_ptr(), kt.data_ptr(), ct.data_ptr(), B, P, NC, K, THR, strict, max_det,
                              kf.t.data_ptr(), kc.t.data_ptr(), ws.data_ptr(), ws_bytes, _stream()), "od_nms")
        torch.cuda.synchronize()
        got = _run_soft_nms(cuda, boxes, keys, counts, NC, K, [("hard", strict, max_det)])[("hard", strict, max_det)]
        assert np.array_equal(got[0], kf.numpy("keep_flat")) and np.array_equal(got[2], kc.numpy("keep_count"))
        assert int(got[2].sum()) > 0


def test_soft_nms_rejects_bad_arguments(cuda):
    _lib, lib, h = _ctx(cuda)
    t = torch.zeros(4096, dtype=torch.int64, device=cuda)
    n = lib.od_nms_workspace_bytes(1, 64)
    ws = torch.zeros(n, dtype=torch.uint8, device=cuda)
    good = dict(method=1, strict=0, max_det=4, iou_threshold=0.3, sigma=0.5, min_conf=0.01)
    for bad, K, nbytes, msg in ((dict(method=3), 64, n, "method"), (dict(method=2, sigma=-1.0), 64, n, "sigma"),
                                (dict(min_conf=0.0), 64, n, "min_conf"), (dict(max_det=0), 64, n, "max_det"),
                                ({}, 2048, n, "K <= 1024"), ({}, 64, n - 1, "workspace")):
        cfg = _lib.SoftNmsCfg(**{**good, **bad})
        with pytest.raises(_lib.OdError, match=msg):
            _lib.check(lib.od_soft_nms(h, t.data_ptr(), t.data_ptr(), t.data_ptr(), 1, 8, 3, K, C.byref(cfg), t.data_ptr(),
                                       t.data_ptr(), t.data_ptr(), None, ws.data_ptr(), nbytes, _stream()), "od_soft_nms")


# ---- (c) od_detect_soft against od_detect_candidates + od_soft_nms ------------------------------------------------------------
@pytest.mark.parametrize("NC", [20, 80])
@pytest.mark.parametrize("mode", ["random", "ties", "few", "none", "all_equal"])
def test_detect_soft_equals_the_split_route(cuda, mode, NC):
    """Both dispatches (NC = 20: whole rows in LDS; NC = 80: streamed).  od_detect_soft alternates with od_detect on the same
    workspaces, and od_detect's results stay what they were."""
    from object_detector_amd.postprocess import Postprocessor
    _lib, lib, h = _ctx(cuda)
    B, K, max_det = 3, 1024, 200
    priors = opp.make_priors((320, 320))
    P = len(priors)
    pp = Postprocessor(B, P, NC, priors, device=cuda, topk=K)
    pred, thr = _regime_pred(mode, np.random.default_rng(L.seed_of("detect_soft", mode, NC)), B, P, NC)
    pt = torch.from_numpy(pred).to(cuda)
    pp.run(pt, thr)
    torch.cuda.synchronize()
    ref_kf, ref_kc, ref_keys = pp.keep_flat.clone(), pp.keep_count.clone(), pp.keys.clone()
    boxes = L.Guarded((B, P, 4), torch.float32, cuda)
    keys = L.Guarded((B, K), torch.int64, cuda)
    counts = L.Guarded((B,), torch.int32, cuda)
    ws2 = torch.empty(pp.ws_nms_bytes, dtype=torch.uint8, device=cuda)
    for method in ("linear", "gaussian", "hard"):
        cfg = _cfg(_lib, method, 0, max_det, thr=0.45, min_conf=max(thr, 1e-6))
        fused, split = _Outs(B, max_det, cuda), _Outs(B, max_det, cuda)
        for _rep in range(2):
            fused.poison(), split.poison()
            boxes.t.zero_(), keys.t.zero_(), counts.t.fill_(-7)
            _lib.check(lib.od_detect_soft(h, pt.data_ptr(), pp.priors.data_ptr(), B, P, NC, pp.loc_scale, 1, float(thr), K,
                                          C.byref(cfg), boxes.t.data_ptr(), None, keys.t.data_ptr(), counts.t.data_ptr(),
                                          fused.kf.t.data_ptr(), fused.kconf.t.data_ptr(), fused.kc.t.data_ptr(),
                                          fused.det.t.data_ptr(), pp.ws_det.data_ptr(), pp.ws_det_bytes, pp.ws_nms.data_ptr(),
                                          pp.ws_nms_bytes, _stream()), "od_detect_soft")
            torch.cuda.synchronize()
            assert np.array_equal(keys.numpy("keys"), ref_keys.cpu().numpy())
            # the split route on the candidates just produced, with a workspace of its own
            _lib.check(lib.od_soft_nms(h, boxes.t.data_ptr(), keys.t.data_ptr(), counts.t.data_ptr(), B, P, NC, K, C.byref(cfg),
                                       split.kf.t.data_ptr(), split.kconf.t.data_ptr(), split.kc.t.data_ptr(),
                                       split.det.t.data_ptr(), ws2.data_ptr(), pp.ws_nms_bytes, _stream()), "od_soft_nms")
            torch.cuda.synchronize()
            for a, b, what in zip(fused.read(), split.read(), ("keep_flat", "keep_conf", "keep_count", "det")):
                assert np.array_equal(a, b), (method, what)
            if method == "hard":
                assert np.array_equal(fused.kf.numpy(), ref_kf.cpu().numpy()) and np.array_equal(fused.kc.numpy(), ref_kc.cpu().numpy())
            pp.run(pt, thr)  # od_detect on the workspaces od_detect_soft left behind
            torch.cuda.synchronize()
            assert torch.equal(pp.keep_flat, ref_kf) and torch.equal(pp.keep_count, ref_kc) and torch.equal(pp.keys, ref_keys)
    n = counts.numpy("counts")
    assert (n == 0).all() if mode == "none" else (n > 0).all()


# ---- (d) the merged variants ------------------------------------------------------------------------------------------------
def _check_block(out, src, kc, b, ref, max_det, what):
    n = len(ref["cls"])
    assert int(kc[b]) == n and int(out[b, :1].view(np.int32)[0]) == n, (what, b, int(kc[b]), n)
    rec = out[b, 1:].reshape(max_det, 6).view(np.uint32)
    assert np.array_equal(src[b, :n], ref["src"]), (what, b)
    assert np.array_equal(rec[:n, 0].view(np.int32), ref["cls"]), (what, b)
    assert np.array_equal(rec[:n, 1], ref["conf_bits"]), (what, b)
    assert np.array_equal(rec[:n, 2:6], ref["boxes"].view(np.uint32)), (what, b)
    assert (rec[n:, 0].view(np.int32) == -1).all() and (rec[n:, 1:] == 0).all() and (src[b, n:] == -1).all(), (what, b)
    return n


@pytest.mark.parametrize("vote_iou", [0.0, 0.5])
@pytest.mark.parametrize("method", list(R.METHODS))
def test_tta_merge_soft_equals_reference(cuda, method, vote_iou):
    """V = 2, one view flipped, B = 2, K = 128, strict 0 and 1; method = hard equals od_tta_merge word for word."""
    _lib, lib, h = _ctx(cuda)
    B, K, NC, P, V, max_det = 2, 128, 20, 4200, 2, 200
    rng = np.random.default_rng(L.seed_of("tta_soft"))
    views = [_make_view(rng, B, K, P, NC, [K, 70 + v], quantise=(v == 0)) + (P, v) for v in range(V)]
    dev = [(_poisoned(k, cuda), _poisoned(c, cuda), _poisoned(bx, cuda)) for k, c, bx, _, _ in views]
    desc = (_lib.TtaView * V)()
    for v, (k, c, bx) in enumerate(dev):
        desc[v] = _lib.TtaView(k.data_ptr(), c.data_ptr(), bx.data_ptr(), P, views[v][4])
    ws_bytes = lib.od_tta_merge_workspace_bytes(B, V, K)
    ws = L.Guarded((ws_bytes,), torch.uint8, cuda)
    out, out_h = L.Guarded((B, 1 + 6 * max_det), torch.float32, cuda), L.Guarded((B, 1 + 6 * max_det), torch.float32, cuda)
    src, src_h = L.Guarded((B, max_det, 2), torch.int32, cuda), L.Guarded((B, max_det, 2), torch.int32, cuda)
    kc, kc_h = L.Guarded((B,), torch.int32, cuda), L.Guarded((B,), torch.int32, cuda)
    for strict in (0, 1):
        cfg = _cfg(_lib, method, strict, max_det, thr=0.45, min_conf=0.011)
        reps = []
        for rep in range(2):
            ws.t.fill_((0xFF, 0x5A)[rep])
            out.t.fill_(float("nan")), src.t.fill_(12345), kc.t.fill_(-9)
            _lib.check(lib.od_tta_merge_soft(h, desc, V, B, NC, K, C.byref(cfg), float(vote_iou), out.t.data_ptr(),
                                             src.t.data_ptr(), kc.t.data_ptr(), ws.t.data_ptr(), ws_bytes, _stream()),
                       "od_tta_merge_soft")
            torch.cuda.synchronize()
            ws.check("workspace")
            reps.append((out.numpy("out").view(np.uint32), src.numpy("src"), kc.numpy("keep_count")))
        assert all(np.array_equal(a, b) for a, b in zip(*reps)), "two calls differ"
        o, s, n = out.numpy(), src.numpy(), kc.numpy()
        kept = []
        for b in range(B):
            views_np = [{"keys": k[b], "count": int(c[b]), "boxes": bx[b], "flip": bool(fl)} for k, c, bx, _, fl in views]
            ref = R.merge_cands(tta_ref.candidates(views_np, NC), K, R.METHODS[method], 0.45, bool(strict), max_det, vote_iou,
                                SIGMA, 0.011)
            kept.append(_check_block(o, s, n, b, ref, max_det, (method, strict)))
        assert 0 < sum(kept) < B * K
        if method == "hard":
            _lib.check(lib.od_tta_merge(h, desc, V, B, NC, K, 0.45, strict, max_det, float(vote_iou), out_h.t.data_ptr(),
                                        src_h.t.data_ptr(), kc_h.t.data_ptr(), ws.t.data_ptr(), ws_bytes, _stream()), "od_tta_merge")
            torch.cuda.synchronize()
            assert np.array_equal(out_h.numpy().view(np.uint32), reps[0][0]) and np.array_equal(src_h.numpy(), s)
            assert np.array_equal(kc_h.numpy(), n)


@pytest.mark.parametrize("vote_iou", [0.0, 0.5])
@pytest.mark.parametrize("method", list(R.METHODS))
def test_slice_merge_soft_equals_reference(cuda, method, vote_iou):
    """G = 2 images of T = 5 tiles (2 x 2 + the full view), K = 128; method = hard equals od_slice_merge word for word."""
    from object_detector_amd import slicing
    _lib, lib, h = _ctx(cuda)
    G, K, NC, P, max_det = 2, 128, 20, 4200, 200
    grid = slicing.SliceGrid(2, 2, 0.2, True, 0.01)
    T = grid.T
    assert T == 5
    rng = np.random.default_rng(L.seed_of("slice_soft"))
    keys, counts = np.zeros((G * T, K), np.uint64), np.zeros(G * T, np.int32)
    boxes, tiles, edge = np.zeros((G * T, P, 4), F), np.zeros((G * T, 4), F), np.zeros(G * T, np.int32)
    sizes = [(640, 480), (677, 491)]
    for g, (w, hh) in enumerate(sizes):
        r = grid.rects(w, hh)
        tiles[g * T:(g + 1) * T], edge[g * T:(g + 1) * T] = slicing.affine(r, w, hh), slicing.edges(r, w, hh)
        for t in range(T):
            row = g * T + t
            counts[row] = K if t == 0 else int(rng.integers(1, K + 1))
            keys[row], boxes[row] = slice_ref.make_row(rng, K, P, NC, int(counts[row]), quantise=(t % 2 == 0))
    lo, hi = grid.edge_lo_hi
    kt, ct, bt = _poisoned(keys, cuda), _poisoned(counts, cuda), _poisoned(boxes, cuda)
    tt, et = _poisoned(tiles, cuda), _poisoned(edge, cuda)
    ws_bytes = lib.od_slice_merge_workspace_bytes(G, T, K)
    ws = L.Guarded((ws_bytes,), torch.uint8, cuda)
    out, out_h = L.Guarded((G, 1 + 6 * max_det), torch.float32, cuda), L.Guarded((G, 1 + 6 * max_det), torch.float32, cuda)
    src, src_h = L.Guarded((G, max_det, 2), torch.int32, cuda), L.Guarded((G, max_det, 2), torch.int32, cuda)
    kc, kc_h = L.Guarded((G,), torch.int32, cuda), L.Guarded((G,), torch.int32, cuda)
    sc = {"T": T, "keys": keys, "counts": counts, "boxes": boxes, "edges": edge, "tiles": tiles}
    cfg = _cfg(_lib, method, 0, max_det, thr=0.45, min_conf=0.011)
    reps = []
    for rep in range(2):
        ws.t.fill_((0xFF, 0x5A)[rep])
        out.t.fill_(float("nan")), src.t.fill_(12345), kc.t.fill_(-9)
        _lib.check(lib.od_slice_merge_soft(h, kt.data_ptr(), ct.data_ptr(), bt.data_ptr(), tt.data_ptr(), et.data_ptr(), G, T, P,
                                           NC, K, lo, hi, C.byref(cfg), float(vote_iou), out.t.data_ptr(), src.t.data_ptr(),
                                           kc.t.data_ptr(), ws.t.data_ptr(), ws_bytes, _stream()), "od_slice_merge_soft")
        torch.cuda.synchronize()
        ws.check("workspace")
        reps.append((out.numpy("out").view(np.uint32), src.numpy("src"), kc.numpy("keep_count")))
    assert all(np.array_equal(a, b) for a, b in zip(*reps)), "two calls differ"
    o, s, n = out.numpy(), src.numpy(), kc.numpy()
    kept = []
    for g in range(G):
        lists, e, aff = slice_ref.image_lists(sc, g)
        cands, _ = slice_ref.candidates(lists, NC, e, aff, lo, hi)
        ref = R.merge_cands(cands, K, R.METHODS[method], 0.45, False, max_det, vote_iou, SIGMA, 0.011)
        kept.append(_check_block(o, s, n, g, ref, max_det, method))
    assert 0 < sum(kept) < G * K
    if method == "hard":
        _lib.check(lib.od_slice_merge(h, kt.data_ptr(), ct.data_ptr(), bt.data_ptr(), tt.data_ptr(), et.data_ptr(), G, T, P, NC, K,
                                      lo, hi, 0.45, 0, max_det, float(vote_iou), out_h.t.data_ptr(), src_h.t.data_ptr(),
                                      kc_h.t.data_ptr(), ws.t.data_ptr(), ws_bytes, _stream()), "od_slice_merge")
        torch.cuda.synchronize()
        assert np.array_equal(out_h.numpy().view(np.uint32), reps[0][0]) and np.array_equal(src_h.numpy(), s)
        assert np.array_equal(kc_h.numpy(), n)


# ---- (e) end to end -------------------------------------------------------------------------------------------------------
E2E_THR = 0.01


def test_detector_soft_linear_end_to_end(cuda):
    """predict_batch_device, submit / collect and predict() (both image routes) agree with each other and with the reference
    applied to the device's own candidates; nms="hard" is the detector built without the argument."""
    from object_detector_amd.detector import ObjectDetector
    B, S = 4, 96
    x = onet.synthetic_images(B, S, seed=0)
    xt = torch.from_numpy(x).to(cuda)
    od = ObjectDetector.synthetic(batch_size=B, input_size=(S, S), seed=2, device=cuda, nms="soft-linear")
    post = od.post
    kf, kc = od.predict_batch_device(xt, conf_threshold=E2E_THR)
    torch.cuda.synchronize()
    kf, kc = kf.cpu().numpy().copy(), kc.cpu().numpy().copy()
    kconf, det = post.keep_conf.cpu().numpy().view(np.uint32).copy(), post.det.cpu().numpy().view(np.uint32).copy()
    keys, counts, boxes = post.keys.cpu().numpy().view(np.uint64), post.counts.cpu().numpy(), post.boxes.cpu().numpy()
    assert int(counts.sum()) > 0 and int(kc.sum()) > 0
    want = _expect(boxes, keys, counts, od.num_classes, "linear", post.strict, post.max_det, thr=post.iou_threshold,
                   sigma=post.soft_sigma, min_conf=E2E_THR)
    for g, w, what in zip((kf, kconf, kc, det), want, ("keep_flat", "keep_conf", "keep_count", "det")):
        assert np.array_equal(g, w), what
    k2, c2 = od.collect(od.submit(xt, conf_threshold=E2E_THR, gather=True))
    assert np.array_equal(k2.cpu().numpy(), kf) and np.array_equal(c2.cpu().numpy(), kc)
    imgs = [x[b] for b in range(B)] + [x[0]]  # a second, partial batch
    host = od.predict(imgs, conf_threshold=E2E_THR, image_decode="host")
    devr = od.predict(imgs, conf_threshold=E2E_THR, image_decode="device")
    assert len(host) == len(devr) == B + 1
    for i, (a, d) in enumerate(zip(host, devr)):
        b, n = i % B, int(kc[i % B])
        rec = det[b, 1:1 + 6 * n].reshape(n, 6)
        for pr in (a, d):
            assert np.array_equal(pr.flat_indices, kf[b, :n]) and np.array_equal(pr.classes, kf[b, :n] % od.num_classes), i
            assert np.array_equal(pr.confs.view(np.uint32), rec[:, 1]), i
            assert np.array_equal(pr.bboxes.view(np.uint32), np.ascontiguousarray(rec[:, 2:6])), i
    od.close_decode_pool()
    # the three-call path goes through od_soft_nms: same kept list
    od.synchronize()
    post.run_unfused(od.net.forward(xt), E2E_THR)
    torch.cuda.synchronize()
    assert np.array_equal(post.keep_flat.cpu().numpy(), kf) and np.array_equal(post.keep_conf.cpu().numpy().view(np.uint32), kconf)

    plain = ObjectDetector.synthetic(batch_size=B, input_size=(S, S), seed=2, device=cuda)
    hard = ObjectDetector.synthetic(batch_size=B, input_size=(S, S), seed=2, device=cuda, nms="hard")
    assert hard.post.keep_conf is None and not hard.post.soft
    a, b = plain.predict_batch_device(xt, conf_threshold=E2E_THR), hard.predict_batch_device(xt, conf_threshold=E2E_THR)
    torch.cuda.synchronize()
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and int(a[1].sum()) > 0
    pa, pb = plain.predict(imgs, conf_threshold=E2E_THR), hard.predict(imgs, conf_threshold=E2E_THR)
    for u, v in zip(pa, pb):
        assert np.array_equal(u.flat_indices, v.flat_indices) and np.array_equal(u.confs.view(np.uint32), v.confs.view(np.uint32))
        assert np.array_equal(u.bboxes.view(np.uint32), v.bboxes.view(np.uint32))


def test_detector_soft_linear_with_flip_tta(cuda):
    from object_detector_amd.detector import ObjectDetector
    B, S = 4, 96
    x = onet.synthetic_images(B, S, seed=0)
    xt = torch.from_numpy(x).to(cuda)
    od = ObjectDetector.synthetic(batch_size=B, input_size=(S, S), seed=2, device=cuda, nms="soft-linear", tta=("flip",))
    det, kcount = od.predict_batch_device(xt, conf_threshold=E2E_THR)
    torch.cuda.synchronize()
    tta, post = od._pipes[0].tta, od.post
    det, kcount, src = det.cpu().numpy().copy(), kcount.cpu().numpy().copy(), tta.src.cpu().numpy().copy()
    cand = [(tta.keys[v].cpu().numpy().view(np.uint64), tta.counts[v].cpu().numpy(), tta.boxes[v].cpu().numpy()) for v in range(2)]
    assert int(kcount.sum()) > 0
    for b in range(B):
        views_np = [{"keys": cand[v][0][b], "count": int(cand[v][1][b]), "boxes": cand[v][2][b], "flip": v == 1} for v in range(2)]
        ref = R.merge_cands(tta_ref.candidates(views_np, od.num_classes), post.K, R.LINEAR, post.iou_threshold, bool(post.strict),
                            post.max_det, od.tta_vote_iou, post.soft_sigma, E2E_THR)
        _check_block(det, src, kcount, b, ref, post.max_det, "tta")
    d2, k2 = od.collect(od.submit(xt, conf_threshold=E2E_THR))
    assert np.array_equal(d2.cpu().numpy().view(np.uint32), det.view(np.uint32)) and np.array_equal(k2.cpu().numpy(), kcount)
    imgs = [x[b] for b in range(B)]
    for route in ("host", "device"):
        for b, pr in enumerate(od.predict(imgs, conf_threshold=E2E_THR, image_decode=route)):
            n = int(kcount[b])
            rec = det[b, 1:1 + 6 * n].reshape(n, 6)
            assert pr.flat_indices is None and np.array_equal(pr.classes, rec[:, 0].copy().view(np.int32))
            assert np.array_equal(pr.confs.view(np.uint32), rec[:, 1].copy().view(np.uint32))
            assert np.array_equal(pr.bboxes.view(np.uint32), np.ascontiguousarray(rec[:, 2:6]).view(np.uint32))
    od.close_decode_pool()


def test_detector_soft_linear_with_slices(cuda):
    """slices=(2, 2) without the full view: T = 4 tiles fill the batch of 4, one image per batch."""
    from object_detector_amd import slicing
    from object_detector_amd.detector import ObjectDetector
    B, S = 4, 96
    od = ObjectDetector.synthetic(batch_size=B, input_size=(S, S), seed=2, device=cuda, nms="soft-linear", slices=(2, 2),
                                  slice_full_view=False, n_inflight=1)
    grid, p = od.slices, od._pipes[0]
    slc, post = p.slc, p.post
    assert grid.T == 4 and slc.G == 1
    img = np.random.default_rng(7).integers(0, 256, (150, 200, 3), dtype=np.uint8)
    lo, hi = grid.edge_lo_hi
    results = {}
    for route in ("host", "device"):
        (pr,) = od.predict([img], conf_threshold=E2E_THR, image_decode=route)
        od.synchronize()
        keys, counts, boxes = slc.keys.cpu().numpy().view(np.uint64), slc.counts.cpu().numpy(), slc.boxes.cpu().numpy()
        r = grid.rects(200, 150)
        lists = [{"keys": keys[q], "count": int(counts[q]), "boxes": boxes[q]} for q in range(4)]
        cands, _ = slice_ref.candidates(lists, od.num_classes, slicing.edges(r, 200, 150), slicing.affine(r, 200, 150), lo, hi)
        ref = R.merge_cands(cands, post.K, R.LINEAR, post.iou_threshold, bool(post.strict), post.max_det, od.slice_vote_iou,
                            post.soft_sigma, E2E_THR)
        n = _check_block(slc.det.cpu().numpy(), slc.src.cpu().numpy(), slc.keep_count.cpu().numpy(), 0, ref, post.max_det, route)
        assert n > 0 and pr.flat_indices is None
        assert np.array_equal(pr.classes, ref["cls"]) and np.array_equal(pr.confs.view(np.uint32), ref["conf_bits"])
        assert np.array_equal(pr.bboxes.view(np.uint32), ref["boxes"].view(np.uint32))
        results[route] = pr
    assert np.array_equal(results["host"].confs.view(np.uint32), results["device"].confs.view(np.uint32))
    od.close_decode_pool()
