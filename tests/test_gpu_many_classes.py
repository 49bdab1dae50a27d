"""Class counts beyond the LDS row block of the VOC kernels (NC > 76 for post-processing, NC > 74 for the loss), up to 1024:
the streamed od_detect / od_head_postprocess / od_gather_detections_pred / od_loss_fwd_bwd paths against the three-call path
and the CPU oracle, end to end through ObjectDetector and Trainer at NC = 80, and the limits."""
import numpy as np
import pytest
import torch

from oracle import loss as oloss
from oracle import network as onet
from oracle import nms as onms
from oracle import postprocess as opp
from oracle.compare import assert_logits, logit_stats

pytestmark = pytest.mark.gpu


def _priors(P, rng):
    ctr = rng.uniform(0.1, 0.9, (P, 2)).astype(np.float32)
    wh = rng.uniform(0.05, 0.3, (P, 2)).astype(np.float32)
    return np.concatenate([ctr - wh / 2, ctr + wh / 2], 1).astype(np.float32)


def _sorted_valid(keys, counts):
    k = keys.cpu().numpy().view(np.uint64)
    c = counts.cpu().numpy()
    return [np.sort(k[b][k[b] != 0])[::-1] for b in range(len(c))], c


def _fused_vs_unfused(cuda, pp, pred, thr, K, max_det):
    """run() (od_detect) vs run_unfused() bit for bit, both vs the CPU oracle fed the device's conf / boxes; -> conf, boxes."""
    pt = torch.from_numpy(pred).to(cuda)
    kf0, kc0 = pp.run_unfused(pt, thr)
    torch.cuda.synchronize()
    ref_keys, ref_counts = _sorted_valid(pp.keys, pp.counts)
    kf0, kc0, boxes0 = kf0.clone(), kc0.clone(), pp.boxes.clone()
    pp.keys.zero_(), pp.counts.zero_(), pp.keep_flat.zero_(), pp.keep_count.zero_(), pp.boxes.zero_()
    kf, kc = pp.run(pt, thr)
    torch.cuda.synchronize()
    got_keys, got_counts = _sorted_valid(pp.keys, pp.counts)
    assert (got_counts == ref_counts).all() and all(np.array_equal(a, b) for a, b in zip(got_keys, ref_keys))
    assert torch.equal(kc, kc0) and torch.equal(kf, kf0) and torch.equal(pp.boxes, boxes0)
    conf, boxes = pp.conf.cpu().numpy(), pp.boxes.cpu().numpy()
    for b in range(pp.B):
        r, *_ = onms.detect_image(conf[b], boxes[b], K=K, conf_threshold=thr, iou_threshold=0.45, max_det=max_det)
        assert int(kc[b]) == len(r) and (kf[b, :len(r)].cpu().numpy() == r).all()
    # the record block: confidences recomputed from pred equal the dense tensor's
    pp.gather()
    torch.cuda.synchronize()
    NC = pp.NC
    for b, (flat, cf, bx) in enumerate(pp.detections_host(pp.B)):
        assert np.array_equal(flat, kf[b, :int(kc[b])].cpu().numpy())
        assert np.array_equal(cf, conf[b].reshape(-1)[flat.astype(np.int64)])
        assert np.array_equal(bx, boxes[b][(flat // NC).astype(np.int64)])
    return conf, boxes, kc.cpu().numpy()


def _tied_at_kth(conf, K, thr):
    """(candidates whose score equals the K-th best, slots left for them) of one image's confidences."""
    c = conf.reshape(-1)
    c = np.sort(c[c > thr])[::-1]
    assert len(c) > K
    return int((c == c[K - 1]).sum()), K - int((c > c[K - 1]).sum())


def _ties_pred(rng, B, P, NC):
    """Equal class logits, and the objectness logit drawn from 37 levels: an image has at most 37 distinct confidences
    (obj / NC, as test_topk_exact's "ties"), every row holds NC equal scores, so the flat index decides the top-K."""
    pred = rng.normal(0, 2, (B, P, NC + 6)).astype(np.float32)
    pred[..., :2 + NC] = 0.0
    pred[..., 1] = np.linspace(-1.0, 3.0, 37, dtype=np.float32)[rng.integers(0, 37, (B, P))]
    return pred


# P = 130 / 258 do not fill a workgroup; P = 1030 / 514 / 258 with odd NC give P * (NC + 6) % 4 != 0 (rows 4-byte aligned).
# The "ties" cases have N = P * NC = 2 mod 4 as well (the three-call path's scalar-load passes) and a K-th score shared by more
# candidates than there are slots left, so the radix refine behind those passes has to run down to the index digits.
_RANDOM_CASES = [(77, 300, 1030, 2), (80, 1024, 130, 3), (91, 1, 514, 2), (200, 1024, 2052, 2), (365, 300, 258, 2),
                 (1000, 1024, 600, 2)]
_TIES_CASES = [(91, 300, 514, 2), (77, 300, 1030, 2)]


@pytest.mark.parametrize("NC,K,P,B,ties",
                         [pytest.param(*c, False, id="-".join(map(str, c))) for c in _RANDOM_CASES]
                         + [pytest.param(*c, True, id="-".join(map(str, c)) + "-ties") for c in _TIES_CASES])
def test_detect_many_classes_equals_the_three_call_path(cuda, NC, K, P, B, ties):
    from object_detector_amd.postprocess import Postprocessor
    rng = np.random.default_rng(NC * 1000 + K)
    priors = _priors(P, rng)
    max_det = min(50, K)
    pp = Postprocessor(B, P, NC, priors, device=cuda, topk=K, max_det=max_det)
    assert pp.fused
    if ties:
        pred, thrs = _ties_pred(rng, B, P, NC), (0.0, 0.005)  # scores are obj / NC: 0.0030 .. 0.0124
        assert (P * NC) % 4 == 2
        host_conf, _ = opp.head_postprocess(pred, priors, num_classes=NC)
        for thr in thrs:
            for b in range(B):  # from the inputs alone: the refine loop must run
                tied, slots = _tied_at_kth(host_conf[b], K, thr)
                assert tied > slots > 0, (thr, b, tied, slots)
    else:
        pred, thrs = rng.normal(0, 2, (B, P, NC + 6)).astype(np.float32), (0.0, 0.05)
    for thr in thrs:
        conf, boxes, _ = _fused_vs_unfused(cuda, pp, pred, thr, K, max_det)
    rconf, rboxes = opp.head_postprocess(pred, priors, num_classes=NC)
    assert (boxes == rboxes).all()  # bit-exact decode
    np.testing.assert_allclose(conf, rconf, rtol=2e-6, atol=1e-7)


# the last case: all scores equal with N = P * NC = 2 mod 4 (the scalar-load passes of the three-call path)
@pytest.mark.parametrize("mode,NC,P", [pytest.param("all_equal", 200, 1030, id="all_equal"), pytest.param("few", 200, 1030, id="few"),
                                       pytest.param("none", 200, 1030, id="none"),
                                       pytest.param("all_equal", 91, 514, id="all_equal-91-514")])
def test_detect_many_classes_degenerate(cuda, mode, NC, P):
    from object_detector_amd.postprocess import Postprocessor
    B, K = 2, 1024
    rng = np.random.default_rng(5)
    priors = _priors(P, rng)
    pp = Postprocessor(B, P, NC, priors, device=cuda, topk=K, max_det=200)
    if mode == "all_equal":  # every one of the P * NC scores is the same: the exact top-K is the K lowest flat indices
        pred = np.zeros((B, P, NC + 6), np.float32)
        thr = 0.0
        assert P * NC > K  # more candidates tied at the K-th score than slots: the refine loop must run
    else:  # objectness ~0 everywhere but on three priors; "none": a threshold no score reaches
        pred = rng.normal(0, 2, (B, P, NC + 6)).astype(np.float32)
        pred[:, :, 0], pred[:, :, 1] = 12.0, -12.0
        pred[:, [7, 300, 1029], 0], pred[:, [7, 300, 1029], 1] = -6.0, 6.0
        thr = 0.005 if mode == "few" else 0.999
    conf, _, kc = _fused_vs_unfused(cuda, pp, pred, thr, K, 200)
    n_cand = (conf.reshape(B, -1) > thr).sum(1)
    counts = pp.counts.cpu().numpy()
    if mode == "all_equal":
        assert (counts == K).all()
        keys = pp.keys.cpu().numpy().view(np.uint64)
        assert ((0xFFFFFFFF - (keys & 0xFFFFFFFF)) == np.arange(K)).all()  # flat indices 0..K-1, in order
    elif mode == "few":
        assert (0 < n_cand).all() and (n_cand < K).all() and (counts == n_cand).all()
    else:
        assert (n_cand == 0).all() and (counts == 0).all() and (kc == 0).all()


def test_detect_workspace_is_bounded_by_priors():
    from object_detector_amd import _lib
    lib = _lib.load()
    assert lib.od_detect_workspace_bytes(16, 67200, 1000, 1024) < 256 * 2**20
    assert lib.od_detect_workspace_bytes(16, 67200, 80, 1024) == lib.od_detect_workspace_bytes(16, 67200, 1000, 1024)


@pytest.mark.parametrize("B,S,precision", [(4, 320, None), (2, 640, None), (2, 320, "mixed")], ids=str)
def test_end_to_end_80_classes(cuda, B, S, precision):
    from object_detector_amd.detector import ObjectDetector
    NC = 80
    x = onet.synthetic_images(B, S, seed=0)
    xt = torch.from_numpy(x).to(cuda)
    od = ObjectDetector.synthetic(B, (S, S), seed=2, num_classes=NC, device=cuda, use_multi_gpu=False, precision=precision)
    assert od.num_classes == NC and od.post.fused
    thr = 0.002  # random-init logits spread a prior's probability over 80 classes
    tickets = [od.submit(xt, conf_threshold=thr) for _ in range(3)]
    outs = []
    for t in tickets:
        keep, cnt = od.collect(t)
        p = od._pipes[t]
        outs.append(dict(pred=p.net.pred.cpu().numpy(), conf=p.post.conf.cpu().numpy(), boxes=p.post.boxes.cpu().numpy(),
                         keep=keep.cpu().numpy(), cnt=cnt.cpu().numpy()))
    for o in outs[1:]:
        assert np.array_equal(o["pred"], outs[0]["pred"]) and np.array_equal(o["keep"], outs[0]["keep"])
    o = outs[0]
    assert o["pred"].shape[-1] == NC + 6
    ref32 = onet.Runner(od.params, storage="f32").forward(x, num_classes=NC)
    if precision == "mixed":
        refm = onet.MixedPlan(od.net.stream_stages, od.net.split, od.net.wide_fpn).runner(od.params).forward(x, num_classes=NC)
        rec = logit_stats(o["pred"], refm, ref32)
        assert rec["max_dev_vs_fp32"] <= 1e-3 * rec["logit_scale"], rec
    else:
        ref = onet.Runner(od.params, storage="f16").forward(x, num_classes=NC)
        assert_logits(logit_stats(o["pred"], ref, ref32), f"{B}x{S} NC={NC}")
    for b in range(B):
        r, *_ = onms.detect_image(o["conf"][b], o["boxes"][b], K=1024, conf_threshold=thr, iou_threshold=0.45, max_det=200)
        assert o["cnt"][b] == len(r) and (o["keep"][b, :len(r)] == r).all(), f"image {b}: kept indices differ"
    if precision is None and S == 320:
        preds = od.predict(list(x[:3]), conf_threshold=0.0)
        assert len(preds) == 3
        for pr in preds:
            assert len(pr.classes) > 0 and pr.classes.min() >= 0 and pr.classes.max() < NC


def _shard(B, S, NC, seed):
    from object_detector_amd.pb import ObjectsAnnotation
    rng = np.random.default_rng(seed)
    anns = []
    for _ in range(B):
        n = int(np.clip(1 + rng.poisson(1.5), 1, 10))
        c = rng.uniform(0, 1, (n, 2))
        wh = np.exp(rng.uniform(np.log(0.05), np.log(0.9), (n, 2)))
        anns.append(ObjectsAnnotation(None, S, S, rng.integers(0, NC, n),
                                      np.clip(np.concatenate([c - wh / 2, c + wh / 2], 1), 0, 1).astype(np.float32)))
    return anns


def _rel(a, b):
    return float(np.linalg.norm(a.astype(np.float64) - b) / max(np.linalg.norm(b), 1e-30))


@pytest.mark.parametrize("B,S,NC", [(4, 320, 80), (2, 160, 1000)], ids=str)
def test_training_step_many_classes(cuda, B, S, NC):
    """One step vs the torch-CPU oracle: at NC = 1000 the prediction conv has Cout = 8048 (backward-data and weight-gradient
    launches at that width)."""
    from object_detector_amd import weights as W
    from object_detector_amd.trainer import Trainer
    from oracle.train_ref import TorchDetector
    params = W.random_init(2, NC)
    x = onet.synthetic_images(B, S, seed=0)
    anns = _shard(B, S, NC, seed=1000)
    LS = 1024.0
    tr = Trainer(params, B, (S, S), device=cuda, lr=0.0, momentum=0.9, loss_scale=LS)
    assert tr.num_classes == NC
    y, npos, _ = tr.pb.encode_batch(anns, return_device=True)
    pred = tr.forward(torch.from_numpy(x).to(cuda)).clone()
    losses = tr.loss(y).clone()
    grads = tr.backward().clone()
    torch.cuda.synchronize()
    assert torch.isfinite(grads).all()
    masks = {}
    for n in tr.nodes:  # the device's LeakyReLU sign pattern (as test_gpu_fullsize._device_slope_masks)
        if n.act and n.act[0] == "leaky":
            masks[n.name] = ((n.z.float() * n.scale + n.shift) > 0).cpu().numpy()
    ref = TorchDetector(params, dtype=torch.float32, slope_masks=masks)
    ref_losses, ref_grads, ref_pred = ref.loss_and_grads(x, y.cpu().numpy(), num_classes=NC)
    scale = max(1.0, float(np.abs(ref_pred).max()))
    assert float(np.abs(pred.cpu().numpy() - ref_pred).max()) <= 3e-2 * scale
    np.testing.assert_allclose(losses.cpu().numpy(), ref_losses, rtol=3e-2)
    g = grads.cpu().numpy() / LS
    worst = {f"{name}.{kind}": _rel(g[o:o + n], ref_grads[f"{name}.{kind}"].reshape(-1)) for (name, kind), (o, n) in tr.seg.items()}
    assert any(k.startswith("h.out") for k in worst)
    top = sorted(worst.items(), key=lambda kv: -kv[1])
    print(f"NC={NC}: worst relative gradient errors {top[:4]}")
    assert top[0][1] < 0.01, top[:6]


@pytest.mark.parametrize("NC", [75, 90, 1000])
@pytest.mark.parametrize("box_mode", ["smooth_l1", "mse"])
def test_loss_many_classes(cuda, NC, box_mode):
    from object_detector_amd import ops
    from object_detector_amd.pb import PriorBoxes
    pb = PriorBoxes((160, 160), NC, device=cuda)
    y, npos, _ = pb.encode_batch(_shard(3, 160, NC, seed=NC), return_device=True)
    assert int(npos.sum()) > 0
    pred = np.random.default_rng(4).normal(0, 1.5, tuple(y.shape)).astype(np.float32)
    losses, grad = ops.loss_fwd_bwd(torch.from_numpy(pred).to(cuda), y, NC, box_mode=box_mode)
    torch.cuda.synchronize()
    rl, rg = oloss.loss_and_grad(pred, y.cpu().numpy(), NC, box_mode=box_mode)
    np.testing.assert_allclose(losses.cpu().numpy(), rl, rtol=2e-5)
    np.testing.assert_allclose(grad.cpu().numpy(), rg, rtol=1e-4, atol=1e-8)


def test_fit_80_classes_halves_the_loss(cuda):
    import sys
    import pathlib
    sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent.parent / "scripts"))
    import _common
    import train as train_script
    from object_detector_amd import od_gen, weights as W
    from object_detector_amd.pb import ObjectsAnnotation
    from object_detector_amd.trainer import Trainer
    B, S, NC, STEPS = 16, 160, 80, 100
    X, y = _common.shapes_dataset(64, seed=0)
    y80 = np.empty(len(y), dtype=object)  # the five shape classes (VOC ids 1..14) spread over 0..79
    y80[:] = [ObjectsAnnotation(a.path, a.width, a.height, a.classes * 5 + 7, a.bboxes, a.difficults) for a in y]
    y = y80
    params0 = train_script.init_for_training(W.random_init(2, NC))
    tr = Trainer(params0, B, (S, S), device=cuda, lr=0.02, momentum=0.9, weight_decay=1e-4, lr_multipliers={"h.": 1.0 / 3.0})
    gen = od_gen.create_generator((S, S), preprocess_input=None, encode_truth=tr.pb.encode_truth_device, device=cuda,
                                  on_device=True, device_cache=True)
    batches, _ = gen.flow(X, y, batch_size=B, data_augmentation=True, shuffle=True, seed=0, prefetch=2)
    hist = tr.fit(batches, STEPS, lr_schedule=train_script.cosine_schedule(0.02, STEPS, 20))
    batches.close()
    torch.cuda.synchronize()
    assert np.isfinite(hist).all()
    first, last = float(hist[:3, 3].mean()), float(hist[-10:, 3].mean())
    print(f"NC=80 total loss {first:.3f} -> {last:.3f}")
    assert last * 2.0 <= first, (first, last)


def test_class_count_limits(cuda):
    from object_detector_amd import _lib, ops
    from object_detector_amd.postprocess import Postprocessor
    priors = _priors(64, np.random.default_rng(0))
    with pytest.raises(_lib.OdError, match="1..1024"):
        Postprocessor(1, 64, 1025, priors, device=cuda)
    pp = Postprocessor(1, 64, 1024, priors, device=cuda)  # the largest supported count builds; od_detect itself rejects 1025
    lib = pp.lib
    rc = lib.od_detect(pp.ctx.handle, pp.priors.data_ptr(), pp.priors.data_ptr(), 1, 64, 1025, 0.1, 1, 0.01, pp.K, 0.45, 0,
                       pp.max_det, pp.boxes.data_ptr(), None, pp.keys.data_ptr(), pp.counts.data_ptr(),
                       pp.keep_flat.data_ptr(), pp.keep_count.data_ptr(), pp.ws_det.data_ptr(), pp.ws_det_bytes,
                       pp.ws_nms.data_ptr(), pp.ws_nms_bytes, None)
    with pytest.raises(_lib.OdError, match="1..1024"):
        _lib.check(rc, "od_detect")
    t = torch.zeros((1, 16, 1025 + 6), device=cuda)
    with pytest.raises(_lib.OdError, match="1..1024"):
        ops.loss_fwd_bwd(t, t.clone(), 1025)
