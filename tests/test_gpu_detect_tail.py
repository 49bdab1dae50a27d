"""GPU: od_detect's per-image tail kernel (refine + sort + gather + greedy suppression in one launch, the candidates never
leaving LDS) and its pass 1 (odd LDS row pitch, compile-time NC = 20, load width chosen by the block's address), bit for bit
against the three-call path od_head_postprocess -> od_topk_scores -> od_nms and against oracle/nms.py fed the device's keys and
boxes.  Nothing here has a tolerance."""
import numpy as np
import pytest
import torch

from oracle import nms as onms

pytestmark = pytest.mark.gpu

F = np.float32
IOU = 0.45

# (B, P, NC, K): every NC x K pair; B in {1, 3} and P in {510, 2100} alternate so that every (B, P) pair meets every NC.
# 510 % 4 == 2: with odd C = NC + 6 (NC = 1, 21) the rows of image 1 start 8 bytes off a 16-byte boundary.  NC = 20 runs the
# compile-time pass 1, NC = 80 the streamed kernels of detect_wide.hip (whose suppression stays a launch of its own).
SHAPES = [(3, 510, 1, 64), (1, 2100, 1, 1000), (3, 2100, 1, 1024),
          (1, 510, 20, 64), (3, 2100, 20, 1000), (3, 510, 20, 1024), (1, 2100, 20, 1024),
          (3, 510, 21, 64), (3, 510, 21, 1000), (1, 2100, 21, 1024),
          (3, 2100, 76, 64), (1, 510, 76, 1000), (3, 510, 76, 1024),
          (1, 2100, 80, 64), (3, 510, 80, 1000), (3, 2100, 80, 1024)]
REGIMES = ["random", "all_equal", "fewer_than_k", "none", "one", "sixty_five", "overlap", "disjoint"]


def _random_priors(rng, P):
    ctr = rng.uniform(0.1, 0.9, (P, 2)).astype(F)
    wh = rng.uniform(0.05, 0.3, (P, 2)).astype(F)
    return np.concatenate([ctr - wh / 2, ctr + wh / 2], 1).astype(F)


def _grid_priors(P):
    """P boxes that share no area: cell (r, c) of a g x g grid holds a box of 0.8 of the cell."""
    g = int(np.ceil(np.sqrt(P)))
    r, c = np.divmod(np.arange(P), g)
    x1, y1 = (c + 0.1) / g, (r + 0.1) / g
    return np.stack([x1, y1, x1 + 0.8 / g, y1 + 0.8 / g], 1).astype(F)


def _hot(pred, rng, b, priors_idx, classes):
    """Exactly one score above any sensible threshold for each listed prior: objectness 0.88..0.998 (distinct), the class
    probability of `classes` 1 - NC e^-24, every other class e^-24."""
    m = len(priors_idx)
    d = rng.uniform(2, 6, m).astype(F)
    pred[b, priors_idx, 0], pred[b, priors_idx, 1] = -d / 2, d / 2
    pred[b, priors_idx, 2 + classes] = 12.0


def _case(regime, rng, B, P, NC, K):
    """-> priors [P,4], pred [B,P,NC+6], threshold, the number of scores above it per image (None = not pinned)."""
    priors = _random_priors(rng, P)
    pred = rng.normal(0, 2, (B, P, NC + 6)).astype(F)
    if regime == "random":
        return priors, pred, 0.01, None
    if regime == "all_equal":  # every score = 0.5 / NC: one histogram bin holds all P * NC of them, the index decides
        pred[...] = 0.0
        return priors, pred, 0.25 / NC, P * NC
    # a dead background (objectness e^-40, class logits -12, zero offsets) and m live priors with one live class each
    pred[..., 0], pred[..., 1] = 20.0, -20.0
    pred[..., 2:2 + NC] = -12.0
    pred[..., 2 + NC:] = 0.0
    m = {"fewer_than_k": min(K, P) // 2, "none": 0, "one": 1, "sixty_five": 65, "overlap": min(P, K + 50),
         "disjoint": min(P, K + 50)}[regime]
    if regime == "overlap":  # one class, every box the same box moved by a few per cent of its size
        ctr = (0.5 + rng.uniform(-0.01, 0.01, (P, 2))).astype(F)
        priors = np.concatenate([ctr - F(0.15), ctr + F(0.15)], 1).astype(F)
    if regime == "disjoint":
        priors = _grid_priors(P)
    for b in range(B):
        idx = rng.choice(P, m, replace=False)
        cls = np.zeros(m, np.int64) if regime == "overlap" else rng.integers(0, NC, m)
        _hot(pred, rng, b, idx, cls)
    return priors, pred, 0.05, m


def _key_sets(keys, counts):
    k = keys.cpu().numpy().view(np.uint64)
    return [np.sort(k[b][k[b] != 0])[::-1] for b in range(k.shape[0])], counts.cpu().numpy()


def _check_against_three_calls(pp, pt, thr, B, NC, K, max_det, strict):
    """One od_detect call against the three-call path and oracle/nms.py; returns (counts, keep_count) as numpy."""
    kf0, kc0 = pp.run_unfused(pt, thr)
    torch.cuda.synchronize()
    ref_keys, ref_counts = _key_sets(pp.keys, pp.counts)
    kf0, kc0, boxes0 = kf0.clone(), kc0.clone(), pp.boxes.clone()
    pp.keys.fill_(-1), pp.counts.fill_(-7), pp.keep_flat.fill_(-9), pp.keep_count.fill_(-9), pp.boxes.fill_(7.0)
    kf, kc = pp.run(pt, thr)
    torch.cuda.synchronize()
    assert torch.equal(pp.boxes, boxes0)
    got_keys, got_counts = _key_sets(pp.keys, pp.counts)
    assert np.array_equal(got_counts, ref_counts), (got_counts, ref_counts)
    raw = pp.keys.cpu().numpy().view(np.uint64)
    boxes = pp.boxes.cpu().numpy()
    for b in range(B):
        n = int(got_counts[b])
        assert np.array_equal(got_keys[b], ref_keys[b]), b
        # od_detect's keys are sorted: (conf desc, flat asc), unused slots 0
        assert np.array_equal(raw[b, :n], ref_keys[b]) and (raw[b, n:] == 0).all(), b
        ref = onms.nms_image(boxes[b], raw[b, :n], NC, IOU, bool(strict), max_det)
        assert int(kc[b]) == len(ref), (b, int(kc[b]), len(ref))
        assert np.array_equal(kf[b, :len(ref)].cpu().numpy(), np.asarray(ref, np.int32)), b
    assert torch.equal(kc, kc0) and torch.equal(kf, kf0)
    return got_counts, kc.cpu().numpy()


@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("B,P,NC,K", SHAPES, ids=lambda v: str(v))
def test_detect_tail_equals_the_three_call_path(cuda, B, P, NC, K, regime):
    """boxes, keys, counts, keep_flat, keep_count of od_detect == the three-call path's, and the kept indices == oracle/nms.py's
    on the device's sorted keys and boxes, for max_det in {K, 10} and class-aware / strict suppression, over the score regimes:
    random logits; all scores equal (the workgroup-local candidate list overflows, the d0 bin holds everything); fewer than K
    scores above the threshold (d0 < 0, and n < 64 at K = 64); none (n = 0); exactly one; 65 (a second block of 64 columns);
    K + 50 heavily overlapping boxes of one class (most rows suppress something, one is kept); K + 50 disjoint boxes (every row
    kept: with max_det = K = 1000 / 1024 and P = 2100 the kept list grows to K and all 16 column blocks are walked, and with
    max_det = 10 the walk stops inside the first)."""
    from object_detector_amd.postprocess import Postprocessor
    rng = np.random.default_rng(P * 100000 + NC * 1000 + K + 7 * REGIMES.index(regime))
    priors, pred, thr, m = _case(regime, rng, B, P, NC, K)
    pt = torch.from_numpy(pred).to(cuda)
    for strict in (False, True):
        for max_det in (K, 10):
            pp = Postprocessor(B, P, NC, priors, device=cuda, topk=K, max_det=max_det, iou_threshold=IOU, strict_nms=strict)
            assert pp.fused
            counts, kept = _check_against_three_calls(pp, pt, thr, B, NC, K, max_det, strict)
            if m is not None:
                assert (counts == min(m, K)).all(), (regime, counts)
            n = int(counts.min())
            if regime == "disjoint":
                assert (kept == min(n, max_det)).all(), kept
            if regime == "overlap" and max_det == K:
                assert (kept < counts // 2).all(), (kept, counts)
            if regime == "none":
                assert (kept == 0).all() and bool((pp.keep_flat == -1).all())


@pytest.mark.parametrize("B,P,NC,K", [(3, 510, 21, 1000), (3, 2100, 20, 1024), (1, 2100, 1, 64)], ids=lambda v: str(v))
def test_od_nms_keeps_what_the_tail_keeps(cuda, B, P, NC, K):
    """od_nms (sort, then the suppression from the workspace: two launches) on the keys, counts and boxes od_detect left behind
    returns the kept indices od_detect's tail returned: the suppression is one piece of code in both."""
    from object_detector_amd.postprocess import Postprocessor
    rng = np.random.default_rng(K + NC)
    for regime in ("random", "overlap", "sixty_five"):
        priors, pred, thr, _ = _case(regime, rng, B, P, NC, K)
        for strict in (False, True):
            pp = Postprocessor(B, P, NC, priors, device=cuda, topk=K, max_det=min(K, 200), iou_threshold=IOU, strict_nms=strict)
            kf, kc = pp.run(torch.from_numpy(pred).to(cuda), thr)
            torch.cuda.synchronize()
            kf, kc = kf.clone(), kc.clone()
            keys, counts = pp.keys.clone(), pp.counts.clone()
            pp.keep_flat.fill_(-9), pp.keep_count.fill_(-9)
            kf2, kc2 = pp.nms(pp.boxes, keys, counts)
            torch.cuda.synchronize()
            assert torch.equal(kc2, kc) and torch.equal(kf2, kf), (regime, strict)


@pytest.mark.parametrize("B,P,NC,K", [(3, 510, 21, 1000), (3, 2100, 20, 1024), (1, 510, 80, 64)], ids=lambda v: str(v))
def test_detect_candidates_returns_what_detect_leaves(cuda, B, P, NC, K):
    """od_detect_candidates (pass 1, pass 2, od_detect_refine_sort) returns the boxes, keys and counts od_detect (pass 1, pass 2,
    the tail) left, and od_detect after it the same kept indices as before it: either leaves the workspaces ready for the other."""
    from object_detector_amd import _lib
    from object_detector_amd.postprocess import Postprocessor
    rng = np.random.default_rng(K * NC)
    for regime in ("random", "all_equal", "fewer_than_k", "none"):
        priors, pred, thr, _ = _case(regime, rng, B, P, NC, K)
        pp = Postprocessor(B, P, NC, priors, device=cuda, topk=K, max_det=min(K, 200), iou_threshold=IOU)
        pt = torch.from_numpy(pred).to(cuda)
        kf, kc = pp.run(pt, thr)
        torch.cuda.synchronize()
        ref = [t.clone() for t in (pp.boxes, pp.keys, pp.counts, kf, kc)]
        boxes, keys, counts = torch.full_like(pp.boxes, 7.0), torch.full_like(pp.keys, -1), torch.full_like(pp.counts, -7)
        stream = torch.cuda.current_stream(torch.device(cuda)).cuda_stream
        _lib.check(pp.lib.od_detect_candidates(pp.ctx.handle, pt.data_ptr(), pp.priors.data_ptr(), B, P, NC, pp.loc_scale, 1,
                                               float(thr), K, boxes.data_ptr(), None, keys.data_ptr(), counts.data_ptr(),
                                               pp.ws_det.data_ptr(), pp.ws_det_bytes, pp.ws_nms.data_ptr(), pp.ws_nms_bytes,
                                               stream), "od_detect_candidates")
        torch.cuda.synchronize()
        assert torch.equal(boxes, ref[0]) and torch.equal(keys, ref[1]) and torch.equal(counts, ref[2]), regime
        pp.keep_flat.fill_(-9), pp.keep_count.fill_(-9)
        kf, kc = pp.run(pt, thr)
        torch.cuda.synchronize()
        assert torch.equal(pp.keys, ref[1]) and torch.equal(pp.counts, ref[2]) and torch.equal(kf, ref[3]) and torch.equal(kc, ref[4])
