"""CPU: the numpy reference of od_tta_merge (tests/tta_ref.py) against oracle.nms, its merged order on hand-made ties, the
mirror, and the validation of ObjectDetector's tta= argument.  No kernel runs here."""
import numpy as np
import pytest

import tta_ref
from oracle import nms as onms

F = np.float32


def _boxes(rng, P):
    c = rng.uniform(0.1, 0.9, (P, 2)).astype(F)
    wh = rng.uniform(0.02, 0.25, (P, 2)).astype(F)
    return np.clip(np.concatenate([c - wh, c + wh], 1), 0, 1).astype(F)


def _key(conf, flat):
    return (np.uint64(np.array([conf], F).view(np.uint32)[0]) << np.uint64(32)) | np.uint64(0xFFFFFFFF - flat)


@pytest.mark.parametrize("strict", [False, True])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_single_view_without_voting_is_oracle_nms(seed, strict):
    rng = np.random.default_rng(seed)
    P, NC, K = 300, 5, 256
    boxes = _boxes(rng, P)
    cluster = rng.integers(0, 12, P)  # crowd the boxes so that suppression happens
    boxes = (boxes[cluster] + rng.normal(0, 0.01, (P, 4))).astype(F)
    boxes = np.clip(np.concatenate([np.minimum(boxes[:, :2], boxes[:, 2:]), np.maximum(boxes[:, :2], boxes[:, 2:])], 1), 0, 1)
    conf = rng.uniform(0, 1, (P, NC)).astype(F) ** 3
    keys = onms.topk_keys(conf.reshape(-1), K, 0.2)
    want = onms.nms_image(boxes, keys, NC, 0.45, strict, 50)
    assert 0 < len(want) < len(keys)
    got = tta_ref.merge_image([{"keys": keys, "count": len(keys), "boxes": boxes, "flip": False}], NC, K, 0.45, strict, 50,
                              vote_iou=0.0)
    assert (got["src"][:, 0] == 0).all()
    assert np.array_equal(got["src"][:, 1], want)
    assert np.array_equal(got["cls"], want % NC)
    assert np.array_equal(got["conf_bits"], conf.reshape(-1)[want].view(np.uint32))
    assert np.array_equal(got["boxes"].view(np.uint32), boxes[want // NC].view(np.uint32))


def test_merged_order_breaks_ties_by_view_then_flat():
    NC = 4
    boxes = np.zeros((8, 4), F)
    # equal confidences everywhere: within a view a list is (conf desc, flat asc), across views the lower view goes first
    v0 = [_key(0.5, 9), _key(0.5, 12), _key(0.25, 3)]
    v1 = [_key(0.75, 30), _key(0.5, 2), _key(0.5, 12), _key(0.25, 1)]
    v2 = [_key(0.5, 0)]
    views = [{"keys": np.array(k, np.uint64), "count": len(k), "boxes": boxes, "flip": False} for k in (v0, v1, v2)]
    order = [(v, flat) for _, v, flat, _, _ in tta_ref.merged_order(tta_ref.candidates(views, NC), 64)]
    assert order == [(1, 30), (0, 9), (0, 12), (1, 2), (1, 12), (2, 0), (0, 3), (1, 1)]
    # K cuts the merged list, not the single lists
    assert [(v, f) for _, v, f, _, _ in tta_ref.merged_order(tta_ref.candidates(views, NC), 4)] == order[:4]
    # a count below the list length hides the tail of that view
    views[1]["count"] = 1
    order = [(v, flat) for _, v, flat, _, _ in tta_ref.merged_order(tta_ref.candidates(views, NC), 64)]
    assert order == [(1, 30), (0, 9), (0, 12), (2, 0), (0, 3)]


def test_mirroring_twice_is_within_one_rounding():
    rng = np.random.default_rng(5)
    boxes = _boxes(rng, 4096)
    for b in boxes:
        m = tta_ref.mirror_box(b)
        assert m[1] == b[1] and m[3] == b[3] and m[0] <= m[2]
        back = tta_ref.mirror_box(m)
        # each of the two subtractions rounds by at most half an ulp of a value in [0, 1] (2^-25)
        assert np.all(np.abs(back.astype(np.float64) - b.astype(np.float64)) <= 2.0 ** -24)
    x = np.array([0.0, 0.25, 1.0, 0.75], F)
    assert np.array_equal(tta_ref.mirror_box(x), np.array([0.0, 0.25, 1.0, 0.75], F))


def test_voting_is_the_confidence_weighted_mean_of_same_class_overlaps():
    NC = 2
    boxes = np.array([[0.10, 0.10, 0.50, 0.50], [0.12, 0.10, 0.52, 0.50], [0.10, 0.10, 0.50, 0.50], [0.7, 0.7, 0.9, 0.9]], F)
    # prior 0 class 0 (kept), prior 1 class 0 (suppressed, votes), prior 2 class 1 (other class: kept, no vote), prior 3 far
    keys = np.array([_key(0.75, 0 * NC), _key(0.5, 1 * NC), _key(0.375, 2 * NC + 1), _key(0.25, 3 * NC)], np.uint64)
    view = {"keys": keys, "count": 4, "boxes": boxes, "flip": False}
    got = tta_ref.merge_image([view], NC, 16, 0.45, False, 10, vote_iou=0.5)
    assert got["src"][:, 1].tolist() == [0, 5, 6]
    w0, w1 = F(0.75), F(0.5)
    want = [F(F(F(0) + F(w0 * boxes[0, k])) + F(w1 * boxes[1, k])) / F(w0 + w1) for k in range(4)]
    assert np.array_equal(got["boxes"][0], np.array(want, F))
    for r, (w, p) in ((1, (F(0.375), 2)), (2, (F(0.25), 3))):  # a lone member: (w * x) / w, the two roundings included
        assert np.array_equal(got["boxes"][r], np.array([F(F(w * boxes[p, k]) / w) for k in range(4)], F))
    assert np.array_equal(got["conf_bits"].view(F), np.array([0.75, 0.375, 0.25], F))
    # voting off: the kept boxes are the original ones
    off = tta_ref.merge_image([view], NC, 16, 0.45, False, 10, vote_iou=0.0)
    assert np.array_equal(off["boxes"], boxes[[0, 2, 3]])


def test_tta_argument_validation():
    from object_detector_amd.detector import ObjectDetector
    from object_detector_amd.tta import normalize_views
    from object_detector_amd import weights as W
    assert normalize_views(None) is None
    assert normalize_views(()) == () and normalize_views([]) == ()
    assert normalize_views(("flip",)) == ("flip",) and normalize_views(["flip"]) == ("flip",)
    for bad in ("flip", ("flop",), ("flip", "scale"), ("flip", "flip"), 1, True, ("flip", None)):
        with pytest.raises(ValueError):
            normalize_views(bad)
        with pytest.raises(ValueError):  # raised before the constructor looks for a GPU
            ObjectDetector(W.random_init(2, 20), 2, (96, 96), tta=bad)
