"""Host logic of mosaic augmentation and of ignore regions: the numpy reference of od_assign_anchors_ign against the oracle,
the box bookkeeping of a mosaic on hand-made cases, RNG isolation of the generator, and the argument checks.  No GPU."""
import pathlib
import sys

import numpy as np
import pytest

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))

import assign_ign_ref as aref  # noqa: E402
from oracle import assign as oassign  # noqa: E402
from oracle import postprocess as opp  # noqa: E402


def _ann(boxes, classes=None, difficults=None, wh=(100, 100)):
    from object_detector_amd.pb import ObjectsAnnotation
    boxes = np.asarray(boxes, np.float32).reshape(-1, 4)
    return ObjectsAnnotation(None, wh[0], wh[1], np.arange(len(boxes)) if classes is None else classes, boxes, difficults)


def _aug(crop=(0.0, 0.0, 1.0, 1.0), flip=False):
    from object_detector_amd import od_gen
    p = od_gen.AugParams()
    p.crop, p.flip = crop, flip
    return p


# ---- od_assign_anchors_ign's reference -------------------------------------------------------------------------------

def test_reference_without_flags_is_the_oracle():
    d = np.load(ROOT / "tests" / "golden" / "assign_loss_128.npz")
    pr = opp.make_priors((128, 128))
    for flags in (None, np.zeros(len(d["gt_boxes"]), np.int32)):
        y, a = aref.encode_truth(d["gt_boxes"], d["gt_classes"], pr, 20, flags=flags)
        assert (y == d["y"]).all() and (a == d["assigned"]).all()
    rng = np.random.default_rng(5)
    pr = opp.make_priors((96, 96))
    for n in (0, 1, 3, 9):
        c = rng.uniform(0, 1, (n, 2))
        wh = np.exp(rng.uniform(np.log(0.05), np.log(0.9), (n, 2)))
        b = np.clip(np.concatenate([c - wh / 2, c + wh / 2], 1), 0, 1).astype(np.float32)
        cl = rng.integers(0, 7, n)
        ry, ra = oassign.encode_truth(b, cl, pr, 7)
        y, a = aref.encode_truth(b, cl, pr, 7, flags=None)
        assert y.tobytes() == ry.tobytes() and (a == ra).all()


def test_reference_region_rule_on_a_hand_case():
    pr = opp.make_priors((64, 64))
    boxes = np.array([[0.05, 0.05, 0.45, 0.45], [0.5, 0.5, 1.0, 1.0]], np.float32)
    y0, a0 = aref.encode_truth(boxes, [1, 2], pr, 5)
    y, a = aref.encode_truth(boxes, [1, 2], pr, 5, flags=[0, 1])
    assert not (a == 1).any() and (a0 == 1).any()           # the region owns no prior
    assert ((a == 0) == (a0 == 0)).all()                    # the other box keeps its priors
    cx, cy = (pr[:, 0] + pr[:, 2]) / 2, (pr[:, 1] + pr[:, 3]) / 2
    small_inside = (pr[:, 0] >= 0.5) & (pr[:, 1] >= 0.5) & (pr[:, 2] <= 1.0) & (pr[:, 3] <= 1.0)
    assert small_inside.any() and (a[small_inside] <= -2).all()  # a prior wholly inside: covered 100 % whatever its IoU
    assert (y[a == -3] == 0).all() and (a == -3).any()
    far = (cx < 0.3) & (cy > 0.7) & (pr[:, 2] < 0.45) & (pr[:, 1] > 0.55)
    assert far.any() and (a[far] == -1).all() and (y[far, 0] == 1).all()  # background outside the region stays background
    # a higher threshold ignores fewer priors; positives never change
    _y9, a9 = aref.encode_truth(boxes, [1, 2], pr, 5, flags=[0, 1], ign_thr=0.9)
    assert (a9 == -3).sum() < (a == -3).sum() and ((a9 >= 0) == (a >= 0)).all()


# ---- mosaic box logic ------------------------------------------------------------------------------------------------

def test_tile_mapping_with_and_without_flip():
    from object_detector_amd import od_gen
    anns = [_ann([[0.25, 0.25, 0.75, 0.75]], [3])] * 4
    tiles = [_aug(), _aug(flip=True), _aug(crop=(0.0, 0.0, 0.5, 1.0)), _aug()]
    tiles[3].crop = (0.25, 0.25, 0.75, 0.75)
    m = od_gen.mosaic_boxes(anns, tiles, (40, 60), (100, 200))  # H = 100, W = 200; split_x = 40, split_y = 60
    # TL tile [0,40)x[0,60): the box's corners at a quarter and three quarters of the tile
    np.testing.assert_allclose(m.bboxes[0], [10 / 200, 15 / 100, 30 / 200, 45 / 100], atol=1e-6)
    # TR tile x in [40,200): symmetric box, the flip leaves it where it is
    np.testing.assert_allclose(m.bboxes[1], [(40 + 40) / 200, 15 / 100, (40 + 120) / 200, 45 / 100], atol=1e-6)
    # BL: the crop keeps the left half: x 0.25..0.75 -> 0.5..1.5, clipped to the tile at 1.0: half of the box is visible
    np.testing.assert_allclose(m.bboxes[2], [20 / 200, (60 + 10) / 100, 40 / 200, (60 + 30) / 100], atol=1e-6)
    # BR: the crop is the box: it fills its tile
    np.testing.assert_allclose(m.bboxes[3], [40 / 200, 60 / 100, 1.0, 1.0], atol=1e-6)
    assert list(m.classes) == [3, 3, 3, 3] and not m.difficults.any() and (m.width, m.height) == (200, 100)
    # an asymmetric box under a flip: x mirrors inside the tile
    m = od_gen.mosaic_boxes([_ann([[0.0, 0.0, 0.25, 1.0]])] * 4, [_aug(flip=True)] * 4, (100, 50), (100, 200))
    np.testing.assert_allclose(m.bboxes[0], [75 / 200, 0.0, 100 / 200, 0.5], atol=1e-6)
    np.testing.assert_allclose(m.bboxes[1], [(100 + 75) / 200, 0.0, 1.0, 0.5], atol=1e-6)


def test_keep_ignore_drop_split_and_stats():
    from object_detector_amd import od_gen
    # the crop keeps x in [0, 0.5] of the source; boxes of width 0.2 whose visible share is 100 %, 50 %, 25 %, 5 %, 0 %
    boxes = [[0.1, 0.1, 0.3, 0.9], [0.4, 0.1, 0.6, 0.9], [0.45, 0.1, 0.65, 0.9], [0.49, 0.1, 0.69, 0.9], [0.7, 0.1, 0.9, 0.9]]
    a = _ann(boxes, [0, 1, 2, 3, 4], [False, True, False, False, False])
    empty = _ann(np.zeros((0, 4)))
    tiles = [_aug(crop=(0.0, 0.0, 0.5, 1.0)), _aug(), _aug(), _aug()]
    st = {}
    m = od_gen.mosaic_boxes([a, empty, empty, empty], tiles, (160, 160), (320, 320), ignore_regions=True, stats=st)
    assert list(m.classes) == [0, 1, 2] and list(m.difficults) == [False, True, True]  # input flag carried; sliver flagged
    assert st == {"boxes_dropped": 2, "boxes_ignored": 1}
    st = {}
    m = od_gen.mosaic_boxes([a, empty, empty, empty], tiles, (160, 160), (320, 320), ignore_regions=False, stats=st)
    assert list(m.classes) == [0, 1] and list(m.difficults) == [False, True]  # a sliver is never a positive: dropped
    assert st == {"boxes_dropped": 3, "boxes_ignored": 0}
    assert (m.bboxes >= 0).all() and (m.bboxes <= 1).all()
    # thinner than two output pixels: dropped although it is wholly visible
    thin = _ann([[0.5, 0.1, 0.505, 0.9]])
    st = {}
    m = od_gen.mosaic_boxes([thin, empty, empty, empty], [_aug()] * 4, (160, 160), (320, 320), ignore_regions=True, stats=st)
    assert m.num_objects == 0 and st["boxes_dropped"] == 1
    # an empty tile shows nothing
    m = od_gen.mosaic_boxes([a, a, a, a], [_aug()] * 4, (320, 320), (320, 320), stats=st)
    assert m.num_objects == 5


def test_more_than_gmax_boxes_rule_and_order():
    from object_detector_amd import od_gen
    # 3 boxes per tile, areas distinct; flags on some
    def tile(k):
        w = np.array([0.2, 0.3, 0.4]) + 0.01 * k
        return _ann([[0.1, 0.1, 0.1 + v, 0.1 + v] for v in w], [k * 3, k * 3 + 1, k * 3 + 2], [k == 1, False, k == 2])
    anns = [tile(k) for k in range(4)]
    st = {}
    m = od_gen.mosaic_boxes(anns, [_aug()] * 4, (160, 160), (320, 320), ignore_regions=True, gmax=9, stats=st)
    # 12 boxes, 9 stay: the two flagged ones go first (classes 3 and 8), then the smallest unflagged one (class 0)
    assert list(m.classes) == [1, 2, 4, 5, 6, 7, 9, 10, 11] and not m.difficults.any()
    assert st["boxes_over_gmax"] == 3
    m = od_gen.mosaic_boxes(anns, [_aug()] * 4, (160, 160), (320, 320), ignore_regions=True, gmax=11)
    assert list(m.classes) == [0, 1, 2, 4, 5, 6, 7, 8, 9, 10, 11]  # of the two flagged boxes the smaller one (class 3)
    many = _ann(np.tile([[0.1, 0.1, 0.6, 0.6]], (60, 1)), np.arange(60))
    st = {"mosaics": 0}
    rng = np.random.default_rng(0)
    mp, m = od_gen.sample_mosaic(rng, [many] * 4, (320, 320), stats=st)  # nothing raises; at most pb.GMAX boxes come back
    assert m.num_objects <= 128 and st["mosaics"] == 1
    assert len(m.classes) == len(m.bboxes) == len(m.difficults)


def test_sample_mosaic_invariants():
    from object_detector_amd import od_gen
    rng = np.random.default_rng(3)
    for trial in range(50):
        anns = []
        for _k in range(4):
            n = int(rng.integers(0, 6))
            c = rng.uniform(0.1, 0.9, (n, 2))
            wh = rng.uniform(0.05, 0.5, (n, 2))
            b = np.clip(np.concatenate([c - wh / 2, c + wh / 2], 1), 0, 1)
            anns.append(_ann(b, rng.integers(0, 20, n), rng.random(n) < 0.2, wh=(int(rng.integers(50, 600)), int(rng.integers(50, 600)))))
        H, W = (320, 320) if trial % 2 else (256, 640)
        st = {}
        mp, m = od_gen.sample_mosaic(rng, anns, (H, W), ignore_regions=bool(trial % 3), stats=st)
        assert 0.3 * W - 1 <= mp.split[0] <= 0.7 * W + 1 and 0.3 * H - 1 <= mp.split[1] <= 0.7 * H + 1
        assert len(mp.tiles) == 4 and all(not t.erase for t in mp.tiles) and len(mp.erase) <= 3
        assert (m.bboxes >= 0).all() and (m.bboxes <= 1).all() and (m.bboxes[:, 2:] > m.bboxes[:, :2]).all()
        assert m.num_objects + st.get("boxes_dropped", 0) == sum(a.num_objects for a in anns)
        for a, t, (_x0, _y0, Wt, Ht) in zip(anns, mp.tiles, od_gen.tile_rects(mp.split, (H, W))):
            x1, y1, x2, y2 = t.crop
            assert 0 <= x1 < x2 <= 1 and 0 <= y1 < y2 <= 1
            d = (Wt / ((x2 - x1) * a.width)) / (Ht / ((y2 - y1) * a.height))
            assert 1 / 1.5 - 1e-6 <= d <= 1.5 + 1e-6, d  # the stated bound on a tile's aspect distortion


def test_select_filters_classes_boxes_and_flags_together():
    a = _ann([[0, 0, 0.5, 0.5], [0.1, 0.1, 0.2, 0.2], [0.5, 0.5, 1, 1]], [4, 5, 6], [False, True, False])
    s = a.select(np.array([False, True, True]))
    assert list(s.classes) == [5, 6] and list(s.difficults) == [True, False] and s.bboxes.shape == (2, 4)
    assert (s.bboxes[0] == a.bboxes[1]).all() and (s.width, s.height) == (a.width, a.height)


# ---- generator arguments ---------------------------------------------------------------------------------------------

def test_mosaic_needs_a_device():
    from object_detector_amd import od_gen
    with pytest.raises(ValueError, match="device"):
        od_gen.create_generator((64, 64), mosaic=0.5)
    with pytest.raises(ValueError):
        od_gen.create_generator((64, 64), mosaic=1.5, device="cuda:0")
    g = od_gen.create_generator((64, 64), mosaic=0.0, ignore_regions=True)  # off: no device needed
    assert g.stats == {"mosaics": 0, "boxes_dropped": 0, "boxes_ignored": 0, "boxes_over_gmax": 0}


def test_mosaic_zero_draws_nothing_extra_from_the_rng():
    """The first batches of a generator built with mosaic=0.0 equal, pixels and boxes, those of one built without the
    argument: with the feature off not one extra number is drawn."""
    sys.path.insert(0, str(ROOT / "scripts"))
    import _common
    from object_detector_amd import od_gen
    X, y = _common.shapes_dataset(6, seed=4, size_range=(40, 70))
    outs = []
    for kw in ({}, {"mosaic": 0.0}, {"mosaic": 0.0, "ignore_regions": True}):
        gen = od_gen.create_generator((48, 64), workers=1, **kw)
        g, _ = gen.flow(X, y, batch_size=4, data_augmentation=True, shuffle=True, seed=7)
        outs.append([next(g) for _ in range(5)])
    for other in outs[1:]:
        for (xa, ya), (xb, yb) in zip(outs[0], other):
            assert np.array_equal(xa, xb)
            for a, b in zip(ya, yb):
                assert np.array_equal(a.bboxes, b.bboxes) and np.array_equal(a.classes, b.classes)
    # ... and sample_params itself still draws what it drew: a fixed seed reproduces these numbers
    p = od_gen.sample_params(np.random.default_rng(0), y[0])
    q = od_gen.sample_params(np.random.default_rng(0), y[0])
    assert (p.crop, p.flip, p.brightness, p.contrast, p.saturation, p.erase) == \
           (q.crop, q.flip, q.brightness, q.contrast, q.saturation, q.erase)


def test_prior_boxes_arguments():
    from object_detector_amd.pb import IGN_THR, PriorBoxes
    pb = PriorBoxes((64, 64), 3, device="cpu")
    assert pb.ignore_regions is False and pb.ign_thr == IGN_THR == 0.5
    assert PriorBoxes((64, 64), 3, device="cpu", ignore_regions=True, ign_thr=0.7).ign_thr == 0.7
    with pytest.raises(ValueError):
        PriorBoxes((64, 64), 3, device="cpu", ignore_regions=True, ign_thr=0.0)


def test_shapes_dataset_marks_do_not_move_the_default_images():
    sys.path.insert(0, str(ROOT / "scripts"))
    import _common
    X0, y0 = _common.shapes_dataset(12, seed=3)
    X1, y1 = _common.shapes_dataset(12, seed=3, difficult_frac=0.3, crowd_frac=0.5)
    assert not any(a.difficults.any() for a in y0)
    assert sum(int(a.difficults.sum()) for a in y1) >= 3
    for a, b in zip(y0, y1):
        assert np.array_equal(a.bboxes, b.bboxes[:a.num_objects]) and np.array_equal(a.classes, b.classes[:a.num_objects])
    assert all(x.shape == z.shape for x, z in zip(X0, X1))
