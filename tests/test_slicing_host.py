"""CPU: sliced inference without a GPU -- the tile geometry and argument checks of object_detector_amd/slicing.py, and the numpy
restatement tests/slice_ref.py against Pillow (tile pixels) and against tta_ref (the merge with one tile), plus the conditions
the generated merge scenarios of tests/test_gpu_slice_merge.py must meet, checked on the reference.  No tolerances."""
import functools

import numpy as np
import pytest

import lattice_ref as L
import slice_ref
import tta_ref
from object_detector_amd import slicing

F = np.float32


# ---- geometry ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("overlap", [0.0, 0.2, 0.5])
@pytest.mark.parametrize("n", [1, 2, 3, 4])
@pytest.mark.parametrize("L_", [1, 7, 96, 333, 1920])
def test_axis_tiles_cover_the_axis(L_, n, overlap):
    tiles = slicing.axis_tiles(L_, n, overlap)
    assert len(tiles) == n
    assert tiles[0][0] == 0 and tiles[-1][1] == L_
    assert len({e - s for s, e in tiles}) == 1 and tiles[0][1] - tiles[0][0] >= 1
    covered = np.zeros(L_, bool)
    for (s, e), nxt in zip(tiles, tiles[1:] + [None]):
        assert 0 <= s < e <= L_
        covered[s:e] = True
        if nxt is not None:
            assert s <= nxt[0] <= e, "neighbours must overlap or touch, in order"
    assert covered.all()
    # rects / edges of a grid built from this axis in x and a single tile in y, with and without the full view
    for full in (False, True):
        g = slicing.SliceGrid(1, n, overlap, full)
        r = g.rects(L_, 5)
        assert r.dtype == np.int32 and r.shape == (n + full, 4)
        assert [tuple(v) for v in r[:n, [0, 2]].tolist()] == tiles and (r[:, 1] == 0).all() and (r[:, 3] == 5).all()
        e = slicing.edges(r, L_, 5)
        for t in range(n):
            want = (slicing.LEFT if tiles[t][0] != 0 else 0) | (slicing.RIGHT if tiles[t][1] != L_ else 0)
            assert e[t] == want
        if full:
            assert r[n].tolist() == [0, 0, L_, 5] and e[n] == 0
    gy = slicing.SliceGrid(n, 1, overlap, False)
    ry = gy.rects(3, L_)
    assert [tuple(v) for v in ry[:, [1, 3]].tolist()] == tiles
    assert (slicing.edges(ry, 3, L_) & (slicing.LEFT | slicing.RIGHT) == 0).all()
    assert [bool(v & slicing.TOP) for v in slicing.edges(ry, 3, L_)] == [s != 0 for s, _ in tiles]
    assert [bool(v & slicing.BOTTOM) for v in slicing.edges(ry, 3, L_)] == [e != L_ for _, e in tiles]


def test_rects_order_and_affine():
    g = slicing.SliceGrid(2, 2, 0.2, True)
    assert g.T == 5
    r = g.rects(200, 150)
    assert r.tolist() == [[0, 0, 112, 84], [88, 0, 200, 84], [0, 66, 112, 150], [88, 66, 200, 150], [0, 0, 200, 150]]
    assert slicing.edges(r, 200, 150).tolist() == [slicing.RIGHT | slicing.BOTTOM, slicing.LEFT | slicing.BOTTOM,
                                                   slicing.RIGHT | slicing.TOP, slicing.LEFT | slicing.TOP, 0]
    a = slicing.affine(r, 200, 150)
    assert a.dtype == F and a.shape == (5, 4)
    assert a[1].tolist() == [F(88) / F(200), F(0), F(112) / F(200), F(84) / F(150)]
    assert a[4].tolist() == [0.0, 0.0, 1.0, 1.0]
    lo, hi = g.edge_lo_hi
    assert lo == float(F(0.01)) and hi == float(F(1 - 0.01))


# ---- arguments -----------------------------------------------------------------------------------------------------------
def test_normalize_accepts_and_rejects():
    assert slicing.normalize(None) is None
    assert slicing.normalize(None, slice_overlap=7, tta=("flip",), keep_aspect=True) is None  # slicing is off
    g = slicing.normalize((2, 2), batch_size=10)
    assert (g.ny, g.nx, g.T, g.overlap, g.full_view, g.edge) == (2, 2, 5, 0.2, True, 0.01)
    assert slicing.normalize([3, 5], batch_size=16).T == 16
    assert slicing.normalize((4, 4), slice_full_view=False, batch_size=16).T == 16
    assert slicing.normalize((1, 1), slice_full_view=False, slice_edge=-1, batch_size=1).T == 1
    for bad in ((2,), (2, 2, 2), "22", 4, (0, 2), (2, -1), (2.0, 2), (True, 2), (None, 2)):
        with pytest.raises(ValueError, match="slices"):
            slicing.normalize(bad, batch_size=32)
    for ov in (-0.01, 0.51, float("nan")):
        with pytest.raises(ValueError, match="slice_overlap"):
            slicing.normalize((2, 2), slice_overlap=ov, batch_size=32)
    with pytest.raises(ValueError, match="at most 16"):
        slicing.normalize((4, 4), batch_size=32)  # 17 with the full view
    with pytest.raises(ValueError, match="batch_size"):
        slicing.normalize((2, 2), batch_size=4)
    with pytest.raises(ValueError, match="tta"):
        slicing.normalize((2, 2), batch_size=32, tta=())
    with pytest.raises(ValueError, match="tta"):
        slicing.normalize((2, 2), batch_size=32, tta=("flip",))
    with pytest.raises(ValueError, match="keep_aspect"):
        slicing.normalize((2, 2), batch_size=32, keep_aspect=True)


def test_detector_checks_slice_arguments_before_the_gpu(monkeypatch):
    """ObjectDetector raises the ValueErrors before anything touches the GPU (torch.cuda is never asked)."""
    import torch
    from object_detector_amd.detector import ObjectDetector

    def boom(*a, **k):
        raise AssertionError("the GPU was touched before the arguments were checked")
    monkeypatch.setattr(torch.cuda, "is_available", boom)
    monkeypatch.setattr(torch.cuda, "device_count", boom)
    for kw, msg in (({"slices": (4, 4)}, "at most 16"), ({"slices": (2, 2), "batch_size": 4}, "batch_size"),
                    ({"slices": (2, 2), "tta": ()}, "tta"), ({"slices": (2, 2), "keep_aspect": True}, "keep_aspect"),
                    ({"slices": (2, 2), "slice_overlap": 0.6}, "slice_overlap"), ({"slices": (2,)}, "slices")):
        kw = {"batch_size": 32, **kw}
        with pytest.raises(ValueError, match=msg):
            ObjectDetector({}, **kw)
    with pytest.raises(ValueError, match="tta"):  # the arguments travel through synthetic() (and load_voc's **kw) as well
        ObjectDetector.synthetic(32, (96, 96), slices=(2, 2), tta=("flip",))


# ---- tile pixels ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["up", "down", "copy", "one_pixel_wide", "mixed_grid", "vertical_first"])
def test_tile_pixels_equal_pillow_crop_resize(case):
    from PIL import Image
    rng = np.random.default_rng(L.seed_of("tile_pixels", case))
    if case == "up":  # a 50 x 40 tile -> 96 x 96
        img, rects, size = rng.integers(0, 256, (70, 90, 3), dtype=np.uint8), [(20, 10, 70, 50)], (96, 96)
    elif case == "down":
        img, rects, size = rng.integers(0, 256, (300, 400, 3), dtype=np.uint8), [(13, 7, 390, 290), (0, 0, 400, 300)], (96, 64)
    elif case == "copy":
        img, rects, size = rng.integers(0, 256, (120, 130, 3), dtype=np.uint8), [(30, 20, 126, 116)], (96, 96)
    elif case == "one_pixel_wide":
        img, rects, size = rng.integers(0, 256, (64, 9, 3), dtype=np.uint8), [(4, 0, 5, 64), (8, 3, 9, 4)], (32, 32)
    elif case == "mixed_grid":
        img = rng.integers(0, 256, (150, 200, 3), dtype=np.uint8)
        rects, size = slicing.SliceGrid(2, 2, 0.2, True).rects(200, 150), (96, 96)
    else:  # more than 100 times as tall as wide, shrinking vertically: Image.resize runs the vertical pass first
        img = rng.integers(0, 256, (6500, 64, 3), dtype=np.uint8)
        rects, size = [(0, 0, 64, 6500), (10, 100, 40, 6400)], (96, 96)
    got = slice_ref.tile_pixels(img, rects, size)
    pil = Image.fromarray(img)
    for t, rc in enumerate(np.asarray(rects).tolist()):
        want = np.asarray(pil.crop(tuple(rc)).resize(size, Image.BILINEAR), np.uint8)
        assert got[t].shape == want.shape == (size[1], size[0], 3)
        assert np.array_equal(got[t], want), (case, t)


def test_host_tiles_equal_the_reference():
    rng = np.random.default_rng(5)
    img = rng.integers(0, 256, (150, 200, 3), dtype=np.uint8)
    g = slicing.SliceGrid(2, 2, 0.2, True)
    out = np.zeros((5, 96, 96, 3), np.uint8)
    assert slicing.host_tiles(img, g, (96, 96), out) == (200, 150)
    assert np.array_equal(out, slice_ref.tile_pixels(img, g.rects(200, 150), (96, 96)))


# ---- merge ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("vote_iou", [0.0, 0.5])
@pytest.mark.parametrize("strict", [False, True])
def test_one_tile_without_the_rule_is_the_tta_merge(strict, vote_iou):
    """T = 1, rule disabled: slice_ref.merge_image == tta_ref.merge_image with one unmirrored view, bit for bit (the map
    0 + 1 * x is exact on [0, 1])."""
    rng = np.random.default_rng(11)
    K, P, NC = 1024, 4200, 20
    keys, boxes = slice_ref.make_row(rng, K, P, NC, 900, quantise=True)
    g = slicing.SliceGrid(1, 1, 0.2, False, -1.0)
    r = g.rects(640, 480)
    lo, hi = g.edge_lo_hi
    a = slice_ref.merge_image([{"keys": keys, "count": 900, "boxes": boxes}], NC, K, slicing.edges(r, 640, 480),
                              slicing.affine(r, 640, 480), lo, hi, 0.45, strict, 200, vote_iou)
    b = tta_ref.merge_image([{"keys": keys, "count": 900, "boxes": boxes, "flip": False}], NC, K, 0.45, strict, 200, vote_iou)
    assert a["dropped"] == 0 and len(a["cls"]) > 0 and len(a["cls"]) < a["merged"]
    assert np.array_equal(a["src"], b["src"]) and np.array_equal(a["cls"], b["cls"])
    assert np.array_equal(a["conf_bits"], b["conf_bits"])
    assert np.array_equal(a["boxes"].view(np.uint32), b["boxes"].view(np.uint32))


def test_vectorised_map_is_the_scalar_statement():
    rng = np.random.default_rng(12)
    sc = slice_ref.scenario("g2_t5")
    lists, edge, aff = slice_ref.image_lists(sc, 1)
    cands, _ = slice_ref.candidates(lists, sc["NC"], edge, aff, -1.0, 2.0)
    for i in rng.integers(0, len(cands), 200):
        _, t, flat, _, box = cands[i]
        assert np.array_equal(box.view(np.uint32), slice_ref.to_image(lists[t]["boxes"][flat // sc["NC"]], aff[t]).view(np.uint32))


def _key(conf, flat):
    return (np.uint64(np.array(conf, F).view(np.uint32)) << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - np.uint64(flat))


def test_seam_case_by_hand():
    """A 200 x 100 image, 1 x 2 tiles ([0,112) and [88,200) in x) and the full view.  One object over x in [60,150): each tile
    sees a part that ends on its interior side, the full view sees it whole.  With the rule only the whole box is kept; with
    slice_edge = -1 the two partial boxes (higher confidence) survive and suppress the whole one."""
    NC, K, P = 20, 8, 4
    w, h = 200, 100
    y1, y2 = F(0.3), F(0.7)

    def lists():
        t0 = np.zeros((P, 4), F)
        t0[2] = [F(60) / F(112), y1, F(1), y2]            # clipped at tile 0's right side (interior)
        t1 = np.zeros((P, 4), F)
        t1[1] = [F(0), y1, F(150 - 88) / F(112), y2]      # clipped at tile 1's left side (interior)
        tf = np.zeros((P, 4), F)
        tf[3] = [F(0.3), y1, F(0.75), y2]
        out = []
        for boxes, conf, prior in ((t0, 0.9, 2), (t1, 0.8, 1), (tf, 0.7, 3)):
            keys = np.zeros(K, np.uint64)
            keys[0] = _key(conf, prior * NC + 7)
            out.append({"keys": keys, "count": 1, "boxes": boxes})
        return out

    for edge_arg, want_tiles in ((0.01, [2]), (-1.0, [0, 1])):
        g = slicing.SliceGrid(1, 2, 0.2, True, edge_arg)
        r = g.rects(w, h)
        assert r.tolist() == [[0, 0, 112, 100], [88, 0, 200, 100], [0, 0, 200, 100]]
        e = slicing.edges(r, w, h)
        assert e.tolist() == [slicing.RIGHT, slicing.LEFT, 0]
        lo, hi = g.edge_lo_hi
        res = slice_ref.merge_image(lists(), NC, K, e, slicing.affine(r, w, h), lo, hi, 0.45, False, 200, 0.0)
        assert res["src"][:, 0].tolist() == want_tiles, (edge_arg, res["src"])
        assert (res["cls"] == 7).all()
        assert res["dropped"] == (2 if edge_arg >= 0 else 0)
        if edge_arg >= 0:
            assert np.array_equal(res["boxes"][0], np.array([0.3, 0.3, 0.75, 0.7], F))
        else:  # the partial boxes, mapped to image coordinates
            assert np.allclose(res["boxes"], [[0.3, 0.3, 0.56, 0.7], [0.44, 0.3, 0.75, 0.7]], atol=1e-6)


@functools.lru_cache(maxsize=None)
def _scenario_reference(name):
    sc = slice_ref.scenario(name)
    out = []
    for g in range(sc["G"]):
        lists, edge, aff = slice_ref.image_lists(sc, g)
        out.append(slice_ref.merge_image(lists, sc["NC"], sc["K"], edge, aff, sc["edge_lo"], sc["edge_hi"], 0.45, False, 200, 0.5))
    return sc, out


@pytest.mark.parametrize("name", list(slice_ref.SCENARIOS))
def test_generated_scenarios_meet_their_conditions(name):
    """What tests/test_gpu_slice_merge.py relies on, shown on the reference: every non-empty scenario in which the rule can
    act (interior sides exist and the rule is on) drops at least one candidate; every non-empty scenario with interior sides
    keeps a detection from a tile that has one, and suppresses at least one candidate."""
    sc, refs = _scenario_reference(name)
    total = int(sc["counts"].sum())
    dropped = sum(r["dropped"] for r in refs)
    kept = sum(len(r["cls"]) for r in refs)
    merged = sum(r["merged"] for r in refs)
    interior = bool(sc["edges"].any())
    if name == "all_empty":
        assert total == 0 and kept == 0
        return
    assert total > 0 and kept > 0
    assert kept < merged, "nothing was suppressed"
    if name == "t1":
        assert not interior and dropped == 0
        return
    assert interior
    if name == "rule_disabled":
        assert dropped == 0 and sc["edge_lo"] < 0
    else:
        assert dropped > 0
    from_interior = sum(int((sc["edges"][g * sc["T"] + r["src"][:, 0]] != 0).sum()) for g, r in enumerate(refs))
    assert from_interior > 0
    if name == "tile_emptied_by_rule":
        assert not (refs[0]["src"][:, 0] == 1).any() and sc["counts"][1] > 0
    if name == "t16_full":
        assert total == 16 * 1024 and merged == 1024
    if name == "t10_ties":  # the same confidence in more than one tile among the merged candidates
        lists, edge, aff = slice_ref.image_lists(sc, 0)
        cands, _ = slice_ref.candidates(lists, sc["NC"], edge, aff, sc["edge_lo"], sc["edge_hi"])
        top = tta_ref.merged_order(cands, sc["K"])
        by_conf = {}
        for bits, t, *_ in top:
            by_conf.setdefault(bits, set()).add(t)
        assert any(len(v) > 1 for v in by_conf.values())
