"""CPU: the COCO bbox protocol's numpy reference on hand-computed cases, and the host side of tk.data.coco's evaluation
(load_gt, to_results, host packing, summary lines) -- nothing here runs a kernel."""
import json
import pathlib
import sys

import numpy as np
import pytest

import pytoolkit as tk
from object_detector_amd import cocoeval as CE
from object_detector_amd.detector import ObjectsPrediction

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent))
import cocoeval_ref as ref  # noqa: E402


def _doc(images, anns, cats=((1, "thing"),)):
    return dict(images=[dict(id=i, file_name=f"{i}.jpg", width=100, height=100) for i in images],
                annotations=[dict(id=n + 1, **a) for n, a in enumerate(anns)],
                categories=[dict(id=c, name=nm) for c, nm in cats])


def _det(img, b, s, c=1):
    return dict(image_id=img, category_id=c, bbox=b, score=s)


def test_case_a_false_positive_first():
    doc = _doc([1], [dict(image_id=1, category_id=1, bbox=[0, 0, 10, 10], area=100.0, iscrowd=0)])
    r = ref.evaluate(doc, [_det(1, [50, 50, 10, 10], 0.9), _det(1, [0, 0, 10, 10], 0.8)])
    np.testing.assert_array_equal(r["stats"], [0.5, 0.5, 0.5, 0.5, -1, -1, 0.0, 1.0, 1.0, 1.0, -1, -1])


def test_case_b_crowd_match_is_ignored():
    doc = _doc([1], [dict(image_id=1, category_id=1, bbox=[0, 0, 10, 10], area=100.0, iscrowd=0),
                     dict(image_id=1, category_id=1, bbox=[0, 0, 100, 100], area=10000.0, iscrowd=1)])
    r = ref.evaluate(doc, [_det(1, [20, 20, 10, 10], 0.9), _det(1, [0, 0, 10, 10], 0.8)])
    p = r["precision"]
    one = 1.0 / (1.0 + np.spacing(1))
    assert (p[:, :, 0, 0, 1:] == one).all() and (p[:, :, 0, 1, 1:] == one).all()
    assert (r["recall"][:, 0, 0, 0] == 0).all()  # AR@1: the only detection of rank 0 is the ignored one
    assert r["stats"][6] == 0.0 and r["stats"][7] == 1.0


def test_case_c_score_ties_in_sorted_image_order():
    doc = _doc([7, 3], [dict(image_id=7, category_id=1, bbox=[0, 0, 10, 10], area=100.0, iscrowd=0),
                        dict(image_id=3, category_id=1, bbox=[0, 0, 10, 10], area=100.0, iscrowd=0)])
    r = ref.evaluate(doc, [_det(7, [0, 0, 10, 10], 0.5), _det(3, [60, 60, 10, 10], 0.5)])
    assert abs(r["stats"][0] - 0.5 * 51 / 101) < 1e-12  # image 3's FP first; JSON order would give 0.50495


def test_iou_exactly_at_threshold_matches():
    assert ref.bb_iou([0, 0, 10, 5], [0, 0, 10, 10], False) == 0.5
    doc = _doc([1], [dict(image_id=1, category_id=1, bbox=[0, 0, 10, 10], area=100.0)])
    r = ref.evaluate(doc, [_det(1, [0, 0, 10, 5], 0.5)])
    assert (r["recall"][0, 0, :, :][[0, 1]] == 1.0).all() and (r["recall"][1:, 0, 0, :] == 0.0).all()


def _write(tmp_path, doc):
    p = tmp_path / "instances.json"
    p.write_text(json.dumps(doc))
    return p


def test_load_gt_defaults_and_class_mapping(tmp_path):
    doc = dict(images=[dict(id=11, file_name="a.jpg", width=200, height=100),
                       dict(id=5, file_name="b.jpg", width=64, height=128)],
               categories=[dict(id=90, name="toothbrush"), dict(id=1, name="person"), dict(id=18, name="dog")],
               annotations=[dict(id=1, image_id=11, category_id=18, bbox=[20, 10, 100, 50], iscrowd=0, area=7.5),
                            dict(id=2, image_id=5, category_id=90, bbox=[16, 32, 32, 64])])
    path = _write(tmp_path, doc)
    gt = tk.data.coco.load_gt(path)
    np.testing.assert_array_equal(gt.image_ids, [11, 5])
    np.testing.assert_array_equal(gt.category_ids, [1, 18, 90])
    assert gt.category_names == ["person", "dog", "toothbrush"]
    np.testing.assert_array_equal(gt.widths, [200, 64])
    np.testing.assert_array_equal(gt.ann_areas, [7.5, 32.0 * 64.0])  # field, else w*h
    np.testing.assert_array_equal(gt.ann_crowd, [False, False])
    np.testing.assert_array_equal(gt.ann_bboxes[1], [16, 32, 32, 64])
    # class i = the i-th smallest category id, as load_od numbers them
    (tmp_path / "img").mkdir()
    X, y, names = tk.data.coco.load_od(path, tmp_path / "img")
    assert names == gt.category_names
    assert [int(c) for c in y[0].classes] + [int(c) for c in y[1].classes] == gt.ann_classes.tolist() == [1, 2]
    bad = dict(doc, annotations=doc["annotations"] + [dict(id=3, image_id=11, category_id=3, bbox=[0, 0, 1, 1])])
    with pytest.raises(ValueError, match="category id 3"):
        tk.data.coco.load_gt(_write(tmp_path, bad))
    bad = dict(doc, annotations=doc["annotations"] + [dict(id=3, image_id=12, category_id=1, bbox=[0, 0, 1, 1])])
    with pytest.raises(ValueError, match="image id 12"):
        tk.data.coco.load_gt(_write(tmp_path, bad))


def test_to_results_box_arithmetic(tmp_path):
    doc = dict(images=[dict(id=4, file_name="a.jpg", width=300, height=200), dict(id=2, file_name="b.jpg", width=64,
                                                                                  height=48)],
               categories=[dict(id=7, name="b"), dict(id=3, name="a")], annotations=[])
    gt = tk.data.coco.load_gt(_write(tmp_path, doc))
    b = np.array([[0.1, 0.2, 0.35, 0.9]], np.float32)
    y = [ObjectsPrediction([1], [0.7], b), ObjectsPrediction([], [], np.zeros((0, 4)))]
    res = tk.data.coco.to_results(gt, y)
    assert len(res) == 1 and res[0]["image_id"] == 4 and res[0]["category_id"] == 7
    b64 = b[0].astype(np.float64)
    assert res[0]["bbox"] == [b64[0] * 300, b64[1] * 200, (b64[2] - b64[0]) * 300, (b64[3] - b64[1]) * 200]
    assert res[0]["score"] == float(np.float32(0.7))
    tk.data.coco.save_results(tmp_path / "r.json", res)
    assert json.loads((tmp_path / "r.json").read_text()) == res
    res2 = tk.data.coco.to_results(gt, [y[1]], image_ids=[2])
    assert res2 == []


def test_summary_lines_format():
    doc = _doc([1], [dict(image_id=1, category_id=1, bbox=[0, 0, 10, 10], area=100.0, iscrowd=0)])
    r = ref.evaluate(doc, [_det(1, [50, 50, 10, 10], 0.9), _det(1, [0, 0, 10, 10], 0.8)])
    stats, lines = CE.summarize(r["precision"], r["recall"])
    np.testing.assert_array_equal(stats, r["stats"])
    assert lines == r["lines"]
    assert lines[0] == " Average Precision  (AP) @[ IoU=0.50:0.95 | area=   all | maxDets=100 ] = 0.500"
    assert lines[1] == " Average Precision  (AP) @[ IoU=0.50      | area=   all | maxDets=100 ] = 0.500"
    assert lines[4] == " Average Precision  (AP) @[ IoU=0.50:0.95 | area=medium | maxDets=100 ] = -1.000"
    assert lines[6] == " Average Recall     (AR) @[ IoU=0.50:0.95 | area=   all | maxDets=  1 ] = 0.000"
    ev = CE.CocoEvaluation(r["precision"], r["recall"], r["scores"], stats, np.array([1]), ["thing"])
    assert ev.summary() == lines and ev.ap_per_class().tolist() == [0.5]


def test_input_checks(tmp_path):
    doc = _doc([1, 2], [dict(image_id=1, category_id=1, bbox=[0, 0, 10, 10])])
    gt = tk.data.coco.load_gt(_write(tmp_path, doc))
    with pytest.raises(ValueError, match="image id 9"):
        CE.pack(gt, CE._as_dets(gt, [_det(9, [0, 0, 1, 1], 0.5)], None))
    with pytest.raises(ValueError, match="non-finite"):
        CE.pack(gt, CE._as_dets(gt, [_det(1, [0, 0, float("nan"), 1], 0.5)], None))
    p = CE.pack(gt, CE._as_dets(gt, [_det(2, [0, 0, 1, 1], 0.5), _det(1, [0, 0, 1, 1], 0.5, c=5)], None), image_ids=[1])
    assert len(p.det_out) == 0 and p.n_groups == 1  # outside the subset / unknown category: left out


def test_packing_against_straightforward_construction(tmp_path):
    doc, results = ref.make_problem(3, n_images=40, n_cats=6, dets_per_image=30)
    gt = tk.data.coco.load_gt(_write(tmp_path, doc))
    p = CE.pack(gt, CE._as_dets(gt, results, None))
    K = len(gt.category_ids)
    cats = sorted(c["id"] for c in doc["categories"])
    imgs = sorted(im["id"] for im in doc["images"])
    groups = {}
    for n, a in enumerate(doc["annotations"]):
        groups.setdefault((imgs.index(a["image_id"]), cats.index(a["category_id"])), ([], []))[0].append(n)
    for n, r in enumerate(results):
        if r["category_id"] in cats:
            groups.setdefault((imgs.index(r["image_id"]), cats.index(r["category_id"])), ([], []))[1].append(n)
    keys = sorted(groups)
    assert p.n_groups == len(keys)
    acc = []  # (category, -score, image position, rank, group, rank) of every kept detection
    for g, key in enumerate(keys):
        gi, di = groups[key]
        assert p.gt_off[g + 1] - p.gt_off[g] == len(gi)
        np.testing.assert_array_equal(p.gt_box[p.gt_off[g]:p.gt_off[g + 1]],
                                      np.array([doc["annotations"][n]["bbox"] for n in gi], np.float64).reshape(-1, 4))
        di = sorted(di, key=lambda n: -results[n]["score"])[:100]  # stable: ties in input order
        assert p.det_off[g + 1] - p.det_off[g] == len(di)
        np.testing.assert_array_equal(p.det_box[p.det_off[g]:p.det_off[g + 1]],
                                      np.array([results[n]["bbox"] for n in di], np.float64).reshape(-1, 4))
        acc += [(key[1], -results[n]["score"], key[0], rk, p.det_off[g] + rk) for rk, n in enumerate(di)]
    acc.sort(key=lambda e: e[:4])
    for slot, (k, negs, _pos, rk, d) in enumerate(acc):
        assert p.det_out[d] == slot and p.acc_rank[slot] == rk and p.acc_score[slot] == -negs
    np.testing.assert_array_equal(np.diff(p.cat_off), np.bincount([e[0] for e in acc], minlength=K))
    for k, cid in enumerate(cats):
        for a, (lo, hi) in enumerate(ref.AREA_RNG):
            n = sum(1 for x in doc["annotations"] if x["category_id"] == cid and not x.get("iscrowd", 0)
                    and lo <= x.get("area", x["bbox"][2] * x["bbox"][3]) <= hi)
            assert p.npig[k, a] == n


def test_evaluate_without_gpu_raises(tmp_path):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from object_detector_amd import _lib
    doc = _doc([1], [dict(image_id=1, category_id=1, bbox=[0, 0, 10, 10])])
    gt = tk.data.coco.load_gt(_write(tmp_path, doc))
    with pytest.raises(_lib.OdError):
        tk.data.coco.evaluate(gt, [_det(1, [0, 0, 10, 10], 0.5)])
