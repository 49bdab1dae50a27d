"""tk.data.coco.load_od on a small COCO-format dataset written to tmp_path (host only)."""
import json

import numpy as np
import pytest
from PIL import Image

import pytoolkit as tk


def _write_dataset(tmp_path):
    img_dir = tmp_path / "images"
    img_dir.mkdir()
    images = [dict(id=11, file_name="a.jpg", width=200, height=100), dict(id=5, file_name="b.jpg", width=64, height=128),
              dict(id=7, file_name="empty.jpg", width=32, height=32)]
    for im in images:
        Image.fromarray(np.full((im["height"], im["width"], 3), 127, np.uint8)).save(img_dir / im["file_name"])
    categories = [dict(id=90, name="toothbrush"), dict(id=1, name="person"), dict(id=18, name="dog")]  # ids not contiguous
    annotations = [
        dict(id=1, image_id=11, category_id=18, bbox=[20, 10, 100, 50], iscrowd=0),
        dict(id=2, image_id=11, category_id=1, bbox=[0, 0, 200, 100], iscrowd=1),  # crowd region
        dict(id=3, image_id=5, category_id=90, bbox=[16, 32, 32, 64], iscrowd=0),
        dict(id=4, image_id=11, category_id=90, bbox=[150, 50, 50, 50], iscrowd=0),
        dict(id=5, image_id=5, category_id=1, bbox=[0, 64, 64, 64]),  # no iscrowd key: not a crowd
    ]
    path = tmp_path / "instances.json"
    path.write_text(json.dumps(dict(images=images, annotations=annotations, categories=categories)))
    return path, img_dir


def test_load_od(tmp_path):
    path, img_dir = _write_dataset(tmp_path)
    X, y, names = tk.data.coco.load_od(path, img_dir)
    assert names == ["person", "dog", "toothbrush"]  # ascending category id -> classes 0, 1, 2
    assert [p.name for p in X] == ["a.jpg", "b.jpg", "empty.jpg"] and all(p.exists() for p in X)
    a, b, e = y
    assert (a.width, a.height) == (200, 100) and a.path == X[0]
    np.testing.assert_array_equal(a.classes, [1, 0, 2])
    np.testing.assert_allclose(a.bboxes, [[0.1, 0.1, 0.6, 0.6], [0, 0, 1, 1], [0.75, 0.5, 1.0, 1.0]], rtol=1e-6)
    np.testing.assert_array_equal(a.difficults, [False, True, False])
    np.testing.assert_array_equal(b.classes, [2, 0])
    np.testing.assert_allclose(b.bboxes, [[0.25, 0.25, 0.75, 0.75], [0, 0.5, 1, 1]], rtol=1e-6)
    np.testing.assert_array_equal(b.difficults, [False, False])
    assert e.num_objects == 0 and e.bboxes.shape == (0, 4) and e.classes.shape == (0,)


def test_evaluate_ground_truth_as_predictions(tmp_path):
    from object_detector_amd.detector import ObjectsPrediction
    path, img_dir = _write_dataset(tmp_path)
    _X, y, names = tk.data.coco.load_od(path, img_dir)
    preds = [ObjectsPrediction(a.classes, np.ones(len(a.classes), np.float32), a.bboxes) for a in y]
    NC = len(names)
    res = tk.data.voc.evaluate(y, preds, num_classes=NC)
    # every class with (non-crowd) objects at AP 1.0
    assert res["mAP"] == pytest.approx(1.0) and res["mAP_VOC"] == pytest.approx(1.0)
    # the crowd region neither counts nor penalises: dropping its prediction changes nothing
    preds[0] = ObjectsPrediction(y[0].classes[[0, 2]], np.ones(2, np.float32), y[0].bboxes[[0, 2]])
    assert tk.data.voc.evaluate(y, preds, num_classes=NC)["mAP"] == pytest.approx(1.0)


def test_too_many_objects_names_the_image(tmp_path):
    from object_detector_amd.pb import GMAX
    images = [dict(id=1, file_name="crowded.jpg", width=10, height=10)]
    anns = [dict(id=i, image_id=1, category_id=3, bbox=[0, 0, 1, 1]) for i in range(GMAX + 1)]
    path = tmp_path / "instances.json"
    path.write_text(json.dumps(dict(images=images, annotations=anns, categories=[dict(id=3, name="x")])))
    with pytest.raises(ValueError, match="crowded.jpg"):
        tk.data.coco.load_od(path, tmp_path)
