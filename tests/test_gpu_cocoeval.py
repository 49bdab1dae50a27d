"""GPU: COCO bbox evaluation (od_coco_match + od_coco_accumulate, tk.data.coco.evaluate) against the numpy reference of the
protocol (cocoeval_ref.py): precision, recall, scores and stats must be bit-identical."""
import json
import os
import pathlib
import subprocess
import sys

import numpy as np
import pytest
from PIL import Image

import pytoolkit as tk
from object_detector_amd import cocoeval as CE
from object_detector_amd.detector import ObjectsPrediction

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent))
import cocoeval_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = pathlib.Path(__file__).resolve().parent.parent


def _gt(tmp_path, doc, name="instances.json"):
    p = tmp_path / name
    p.write_text(json.dumps(doc))
    return tk.data.coco.load_gt(p), p


def _assert_same(ev, r):
    for k in ("precision", "recall", "scores", "stats"):
        got = getattr(ev, k)
        assert got.shape == r[k].shape and np.array_equal(got, r[k]), \
            (k, np.argwhere(got != r[k])[:5].tolist() if got.shape == r[k].shape else got.shape)


@pytest.mark.parametrize("seed,kw", [(1, {}), (2, dict(n_images=200, n_cats=14)), (3, dict(n_images=80, n_cats=4))])
def test_generated_problems_bit_identical(cuda, tmp_path, seed, kw):
    doc, results = ref.make_problem(seed, **kw)
    gt, _ = _gt(tmp_path, doc)
    ev = tk.data.coco.evaluate(gt, results)
    r = ref.evaluate(doc, results)
    _assert_same(ev, r)
    assert ev.summary() == r["lines"]
    # the categories without GT stay -1 everywhere
    assert (ev.precision[:, :, -2:] == -1).all() and (ev.recall[:, -2:] == -1).all()
    assert (ev.ap_per_class()[-2:] == -1).all() and (ev.ap_per_class()[:-2] > -1).all()
    # an image_ids subset (results of other GT images are left out)
    sub = [im["id"] for im in doc["images"][::3]]
    _assert_same(tk.data.coco.evaluate(gt, results, image_ids=sub), ref.evaluate(doc, results, image_ids=sub))


def test_large_category_multichunk_and_reproducible(cuda, tmp_path):
    doc, results = ref.make_problem(5, n_images=250, n_cats=6, dets_per_image=10, edge_cases=False,
                                    big_category_dets=20000)
    gt, _ = _gt(tmp_path, doc)
    t = {}
    ev = tk.data.coco.evaluate(gt, results, timings=t)
    assert t["match_ms"] > 0 and t["accumulate_ms"] > 0
    p = CE.pack(gt, CE._as_dets(gt, results, None))
    assert np.diff(p.cat_off)[0] > 19000
    _assert_same(ev, ref.evaluate(doc, results))
    ev2 = tk.data.coco.evaluate(gt, results)
    for k in ("precision", "recall", "scores"):
        assert getattr(ev, k).tobytes() == getattr(ev2, k).tobytes()


def _random_predictions(gt, seed, n_per_image=30):
    rng = np.random.default_rng(seed)
    out = []
    for _ in gt.image_ids:
        n = int(rng.integers(0, n_per_image + 1))
        c = rng.uniform(0, 1, (n, 2))
        wh = rng.uniform(0.02, 0.7, (n, 2))
        b = np.clip(np.concatenate([c - wh / 2, c + wh / 2], 1), 0, 1).astype(np.float32)
        conf = np.round(rng.uniform(0, 1, n), 2).astype(np.float32)  # f32 ties
        out.append(ObjectsPrediction(rng.integers(0, len(gt.category_ids), n), conf, b))
    return out


def test_prediction_dict_and_json_forms_identical(cuda, tmp_path):
    doc, _ = ref.make_problem(4, n_images=60, n_cats=8)
    gt, _ = _gt(tmp_path, doc)
    y = _random_predictions(gt, 4)
    res = tk.data.coco.to_results(gt, y)
    tk.data.coco.save_results(tmp_path / "res.json", res)
    a = tk.data.coco.evaluate(gt, y)
    b = tk.data.coco.evaluate(gt, res)
    c = tk.data.coco.evaluate(gt, tmp_path / "res.json")
    for k in ("precision", "recall", "scores", "stats"):
        assert getattr(a, k).tobytes() == getattr(b, k).tobytes() == getattr(c, k).tobytes(), k
    _assert_same(a, ref.evaluate(doc, res))
    sub = list(gt.image_ids[5:25])
    _assert_same(tk.data.coco.evaluate(gt, y[5:25], image_ids=sub), ref.evaluate(doc, res, image_ids=sub))


def _write_coco_dir(tmp_path, n=12, seed=0):
    rng = np.random.default_rng(seed)
    img_dir = tmp_path / "images"
    img_dir.mkdir()
    cats = [dict(id=c, name=f"cat{c}") for c in (90, 3, 17, 44)]  # non-contiguous, not sorted
    images, anns = [], []
    for i in range(n):
        iid = int(1000 - 37 * i)
        w, h = int(rng.integers(96, 200)), int(rng.integers(96, 200))
        Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(img_dir / f"{iid}.jpg", quality=90)
        images.append(dict(id=iid, file_name=f"{iid}.jpg", width=w, height=h))
        for _ in range(int(rng.integers(0, 4))):
            bw, bh = float(rng.uniform(8, w / 2)), float(rng.uniform(8, h / 2))
            anns.append(dict(id=len(anns) + 1, image_id=iid, category_id=int(rng.choice([90, 3, 17, 44])),
                             bbox=[float(rng.uniform(0, w - bw)), float(rng.uniform(0, h - bh)), bw, bh],
                             area=bw * bh, iscrowd=0))
    doc = dict(images=images, annotations=anns, categories=cats)
    (tmp_path / "instances.json").write_text(json.dumps(doc))
    return doc, tmp_path / "instances.json", img_dir


def test_end_to_end_predict_evaluate(cuda, tmp_path):
    from object_detector_amd.detector import ObjectDetector
    doc, path, img_dir = _write_coco_dir(tmp_path)
    X, _, names = tk.data.coco.load_od(path, img_dir)
    gt = tk.data.coco.load_gt(path)
    assert names == gt.category_names
    od = ObjectDetector.synthetic(4, (128, 128), num_classes=len(names), n_inflight=1)
    y = od.predict(X)
    assert sum(len(p) for p in y) > 0
    ev = tk.data.coco.evaluate(gt, y)
    _assert_same(ev, ref.evaluate(doc, tk.data.coco.to_results(gt, y)))


def test_coco_evaluate_script(cuda, tmp_path):
    from object_detector_amd import weights as W
    doc, path, img_dir = _write_coco_dir(tmp_path, n=8, seed=1)
    names = [c["name"] for c in sorted(doc["categories"], key=lambda c: c["id"])]
    W.save(tmp_path / "w.npz", W.random_init(3, len(names)), {"class_names": np.asarray(names)})
    script = str(ROOT / "scripts" / "coco_evaluate.py")
    base = [sys.executable, script, "--coco-json", str(path), "--coco-image-dir", str(img_dir)]
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}

    def run(*extra):
        r = subprocess.run(base + list(extra), capture_output=True, text=True, timeout=300, env=env, cwd=tmp_path)
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
        out = r.stdout + r.stderr
        return [ln[ln.index(" Average"):] for ln in out.splitlines() if " Average " in ln and "maxDets" in ln], out

    lines, out = run("--weights", str(tmp_path / "w.npz"), "--input-size", "128", "128", "--batch-size", "4",
                     "--save-results", str(tmp_path / "res.json"))
    assert len(lines) == 12 and "cat17" in out
    lines2, _ = run("--results-json", str(tmp_path / "res.json"))
    assert lines2 == lines
    # weights for another class count, or other class names, are refused
    W.save(tmp_path / "w5.npz", W.random_init(3, 5))
    r = subprocess.run(base + ["--weights", str(tmp_path / "w5.npz"), "--input-size", "128", "128"], capture_output=True,
                       text=True, timeout=300, env=env, cwd=tmp_path)
    assert r.returncode != 0 and "class" in (r.stdout + r.stderr)
    W.save(tmp_path / "wn.npz", W.random_init(3, len(names)), {"class_names": np.asarray(["a", "b", "c", "d"])})
    r = subprocess.run(base + ["--weights", str(tmp_path / "wn.npz"), "--input-size", "128", "128"], capture_output=True,
                       text=True, timeout=300, env=env, cwd=tmp_path)
    assert r.returncode != 0 and "class" in (r.stdout + r.stderr)
