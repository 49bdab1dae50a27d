"""The acceptance loop of tests/test_gpu_functional_loop.py with the two opt-in features on: scripts/train.py --mosaic 0.5
--ignore-regions on a generated "shapes" set that HAS difficult objects and crowd regions, then scripts/voc_validate.py on
held-out images -- every script a fresh child process.  Same recipe (512 images, 1200 steps of 32 x 320^2, lr 0.02, cosine
schedule with 50 warm-up steps, base network at the full rate, seed 0) and the same demands: finite loss, no skipped step,
loss down by a factor of 10, and the existing test's own floor of 80 for the mAP that voc_validate logs.

A shapes set cannot show that mosaic HELPS on real data (its objects are flat rectangles that a detector learns in a few
hundred steps either way); what this pins is that the whole path -- partner draws, od_augment_mosaic, slivers and marked
boxes as ignore regions through od_assign_anchors_ign, the all-zero rows in the loss -- trains a detector that works."""
import json
import pathlib
import re
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "scripts"))

STEPS = 1200


def test_train_with_mosaic_and_ignore_regions_then_voc_validate(cuda, tmp_path):
    import _common
    from object_detector_amd import weights as W
    wpath = tmp_path / "trained.npz"
    r = subprocess.run([sys.executable, str(ROOT / "scripts" / "train.py"), "--shapes", "512", "--shapes-difficult", "0.1",
                        "--shapes-crowd", "0.25", "--steps", str(STEPS), "--from-scratch", "--mosaic", "0.5",
                        "--ignore-regions", "--seed", "0", "--result-dir", str(tmp_path / "train"), "--out", str(wpath)],
                       capture_output=True, text=True, cwd=str(tmp_path), timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    log = (tmp_path / "train" / "train.log").read_text()
    m = re.search(r"skipped (\d+), loss scale", log)
    assert m and int(m.group(1)) == 0, log[-2000:]
    stats = re.search(r"mosaic: (\{.*\})", log)
    assert stats, log[-2000:]
    stats = json.loads(stats.group(1).replace("'", '"'))
    print("generator stats:", stats)
    assert 0 < stats["mosaics"] < (STEPS + 8) * 32 and stats["boxes_ignored"] > 0
    _params, meta = W.load(wpath)
    hist = np.asarray(meta["loss_history"], np.float64)
    assert len(hist) == STEPS and np.isfinite(hist).all()
    first, last = float(hist[:3].mean()), float(hist[-50:].mean())
    print(f"total loss: first 3 steps {first:.3f} -> last 50 steps {last:.3f} ({first / last:.1f}x)")
    assert last * 10.0 <= first, (first, last)
    Xv, yv = _common.shapes_dataset(64, seed=1000)  # held out, and plain: what test_gpu_functional_loop.py validates on
    _common.write_voc_layout(tmp_path / "VOCdevkit", Xv, yv)
    res = tmp_path / "results"
    r = subprocess.run([sys.executable, str(ROOT / "scripts" / "voc_validate.py"), "--vocdevkit-dir", str(tmp_path / "VOCdevkit"),
                        "--result-dir", str(res), "--weights", str(wpath)], capture_output=True, text=True, cwd=str(tmp_path),
                       timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    line = [ln for ln in (res / "validate.log").read_text().splitlines() if "mAP=" in ln]
    assert len(line) == 1
    m_all, m07 = (float(line[0].split(tag)[1].split()[0]) for tag in ("mAP=", "mAP(VOC2007)="))
    print(line[0])
    print(json.dumps({"train_steps": STEPS, "mosaic": 0.5, "ignore_regions": True, "loss_first3": first, "loss_last50": last,
                      "mAP": m_all, "mAP_VOC2007": m07, "generator_stats": stats}))  # profiles/mosaic_ignore keeps one
    assert m07 >= 80.0 and m_all >= 80.0, line[0]
