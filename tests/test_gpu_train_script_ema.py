"""GPU: scripts/train.py with --ema, --save-state-every and --resume: a 40-step run that leaves a state file, and a second
process that continues it to step 60."""
import pathlib
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = pathlib.Path(__file__).resolve().parent.parent
TIMEOUT = 600  # seconds per run; a run needs well under a minute


def _train(args, cwd):
    r = subprocess.run([sys.executable, str(ROOT / "scripts" / "train.py")] + [str(a) for a in args], capture_output=True,
                       text=True, cwd=str(cwd), timeout=TIMEOUT)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-2500:])


def test_train_save_state_resume_and_ema_weights(cuda, tmp_path):
    from object_detector_amd import weights as W
    from object_detector_amd.detector import ObjectDetector
    common = ["--shapes", 64, "--batch-size", 8, "--input-size", 96, 96, "--from-scratch", "--ema", 0.99,
              "--save-state-every", 20, "--log-every", 20]
    one, two = tmp_path / "one", tmp_path / "two"
    _train(["--result-dir", one, "--steps", 40] + common, tmp_path)
    state = one / "state.npz"
    assert (one / "trained.npz").exists() and (one / "trained_ema.npz").exists() and state.exists()
    assert not (one / "state.npz.tmp").exists()
    log1 = (one / "train.log").read_text()
    assert "state of step 20 written" in log1 and "state of step 40 written" in log1 and "resumed from" not in log1
    sd = W.load_state(state)
    assert int(sd["step"]) == 40 and int(sd["ema_updates"]) == 40 and float(sd["ema_decay"]) == 0.99
    for k in ("params", "mom", "run_stats", "ema", "ema_run_stats"):
        assert sd[k].dtype == np.float32 and np.isfinite(sd[k]).all(), k
    assert (sd["ema"] != sd["params"]).any()

    _train(["--result-dir", two, "--steps", 60, "--resume", state] + common, tmp_path)
    log2 = (two / "train.log").read_text()
    assert re.search(r"resumed from \S+state\.npz: starting at step 40\b", log2), log2[-1500:]
    assert re.search(r"\bstep 60/60\b", log2) and not re.search(r"\bstep 20/", log2)
    assert re.search(r"ema_updates 60\b", log2.split("weight average:")[-1]), log2[-1500:]
    sd2 = W.load_state(two / "state.npz")
    assert int(sd2["step"]) == 60 and int(sd2["ema_updates"]) == 60
    assert (sd2["params"] != sd["params"]).any() and (sd2["mom"] != sd["mom"]).any()
    for d, steps_run in ((one, 40), (two, 20)):
        for name in ("trained.npz", "trained_ema.npz"):
            params, meta = W.load(d / name)
            assert float(meta["ema_decay"]) == 0.99 and len(meta["loss_history"]) == steps_run, (d, name)
            assert all(np.isfinite(v).all() for v in params.values())
    plain, _ = W.load(two / "trained.npz")
    avg, _ = W.load(two / "trained_ema.npz")
    assert list(plain) == list(avg) and any((plain[k] != avg[k]).any() for k in plain)
    od = ObjectDetector(avg, 2, (96, 96), device=cuda)
    from oracle import network as onet
    keep, cnt = od.predict_batch_device(torch.from_numpy(onet.synthetic_images(2, 96, seed=0)).to(cuda), conf_threshold=0.01)
    torch.cuda.synchronize()
    assert torch.isfinite(od.net.pred).all() and int(cnt.min()) >= 0
