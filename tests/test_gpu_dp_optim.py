"""GPU: AdamW with gradient clipping under data parallelism -- two gloo ranks on the one GPU (the launch of
tests/test_gpu_dp.py), two steps on different shards.  Nothing new is exchanged: every rank takes the norm of the identical
all-reduced buffer in the same fixed order, so the clipping coefficient, the bias correction and the update are the same
bits on both ranks."""
import os
import pathlib
import socket
import subprocess
import sys

import numpy as np
import pytest

import optim2_ref as R2

pytestmark = pytest.mark.gpu

ROOT = pathlib.Path(__file__).resolve().parent.parent
TIMEOUT = 300  # seconds per rank; a rank needs about ten
CLIP = 0.05    # far below the gradient norm of a randomly initialised detector (asserted: the clipping engages)


def _free_port():
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        return sk.getsockname()[1]


def _launch(tmp_path):
    port = _free_port()
    procs = []
    for r in range(2):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
        procs.append(subprocess.Popen([sys.executable, str(ROOT / "tests" / "dp_optim_worker.py"), str(tmp_path), str(CLIP)],
                                      env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    outs = []
    try:
        for p in procs:
            outs.append(p.communicate(timeout=TIMEOUT)[0])
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
                p.communicate()
    bad = [f"--- rank {r} (rc {p.returncode}) ---\n{o[-2500:]}" for r, (p, o) in enumerate(zip(procs, outs)) if p.returncode != 0]
    assert not bad and len(outs) == 2, "\n".join(bad)


def test_two_ranks_adamw_clipped_same_bits(cuda, tmp_path):
    from object_detector_amd import _lib
    sys.path.insert(0, str(ROOT / "tests"))
    import dp_optim_worker as D
    _launch(tmp_path)
    r0, r1 = (np.load(tmp_path / f"rank{r}.npz") for r in range(2))
    for k in ("params", "mom", "mom2") + tuple(f"optim_state{s}" for s in range(D.STEPS)):
        a, b = r0[k].view(np.uint32), r1[k].view(np.uint32)
        assert np.array_equal(a, b), f"{k}: {int((a != b).sum())} of {a.size} words differ between the ranks"
    assert np.abs(r0["mom2"]).max() > 0 and np.isfinite(r0["params"]).all()
    # the norm, the coefficient and the bias correction are prepare_ref's on the reduced gradient rank 0 saved
    inv = 1.0 / (float(r0["loss_scale"]) * int(r0["world"]))
    st = R2.new_state()
    for s in range(D.STEPS):
        assert int(r0[f"flag{s}"][0]) == 0
        flag, ssq = R2.grad_stats_ref(r0[f"grads{s}"])
        got = _lib.OptimState.from_buffer_copy(r0[f"optim_state{s}"].tobytes())
        # (the device adds the squares in another order than numpy: both are tree-like sums whose f64 results agree to a few
        # 1e-15 relative, and the rounding to f32 in front of the square root keeps 6e-8 of that)
        st = R2.prepare_ref(st, ssq, flag, inv, CLIP, *D.BETAS)
        print(f"step {s}: grad_norm {got.grad_norm!r} clip_coef {got.clip_coef!r} (prepare_ref {st['grad_norm']!r})")
        for k in ("grad_norm", "clip_coef", "inv_scale_eff", "b1pow", "b2pow", "bc1", "bc2"):
            assert np.float32(getattr(got, k)).view(np.uint32) == np.float32(st[k]).view(np.uint32), (s, k)
        assert got.step == st["step"] == s + 1 and 0.0 < got.clip_coef < 1.0, "the clipping did not engage"
