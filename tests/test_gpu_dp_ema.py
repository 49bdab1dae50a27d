"""GPU: the averaged model under data parallelism -- two gloo ranks on the one GPU (the launch of tests/test_gpu_dp.py), three
steps on different shards.  Nothing new is exchanged: every rank applies the same update to the same masters, so the averages
stay identical."""
import json
import os
import pathlib
import socket
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = pathlib.Path(__file__).resolve().parent.parent
TIMEOUT = 300  # seconds per rank; a rank needs about ten


def _free_port():
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        return sk.getsockname()[1]


def test_two_ranks_keep_the_same_average(cuda, tmp_path):
    port = _free_port()
    procs = []
    for r in range(2):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
        procs.append(subprocess.Popen([sys.executable, str(ROOT / "tests" / "dp_ema_worker.py"), str(tmp_path)], env=env,
                                      stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
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
    r0, r1 = (json.loads((tmp_path / f"rank{r}.json").read_text()) for r in range(2))
    assert (r0["rank"], r1["rank"]) == (0, 1)
    for k in ("ema", "params", "initial_params", "initial_ema"):
        assert r0[k] == r1[k], k
    assert r0["ema_updates"] == r1["ema_updates"] == 3 and r0["skipped"] == r1["skipped"] == 0
    # the average moved, and is neither the starting point nor the last iterate
    assert r0["initial_ema"] == r0["initial_params"]
    assert r0["ema"] != r0["initial_params"] and r0["ema"] != r0["params"] and r0["params"] != r0["initial_params"]
    # BatchNorm statistics are per rank (each saw its own shard), and so are their averages
    assert r0["run_stats"] != r1["run_stats"] and r0["ema_run_stats"] != r1["ema_run_stats"]
