"""The real data-parallel path with N > 1 ranks, on the one GPU the test box has (reference knob
use_multi_gpu=True, check_assign.py:19 / voc_validate.py:26): two fresh child processes on cuda:0, gloo collectives, each
running `Trainer.step` on its half of a global batch with the BUCKETED, OVERLAPPED all-reduce enabled (buckets routed through
torch.distributed when there is no RCCL communicator).  On an 8-GPU node the same code runs with backend nccl = RCCL."""
import os
import pathlib
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = pathlib.Path(__file__).resolve().parent.parent


def _free_port():
    """A port that is free NOW, chosen by the kernel (a fixed port number fails the whole test when something else holds it)."""
    import socket
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        return sk.getsockname()[1]


def _launch(world, args, cwd=None, script=None, extra_env=None):
    procs = []
    port = _free_port()
    for r in range(world):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0", **(extra_env or {}))
        procs.append(subprocess.Popen([sys.executable, str(script or ROOT / "tests" / "dp_worker.py")] + list(args), env=env,
                                      cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    outs = [p.communicate(timeout=600)[0] for p in procs]
    bad = [f"--- rank {r} (rc {p.returncode}) ---\n{o[-2500:]}" for r, (p, o) in enumerate(zip(procs, outs)) if p.returncode != 0]
    assert not bad, "\n".join(bad)
    return outs


@pytest.fixture(scope="module")
def sequential_shards(cuda):
    """The two shards' gradients computed one after the other in THIS process (world 1, no exchange)."""
    sys.path.insert(0, str(ROOT / "tests"))
    import dp_worker as D
    from object_detector_amd import weights as W
    from object_detector_amd.trainer import Trainer
    x, anns = D.make_batch(D.GLOBAL_B, D.S)
    per = D.GLOBAL_B // 2
    gs = []
    for r in range(2):
        tr = Trainer(W.random_init(2), per, (D.S, D.S), device=cuda, lr=D.LR, momentum=0.9, loss_scale=D.LS)
        y, _n, _ = tr.pb.encode_batch(anns[r * per:(r + 1) * per], return_device=True)
        tr.forward(torch.from_numpy(x[r * per:(r + 1) * per]).to(cuda))
        tr.loss(y)
        gs.append(tr.backward().cpu().numpy().copy())
        seg = dict(tr.seg)
        params0 = tr.params.cpu().numpy().copy()
    return gs, seg, params0, D


def test_two_ranks_bucketed_allreduce_equals_sum_of_shards(cuda, sequential_shards, tmp_path):
    (g0, g1), seg, params0, D = sequential_shards
    _launch(2, [str(tmp_path), "f32", "8"])
    r0 = np.load(tmp_path / "rank0_f32_8.npz")
    r1 = np.load(tmp_path / "rank1_f32_8.npz")
    assert int(r0["nbuckets"]) >= 4
    # both ranks end the step with bit-identical gradients, momentum and parameters
    for k in ("grads", "mom", "params"):
        assert np.array_equal(r0[k], r1[k]), k
    # and the exchanged gradient is the f32 sum of the two shards' gradients (one addition per element: order-free), for
    # EVERY element: since round 2 the first layer's weight gradient is a fixed-order slab sum too, nothing uses atomics
    mask = np.ones(g0.size, bool)
    want = g0 + g1
    assert np.array_equal(r0["grads"], want)
    # the optimizer averaged over the ranks: w1 = w0 - lr_seg * (sum / (loss_scale * world))   (momentum buffer was zero)
    from object_detector_amd.trainer import lr_multiplier
    for (name, kind), (o, n) in list(seg.items())[::17]:
        step = D.LR * lr_multiplier(name) * want[o:o + n] / (D.LS * 2)
        np.testing.assert_allclose(r0["params"][o:o + n], params0[o:o + n] - step, rtol=1e-5, atol=1e-7)
    # one collective after backward instead of overlapped buckets: same numbers
    _launch(2, [str(tmp_path), "f32", "0"])
    assert np.array_equal(np.load(tmp_path / "rank0_f32_0.npz")["grads"][mask], r0["grads"][mask])


def test_two_ranks_bf16_payload_cost(cuda, sequential_shards, tmp_path):
    """BASELINE.json configs[4]: bf16 gradient payload.  Its accuracy cost against the f32 payload, per parameter segment."""
    (g0, g1), seg, _p0, D = sequential_shards
    _launch(2, [str(tmp_path), "bf16", "8"])
    r0 = np.load(tmp_path / "rank0_bf16_8.npz")
    r1 = np.load(tmp_path / "rank1_bf16_8.npz")
    assert np.array_equal(r0["grads"], r1["grads"]) and np.array_equal(r0["params"], r1["params"])
    want = (g0 + g1).astype(np.float64)
    rel = {}
    for (name, kind), (o, n) in seg.items():
        rel[f"{name}.{kind}"] = float(np.linalg.norm(r0["grads"][o:o + n] - want[o:o + n]) / max(np.linalg.norm(want[o:o + n]), 1e-30))
    worst = sorted(rel.items(), key=lambda kv: -kv[1])[:4]
    print("bf16 payload vs f32 payload, relative L2 per segment: worst", worst, "median", float(np.median(list(rel.values()))))
    # two roundings to bf16 (8-bit mantissa: 2^-9 relative each) + one bf16 sum
    assert worst[0][1] < 6e-3 and np.median(list(rel.values())) < 4e-3
    # every value the ranks hold is a bf16 number widened to f32
    assert (r0["grads"].view(np.uint32) & 0xFFFF == 0).all()


def test_voc_validate_two_ranks(cuda, tmp_path):
    """scripts/voc_validate.py under a 2-rank launch (use_multi_gpu=True did nothing in the entry points): the
    ranks shard the images, ONE validate.log is written, and its mAP line equals the single-process run's."""
    args = ["--synthetic", "6", "--batch-size", "2", "--input-size", "96", "96"]
    one = tmp_path / "one"
    two = tmp_path / "two"
    r = subprocess.run([sys.executable, str(ROOT / "scripts" / "voc_validate.py"), "--result-dir", str(one)] + args,
                       capture_output=True, text=True, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-2000:]
    _launch(2, ["--result-dir", str(two)] + args, cwd=str(tmp_path), script=ROOT / "scripts" / "voc_validate.py",
            extra_env={"OD_DIST_BACKEND": "gloo"})
    get = lambda p: [ln.split("] ", 1)[1] for ln in (p / "validate.log").read_text().splitlines() if "mAP=" in ln]
    assert len(get(two)) == 1 and get(two) == get(one), (get(one), get(two))


def test_train_script_two_ranks_learns_and_ranks_agree(cuda, tmp_path):
    """scripts/train.py under a 2-rank launch (gloo on the one GPU; RCCL on a real node): every rank trains on ITS shard of the
    generated images, gradients are all-reduced every step, rank 0 writes ONE weights file -- and the loss falls like the
    single-process run's (data-parallel SGD on 2 x 16 images = the 32-image batch in expectation)."""
    args = ["--shapes", "128", "--steps", "120", "--warmup", "10", "--batch-size", "16", "--input-size", "160", "160",
            "--from-scratch", "--log-every", "40"]
    two = tmp_path / "two"
    _launch(2, ["--result-dir", str(two)] + args, cwd=str(tmp_path), script=ROOT / "scripts" / "train.py",
            extra_env={"OD_DIST_BACKEND": "gloo"})
    log = (two / "train.log").read_text()
    assert log.count("weights written to") == 1 and (two / "trained.npz").exists()
    with np.load(two / "trained.npz") as z:
        hist = z["__meta__.loss_history"]
        assert all(np.isfinite(z[k]).all() for k in z.files)
    assert len(hist) == 120 and np.isfinite(hist).all()
    first, last = float(hist[:3].mean()), float(hist[-20:].mean())
    print(f"2-rank train.py: loss {first:.3f} -> {last:.3f}")
    assert last * 1.8 <= first, (first, last)  # (120 short steps at 160^2: measured 8.76 -> 4.12)


def test_two_ranks_with_different_timing_keep_one_loss_scale_schedule(cuda, tmp_path):
    """tests/dp_schedule_worker.py: 8 steps on two ranks whose hosts run as differently as they can -- rank 0 waits for the
    device after every step and alone calls state_dict() after step 3, rank 1 holds every sgd() back with a spin kernel
    four single-process steps long -- with an Inf in rank 1's loss gradient at steps 2 and 5.  Both ranks apply each flag two
    steps behind its step: one history of control values, the reference's, and bit-identical params and momentum.  (A rank
    that halved its scale one step before the other would scale its dz and unscale the summed gradient by another factor than
    its peer, and nothing brings the weights together again.)"""
    sys.path.insert(0, str(ROOT / "tests"))
    import dp_worker as D
    import loss_scale_sched as L
    import optim_ref as R
    from object_detector_amd import weights as W
    from object_detector_amd.trainer import Trainer
    x, anns = D.make_batch(D.GLOBAL_B, D.S)
    tr = Trainer(W.random_init(2), 2, (D.S, D.S), device=cuda, lr=D.LR, momentum=0.9, loss_scale=D.LS)
    y = tr.pb.encode_batch(anns[:2], return_device=True)[0]
    step_ms = L.measure_step_ms(tr, torch.from_numpy(x[:2]).to(cuda), y)
    del tr, y
    torch.cuda.empty_cache()
    print(f"single-process step {step_ms:.2f} ms, rank 1 spins {L.SPIN_STEPS * step_ms:.1f} ms in front of sgd()")
    _launch(2, [str(tmp_path), f"{L.SPIN_STEPS * step_ms:.3f}"], script=ROOT / "tests" / "dp_schedule_worker.py")
    r0 = np.load(tmp_path / "schedule_rank0.npz")
    r1 = np.load(tmp_path / "schedule_rank1.npz")
    want = R.loss_scale_ref(L.FLAGS, L.LAG, D.LS, L.INTERVAL, steps=8 + L.LAG)
    h0, h1 = ([tuple(row) for row in r["history"].tolist()] for r in (r0, r1))
    print("rank 0", h0, "\nrank 1", h1, "\nref   ", want[:8])
    assert int(r1["spin_ticks"]) > 0 and int(r0["spin_ticks"]) == 0
    assert r0["flags"].tolist() == r1["flags"].tolist() == L.FLAGS, "rank 1's Inf did not reach both ranks' flags"
    # every statement is looked at before the test fails, so that one failure shows what went apart and what followed from it
    wrong = []
    if h0 != want[:8]:
        wrong.append(f"rank 0 (eager, state_dict() after step 3) leaves the reference at step {[a == b for a, b in zip(h0, want)].index(False)}")
    if h1 != want[:8]:
        wrong.append(f"rank 1 (lazy) leaves the reference at step {[a == b for a, b in zip(h1, want)].index(False)}")
    for k in ("params", "mom"):
        differ = int((r0[k].view(np.uint32) != r1[k].view(np.uint32)).sum())
        if differ:
            wrong.append(f"{k}: {differ} of {r0[k].size} elements differ between the ranks")
    if not np.isfinite(r0["params"]).all():
        wrong.append("rank 0's params are not finite")
    for rank, r in enumerate((r0, r1)):
        if int(r["pending"]) != L.LAG:
            wrong.append(f"rank {rank} ends the run with {int(r['pending'])} flags pending, not {L.LAG}")
        if tuple(r["final"].tolist()) != want[8 + L.LAG - 1] or int(r["final"][1]) != 2:
            wrong.append(f"rank {rank} after the final drain: {tuple(r['final'].tolist())}, reference {want[8 + L.LAG - 1]}")
    assert not wrong, "\n".join(wrong)
