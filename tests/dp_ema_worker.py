"""Child process of tests/test_gpu_dp_ema.py: ONE data-parallel rank of a Trainer that keeps an averaged model, on cuda:0
(gloo collectives, as tests/dp_worker.py).  Not a test module.

usage (environment RANK / LOCAL_RANK / WORLD_SIZE / MASTER_ADDR / MASTER_PORT set by the parent):
    python tests/dp_ema_worker.py <out_dir>
"""
import hashlib
import json
import os
import pathlib
import sys

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

STEPS, DECAY = 3, 0.999


def digest(t):
    return hashlib.sha256(t.detach().cpu().numpy().tobytes()).hexdigest()


def main():
    out = pathlib.Path(sys.argv[1])
    os.environ["OD_TRAIN_BUCKET_MB"] = "8"
    os.environ["OD_DIST_BACKEND"] = "gloo"
    import torch
    import pytoolkit as tk
    from dp_worker import GLOBAL_B, LR, LS, S, make_batch
    from object_detector_amd import weights as W
    from object_detector_amd.trainer import Trainer
    with tk.dl.session():  # creates the gloo group from the launcher environment, pins cuda:0
        rank, world = torch.distributed.get_rank(), torch.distributed.get_world_size()
        per = GLOBAL_B // world
        tr = Trainer(W.random_init(2), per, (S, S), device="cuda:0", lr=LR, momentum=0.9, loss_scale=LS, comm=None,
                     world_size=world, ema_decay=DECAY)
        rec = {"rank": rank, "initial_params": digest(tr.params), "initial_ema": digest(tr.ema)}
        for step in range(STEPS):  # another global batch every step, this rank's shard of it
            x, anns = make_batch(GLOBAL_B, S, seed=5 + step)
            tr.step(torch.from_numpy(x[rank * per:(rank + 1) * per]).to("cuda:0"), anns[rank * per:(rank + 1) * per])
        tr._poll_nonfinite(wait=True)
        torch.cuda.synchronize()
        rec.update(ema=digest(tr.ema), ema_run_stats=digest(tr.ema_run_stats), params=digest(tr.params),
                   run_stats=digest(tr.run_stats), ema_updates=tr.ema_updates, skipped=tr.skipped_steps)
        (out / f"rank{rank}.json").write_text(json.dumps(rec))


if __name__ == "__main__":
    main()
