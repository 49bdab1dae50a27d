"""Child process of tests/test_gpu_dp.py: ONE data-parallel rank of a Trainer on cuda:0 (gloo collectives, as
tests/dp_worker.py) running 8 steps in which the ranks' timing differs as much as it can: rank 0 waits for the device after
every step and alone calls state_dict() after step 3 (what scripts/train.py --save-state-every does on the main process), rank
1 keeps a spin kernel in front of every sgd().  An Inf goes into rank 1's loss gradient at steps 2 and 5; after the all-reduce
both ranks' flags are set.  Every rank issues the same collectives in the same order whatever its loss-scale control does.
Not a test module.

usage (environment RANK / LOCAL_RANK / WORLD_SIZE / MASTER_ADDR / MASTER_PORT set by the parent):
    python tests/dp_schedule_worker.py <out_dir> <spin_ms>
"""
import os
import pathlib
import sys

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

STEPS = 8


def main():
    out, spin_ms = pathlib.Path(sys.argv[1]), float(sys.argv[2])
    os.environ["OD_TRAIN_BUCKET_MB"] = "8"
    os.environ["OD_DIST_BACKEND"] = "gloo"
    import torch
    import pytoolkit as tk
    import loss_scale_sched as L
    from dp_worker import GLOBAL_B, LR, LS, S, make_batch
    from object_detector_amd import weights as W
    from object_detector_amd.trainer import Trainer
    with tk.dl.session():  # creates the gloo group from the launcher environment, pins cuda:0
        rank, world = torch.distributed.get_rank(), torch.distributed.get_world_size()
        x, anns = make_batch(GLOBAL_B, S)
        per = GLOBAL_B // world
        tr = Trainer(W.random_init(2), per, (S, S), device="cuda:0", lr=LR, momentum=0.9, loss_scale=LS, comm=None,
                     world_size=world)
        tr.loss_scale_growth_interval = L.INTERVAL
        xt = torch.from_numpy(x[rank * per:(rank + 1) * per]).to("cuda:0")
        y = tr.pb.encode_batch(anns[rank * per:(rank + 1) * per], return_device=True)[0]
        lazy = rank == 1
        spin = int(spin_ms * L.ticks_per_ms()) if lazy else 0

        def after(i):
            if rank == 0 and i == 3:
                tr.state_dict()
        hist, flags = L.run_steps(tr, xt, y, STEPS, inject=L.INJECT if rank == 1 else (), spin=spin, eager=not lazy,
                                  after_step=after)
        torch.cuda.synchronize()
        pending = len(tr._flag_queue)
        tr._poll_nonfinite(wait=True)
        np.savez(out / f"schedule_rank{rank}.npz", history=np.array(hist, np.float64), flags=flags.cpu().numpy(),
                 final=np.array(L.control(tr), np.float64), pending=pending, params=tr.params.cpu().numpy(),
                 mom=tr.mom.cpu().numpy(), spin_ticks=spin)


if __name__ == "__main__":
    main()
