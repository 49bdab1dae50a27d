"""Child process of tests/test_gpu_dp_optim.py: ONE data-parallel rank of a Trainer that runs AdamW with gradient clipping,
on cuda:0 (gloo collectives, as tests/dp_worker.py).  Not a test module.

usage (environment RANK / LOCAL_RANK / WORLD_SIZE / MASTER_ADDR / MASTER_PORT set by the parent):
    python tests/dp_optim_worker.py <out_dir> <clip_grad_norm>
"""
import os
import pathlib
import sys

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

STEPS, ADAM_LR, BETAS, EPS, WD = 2, 1e-3, (0.9, 0.999), 1e-8, 1e-2


def main():
    out, clip = pathlib.Path(sys.argv[1]), float(sys.argv[2])
    os.environ["OD_TRAIN_BUCKET_MB"] = "8"
    os.environ["OD_DIST_BACKEND"] = "gloo"
    import torch
    import pytoolkit as tk
    from dp_worker import GLOBAL_B, LS, S, make_batch
    from object_detector_amd.trainer import Trainer
    from object_detector_amd import weights as W
    with tk.dl.session():  # creates the gloo group from the launcher environment, pins cuda:0
        rank, world = torch.distributed.get_rank(), torch.distributed.get_world_size()
        per = GLOBAL_B // world
        tr = Trainer(W.random_init(2), per, (S, S), device="cuda:0", lr=ADAM_LR, weight_decay=WD, loss_scale=LS, comm=None,
                     world_size=world, optimizer="adamw", betas=BETAS, adam_eps=EPS, clip_grad_norm=clip)
        rec = {}
        for step in range(STEPS):  # another global batch every step, this rank's shard of it
            x, anns = make_batch(GLOBAL_B, S, seed=5 + step)
            y = tr.pb.encode_batch(anns[rank * per:(rank + 1) * per], return_device=True)[0]
            tr._poll_nonfinite()
            tr.forward(torch.from_numpy(x[rank * per:(rank + 1) * per]).to("cuda:0"))
            tr.loss(y)
            tr.backward()
            tr.allreduce()
            torch.cuda.synchronize()
            rec[f"grads{step}"] = tr.grads.cpu().numpy()  # the reduced gradient this step's norm is taken from
            tr.sgd()
            torch.cuda.synchronize()
            rec[f"optim_state{step}"] = tr.optim_state.cpu().numpy()
            rec[f"flag{step}"] = tr.nonfinite.cpu().numpy()
        rec.update(params=tr.params.cpu().numpy(), mom=tr.mom.cpu().numpy(), mom2=tr.mom2.cpu().numpy(),
                   loss_scale=np.float64(tr.loss_scale), world=np.int64(world))
        if rank != 0:  # rank 0 alone keeps the gradients: 2 x 170 MB would be written for nothing
            rec = {k: v for k, v in rec.items() if not k.startswith("grads")}
        np.savez(out / f"rank{rank}.npz", **rec)


if __name__ == "__main__":
    main()
