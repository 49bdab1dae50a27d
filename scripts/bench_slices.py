#!/usr/bin/env python3
"""Step time of sliced inference against the plain step and the tta=() step, in ONE process: bench.py's default configuration
(a uint8 batch resident in HBM, 3 batches in flight, conf_threshold 0.01) at 30 x 320^2 and 15 x 640^2, where slices=(2, 2)
packs T = 5 tiles per image and G = 6 / 3 images per batch.  The plain, the tta=() and the sliced detector are timed
alternately (the same windows see the same machine).  Prints one JSON line.

The yardstick of the sliced step is the tta=() step at the same batch: both run the network once, take candidates, merge and
copy one record block; the sliced step adds the tile cutter (od_tiles_resize, from source images twice the input size that are
resident in HBM like the other detectors' batch) and ranks five lists per image.  `sliced_over_vote_only` is
sliced / vote_only - 1 (DESIGN.md "Sliced inference")."""
import argparse
import json
import time

import _common  # noqa: F401
import numpy as np
import torch


def _window(od, x, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        od.submit(x, conf_threshold=0.01)
    od.synchronize()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps


def _window_sliced(od, images, sizes, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        od._submit_sliced(0.01, sizes=sizes, images=images, cut_only=True)  # the images were uploaded by the warm-up
    od.synchronize()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps


def _median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2] if len(xs) % 2 else 0.5 * (xs[len(xs) // 2 - 1] + xs[len(xs) // 2])


def measure(params, size, batch, a, dev):
    from object_detector_amd.detector import ObjectDetector
    rng = np.random.default_rng(1000)
    x = torch.from_numpy(rng.integers(0, 256, (batch, size, size, 3), dtype=np.uint8)).to(dev)
    kw = dict(device=dev, use_multi_gpu=False, n_inflight=a.inflight)
    ods = {"plain": ObjectDetector(params, batch, (size, size), **kw),
           "vote_only": ObjectDetector(params, batch, (size, size), tta=(), **kw),
           "sliced": ObjectDetector(params, batch, (size, size), slices=(2, 2), **kw)}
    G = batch // ods["sliced"].slices.T
    images = [rng.integers(0, 256, (2 * size, 2 * size, 3), dtype=np.uint8) for _ in range(G)]
    sizes = [(2 * size, 2 * size)] * G
    for _ in range(a.inflight):  # every pipeline uploads the source images once
        ods["sliced"]._submit_sliced(0.01, images=images)
    ods["sliced"].synchronize()

    def window(k, steps):
        return _window_sliced(ods[k], images, sizes, steps) if k == "sliced" else _window(ods[k], x, steps)

    for k in ods:
        window(k, a.warmup)
    times = {k: [] for k in ods}
    for _ in range(a.reps):
        for k in ods:  # alternate: every repetition times all three next to each other
            times[k].append(window(k, a.steps))
    ms = {k: _median(v) * 1e3 for k, v in times.items()}
    rec = {"workload": f"inference {size}x{size} batch {batch}, {a.inflight} in flight; sliced: {G} images of "
                       f"{2 * size}x{2 * size}, 5 tiles each",
           "ms_per_step": {k: round(v, 4) for k, v in ms.items()},
           "ms_per_step_reps": {k: [round(t * 1e3, 4) for t in v] for k, v in times.items()},
           "sliced_over_vote_only": round(ms["sliced"] / ms["vote_only"] - 1, 4),
           "vote_only_over_plain": round(ms["vote_only"] / ms["plain"] - 1, 4)}
    del ods
    torch.cuda.empty_cache()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inflight", type=int, default=3)
    a = ap.parse_args()
    from object_detector_amd import weights as W
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    params = W.random_init(2)
    out = {"metric": "slices_step_time", "steps": a.steps, "warmup": a.warmup, "reps": a.reps,
           "320_b30": measure(params, 320, 30, a, dev), "640_b15": measure(params, 640, 15, a, dev)}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
