#!/usr/bin/env python3
"""Step time of flip test-time augmentation against the plain step, in ONE process: bench.py's default configuration (a
uint8 batch resident in HBM, submit() on 3 batches in flight, conf_threshold 0.01) at 32 x 320^2 and 16 x 640^2, the plain
detector and the tta=("flip",) detector timed alternately (the same windows see the same machine).  Prints one JSON line.

A TTA step runs the network twice, so the yardstick is TWICE the plain step: `over_2x` is tta / (2 * plain) - 1 (target
<= 0.10; DESIGN.md "Flip test-time augmentation")."""
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


def _median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2] if len(xs) % 2 else 0.5 * (xs[len(xs) // 2 - 1] + xs[len(xs) // 2])


def measure(params, size, batch, a, dev):
    from object_detector_amd.detector import ObjectDetector
    x = torch.from_numpy(np.random.default_rng(1000).integers(0, 256, (batch, size, size, 3), dtype=np.uint8)).to(dev)
    ods = {"plain": ObjectDetector(params, batch, (size, size), device=dev, use_multi_gpu=False, n_inflight=a.inflight),
           "vote_only": ObjectDetector(params, batch, (size, size), device=dev, use_multi_gpu=False, n_inflight=a.inflight,
                                       tta=()),
           "flip": ObjectDetector(params, batch, (size, size), device=dev, use_multi_gpu=False, n_inflight=a.inflight,
                                  tta=("flip",))}
    for od in ods.values():
        _window(od, x, a.warmup)
    times = {k: [] for k in ods}
    for _ in range(a.reps):
        for k, od in ods.items():  # alternate: every repetition times all three next to each other
            times[k].append(_window(od, x, a.steps))
    ms = {k: _median(v) * 1e3 for k, v in times.items()}
    rec = {"workload": f"inference {size}x{size} batch {batch}, {a.inflight} in flight, submit() per step",
           "ms_per_step": {k: round(v, 4) for k, v in ms.items()},
           "ms_per_step_reps": {k: [round(t * 1e3, 4) for t in v] for k, v in times.items()},
           "images_per_sec": {k: round(batch / v * 1e3, 1) for k, v in ms.items()},
           "flip_over_2x_plain": round(ms["flip"] / (2 * ms["plain"]) - 1, 4),
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
    out = {"metric": "tta_step_time", "steps": a.steps, "warmup": a.warmup, "reps": a.reps,
           "320_b32": measure(params, 320, 32, a, dev), "640_b16": measure(params, 640, 16, a, dev)}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
