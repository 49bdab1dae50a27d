#!/usr/bin/env python3
"""Step time of Soft-NMS against the greedy step, in ONE process: bench.py's default configuration (a uint8 batch resident in
HBM, submit() on 3 batches in flight, conf_threshold 0.01) at 32 x 320^2, detectors built with nms="hard", "soft-linear" and
"soft-gaussian" timed alternately (the same windows see the same machine) -- and the stand-alone time of the suppression
call on a worst-case list: K = 1024 candidates of one class in one cluster, a Gaussian decay wide enough that every round
rescales every candidate and max_det = 200 are kept (od_soft_nms), beside od_nms on the same list.  Prints one JSON line.

The yardstick is the hard step of the same run (DESIGN.md "Soft-NMS")."""
import argparse
import ctypes as C
import json
import time

import _common  # noqa: F401
import numpy as np
import torch

METHODS = ("hard", "soft-linear", "soft-gaussian")


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


def measure_step(params, size, batch, a, dev):
    from object_detector_amd.detector import ObjectDetector
    x = torch.from_numpy(np.random.default_rng(1000).integers(0, 256, (batch, size, size, 3), dtype=np.uint8)).to(dev)
    ods = {m: ObjectDetector(params, batch, (size, size), device=dev, use_multi_gpu=False, n_inflight=a.inflight, nms=m)
           for m in METHODS}
    for od in ods.values():
        _window(od, x, a.warmup)
    times = {k: [] for k in ods}
    for _ in range(a.reps):
        for k, od in ods.items():  # alternate: every repetition times all three next to each other
            times[k].append(_window(od, x, a.steps))
    ms = {k: _median(v) * 1e3 for k, v in times.items()}
    kept = {}
    for k, od in ods.items():
        _, kc = od.collect(od.submit(x, conf_threshold=0.01))
        kept[k] = round(float(kc.float().mean()), 1)
    rec = {"workload": f"inference {size}x{size} batch {batch}, {a.inflight} in flight, submit() per step",
           "ms_per_step": {k: round(v, 4) for k, v in ms.items()},
           "ms_per_step_reps": {k: [round(t * 1e3, 4) for t in v] for k, v in times.items()},
           "images_per_sec": {k: round(batch / v * 1e3, 1) for k, v in ms.items()},
           "kept_per_image": kept,
           "over_hard": {k: round(ms[k] / ms["hard"] - 1, 4) for k in METHODS[1:]}}
    del ods
    torch.cuda.empty_cache()
    return rec


def worst_case_list(B, K, P, seed=1):
    """One class, one cluster: every box holds the image centre, so every pair overlaps.  -> boxes [B,P,4], keys u64 [B,K]."""
    rng = np.random.default_rng(seed)
    lo = 0.48 - 0.45 * rng.random((B, P, 2))
    hi = 0.52 + 0.45 * rng.random((B, P, 2))
    boxes = np.concatenate([lo, hi], 2).astype(np.float32)
    conf = (1.0 - 0.5 * np.arange(K) / K).astype(np.float32)  # descending, candidate r sits on prior r (NC = 1)
    keys = (conf.view(np.uint32).astype(np.uint64) << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - np.arange(K, dtype=np.uint64))
    return boxes, np.broadcast_to(keys, (B, K)).copy()


def measure_scan(a, dev):
    from object_detector_amd import _lib
    from object_detector_amd.net import Context
    ctx = Context.get(dev)
    lib, h = ctx.lib, ctx.handle
    K = P = 1024
    out = {}
    for B in (1, 32):
        boxes, keys = worst_case_list(B, K, P)
        bt, kt = torch.from_numpy(boxes).to(dev), torch.from_numpy(keys.view(np.int64)).to(dev)
        ct = torch.full((B,), K, dtype=torch.int32, device=dev)
        kf = torch.empty((B, 200), dtype=torch.int32, device=dev)
        kconf = torch.empty((B, 200), dtype=torch.float32, device=dev)
        kc = torch.empty((B,), dtype=torch.int32, device=dev)
        det = torch.empty((B, 1201), dtype=torch.float32, device=dev)
        nb = lib.od_nms_workspace_bytes(B, K)
        ws = torch.empty((nb,), dtype=torch.uint8, device=dev)
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        # sigma = 50: a weight of exp(-iou^2 / 50) >= 0.98 per round, so no score falls to min_conf within 200 rounds
        cfg = _lib.SoftNmsCfg(_lib.OD_NMS_SOFT_GAUSSIAN, 0, 200, 0.45, 50.0, 1e-6)

        def soft():
            _lib.check(lib.od_soft_nms(h, bt.data_ptr(), kt.data_ptr(), ct.data_ptr(), B, P, 1, K, C.byref(cfg), kf.data_ptr(),
                                       kconf.data_ptr(), kc.data_ptr(), det.data_ptr(), ws.data_ptr(), nb, st), "od_soft_nms")

        def hard():
            _lib.check(lib.od_nms(h, bt.data_ptr(), kt.data_ptr(), ct.data_ptr(), B, P, 1, K, 0.45, 0, 200, kf.data_ptr(),
                                  kc.data_ptr(), ws.data_ptr(), nb, st), "od_nms")

        rec = {}
        for name, fn in (("od_soft_nms", soft), ("od_nms", hard)):
            for _ in range(3):
                fn()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.scan_reps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            rec[name + "_us"] = round(e0.elapsed_time(e1) * 1e3 / a.scan_reps, 2)
            rec[name + "_kept"] = int(kc[0])
        out[f"B{B}"] = rec
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inflight", type=int, default=3)
    ap.add_argument("--scan-reps", type=int, default=50)
    a = ap.parse_args()
    from object_detector_amd import weights as W
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    params = W.random_init(2)
    out = {"metric": "soft_nms_step_time", "steps": a.steps, "warmup": a.warmup, "reps": a.reps,
           "320_b32": measure_step(params, 320, 32, a, dev),
           "worst_case_scan": {"list": "K = 1024, one class, one cluster, gaussian sigma 50, max_det 200", **measure_scan(a, dev)}}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
