#!/usr/bin/env python3
"""Trainer -> detector weight refresh on the GPU (ObjectDetector.refresh_from: one od_net_refresh launch) against the host
route it replaces (Trainer.export_params + a new ObjectDetector), in ONE process.  Prints one JSON line.

Per input size (320^2 and 640^2; the weights, and so the bytes the launch moves, are the same at both):
  refresh_us       raw and averaged weights: median over `reps` windows of `calls` refresh_from() calls after `warmup`,
                   one HIP-event pair per call (event wait, launch, event record: what a caller pays on the stream)
  refresh_gbps     the bytes the launch must move (f32 sources read once, every destination element written once,
                   counted from the table) over that time
  copy_gbps        a device-to-device copy that reads and writes the same number of bytes, timed the same way: the
                   bandwidth the launch is judged against
  host_route_s     export_params() + ObjectDetector(params, ...) + a device synchronise, host clock, median of 3
  validation_s     one Validator pass over 64 generated images (refresh, predict, VOC evaluate), host clock: the first
                   pass and the median of the next three"""
import argparse
import json
import time

import _common
import numpy as np
import torch


def _events(fn, calls):
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(calls)]
    torch.cuda.synchronize()
    for a, b in evs:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return [a.elapsed_time(b) * 1e3 for a, b in evs]  # microseconds


def _table_bytes(net, trainer):
    """(bytes read, bytes written) by one od_net_refresh over `net`'s table."""
    from object_detector_amd.net import refresh_layers
    rd = wr = 0
    for L in refresh_layers(trainer, net._dev):
        rd += 4 * L.Cout * L.ksize * L.ksize * L.Cin
        wr += 2 * L.Cout_pad * L.Kpad
        if L.scale_dst:
            rd += 4 * L.Cout * (4 if L.has_bn else 1)
            wr += 8 * L.Cout_pad
    return rd, wr


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[320, 640])
    ap.add_argument("--batch", type=int, default=16, help="batch size of the detector")
    ap.add_argument("--train-batch", type=int, default=2, help="batch size of the trainer (its weights are what is read)")
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--val-images", type=int, default=64)
    a = ap.parse_args()
    from object_detector_amd import weights as W
    from object_detector_amd.detector import ObjectDetector
    from object_detector_amd.trainer import Trainer
    from object_detector_amd.validate import Validator
    dev = torch.device("cuda:0")
    rec = {"workload": f"refresh of a Darknet53 detector (batch {a.batch}) from a live Trainer, {a.reps} x {a.calls} calls "
                       f"after {a.warmup}", "sizes": {}}
    Xv, yv = _common.shapes_dataset(a.val_images, seed=1000)
    for size in a.sizes:
        tr = Trainer(W.random_init(2), a.train_batch, (size, size), device=dev, ema_decay=0.999)
        od = ObjectDetector.from_trainer(tr, batch_size=a.batch)
        rd, wr = _table_bytes(od.net, tr)
        src = torch.empty((rd + wr) // 2, dtype=torch.uint8, device=dev)
        dst = torch.empty_like(src)
        fns = {"raw": lambda: od.refresh_from(tr), "ema": lambda: od.refresh_from(tr, ema=True),
               "copy": lambda: dst.copy_(src, non_blocking=True)}
        times = {k: [] for k in fns}
        for fn in fns.values():
            _events(fn, a.warmup)
        for _ in range(a.reps):  # alternating: the same windows see the same machine
            for k, fn in fns.items():
                times[k].append(_events(fn, a.calls))
        med = {k: float(np.median(np.concatenate(v))) for k, v in times.items()}
        spread = {k: float(max(np.median(w) for w in v) - min(np.median(w) for w in v)) for k, v in times.items()}
        host = []
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            od2 = ObjectDetector(tr.export_params(), a.batch, (size, size), device=dev)
            torch.cuda.synchronize()
            host.append(time.perf_counter() - t0)
            del od2
        v = Validator(od, Xv, yv)
        val = []
        for i in range(4):
            t0 = time.perf_counter()
            v(tr, i)
            val.append(time.perf_counter() - t0)
        gbps = lambda us: round((rd + wr) / (us * 1e-6) / 1e9, 1)  # noqa: E731
        rec["sizes"][str(size)] = {
            "bytes_read": rd, "bytes_written": wr,
            "refresh_us": {k: round(med[k], 2) for k in ("raw", "ema")},
            "refresh_spread_us": {k: round(spread[k], 2) for k in ("raw", "ema")},
            "refresh_gbps": {k: gbps(med[k]) for k in ("raw", "ema")},
            "copy_us": round(med["copy"], 2), "copy_gbps": gbps(med["copy"]),
            "refresh_over_copy_bandwidth": round(med["copy"] / med["raw"], 3),
            "host_route_s": round(float(np.median(host)), 3),
            "host_route_over_refresh": round(float(np.median(host)) / (med["raw"] * 1e-6)),
            "validation_s": {"first": round(val[0], 3), "next": round(float(np.median(val[1:])), 3),
                             "images": a.val_images}}
        del tr, od, v, src, dst
        torch.cuda.empty_cache()
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
