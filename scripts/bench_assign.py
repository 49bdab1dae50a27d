#!/usr/bin/env python3
"""Time of the three prior-box assigners, in ONE process: od_assign_anchors (the default rule and the yardstick),
od_assign_atss at topk = 9 and od_assign_tal at topk = 13 (on a random pred: logits N(0, 2), offsets N(0, 0.5)) on the same
inputs -- B = 32 at 320^2 (P = 16 800) and B = 16 at 640^2 (P = 67 200), 8 and 64 boxes per image, NC = 20 -- timed with device
events, alternately, median over repetitions; and the training step at 32 x 320^2 (bench.py's training workload:
step(x, annotations) on a resident batch) under the three assigners: the ATSS call as a share of the default step, and the
"tal" step, whose assignment sits between forward and loss, as a ratio of the default step.  `tal_prior_pass` gives the
bytes od_tal_prior must read (B * P * (NC + 6) * 4) and their time at the HBM peak; the kernel's own time comes from a
kernel trace of this script (--no-step).  Prints one JSON line.  (DESIGN.md "ATSS assignment", "Task-aligned assignment")"""
import argparse
import ctypes as C
import json
import time

import _common  # noqa: F401
import numpy as np
import torch


def _median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2] if len(xs) % 2 else 0.5 * (xs[len(xs) // 2 - 1] + xs[len(xs) // 2])


def _boxes(rng, n):
    c = rng.uniform(0, 1, (n, 2))
    wh = np.exp(rng.uniform(np.log(0.05), np.log(0.9), (n, 2)))
    return np.clip(np.concatenate([c - wh / 2, c + wh / 2], 1), 0, 1).astype(np.float32)


HBM_PEAK_TBS, HBM_COPY_TBS = 8.0, 6.29  # MI355X: specified peak, and what a float4 copy reaches


def measure_calls(size, B, G, a, dev, NC=20, topk=9, tal_topk=13):
    from object_detector_amd import _lib, pb, priors as PR
    from object_detector_amd.net import Context
    ctx = Context.get(dev)
    lib, h = ctx.lib, ctx.handle
    rng = np.random.default_rng(7)
    pri = torch.from_numpy(PR.make_priors((size, size))).to(dev)
    P = len(pri)
    levels = PR.level_shapes((size, size))
    grid_hw = (C.c_int32 * (2 * len(levels)))(*[v for hw in levels for v in hw])
    gb = torch.from_numpy(np.stack([_boxes(rng, G) for _ in range(B)])).to(dev)
    gc = torch.from_numpy(rng.integers(0, NC, (B, G)).astype(np.int32)).to(dev)
    gn = torch.full((B,), G, dtype=torch.int32, device=dev)
    y = torch.empty((B, P, NC + 6), dtype=torch.float32, device=dev)
    asg = torch.empty((B, P), dtype=torch.int32, device=dev)
    npos = torch.empty((B,), dtype=torch.int32, device=dev)
    nb = max(lib.od_assign_workspace_bytes(B, P, G), lib.od_assign_atss_workspace_bytes(B, P, G),
             lib.od_assign_tal_workspace_bytes(B, P, G))
    pred = torch.from_numpy(np.concatenate([rng.normal(0, 2, (B, P, 2 + NC)), rng.normal(0, 0.5, (B, P, 4))], 2)
                            .astype(np.float32)).to(dev)
    metric = torch.empty((B, P), dtype=torch.float32, device=dev)
    ws = torch.empty((nb,), dtype=torch.uint8, device=dev)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def max_iou():
        _lib.check(lib.od_assign_anchors(h, pri.data_ptr(), gb.data_ptr(), gc.data_ptr(), gn.data_ptr(), B, P, G, NC, pb.POS_THR,
                                         pb.NEG_THR, pb.LOC_SCALE, y.data_ptr(), asg.data_ptr(), npos.data_ptr(), ws.data_ptr(),
                                         nb, st), "od_assign_anchors")

    def atss():
        _lib.check(lib.od_assign_atss(h, pri.data_ptr(), grid_hw, len(levels), PR.NUM_PRIORS, gb.data_ptr(), gc.data_ptr(),
                                      gn.data_ptr(), None, 0.0, topk, B, P, G, NC, pb.LOC_SCALE, y.data_ptr(), asg.data_ptr(),
                                      npos.data_ptr(), ws.data_ptr(), nb, st), "od_assign_atss")

    def tal():
        _lib.check(lib.od_assign_tal(h, pri.data_ptr(), grid_hw, len(levels), PR.NUM_PRIORS, pred.data_ptr(), gb.data_ptr(),
                                     gc.data_ptr(), gn.data_ptr(), None, 0.0, pb.TAL_ALPHA, pb.TAL_BETA, tal_topk, B, P, G, NC,
                                     pb.LOC_SCALE, y.data_ptr(), asg.data_ptr(), npos.data_ptr(), metric.data_ptr(),
                                     ws.data_ptr(), nb, st), "od_assign_tal")

    fns = {"od_assign_anchors": max_iou, "od_assign_atss": atss, "od_assign_tal": tal}
    times, pos = {k: [] for k in fns}, {}
    for k, fn in fns.items():
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        pos[k] = round(float(npos.float().mean()), 1)
    for _ in range(a.reps):
        for k, fn in fns.items():  # alternate: every repetition times both next to each other
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.calls):
                fn()
            e1.record()
            torch.cuda.synchronize()
            times[k].append(e0.elapsed_time(e1) * 1e3 / a.calls)
    us = {k: _median(v) for k, v in times.items()}
    pred_bytes = B * P * (NC + 6) * 4
    return {"workload": f"B {B} at {size}x{size} (P {P}), {G} boxes per image, NC {NC}, topk {topk} (atss) / {tal_topk} (tal)",
            "tal_prior_pass": {"pred_bytes": pred_bytes, "us_at_hbm_peak": round(pred_bytes / HBM_PEAK_TBS * 1e-6, 2),
                               "us_at_hbm_copy_rate": round(pred_bytes / HBM_COPY_TBS * 1e-6, 2)},
            "tal_over_max_iou": round(us["od_assign_tal"] / us["od_assign_anchors"], 3),
            "us_per_call": {k: round(v, 2) for k, v in us.items()},
            "us_per_call_reps": {k: [round(t, 2) for t in v] for k, v in times.items()},
            "positives_per_image": pos,
            "y_bytes": B * P * (NC + 6) * 4,
            "atss_over_max_iou": round(us["od_assign_atss"] / us["od_assign_anchors"], 3)}


def measure_step(size, batch, G, a, dev):
    from object_detector_amd import weights as W
    from object_detector_amd.pb import ObjectsAnnotation
    from object_detector_amd.trainer import Trainer
    params = W.random_init(2)
    rng = np.random.default_rng(1000)
    x = torch.from_numpy(rng.integers(0, 256, (batch, size, size, 3), dtype=np.uint8)).to(dev)
    anns = [ObjectsAnnotation(None, size, size, rng.integers(0, 20, G), _boxes(rng, G)) for _ in range(batch)]
    trs = {k: Trainer(params, batch, (size, size), device=dev, lr=1e-3, momentum=0.9, loss_scale=1024.0, assigner=k)
           for k in ("max-iou", "atss", "tal")}

    def window(tr, steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            tr.step(x, anns)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / steps

    for tr in trs.values():
        window(tr, a.step_warmup)
    times = {k: [] for k in trs}
    for _ in range(a.step_reps):
        for k, tr in trs.items():
            times[k].append(window(tr, a.steps))
    ms = {k: _median(v) * 1e3 for k, v in times.items()}
    return {"workload": f"training step {size}x{size} batch {batch}, {G} boxes per image, step(x, annotations)",
            "ms_per_step": {k: round(v, 4) for k, v in ms.items()},
            "ms_per_step_reps": {k: [round(t * 1e3, 4) for t in v] for k, v in times.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50, help="assigner calls per timed window")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--steps", type=int, default=20, help="training steps per timed window")
    ap.add_argument("--step-warmup", type=int, default=5)
    ap.add_argument("--step-reps", type=int, default=5)
    ap.add_argument("--no-step", action="store_true", help="skip the training-step windows")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    out = {"metric": "assign_call_time", "calls": a.calls, "warmup": a.warmup, "reps": a.reps}
    for size, B in ((320, 32), (640, 16)):
        for G in (8, 64):
            out[f"{size}_b{B}_g{G}"] = measure_calls(size, B, G, a, dev)
    if not a.no_step:
        step = measure_step(320, 32, 8, a, dev)
        step["atss_call_share_of_max_iou_step"] = round(
            out["320_b32_g8"]["us_per_call"]["od_assign_atss"] * 1e-3 / step["ms_per_step"]["max-iou"], 4)
        step["max_iou_call_share_of_max_iou_step"] = round(
            out["320_b32_g8"]["us_per_call"]["od_assign_anchors"] * 1e-3 / step["ms_per_step"]["max-iou"], 4)
        step["tal_step_over_max_iou_step"] = round(step["ms_per_step"]["tal"] / step["ms_per_step"]["max-iou"], 4)
        out["train_320_b32"] = step
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
