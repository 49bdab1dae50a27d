#!/usr/bin/env python3
"""Time of the quality-aware objectness path, in ONE process, at the training shard (B = 32 at 320^2, P = 16 800, 8 boxes per
image, NC = 20; targets, assigned_gt and metric from od_assign_tal on a random pred: logits N(0, 2), offsets N(0, 0.5)):
the two quality entries (od_quality_iou, od_quality_tal) and the loss in its three objectness modes (od_loss_fwd_bwd_iou =
focal, od_loss_fwd_bwd_quality with qfl / vfl), timed with device events, alternately, median over repetitions; and the
training step (bench.py's training workload: step(x, annotations) on a resident batch) for focal, qfl + iou (both under
max-iou), focal and qfl + tal (both under the task-aligned assigner), alternating.  `quality_share_of_step` is the quality
launch as a share of the focal step.  Prints one JSON line.  (DESIGN.md "Quality-aware objectness")"""
import argparse
import ctypes as C
import json
import time

import _common  # noqa: F401
import numpy as np
import torch

from bench_assign import _boxes, _median


def measure_calls(size, B, G, a, dev, NC=20):
    from object_detector_amd import _lib, ops
    from object_detector_amd.net import Context
    from object_detector_amd.pb import ObjectsAnnotation, PriorBoxes
    ctx = Context.get(dev)
    lib, h = ctx.lib, ctx.handle
    rng = np.random.default_rng(7)
    pb = PriorBoxes((size, size), NC, device=dev, assigner="tal")
    P = len(pb)
    anns = [ObjectsAnnotation(None, size, size, rng.integers(0, NC, G), _boxes(rng, G)) for _ in range(B)]
    pred = torch.from_numpy(np.concatenate([rng.normal(0, 2, (B, P, 2 + NC)), rng.normal(0, 0.5, (B, P, 4))], 2)
                            .astype(np.float32)).to(dev)
    up = pb.upload_batch(anns)
    y, npos, asg = pb.encode_uploaded(up, return_device=True, pred=pred)
    metric, gb, pri = pb.last_metric, up[2].contiguous(), pb.priors_device
    q = torch.empty((B, P), dtype=torch.float32, device=dev)
    grad = torch.empty_like(pred)
    losses = torch.empty((4,), dtype=torch.float32, device=dev)
    qwsb = lib.od_quality_tal_workspace_bytes(B, G)
    qws = torch.empty((qwsb,), dtype=torch.uint8, device=dev)
    lwsb = lib.od_loss_workspace_bytes(B, P)
    lws = torch.empty((lwsb,), dtype=torch.uint8, device=dev)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def q_iou():
        _lib.check(lib.od_quality_iou(h, pred.data_ptr(), y.data_ptr(), pri.data_ptr(), pb.loc_scale, B, P, NC, q.data_ptr(), st),
                   "od_quality_iou")

    def q_tal():
        _lib.check(lib.od_quality_tal(h, pred.data_ptr(), y.data_ptr(), pri.data_ptr(), pb.loc_scale, gb.data_ptr(),
                                      asg.data_ptr(), metric.data_ptr(), B, P, G, NC, q.data_ptr(), qws.data_ptr(), qwsb, st),
                   "od_quality_tal")

    def loss(mode):
        def run():
            head = (h, pred.data_ptr(), y.data_ptr(), pri.data_ptr(), grad.data_ptr(), losses.data_ptr(), B, P, NC, 0.25, 2.0,
                    ops.BOX_MODES["smooth_l1"], pb.loc_scale, 1.0, 1.0, 1.0)
            if mode == "focal":
                _lib.check(lib.od_loss_fwd_bwd_iou(*head, lws.data_ptr(), lwsb, st), "od_loss_fwd_bwd_iou")
            else:
                _lib.check(lib.od_loss_fwd_bwd_quality(*head, q.data_ptr(), ops.OBJ_MODES[mode], lws.data_ptr(), lwsb, st),
                           "od_loss_fwd_bwd_quality")
        return run

    q_tal()  # the loss modes below read this q
    fns = {"od_quality_iou": q_iou, "od_quality_tal": q_tal, "loss_focal": loss("focal"), "loss_qfl": loss("qfl"),
           "loss_vfl": loss("vfl")}
    times = {k: [] for k in fns}
    for fn in fns.values():
        for _ in range(a.warmup):
            fn()
    torch.cuda.synchronize()
    q_tal()
    for _ in range(a.reps):
        for k, fn in fns.items():  # alternate: every repetition times all of them next to each other
            if k.startswith("loss"):
                q_tal()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.calls):
                fn()
            e1.record()
            torch.cuda.synchronize()
            times[k].append(e0.elapsed_time(e1) * 1e3 / a.calls)
    us = {k: _median(v) for k, v in times.items()}
    return {"workload": f"B {B} at {size}x{size} (P {P}), {G} boxes per image, NC {NC}, targets of od_assign_tal (topk 13)",
            "positives_per_image": round(float(npos.float().mean()), 1),
            "us_per_call": {k: round(v, 2) for k, v in us.items()},
            "us_per_call_reps": {k: [round(t, 2) for t in v] for k, v in times.items()}}


CONFIGS = {"focal": dict(), "qfl+iou": dict(objectness="qfl", quality="iou"), "tal focal": dict(assigner="tal"),
           "tal qfl+tal": dict(assigner="tal", objectness="qfl", quality="tal")}


def measure_step(size, batch, G, a, dev):
    from object_detector_amd import weights as W
    from object_detector_amd.pb import ObjectsAnnotation
    from object_detector_amd.trainer import Trainer
    params = W.random_init(2)
    rng = np.random.default_rng(1000)
    x = torch.from_numpy(rng.integers(0, 256, (batch, size, size, 3), dtype=np.uint8)).to(dev)
    anns = [ObjectsAnnotation(None, size, size, rng.integers(0, 20, G), _boxes(rng, G)) for _ in range(batch)]
    trs = {k: Trainer(params, batch, (size, size), device=dev, lr=1e-3, momentum=0.9, loss_scale=1024.0, **kw)
           for k, kw in CONFIGS.items()}

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
    ap.add_argument("--calls", type=int, default=50, help="calls per timed window")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--steps", type=int, default=20, help="training steps per timed window")
    ap.add_argument("--step-warmup", type=int, default=5)
    ap.add_argument("--step-reps", type=int, default=5)
    ap.add_argument("--no-step", action="store_true", help="skip the training-step windows")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    out = {"metric": "quality_call_time", "calls": a.calls, "warmup": a.warmup, "reps": a.reps}
    out["320_b32_g8"] = calls = measure_calls(320, 32, 8, a, dev)
    if not a.no_step:
        step = measure_step(320, 32, 8, a, dev)
        focal = step["ms_per_step"]["focal"]
        step["quality_share_of_step"] = {k: round(calls["us_per_call"][k] * 1e-3 / focal, 5)
                                         for k in ("od_quality_iou", "od_quality_tal")}
        step["qfl_iou_step_over_focal_step"] = round(step["ms_per_step"]["qfl+iou"] / focal, 4)
        step["qfl_tal_step_over_tal_focal_step"] = round(step["ms_per_step"]["tal qfl+tal"] / step["ms_per_step"]["tal focal"], 4)
        out["train_320_b32"] = step
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
