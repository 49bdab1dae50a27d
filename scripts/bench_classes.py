#!/usr/bin/env python3
"""Cost of the class count: the predict step, od_detect alone, its workspace and the loss, at NC = 20 (VOC: the LDS kernels,
the same step bench.py times), 80 (COCO) and 365 (the streamed kernels of detect_wide.hip / od_loss_rows_wide).

Prints ONE JSON line: per NC
  images/s of the submit / collect predict step (3 batches in flight, random-init weights, synthetic images resident in HBM)
    at 32 x 320^2 and 16 x 640^2, timed like bench.py (warm-up, then exactly --steps steps between synchronizes);
  od_detect alone on one batch's pred (the network's own output), on a quiet stream, hipEvents around --steps calls;
  od_detect's workspace bytes, and pass 1's HBM floor: B * P * (NC + 6) * 4 bytes at 6.3 TB/s;
  od_loss_fwd_bwd_iou at the training shard (32 x 320^2, bench.py's ground-truth recipe with NC classes) with the box loss
    --box-loss names, hipEvents."""
import argparse
import json
import pathlib
import sys
import time

import numpy as np
import torch

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

HBM_BYTES_PER_S = 6.3e12


def _events_ms(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / n


def predict(nc, size, batch, steps, warmup, dev):
    from object_detector_amd import weights as W
    from object_detector_amd.detector import ObjectDetector
    od = ObjectDetector(W.random_init(2, nc), batch, (size, size), device=dev, use_multi_gpu=False, n_inflight=3)
    x = torch.from_numpy(np.random.default_rng(1000).integers(0, 256, (batch, size, size, 3), dtype=np.uint8)).to(dev)
    for _ in range(warmup):
        od.submit(x, conf_threshold=0.01)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        od.submit(x, conf_threshold=0.01)
    torch.cuda.synchronize()
    el = time.perf_counter() - t0
    # od_detect alone: pipeline 0's pred, one batch at a time on the (otherwise idle) current stream
    post, pred = od.post, od.net.pred
    torch.cuda.synchronize()
    ms = _events_ms(lambda: post.run(pred, 0.01), steps)
    P = od.net.P
    floor_us = batch * P * (nc + 6) * 4 / HBM_BYTES_PER_S * 1e6
    rec = {"images_per_sec": round(batch * steps / el, 1), "od_detect_us": round(ms * 1e3, 1),
           "od_detect_workspace_bytes": int(post.ws_det_bytes), "pass1_hbm_floor_us": round(floor_us, 1),
           "pred_bytes": batch * P * (nc + 6) * 4, "priors": P}
    del od, post, pred
    torch.cuda.empty_cache()
    return rec


def loss(nc, size, batch, steps, dev, box_loss="smooth_l1"):
    from object_detector_amd.net import Context, _stream_ptr
    from object_detector_amd.pb import ObjectsAnnotation, PriorBoxes
    from object_detector_amd import _lib
    from object_detector_amd.ops import BOX_MODES
    rng = np.random.default_rng(1000)
    anns = []
    for _ in range(batch):  # bench.py's ground-truth recipe, classes drawn from 0..nc-1
        n = int(np.clip(1 + rng.poisson(1.5), 1, 10))
        c = rng.uniform(0, 1, (n, 2))
        wh = np.exp(rng.uniform(np.log(0.05), np.log(0.9), (n, 2)))
        anns.append(ObjectsAnnotation(None, size, size, rng.integers(0, nc, n),
                                      np.clip(np.concatenate([c - wh / 2, c + wh / 2], 1), 0, 1).astype(np.float32)))
    pb = PriorBoxes((size, size), nc, device=dev)
    y, _npos, _ = pb.encode_batch(anns, return_device=True)
    B, P, C = y.shape
    pred = torch.randn((B, P, C), device=dev)
    grad = torch.empty_like(pred)
    losses = torch.empty((4,), device=dev)
    ctx = Context.get(dev)
    wsb = ctx.lib.od_loss_workspace_bytes(B, P)
    ws = torch.empty((wsb,), dtype=torch.uint8, device=dev)

    def call():
        _lib.check(ctx.lib.od_loss_fwd_bwd_iou(ctx.handle, pred.data_ptr(), y.data_ptr(), pb.priors_device.data_ptr(),
                                               grad.data_ptr(), losses.data_ptr(), B, P, nc, 0.25, 2.0, BOX_MODES[box_loss],
                                               pb.loc_scale, 1.0, 1.0, 1.0, ws.data_ptr(), wsb, _stream_ptr()),
                   "od_loss_fwd_bwd_iou")
    call()
    torch.cuda.synchronize()
    ms = _events_ms(call, steps)
    return {"loss_us": round(ms * 1e3, 1), "loss_bytes": 3 * B * P * C * 4, "loss_box_mode": box_loss,
            "loss_assigned_rows": int(_npos.sum().item())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--classes", type=int, nargs="+", default=[20, 80, 365])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--box-loss", default="smooth_l1", choices=("smooth_l1", "mse", "giou", "diou", "ciou"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    out = {}
    for nc in a.classes:
        row = {}
        for size, batch in ((320, 32), (640, 16)):
            for k, v in predict(nc, size, batch, a.steps, a.warmup, dev).items():
                row[f"{k}_{batch}x{size}"] = v
        row.update(loss(nc, 320, 32, a.steps, dev, a.box_loss))
        out[str(nc)] = row
    print(json.dumps({"metric": "class_count_scaling", "unit": "see keys", "by_num_classes": out}))


if __name__ == "__main__":
    main()
