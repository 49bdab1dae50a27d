#!/usr/bin/env python3
"""Time of Trainer.sgd() (od_grad_nonfinite + the optimizer launch + od_copy_if_nonzero [+ od_ema_update] + the f16
re-pack) at 32 x 320^2, in ONE process, as HIP-event times.  Prints one JSON line.

Three variants, timed alternately so that the same windows see the same machine:
  off      Trainer(ema_decay=None): od_sgd_step_multi, 5 x 4 B per parameter
  fused    Trainer(ema_decay=0.999): od_sgd_step_multi_ema, 7 x 4 B per parameter
  unfused  the same trainer with the fusion taken apart: od_sgd_step_multi, then od_ema_update over the whole flat buffer
           (w read a third time: 8 x 4 B per parameter and one more launch)
Per variant: `reps` windows of `calls` sgd() calls after `warmup` calls, one event pair per call; the figure is the median
over all timed calls, `spread_us` the distance between the smallest and the largest window median.

On a tree whose Trainer has no ema_decay keyword only `off` is measured: that run is the baseline the other figures are
judged against (DESIGN.md "Weight EMA")."""
import argparse
import inspect
import json

import _common  # noqa: F401
import numpy as np
import torch


class _Unfused:
    """The trainer's library handle with od_sgd_step_multi_ema replaced by the two launches it fuses."""

    def __init__(self, lib, n_flat):
        self._lib, self._n = lib, n_flat

    def __getattr__(self, name):
        return getattr(self._lib, name)

    def od_sgd_step_multi_ema(self, ctx, w, m, g, ema, segs, nseg, momentum, inv, omd, skip, stream):
        rc = self._lib.od_sgd_step_multi(ctx, w, m, g, segs, nseg, momentum, inv, skip, stream)
        return rc or self._lib.od_ema_update(ctx, ema, w, self._n, omd, skip, stream)


def _window(tr, calls):
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(calls)]
    torch.cuda.synchronize()
    for a, b in evs:
        tr._poll_nonfinite()
        a.record()
        tr.sgd()
        b.record()
    torch.cuda.synchronize()
    tr._poll_nonfinite(wait=True)
    return [a.elapsed_time(b) * 1e3 for a, b in evs]  # microseconds


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=320)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    from object_detector_amd import weights as W
    from object_detector_amd.trainer import Trainer
    dev = torch.device("cuda:0")
    has_ema = "ema_decay" in inspect.signature(Trainer.__init__).parameters
    kw = dict(device=dev, lr=0.01, momentum=0.9, weight_decay=1e-4, loss_scale=256.0)
    params = W.random_init(2)
    trs = {"off": Trainer(params, a.batch, (a.size, a.size), **kw)}
    libs = {"off": trs["off"].lib}
    if has_ema:
        # ONE trainer for both EMA variants, so that they stream the same buffers: where the allocator put a buffer moves
        # sgd() by several per cent from process to process, more than the difference looked for
        trs["fused"] = trs["unfused"] = Trainer(params, a.batch, (a.size, a.size), ema_decay=0.999, **kw)
        libs["fused"] = trs["fused"].lib
        libs["unfused"] = _Unfused(trs["fused"].lib, trs["fused"].n_flat)
    g = torch.from_numpy(np.random.default_rng(0).normal(0, 1e-2, trs["off"].n_flat).astype(np.float32)).to(dev)
    for k, tr in trs.items():
        tr.grads.copy_(g)
        tr.lib = libs[k]
        _window(tr, a.warmup)
    times = {k: [] for k in trs}
    for _ in range(a.reps):
        for k, tr in trs.items():
            tr.lib = libs[k]
            times[k].append(_window(tr, a.calls))
    med = {k: float(np.median(np.concatenate(v))) for k, v in times.items()}
    rec = {"workload": f"Trainer.sgd() at {a.batch} x {a.size}^2, {trs['off'].n_flat} f32 parameters, "
                       f"{a.reps} x {a.calls} calls after {a.warmup}",
           "sgd_us": {k: round(v, 2) for k, v in med.items()},
           "window_medians_us": {k: [round(float(np.median(w)), 2) for w in v] for k, v in times.items()},
           "spread_us": {k: round(float(max(np.median(w) for w in v) - min(np.median(w) for w in v)), 2)
                         for k, v in times.items()}}
    if has_ema:
        rec["fused_added_us"] = round(med["fused"] - med["off"], 2)
        rec["fused_added_over_off"] = round((med["fused"] - med["off"]) / med["off"], 4)
        rec["fused_over_unfused"] = round(med["fused"] / med["unfused"], 4)
        assert all(tr.skipped_steps == 0 for tr in trs.values())
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
