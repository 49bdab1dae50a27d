#!/usr/bin/env python3
"""Time of Trainer.sgd() per optimizer and of the launches it is made of, at 32 x 320^2, in ONE process, as HIP-event times.
Prints one JSON line.

sgd() variants, each without and with the weight average (ema_decay=0.999), timed alternately so that the same windows see
the same machine:
  sgd           the default path: od_grad_nonfinite -> od_sgd_step_multi[_ema]
  sgd_clip      od_grad_stats -> od_optim_prepare -> od_optim_step_multi(OD_OPT_SGD), clip_grad_norm=1.0
  nesterov      the same launches, OD_OPT_NESTEROV, no clipping
  adamw_clip    OD_OPT_ADAMW, clip_grad_norm=1.0
Per variant: `reps` windows of `calls` sgd() calls after `warmup` calls, one event pair per call; the figure is the median
over all timed calls, `spread_us` the distance between the smallest and the largest window median.

Single launches, all on one set of buffers, with the achieved bytes/s counted from the algorithmic bytes: 4 B per
parameter for the two gradient scans; 20 B per parameter for the SGD kinds (w, m, g read; w, m written), 28 B for AdamW (v read
and written as well), 8 B more with the average.

On a tree whose Trainer has no `optimizer` keyword only the default path and its two launches are measured: that run is
the baseline the other figures are judged against (DESIGN.md "Optimizers and gradient clipping")."""
import argparse
import ctypes as C
import inspect
import json

import _common  # noqa: F401
import numpy as np
import torch


def _sgd_window(tr, calls):
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


def _launch_window(fn, calls):
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(calls)]
    torch.cuda.synchronize()
    for a, b in evs:
        a.record()
        rc = fn()
        b.record()
        assert rc == 0, rc
    torch.cuda.synchronize()
    return [a.elapsed_time(b) * 1e3 for a, b in evs]


def _summary(windows):
    meds = [float(np.median(w)) for w in windows]
    return round(float(np.median(np.concatenate(windows))), 2), round(max(meds) - min(meds), 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=320)
    ap.add_argument("--calls", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    from object_detector_amd import _lib, weights as W
    from object_detector_amd.net import _stream_ptr
    from object_detector_amd.trainer import Trainer
    dev = torch.device("cuda:0")
    has_optim = "optimizer" in inspect.signature(Trainer.__init__).parameters
    kw = dict(device=dev, lr=0.001, momentum=0.9, weight_decay=1e-4, loss_scale=256.0)
    variants = {"sgd": {}}
    if has_optim:
        variants.update(sgd_clip=dict(optimizer="sgd", clip_grad_norm=1.0), nesterov=dict(optimizer="nesterov"),
                        adamw_clip=dict(optimizer="adamw", clip_grad_norm=1.0))
    params = W.random_init(2)
    trs = {}
    for name, okw in variants.items():
        trs[name] = Trainer(params, a.batch, (a.size, a.size), **okw, **kw)
        trs[name + "+ema"] = Trainer(params, a.batch, (a.size, a.size), ema_decay=0.999, **okw, **kw)
    n = trs["sgd"].n_flat
    g = torch.from_numpy(np.random.default_rng(0).normal(0, 1e-2, n).astype(np.float32)).to(dev)
    for tr in trs.values():
        tr.grads.copy_(g)
        _sgd_window(tr, a.warmup)
    times = {k: [] for k in trs}
    for _ in range(a.reps):
        for k, tr in trs.items():
            times[k].append(_sgd_window(tr, a.calls))
    assert all(tr.skipped_steps == 0 for tr in trs.values())
    rec = {"workload": f"Trainer.sgd() at {a.batch} x {a.size}^2, {n} f32 parameters, {a.reps} x {a.calls} calls after "
                       f"{a.warmup}",
           "sgd_us": {k: _summary(v)[0] for k, v in times.items()}, "spread_us": {k: _summary(v)[1] for k, v in times.items()}}

    # ---- single launches -------------------------------------------------------------------------------------------------
    # every launch runs on the SAME buffers (those of the default trainer that keeps an average; AdamW's second moment is
    # borrowed from its own trainer): where the allocator put a buffer moves a streaming launch by several per cent, more
    # than the differences looked for
    T = trs["sgd+ema"]
    lib, h = T.lib, T.ctx.handle
    inv = 1.0 / 256.0
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    w, m, gr, ema, tbl, nseg = (T.params.data_ptr(), T.mom.data_ptr(), T.grads.data_ptr(), T.ema.data_ptr(),
                                T._sgd_table.data_ptr(), T._sgd_n)
    launches = {}  # name -> (callable, algorithmic bytes per parameter)
    launches["od_grad_nonfinite"] = (lambda: lib.od_grad_nonfinite(h, gr, n, flag.data_ptr(), _stream_ptr()), 4)
    launches["od_sgd_step_multi"] = (lambda: lib.od_sgd_step_multi(h, w, m, gr, tbl, nseg, 0.9, inv, flag.data_ptr(),
                                                                   _stream_ptr()), 20)
    launches["od_sgd_step_multi_ema"] = (lambda: lib.od_sgd_step_multi_ema(h, w, m, gr, ema, tbl, nseg, 0.9, inv, 0.001,
                                                                           flag.data_ptr(), _stream_ptr()), 28)
    if has_optim:
        A = trs["adamw_clip"]
        ws, st, v = A._stats_ws, A.optim_state, A.mom2.data_ptr()
        launches["od_grad_stats"] = (lambda: lib.od_grad_stats(h, gr, n, flag.data_ptr(), ws.data_ptr(), _stream_ptr()), 4)
        for kind, name in ((_lib.OD_OPT_SGD, "sgd"), (_lib.OD_OPT_NESTEROV, "nesterov"), (_lib.OD_OPT_ADAMW, "adamw")):
            for with_ema in (False, True):
                cfg = _lib.OptimCfg()
                cfg.kind, cfg.momentum, cfg.beta2, cfg.eps, cfg.inv_loss_scale = kind, 0.9, 0.999, 1e-8, inv
                cfg.max_grad_norm, cfg.ema_one_minus_decay = 1.0, 0.001
                adam = kind == _lib.OD_OPT_ADAMW

                def call(cfg=cfg, adam=adam, with_ema=with_ema):
                    return lib.od_optim_step_multi(h, C.byref(cfg), w, m, v if adam else None, gr, ema if with_ema else None,
                                                   tbl, nseg, st.data_ptr(), flag.data_ptr(), _stream_ptr())
                launches[f"od_optim_step_multi[{name}{'+ema' if with_ema else ''}]"] = (
                    call, (28 if adam else 20) + (8 if with_ema else 0))
        cfgp = _lib.OptimCfg()
        cfgp.kind, cfgp.momentum, cfgp.beta2, cfgp.eps = _lib.OD_OPT_ADAMW, 0.9, 0.999, 1e-8
        cfgp.inv_loss_scale, cfgp.max_grad_norm = inv, 1.0
        launches["od_optim_prepare"] = (lambda: lib.od_optim_prepare(h, C.byref(cfgp), ws.data_ptr(), n, flag.data_ptr(),
                                                                     st.data_ptr(), _stream_ptr()), 0)
    ltimes = {k: [] for k in launches}
    for k, (fn, _b) in launches.items():
        _launch_window(fn, a.warmup)
    for _ in range(a.reps):
        for k, (fn, _b) in launches.items():
            ltimes[k].append(_launch_window(fn, a.calls))
    rec["launch_us"] = {k: _summary(v)[0] for k, v in ltimes.items()}
    rec["launch_spread_us"] = {k: _summary(v)[1] for k, v in ltimes.items()}
    rec["launch_bytes_per_param"] = {k: b for k, (_f, b) in launches.items()}
    rec["launch_TB_per_s"] = {k: round(launches[k][1] * n / (rec["launch_us"][k] * 1e-6) / 1e12, 3) for k in launches
                              if launches[k][1]}
    assert int(flag.item()) == 0
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
