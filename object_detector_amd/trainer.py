"""Training step of the detector on MI355X: forward in BatchNorm-training mode, prior-box assignment, loss,
backward through every conv / BN / activation, data-parallel gradient all-reduce, SGD with per-layer LR multipliers.

reference: the (unseen) `fit` path of tk.dl.od.ObjectDetector -- generator -> encode_truth (check_assign.py:21) ->
losses (docs/MODEL.md:33-52) -> per-layer learning rates (docs/MODEL.md:84-90: shared prediction-module layers x 1/3,
base network x 1/100).  Every tensor op is a libodhip.so kernel; torch owns the HBM buffers and the process group.

Numerics: activations and activation gradients f16 (gradients multiplied by `loss_scale`), MFMA accumulation and all
statistics / parameter gradients / master weights f32.  BatchNorm statistics are per rank [BUILD-DEFINED, SURVEY.md §7];
only gradients are exchanged.
"""
from __future__ import annotations

import ctypes as C
import math
import os

import numpy as np
import torch

from . import _lib, desc, weights as W
from .net import Context, _stream_ptr
from .ops import BOX_MODES, OBJ_MODES, QUALITY_MODES
from .pb import ATSS_TOPK, GMAX, TAL_ALPHA, TAL_BETA, TAL_TOPK, PriorBoxes, check_assigner, check_tal

BN_MOMENTUM = 0.99  # Keras default


LR_MULTIPLIERS = {"b.": 0.01, "h.": 1.0 / 3.0}  # docs/MODEL.md:84-90: base network x 1/100, shared layers x 1/(times shared)


def lr_multiplier(name: str, table=None) -> float:
    """docs/MODEL.md:84-90.  `table`: {layer-name prefix: multiplier}, first matching prefix wins, no match = 1."""
    for prefix, m in (LR_MULTIPLIERS if table is None else table).items():
        if name.startswith(prefix):
            return float(m)
    return 1.0


def ema_decay_at(n: int, decay: float, warmup: bool = True) -> float:
    """Decay of the weight average at its update number `n` (= sgd() calls made before this one, skipped steps included),
    in float64: with warm-up min(decay, (1 + n) / (10 + n)), so that the average forgets its starting point quickly (0.1 at
    n = 0, 0.55 at n = 10, 0.918 at n = 100; the ramp meets decay = 0.999 at n = 8990); without, `decay`."""
    decay = float(decay)
    return min(decay, (1.0 + n) / (10.0 + n)) if warmup else decay


def ema_omd(n: int, decay: float, warmup: bool = True) -> np.float32:
    """The kernels' one_minus_decay argument of update `n`: 1 - ema_decay_at(...) in float64, rounded once to f32."""
    return np.float32(1.0 - ema_decay_at(n, decay, warmup))


LAG = 2  # the non-finite flag of step j is applied at the start of step j + LAG, on every rank, whatever the timing
LOSS_SCALE_MIN, LOSS_SCALE_MAX = 1.0, 65536.0


class LossScaleControl:
    """The host rule of the dynamic loss scale and its fixed-lag queue (no GPU, no library): a pure function of the flags.

    apply(flag): any non-zero flag is a skipped step -- skipped_steps and consecutive_skips go up, good_steps back to 0 and
    the scale is halved (floor LOSS_SCALE_MIN); a zero flag ends the run of skips, and the `interval`-th clean flag in a row
    doubles the scale (cap LOSS_SCALE_MAX) and starts the count again.  dynamic=False moves the counters and not the scale.

    pending: the flags of the steps not applied yet, oldest first.  A step calls begin_step() first and push()es its own
    flag last, so begin_step() of step i finds the flags of steps .. i-1 and applies those of steps .. i-lag: one per step
    in a run, none before `lag` steps have been pushed.  drain() applies everything pending, in order (end of a run, tests).
    An entry is whatever `read` turns into an int -- the trainer's are (event, pinned host flag) pairs whose copy it waits
    for; both calls return the entries they consumed."""

    def __init__(self, loss_scale, interval=2000, dynamic=True, lag=LAG, read=int):
        self.loss_scale, self.interval, self.dynamic = float(loss_scale), interval, bool(dynamic)
        self.lag, self.read = int(lag), read
        self.skipped_steps = self.good_steps = self.consecutive_skips = 0
        self.pending = []

    def apply(self, flag):
        if int(flag) != 0:
            self.skipped_steps += 1
            self.consecutive_skips += 1
            self.good_steps = 0
            if self.dynamic:
                self.loss_scale = max(LOSS_SCALE_MIN, self.loss_scale * 0.5)
        else:
            self.consecutive_skips = 0
            self.good_steps += 1
            if self.dynamic and self.good_steps >= self.interval:
                self.loss_scale, self.good_steps = min(self.loss_scale * 2.0, LOSS_SCALE_MAX), 0

    def push(self, entry):
        self.pending.append(entry)

    def _consume(self, keep):
        done = []
        while len(self.pending) > keep:
            done.append(self.pending.pop(0))
            self.apply(self.read(done[-1]))
        return done

    def begin_step(self):
        return self._consume(self.lag - 1)

    def drain(self):
        return self._consume(0)

    def pending_flags(self):
        """The values of the pending flags, oldest first; applies none."""
        return [int(self.read(e)) for e in self.pending]

    def values(self):
        return self.loss_scale, self.skipped_steps, self.good_steps, self.consecutive_skips


def _flag_value(entry):
    """LossScaleControl.read of the trainer: an (event, pinned host flag) pair is waited for (its copy was queued at least
    one whole step ago when a step asks, so the wait does not stall), anything else is the value itself."""
    if isinstance(entry, tuple):
        ev, host = entry
        ev.synchronize()
        return int(host[0])
    return int(entry)


def _ctl_attr(name):
    """Trainer attribute that lives in its LossScaleControl (read and set under the trainer's own name)."""
    return property(lambda self: getattr(self._ctl, name), lambda self, v: setattr(self._ctl, name, v))


class _Node:
    __slots__ = ("name", "x", "out", "res", "res_mode", "H", "W", "Cin", "Cout", "k", "stride", "act", "bn", "z",
                 "mean", "rstd", "scale", "shift", "first", "pred_off", "pred_rows", "need_dx",
                 # constants of the node, computed once: output size, rows, od_scale_act / od_bn_bwd arguments, od_bn_stats workspace
                 "Ho", "Wo", "M", "act_enum", "alpha", "res_code", "bn_wsb")


class Trainer:
    # the loss-scale control's values (LossScaleControl), under the names the trainer has always had
    loss_scale, skipped_steps = _ctl_attr("loss_scale"), _ctl_attr("skipped_steps")
    _good_steps, _consecutive_skips = _ctl_attr("good_steps"), _ctl_attr("consecutive_skips")
    dynamic_loss_scale, loss_scale_growth_interval = _ctl_attr("dynamic"), _ctl_attr("interval")

    def __init__(self, params, batch_size, input_size=(320, 320), device="cuda:0", lr=1e-3, momentum=0.9,
                 weight_decay=0.0, loss_scale=1024.0, box_mode="smooth_l1", backbone_act=("leaky", 0.1),
                 head_act=("elu", 1.0), comm=None, world_size=1, grad_payload=None, dynamic_loss_scale=True,
                 lr_multipliers=None, prior_wh=None, ignore_regions=False, ign_thr=None, loss_weights=(1.0, 1.0, 1.0),
                 ema_decay=None, ema_warmup=True, assigner="max-iou", atss_topk=ATSS_TOPK, tal_topk=TAL_TOPK,
                 tal_alpha=TAL_ALPHA, tal_beta=TAL_BETA, objectness="focal", quality="iou", optimizer="sgd",
                 betas=(0.9, 0.999), adam_eps=1e-8, clip_grad_norm=None):
        # ema_decay: None = no averaged model (no extra buffers, sgd() launches od_sgd_step_multi); 0 < ema_decay < 1 keeps
        # an exponential moving average of the masters (self.ema) and of the BatchNorm running statistics
        # (self.ema_run_stats), updated inside sgd() with the decay ema_decay_at(self.ema_updates, ema_decay, ema_warmup)
        if ema_decay is not None and not 0.0 < float(ema_decay) < 1.0:
            raise ValueError(f"ema_decay must be None or lie in (0, 1), got {ema_decay!r}")
        self.ema_decay = None if ema_decay is None else float(ema_decay)
        self.ema_warmup = bool(ema_warmup)
        check_assigner(assigner, atss_topk)  # a bad assigner fails here, before the device is touched
        check_tal(tal_topk, tal_alpha, tal_beta)
        # objectness "qfl" | "vfl": quality focal / varifocal loss towards the quality targets of `quality` ("iou": IoU of the
        # decoded target and predicted boxes, behind any assigner; "tal": TOOD's normalised metric, assigner="tal" only),
        # computed between the forward pass (and the TAL encode) and the loss; "focal" keeps hard targets and launches nothing
        check_objectness_args(objectness, quality, assigner)
        self.objectness, self.quality = objectness, quality
        # optimizer "sgd" | "nesterov" | "adamw" (momentum is the SGD kinds', betas / adam_eps are AdamW's); clip_grad_norm:
        # None, or the global gradient norm above which a step is scaled down (torch's clip_grad_norm_).  The defaults run
        # od_grad_nonfinite -> od_sgd_step_multi[_ema]; anything else od_grad_stats -> od_optim_prepare -> od_optim_step_multi
        self.optimizer, self.betas, self.adam_eps, self.clip_grad_norm = check_optimizer_args(optimizer, betas, adam_eps,
                                                                                             clip_grad_norm)
        self._optim_path = self.optimizer != "sgd" or self.clip_grad_norm is not None
        self.ctx = Context.get(device)
        self.lib = self.ctx.lib
        self.device = torch.device(device)
        self.B = int(batch_size)
        self.H0, self.W0 = int(input_size[0]), int(input_size[1])
        self.num_classes, self.neck_ch, self.tower = W.infer_arch(params)
        self.C = self.num_classes + 6
        self.lr, self.momentum, self.weight_decay = float(lr), float(momentum), float(weight_decay)
        # loss-scale guard: a non-finite value in the flat gradient buffer (one f16 overflow in a loss-scaled dz is enough)
        # makes the device skip the update; the host applies the flag exactly LAG steps later (_poll_nonfinite) and halves
        # the scale.  self._flag_queue IS the control's pending list: (event, pinned host flag) of the steps whose flag is
        # not applied yet, or plain ints (load_state_dict)
        self._ctl = LossScaleControl(loss_scale, 2000, dynamic_loss_scale, read=_flag_value)
        self._flag_queue, self._flag_pool = self._ctl.pending, []
        self.max_consecutive_skips = 50  # fit() gives up after this many skipped steps in a row (see diverged())
        self.box_mode = box_mode
        # box_mode "giou" | "diou" | "ciou": the box loss is taken on the boxes decoded with self.pb's priors and loc_scale;
        # loss_weights = (objectness, class, box) multiply the three components
        if box_mode not in BOX_MODES:
            raise ValueError(f"box_mode must be one of {sorted(BOX_MODES)}, got {box_mode!r}")
        self.loss_weights = tuple(float(v) for v in loss_weights)
        if len(self.loss_weights) != 3:
            raise ValueError(f"loss_weights must be (objectness, class, box), got {loss_weights!r}")
        # per-layer learning-rate multipliers (docs/MODEL.md:84-90 by default: the reference fine-tunes a PRE-TRAINED base
        # network at 1/100; a from-scratch run passes {"h.": 1/3} to train the base network at the full rate)
        self.lr_multipliers = dict(LR_MULTIPLIERS if lr_multipliers is None else lr_multipliers)
        self.comm, self.world = comm, int(world_size)
        # gradient all-reduce payload: "f32" (exact sum) or "bf16" (BASELINE.json configs[4]: half the xGMI bytes; each rank's
        # f32 gradients are rounded to bf16, summed by RCCL in bf16, widened back to f32 before the optimizer)
        self.grad_payload = grad_payload or os.environ.get("OD_TRAIN_GRAD_PAYLOAD", "f32")
        if self.grad_payload not in ("f32", "bf16"):
            raise ValueError(f"grad_payload must be 'f32' or 'bf16', got {self.grad_payload!r}")
        # prior_wh: the [3, 8, 2] table of prior sizes in grid-cell units (priors.fit: KMeans over the training boxes,
        # docs/MODEL.md:29-31); None = the frozen default table
        # ignore_regions / ign_thr: handed to the PriorBoxes (pb.py): annotations' `difficults` become ignore regions in
        # step(x, annotations=...) and in tr.pb.encode_truth_device, the generator callback
        # assigner / atss_topk: "max-iou" (od_assign_anchors) or "atss" (od_assign_atss), handed to the PriorBoxes as well
        # assigner "tal" (od_assign_tal; tal_topk / tal_alpha / tal_beta): assignment from this step's predictions, so step()
        # encodes BEHIND the forward pass and takes annotations only
        self.pb = PriorBoxes((self.H0, self.W0), self.num_classes, device=self.device, ignore_regions=ignore_regions,
                             assigner=assigner, atss_topk=atss_topk, tal_topk=tal_topk, tal_alpha=tal_alpha,
                             tal_beta=tal_beta,
                             **({} if prior_wh is None else {"prior_wh": prior_wh}),
                             **({} if ign_thr is None else {"ign_thr": ign_thr}))
        self.P = len(self.pb)
        dev = self.device

        # ---- flat f32 parameter / gradient / momentum buffers -------------------------------------------------
        self.specs = {s[0]: s for s in W.layer_specs(self.num_classes, self.neck_ch, self.tower)}
        self.seg = {}  # (layer, kind) -> (offset, numel)
        off = 0
        for name, (_n, cin, cout, k, _s, bn) in self.specs.items():
            for kind, n in (("w", cout * k * k * cin),) + ((("gamma", cout), ("beta", cout)) if bn else (("bias", cout),)):
                self.seg[(name, kind)] = (off, n)
                off += desc.pad_to(n, 4)
        self.n_flat = off
        host = np.zeros(off, np.float32)
        for (name, kind), (o, n) in self.seg.items():
            host[o:o + n] = np.asarray(params[f"{name}.{kind}"], np.float32).reshape(-1)
        self.params = torch.from_numpy(host).to(dev)
        self.grads = torch.zeros_like(self.params)
        self.mom = torch.zeros_like(self.params)
        # BatchNorm running statistics: ONE flat buffer (views per layer), so that a skipped step can put back the copy taken
        # before its forward pass with one launch (od_copy_if_nonzero)
        roff, rviews = 0, {}
        for n, sp in self.specs.items():
            if sp[5]:
                rviews[n] = roff
                roff += 2 * desc.pad_to(sp[2], 4)
        rhost = np.zeros(max(roff, 4), np.float32)
        for n, o in rviews.items():
            c = self.specs[n][2]
            cp = desc.pad_to(c, 4)
            rhost[o:o + c] = np.asarray(params[n + ".mean"], np.float32)
            rhost[o + cp:o + cp + c] = np.asarray(params[n + ".var"], np.float32)
        self.run_stats = torch.from_numpy(rhost).to(dev)
        self.run_stats_saved = torch.empty_like(self.run_stats)
        self.run_mean = {n: self.run_stats[o:o + self.specs[n][2]] for n, o in rviews.items()}
        self.run_var = {n: self.run_stats[o + desc.pad_to(self.specs[n][2], 4):][:self.specs[n][2]] for n, o in rviews.items()}
        self._run_off = rviews  # layer -> offset of its (mean, var) pair in run_stats
        # the averaged model: same layouts, starts as a copy.  ema_updates counts sgd() calls, skipped steps included
        self.ema = self.params.clone() if self.ema_decay is not None else None
        self.ema_run_stats = self.run_stats.clone() if self.ema_decay is not None else None
        self.ema_updates = 0
        self.steps_issued = 0  # sgd() calls of this object, skipped steps included: what ObjectDetector.refreshed_from records
        # the new optimizer path's buffers (none on the default path): AdamW's second moment, the device od_optim_state
        # (int32 step, then seven f32: _lib.OptimState), the per-workgroup f64 partials of od_grad_stats
        self.mom2 = torch.zeros_like(self.params) if self.optimizer == "adamw" else None
        self.optim_state = self.last_grad_norm = self._stats_ws = None
        if self._optim_path:
            st0 = _lib.OptimState()
            st0.b1pow = st0.b2pow = 1.0
            self.optim_state = torch.frombuffer(bytearray(bytes(st0)), dtype=torch.int32).to(dev)
            # the step's true gradient norm (unscaled, before clipping) as a device f32 view: read it when it is wanted
            self.last_grad_norm = self.optim_state.view(torch.float32)[3:4]
            self._stats_ws = torch.empty(self.lib.od_grad_stats_workspace_bytes(self.n_flat) // 8, dtype=torch.float64,
                                         device=dev)
        # per-channel stand-ins (scale / shift / bias / sink) cover every layer's Cout, read in whole 256-channel pads: the
        # prediction conv of a many-class head has Cout = 8 * (NC + 6), beyond the backbone's widths from NC = 251
        maxpad = max(2048, max(desc.pad_to(s[2], 256) for s in self.specs.values()))
        self.ones = torch.ones(maxpad, dtype=torch.float32, device=dev)
        self.zeros = torch.zeros(maxpad, dtype=torch.float32, device=dev)
        self.in_scale = torch.full((32,), 1.0 / 255.0, dtype=torch.float32, device=dev)
        self.scratch = torch.zeros(maxpad, dtype=torch.float32, device=dev)  # sink for unused per-channel outputs
        # ---- f16 packs ------------------------------------------------------------------------------------------
        self.wf, self.wb = {}, {}
        for name, (_n, cin, cout, k, _s, _bn) in self.specs.items():
            if name == "b.conv0":
                self.wf[name] = torch.zeros((32, 32), dtype=torch.float16, device=dev)
                continue
            cp, kp = _lib.conv_weight_dims(cout, cin, k)
            self.wf[name] = torch.zeros((cp, kp), dtype=torch.float16, device=dev)
            cp2, kp2 = _lib.conv_weight_dims(cin, cout, k)
            self.wb[name] = torch.zeros((cp2, kp2), dtype=torch.float16, device=dev)
        layers = []
        for name, (_n, cin, cout, k, _s, _bn) in self.specs.items():
            if name == "b.conv0":
                continue
            L = _lib.PackLayer()
            L.w_offset = self.seg[(name, "w")][0]
            L.w_fwd, L.w_bwd = self.wf[name].data_ptr(), self.wb[name].data_ptr()
            L.Cout, L.Cin, L.ksize = cout, cin, k
            layers.append(L)
        self._pack_table, self._pack_n = self._device_table(layers), len(layers)
        self._repack()
        self._sgd_key = None  # (lr, weight decay, multipliers) of the device table sgd() last built
        # ---- graph ------------------------------------------------------------------------------------------------
        self.tensors = {"img": torch.zeros((self.B, self.H0, self.W0, 3), dtype=torch.uint8, device=dev)}
        self.gradbuf = {}
        self.nodes = []
        self._build(backbone_act, head_act)
        self.pred = torch.zeros((self.B, self.P, self.C), dtype=torch.float32, device=dev)
        self.grad_pred = torch.zeros_like(self.pred)
        self.losses = torch.zeros(4, dtype=torch.float32, device=dev)
        self.last_npos = None  # positives per image [B] (device, i32) of the last step that encoded annotations
        self.last_target = None  # the target [B,P,C] the last step's loss was taken on (device; the caller's y_target or the encode's)
        self.loss_ws = torch.empty(self.lib.od_loss_workspace_bytes(self.B, self.P), dtype=torch.uint8, device=dev)
        # quality targets [B,P] of the last step (objectness "qfl" | "vfl"); focal keeps no buffer
        self.last_quality = (torch.zeros((self.B, self.P), dtype=torch.float32, device=dev) if objectness != "focal"
                             else None)
        # od_quality_tal's two [B,Gmax] tables, for the largest Gmax an upload can have
        self.quality_ws = (torch.empty(self.lib.od_quality_tal_workspace_bytes(self.B, GMAX), dtype=torch.uint8, device=dev)
                           if objectness != "focal" and quality == "tal" else None)
        mx = max(n.M * n.Cout for n in self.nodes)
        # dz of the node being processed: three rotating buffers, because the weight gradient of node k runs on a second
        # stream while the main stream already computes node k-1's dz (backward())
        self.dzs = [torch.empty(mx, dtype=torch.float16, device=dev) for _ in range(3)]
        self.dz = self.dzs[0]
        # the side streams (weight gradients, collectives) must sit on other hardware queues than the main stream, or nothing
        # overlaps: which queue a fresh stream lands on depends on how many streams the process created before, so they are
        # picked with the measured queue-overlap probe of detector.stream_queue_sets (12.9 instead of 10.6 ms per step when
        # the trainer was built after a few detectors in one process)
        from .detector import stream_queue_sets
        with torch.cuda.device(dev):
            side = stream_queue_sets(dev, 2, beside=torch.cuda.current_stream(dev))
        self._side_streams = side
        self.wstream = side[0]
        self._wg_done = [None] * len(self.dzs)
        # gradient exchange: buckets of whole layers from the END of the flat buffer (the order backward finishes them),
        # each all-reduced on its own stream as soon as its last layer is final -> the RCCL traffic overlaps the rest of
        # the backward pass.  OD_TRAIN_BUCKET_MB=0 -> one all-reduce after backward.
        self.bucket_mb = float(os.environ.get("OD_TRAIN_BUCKET_MB", "32"))
        # with an RCCL communicator (comm) the collectives go through od_allreduce; without one but world_size > 1 they go
        # through torch.distributed's default group (gloo rehearsals on one GPU, CPU-side tests) -- same buckets, same streams
        need_c = (self.comm is not None or self.world > 1) and self.bucket_mb > 0
        self.cstream = (self._side_streams[1] or torch.cuda.Stream(device=dev)) if need_c else None
        self.payload_buf = (torch.empty(self.n_flat, dtype=torch.bfloat16, device=dev) if self.grad_payload == "bf16"
                            else None)
        self.nonfinite = torch.zeros(1, dtype=torch.int32, device=dev)
        self._buckets = self._make_buckets(int(self.bucket_mb * (1 << 20) / 4)) if self.cstream is not None else []
        self._next_bucket = 0
        self.bn_ws = torch.empty(max(n.bn_wsb + 2 * n.Cout * 4 for n in self.nodes), dtype=torch.uint8, device=dev)
        # BatchNorm statistics from the conv epilogue (od_conv_desc.bn_partials): one partial row per m-tile, at most M / 64
        # rows of 2 x Cout floats.  OFF by default: measured neutral (profiles/r02/train_bn_stats_fusion.txt: the separate
        # pass reads z hot out of L2 / MALL for 0.46 ms per step; the epilogue sums + more partial rows + giving up the
        # 8-wave kernel for those layers cost 0.5 ms).  OD_TRAIN_FUSE_BN_STATS=1 turns it on.
        self.fuse_bn_stats = os.environ.get("OD_TRAIN_FUSE_BN_STATS", "0") == "1"
        self.bn_part = torch.empty(max(desc.pad_to(n.M, 64) // 64 * 2 * n.Cout for n in self.nodes), dtype=torch.float32,
                                   device=dev)
        self._bn_rows = {}  # node -> partial rows its statistics launch writes
        for n in self.nodes if self.fuse_bn_stats else ():
            if n.first or n.pred_off is not None:
                continue
            d = self._fwd_desc(n, self.tensors[n.x], n.z, bn_partials=self.bn_part)
            rows = self._bn_rows[n] = self.lib.od_conv2d_fwd_bn_rows(self.ctx.handle, C.byref(d))
            if rows <= 0 or rows * 2 * n.Cout > self.bn_part.numel():
                raise _lib.OdError(f"bn_partials too small for {n.name}: {rows} rows")
        # the prediction conv's bias, read in whole 256-channel pads like every scale / bias vector
        nb = self.seg[("h.out", "bias")][1]
        self._bias_pad = torch.zeros(desc.pad_to(nb, 256), dtype=torch.float32, device=dev) if nb % 256 else None
        self._first_ws = torch.empty(self.lib.od_conv_first_bwd_weight_workspace_bytes(self.ctx.handle, self.B, self.H0, self.W0),
                                     dtype=torch.uint8, device=dev)

    # ------------------------------------------------------------------------------------------------------------
    def _make_buckets(self, min_elems):
        layers = []  # (lo, hi, name) per layer, in buffer order
        for name in self.specs:
            offs = [(o, o + desc.pad_to(n, 4)) for (nm, _k), (o, n) in self.seg.items() if nm == name]
            layers.append((min(o for o, _ in offs), max(h for _, h in offs), name))
        return make_buckets(layers, self.n_flat, min_elems)

    def _launch_ready_buckets(self, done_layers, main):
        """All-reduce every not-yet-launched bucket whose layers are all final (in order), on the communication stream."""
        while self._next_bucket < len(self._buckets):
            lo, hi, names = self._buckets[self._next_bucket]
            if not names <= done_layers:
                return
            self.cstream.wait_stream(main)  # BatchNorm / bias gradients of these layers
            self.cstream.wait_stream(self.wstream)  # their weight gradients (slab reduce)
            with torch.cuda.stream(self.cstream):
                self._reduce_range(lo, hi)
            self._next_bucket += 1

    def _reduce_range(self, lo, hi):
        """Sum grads[lo:hi] over the data-parallel ranks on the CURRENT stream, in the configured payload type."""
        lib, h, s = self.lib, self.ctx.handle, _stream_ptr()
        g = self.grads[lo:hi]
        if self.grad_payload == "bf16":
            pb = self.payload_buf[lo:hi]
            _lib.check(lib.od_cast_f32_bf16(h, g.data_ptr(), pb.data_ptr(), hi - lo, s), "od_cast_f32_bf16")
            if self.comm is not None:
                _lib.check(lib.od_allreduce(self.comm, pb.data_ptr(), hi - lo, _lib.OD_DT_BF16, s), "od_allreduce(bf16)")
            else:
                dp_allreduce_(pb)
            _lib.check(lib.od_cast_bf16_f32(h, pb.data_ptr(), g.data_ptr(), hi - lo, s), "od_cast_bf16_f32")
        elif self.comm is not None:
            _lib.check(lib.od_allreduce(self.comm, g.data_ptr(), hi - lo, _lib.OD_DT_F32, s), "od_allreduce")
        else:
            dp_allreduce_(g)

    def view(self, buf, name, kind):
        o, n = self.seg[(name, kind)]
        return buf[o:o + n]

    def _device_table(self, structs):
        """ctypes structs -> one device buffer (uploaded once; the multi-tensor kernels read it)"""
        raw = b"".join(bytes(st) for st in structs)
        return torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(self.device)

    def _repack(self):
        w0 = self.view(self.params, "b.conv0", "w")
        wf0 = self.wf["b.conv0"]
        wf0.zero_()
        wf0[:, :27] = w0.view(32, 27).to(torch.float16)  # 1.7 KB: plain torch copy is fine here
        _lib.check(self.lib.od_pack_weights_multi(self.ctx.handle, self.params.data_ptr(), self._pack_table.data_ptr(),
                                                  self._pack_n, _stream_ptr()), "od_pack_weights_multi")

    def _repack_per_layer(self):
        for name, (_n, cin, cout, k, _s, _bn) in self.specs.items():
            w = self.view(self.params, name, "w")
            if name == "b.conv0":
                wf = self.wf[name]
                wf.zero_()
                wf[:, :27] = w.view(32, 27).to(torch.float16)  # 1.7 KB: plain torch copy is fine here
                continue
            _lib.check(self.lib.od_pack_weights(self.ctx.handle, w.data_ptr(), self.wf[name].data_ptr(),
                                                self.wb[name].data_ptr(), cout, cin, k, _stream_ptr()), "od_pack_weights")

    def _add_node(self, name, x, out, H, Wd, act, res=None, res_mode="none", first=False, pred_off=None, pred_rows=0,
                  need_dx=True):
        _n, cin, cout, k, stride, bn = self.specs[name]
        n = _Node()
        n.name, n.x, n.out, n.res, n.res_mode = name, x, out, res, res_mode
        n.H, n.W, n.Cin, n.Cout, n.k, n.stride, n.act, n.bn = H, Wd, cin, cout, k, stride, act, bn
        n.first, n.pred_off, n.pred_rows, n.need_dx = first, pred_off, pred_rows, need_dx
        Ho, Wo = n.Ho, n.Wo = H // stride, Wd // stride
        n.M = self.B * Ho * Wo
        n.act_enum, n.alpha = desc.act_pair(act)
        n.res_code = desc.res_code(res_mode)
        n.bn_wsb = self.lib.od_bn_workspace_bytes(n.M, cout)  # a pure function of (M, C): asked once, not per step
        dev = self.device
        if pred_off is None:
            n.z = torch.empty((self.B, Ho, Wo, cout), dtype=torch.float16, device=dev)
            self.tensors[out] = torch.empty((self.B, Ho, Wo, cout), dtype=torch.float16, device=dev)
            n.mean, n.rstd, n.scale, n.shift = (torch.empty(cout, dtype=torch.float32, device=dev) for _ in range(4))
        else:
            n.z = None
        self.nodes.append(n)
        return Ho, Wo

    def _build(self, bact, hact):
        H, Wd = self._add_node("b.conv0", "img", "t0", self.H0, self.W0, bact, first=True, need_dx=False)
        cur = "t0"
        taps = []
        for si, (nblk, _ch) in enumerate(W.STAGES, start=1):
            H, Wd = self._add_node(f"b.down{si}", cur, f"s{si}.d", H, Wd, bact)
            cur = f"s{si}.d"
            for r in range(nblk):
                self._add_node(f"b.s{si}.{r}.a", cur, f"s{si}.{r}.a", H, Wd, bact)
                self._add_node(f"b.s{si}.{r}.b", f"s{si}.{r}.a", f"s{si}.{r}.b", H, Wd, bact, res=cur, res_mode="same")
                cur = f"s{si}.{r}.b"
            taps.append((cur, H, Wd))
        (c3, h3, w3), (c4, h4, w4), (c5, h5, w5) = taps[2], taps[3], taps[4]
        self._add_node("n.lat5", c5, "p5", h5, w5, hact)
        self._add_node("n.lat4", c4, "m4", h4, w4, hact, res="p5", res_mode="up2")
        self._add_node("n.out4", "m4", "p4", h4, w4, hact)
        self._add_node("n.lat3", c3, "m3", h3, w3, hact, res="p4", res_mode="up2")
        self._add_node("n.out3", "m3", "p3", h3, w3, hact)
        off = 0
        for li, (lv, h, w) in enumerate((("p3", h3, w3), ("p4", h4, w4), ("p5", h5, w5))):
            cur = lv
            for t in range(self.tower):
                self._add_node(f"h.t{t}", cur, f"L{li}.t{t}", h, w, hact)
                cur = f"L{li}.t{t}"
            rows = h * w * W.NUM_PRIORS
            self._add_node("h.out", cur, f"L{li}.out", h, w, None, pred_off=off, pred_rows=rows)
            off += rows
        assert off == self.P
        self._build_wgrad_slabs()

    # ------------------------------------------------------------------------------------------------------------
    def _fwd_desc(self, n, x, out, bias=None, bn_partials=None):
        """od_conv_desc of node n's raw forward convolution (identity scale, linear epilogue): z f16 into `out`, or for a
        prediction conv f32 logits plus `bias` into the level's rows of pred (`out` = the address of the first of them)."""
        pred = n.pred_off is not None
        return desc.conv(x, self.wf[n.name], self.ones, self.zeros if bias is None else bias, out, self.B, n.H, n.W, n.Cin,
                         n.Cout, n.k, n.stride, out_f32=pred, out_batch_stride=self.P * self.C if pred else 0,
                         out_pix_stride=n.Cout if pred else 0,
                         bn_partials=None if bn_partials is None else (bn_partials, bn_partials.numel() * 4))

    def _conv_raw(self, n, x, out, bias=None, bn_partials=None):
        d = self._fwd_desc(n, x, out, bias, bn_partials)
        _lib.check(self.lib.od_conv2d_fwd(self.ctx.handle, C.byref(d), _stream_ptr()), f"conv fwd {n.name}")

    def forward(self, x_u8):
        """uint8 [B,H,W,3] (device) -> pred f32 [B,P,C]; keeps z / statistics of every layer for the backward pass."""
        self.tensors["img"].copy_(x_u8, non_blocking=True)
        lib, h = self.lib, self.ctx.handle
        s = _stream_ptr()
        self.run_stats_saved.copy_(self.run_stats, non_blocking=True)  # put back by sgd() when the step is skipped
        for n in self.nodes:
            x = self.tensors[n.x]
            fused_stats = self.fuse_bn_stats and not n.first  # BatchNorm partial sums from the conv epilogue
            if n.first:
                _lib.check(lib.od_conv_first_fwd(h, x.data_ptr(), self.wf[n.name].data_ptr(), self.in_scale.data_ptr(),
                                                 self.zeros.data_ptr(), n.z.data_ptr(), self.B, n.H, n.W, n.Cout,
                                                 _lib.OD_ACT_LINEAR, 0.0, s), "conv_first")
            elif n.pred_off is not None:
                bias = self.view(self.params, n.name, "bias")
                if self._bias_pad is not None:
                    self._bias_pad[:bias.numel()].copy_(bias)
                    bias = self._bias_pad
                self._conv_raw(n, x, self.pred.data_ptr() + n.pred_off * self.C * 4, bias=bias)
                continue
            else:
                self._conv_raw(n, x, n.z, bn_partials=self.bn_part if fused_stats else None)
            stats = (self.view(self.params, n.name, "gamma").data_ptr(), self.view(self.params, n.name, "beta").data_ptr(),
                     W.BN_EPS, n.mean.data_ptr(), n.rstd.data_ptr(), n.scale.data_ptr(), n.shift.data_ptr(),
                     self.run_mean[n.name].data_ptr(), self.run_var[n.name].data_ptr(), BN_MOMENTUM)
            if fused_stats:
                _lib.check(lib.od_bn_stats_from_partials(h, self.bn_part.data_ptr(), self._bn_rows[n], n.M, n.Cout, *stats, s),
                           "od_bn_stats_from_partials")
            else:
                _lib.check(lib.od_bn_stats(h, n.z.data_ptr(), n.M, n.Cout, *stats, self.bn_ws.data_ptr(), n.bn_wsb, s),
                           "od_bn_stats")
            _lib.check(lib.od_scale_act(h, n.z.data_ptr(), n.scale.data_ptr(), n.shift.data_ptr(),
                                        self.tensors[n.res].data_ptr() if n.res else None, n.res_code,
                                        self.tensors[n.out].data_ptr(), self.B, n.Ho, n.Wo, n.Cout, n.act_enum, n.alpha, s),
                       "od_scale_act")
        return self.pred

    def quality_targets(self, y_target, tal_inputs=None):
        """pred (from forward) + targets f32 [B,P,C] -> self.last_quality f32 [B,P] (objectness "qfl" | "vfl"), on the current
        stream: od_quality_iou, or with quality="tal" od_quality_tal on tal_inputs = (gt_boxes f32 [B,Gmax,4], assigned_gt i32
        [B,P]) of the od_assign_tal call that made y_target from THIS pred, and self.pb.last_metric."""
        h, q, s = self.ctx.handle, self.last_quality, _stream_ptr()
        if self.quality == "tal":
            if tal_inputs is None:
                raise ValueError('quality="tal" needs tal_inputs=(gt_boxes, assigned_gt) of the task-aligned assignment of '
                                 'this pred; step(x, annotations=...) passes them')
            gb, assigned = tal_inputs
            _lib.check(self.lib.od_quality_tal(h, self.pred.data_ptr(), y_target.data_ptr(), self.pb.priors_device.data_ptr(),
                                               self.pb.loc_scale, gb.data_ptr(), assigned.data_ptr(),
                                               self.pb.last_metric.data_ptr(), self.B, self.P, gb.shape[1], self.num_classes,
                                               q.data_ptr(), self.quality_ws.data_ptr(), self.quality_ws.numel(), s),
                       "od_quality_tal")
        else:
            _lib.check(self.lib.od_quality_iou(h, self.pred.data_ptr(), y_target.data_ptr(), self.pb.priors_device.data_ptr(),
                                               self.pb.loc_scale, self.B, self.P, self.num_classes, q.data_ptr(), s),
                       "od_quality_iou")
        return q

    def loss(self, y_target, tal_inputs=None):
        """pred (from forward) + targets f32 [B,P,C] -> losses [4] on device; fills grad_pred.  objectness "qfl" | "vfl":
        the quality targets of this pred and y_target are computed first (quality_targets; quality="tal" needs tal_inputs)
        and stay in self.last_quality."""
        w = self.loss_weights
        if self.objectness != "focal":
            self.quality_targets(y_target, tal_inputs)
            _lib.check(self.lib.od_loss_fwd_bwd_quality(self.ctx.handle, self.pred.data_ptr(), y_target.data_ptr(),
                                                        self.pb.priors_device.data_ptr(), self.grad_pred.data_ptr(),
                                                        self.losses.data_ptr(), self.B, self.P, self.num_classes, 0.25, 2.0,
                                                        BOX_MODES[self.box_mode], self.pb.loc_scale, w[0], w[1], w[2],
                                                        self.last_quality.data_ptr(), OBJ_MODES[self.objectness],
                                                        self.loss_ws.data_ptr(), self.loss_ws.numel(), _stream_ptr()),
                       "od_loss_fwd_bwd_quality")
            return self.losses
        _lib.check(self.lib.od_loss_fwd_bwd_iou(self.ctx.handle, self.pred.data_ptr(), y_target.data_ptr(),
                                                self.pb.priors_device.data_ptr(), self.grad_pred.data_ptr(),
                                                self.losses.data_ptr(), self.B, self.P, self.num_classes, 0.25, 2.0,
                                                BOX_MODES[self.box_mode], self.pb.loc_scale, w[0], w[1], w[2],
                                                self.loss_ws.data_ptr(), self.loss_ws.numel(), _stream_ptr()),
                   "od_loss_fwd_bwd_iou")
        return self.losses

    def _grad(self, key):
        t = self.gradbuf.get(key)
        if t is None:
            t = self.gradbuf[key] = torch.empty_like(self.tensors[key])
        return t

    def _build_wgrad_slabs(self):
        """Slab regions of the deterministic weight-gradient path: per layer, the slabs of all its nodes (a shared layer has
        one node per pyramid level) are contiguous so that one table entry sums them."""
        lib, h = self.lib, self.ctx.handle
        per_layer = {}
        for n in self.nodes:
            if n.first:
                continue
            sp = lib.od_conv2d_bwd_weight_splits(h, self.B, n.H, n.W, n.Cin, n.Cout, n.k, n.stride)
            assert sp > 0
            per_layer.setdefault(n.name, []).append((n, sp))
        total = sum(sum(sp for _n, sp in lst) * lst[0][0].Cout * lst[0][0].k ** 2 * lst[0][0].Cin for lst in per_layer.values())
        self.wgrad_slabs = torch.empty(total, dtype=torch.float32, device=self.device)
        self._slab_ptr, entries, off = {}, [], 0
        for name, lst in per_layer.items():
            n0 = lst[0][0]
            count = n0.Cout * n0.k ** 2 * n0.Cin
            e = _lib.WgradRed()
            e.dw_offset, e.count = self.seg[(name, "w")][0], count
            e.slabs = self.wgrad_slabs.data_ptr() + 4 * off
            e.nslabs = sum(sp for _n, sp in lst)
            entries.append(e)
            for n, sp in lst:
                self._slab_ptr[id(n)] = self.wgrad_slabs.data_ptr() + 4 * off
                off += sp * count
        self._wgrad_table, self._wgrad_n = self._device_table(entries), len(entries)
        # per-layer reduce right behind the layer's last weight-gradient launch (slabs still in L2 / MALL)
        self._wgrad_entry = {name: i for i, name in enumerate(per_layer)}
        self._wgrad_nodes = {name: len(lst) for name, lst in per_layer.items()}

    def backward(self):
        """grad_pred -> self.grads (f32, loss-scaled sums over this rank's batch)."""
        lib, h = self.lib, self.ctx.handle
        s = _stream_ptr()
        self.grads.zero_()
        have = set()
        pending = dict(self._wgrad_nodes)
        esz = C.sizeof(_lib.WgradRed)
        main = torch.cuda.current_stream(self.device)
        done_layers = set()
        self._next_bucket = 0
        if self.cstream is not None:
            self.cstream.wait_stream(main)  # grads.zero_() above
        for k, n in enumerate(reversed(self.nodes)):
            M, Ho, Wo = n.M, n.Ho, n.Wo
            slot = k % len(self.dzs)
            if self._wg_done[slot] is not None:
                main.wait_event(self._wg_done[slot])  # the weight gradient that read this buffer three nodes ago
            dz = self.dzs[slot][:M * n.Cout]
            wsb = n.bn_wsb + 2 * n.Cout * 4
            if n.pred_off is not None:
                _lib.check(lib.od_pred_grad_to_level(h, self.grad_pred.data_ptr(), dz.data_ptr(), self.B, self.P, self.C,
                                                     n.pred_off, n.pred_rows, self.loss_scale, s), "od_pred_grad_to_level")
                _lib.check(lib.od_bn_bwd(h, dz.data_ptr(), dz.data_ptr(), self.ones.data_ptr(), self.zeros.data_ptr(),
                                         None, None, M, n.Cout, _lib.OD_ACT_LINEAR, 0.0, 0,
                                         self.scratch.data_ptr(), self.view(self.grads, n.name, "bias").data_ptr(),
                                         dz.data_ptr(), self.bn_ws.data_ptr(), wsb, s), "od_bn_bwd(bias)")
            else:
                assert n.out in have, f"no gradient reached {n.out}"
                dy = self.gradbuf[n.out]
                if n.res:
                    if n.res_mode == "same" and n.res not in have:
                        # first gradient to reach the shortcut's source: d(res) = dy.  No copy -- the source's gradient
                        # tensor IS dy's buffer from here on (dy has no reader after this node's od_bn_bwd below, every
                        # later contribution accumulates in place, all on this stream): a whole stage's residual stream
                        # shares one gradient buffer, and 22 full-tensor copies per step (0.4 ms at 32 x 320^2) are gone
                        self.gradbuf[n.res] = dy
                        g = dy
                    else:
                        g = self._grad(n.res)
                    if n.res_mode == "same":
                        if n.res in have:
                            _lib.check(lib.od_add_f16(h, g.data_ptr(), dy.data_ptr(), dy.numel(), s), "od_add_f16")
                    else:
                        _lib.check(lib.od_down2_sum_add(h, dy.data_ptr(), g.data_ptr(), self.B, Ho // 2, Wo // 2, n.Cout,
                                                        int(n.res in have), s), "od_down2_sum_add")
                    have.add(n.res)
                _lib.check(lib.od_bn_bwd(h, n.z.data_ptr(), dy.data_ptr(), n.scale.data_ptr(), n.shift.data_ptr(),
                                         n.mean.data_ptr(), n.rstd.data_ptr(), M, n.Cout,
                                         n.act_enum, n.alpha, 1,
                                         self.view(self.grads, n.name, "gamma").data_ptr(),
                                         self.view(self.grads, n.name, "beta").data_ptr(), dz.data_ptr(),
                                         self.bn_ws.data_ptr(), wsb, s), f"od_bn_bwd {n.name}")
            dw = self.view(self.grads, n.name, "w")
            x = self.tensors[n.x]
            # weight gradient: needs only dz and the saved input -> second stream, beside the dz -> dx -> ... chain
            ev = torch.cuda.Event()
            ev.record(main)
            self.wstream.wait_event(ev)
            ws = C.c_void_p(self.wstream.cuda_stream)
            if n.first:
                _lib.check(lib.od_conv_first_bwd_weight(h, x.data_ptr(), dz.data_ptr(), dw.data_ptr(), self.B, n.H, n.W,
                                                        n.Cout, 1.0 / 255.0, self._first_ws.data_ptr(),
                                                        self._first_ws.numel(), ws), "od_conv_first_bwd_weight")
            else:
                _lib.check(lib.od_conv2d_bwd_weight_slabs(h, x.data_ptr(), dz.data_ptr(), self._slab_ptr[id(n)], self.B, n.H,
                                                          n.W, n.Cin, n.Cout, n.k, n.stride, ws), f"wgrad {n.name}")
                pending[n.name] -= 1
                if pending[n.name] == 0:  # every node of the (possibly shared) layer has written its slabs: fixed-order sum
                    _lib.check(lib.od_wgrad_reduce_multi(h, self._wgrad_table.data_ptr() + esz * self._wgrad_entry[n.name],
                                                         1, self.grads.data_ptr(), ws), f"wgrad reduce {n.name}")
            done = torch.cuda.Event()
            done.record(self.wstream)
            self._wg_done[slot] = done
            if n.first or pending[n.name] == 0:
                done_layers.add(n.name)
                if self.cstream is not None:
                    self._launch_ready_buckets(done_layers, main)
            if n.first or not n.need_dx:
                continue
            g = self._grad(n.x)
            # dx = backward-data of dz (the transposed form for stride 2), accumulated in place when n.x already has a gradient
            _lib.check(lib.od_conv2d_bwd_data(h, dz.data_ptr(), self.wb[n.name].data_ptr(), g.data_ptr() if n.x in have else None,
                                              g.data_ptr(), self.B, Ho, Wo, n.Cin, n.Cout, n.k, n.stride, s), f"dgrad {n.name}")
            have.add(n.x)
        main.wait_stream(self.wstream)
        self._wg_done = [None] * len(self.dzs)
        # (conv weight gradients: each layer's per-split slabs were summed in a fixed order right behind its last
        # weight-gradient launch -- no atomics, and the slabs are still cache-resident when they are read back)
        # shared-layer BN gradients were accumulated over the three levels inside od_bn_bwd
        return self.grads

    def allreduce(self):
        """Sum the flat f32 gradient buffer over the data-parallel ranks: bucketed all-reduces launched during backward on
        the communication stream (RCCL through the C ABI), or one collective after backward (47 M floats)."""
        if self.cstream is not None:  # bucketed: every bucket was launched during backward, join the communication stream
            assert self._next_bucket == len(self._buckets), "a gradient bucket was never launched"
            torch.cuda.current_stream(self.device).wait_stream(self.cstream)
            return
        if self.world <= 1 and self.comm is None:
            return
        self._reduce_range(0, self.n_flat)

    def sgd(self):
        """One multi-tensor launch over the flat parameter buffer (per-segment LR multipliers of docs/MODEL.md:84-90 and
        weight decay in a device table), one multi-layer re-pack launch."""
        inv = dp_effective_scale(self.loss_scale, self.world)  # grads are averaged over ranks
        # after the all-reduce, so every rank sees the same flag: Inf / NaN anywhere -> this step's update is skipped
        if self._optim_path:  # the same scan, with the sum of squares the global norm is taken from
            _lib.check(self.lib.od_grad_stats(self.ctx.handle, self.grads.data_ptr(), self.n_flat, self.nonfinite.data_ptr(),
                                              self._stats_ws.data_ptr(), _stream_ptr()), "od_grad_stats")
        else:
            _lib.check(self.lib.od_grad_nonfinite(self.ctx.handle, self.grads.data_ptr(), self.n_flat,
                                                  self.nonfinite.data_ptr(), _stream_ptr()), "od_grad_nonfinite")
        key = (self.lr, self.weight_decay, tuple(sorted(self.lr_multipliers.items())))
        if self._sgd_key != key:
            segs = []
            for (name, kind), (o, n) in self.seg.items():
                sg = _lib.SgdSeg()
                sg.offset, sg.count = o, n
                sg.lr = self.lr * lr_multiplier(name, self.lr_multipliers)
                sg.weight_decay = self.weight_decay if kind == "w" else 0.0
                segs.append(sg)
            self._sgd_table, self._sgd_n, self._sgd_key = self._device_table(segs), len(segs), key
        omd = None if self.ema_decay is None else float(ema_omd(self.ema_updates, self.ema_decay, self.ema_warmup))
        if self._optim_path:
            # norm, clipping coefficient and bias correction are computed on the device (od_optim_prepare) from the
            # identical all-reduced buffer in a fixed order: every rank gets the same bits, and the host waits for nothing
            cfg = _lib.OptimCfg()
            cfg.kind = _lib.OPTIMIZERS[self.optimizer]
            cfg.momentum = self.betas[0] if self.optimizer == "adamw" else self.momentum
            cfg.beta2, cfg.eps, cfg.inv_loss_scale = self.betas[1], self.adam_eps, inv
            cfg.max_grad_norm = 0.0 if self.clip_grad_norm is None else self.clip_grad_norm
            cfg.ema_one_minus_decay = 0.0 if omd is None else omd
            _lib.check(self.lib.od_optim_prepare(self.ctx.handle, C.byref(cfg), self._stats_ws.data_ptr(), self.n_flat,
                                                 self.nonfinite.data_ptr(), self.optim_state.data_ptr(), _stream_ptr()),
                       "od_optim_prepare")
            _lib.check(self.lib.od_optim_step_multi(self.ctx.handle, C.byref(cfg), self.params.data_ptr(), self.mom.data_ptr(),
                                                    None if self.mom2 is None else self.mom2.data_ptr(),
                                                    self.grads.data_ptr(), None if self.ema is None else self.ema.data_ptr(),
                                                    self._sgd_table.data_ptr(), self._sgd_n, self.optim_state.data_ptr(),
                                                    self.nonfinite.data_ptr(), _stream_ptr()), "od_optim_step_multi")
        elif self.ema_decay is None:
            _lib.check(self.lib.od_sgd_step_multi(self.ctx.handle, self.params.data_ptr(), self.mom.data_ptr(),
                                                  self.grads.data_ptr(), self._sgd_table.data_ptr(), self._sgd_n,
                                                  self.momentum, inv, self.nonfinite.data_ptr(), _stream_ptr()),
                       "od_sgd_step_multi")
        else:
            # the decay follows the number of sgd() calls made so far, skipped steps INCLUDED: the host learns of a skip
            # LAG steps late (_poll_nonfinite), so a schedule that counted applied updates would lag the device by as
            # much.  The device skips the update itself.
            _lib.check(self.lib.od_sgd_step_multi_ema(self.ctx.handle, self.params.data_ptr(), self.mom.data_ptr(),
                                                      self.grads.data_ptr(), self.ema.data_ptr(), self._sgd_table.data_ptr(),
                                                      self._sgd_n, self.momentum, inv, omd, self.nonfinite.data_ptr(),
                                                      _stream_ptr()), "od_sgd_step_multi_ema")
        # a skipped step also takes back what its forward pass did to the BatchNorm running statistics: when the Inf / NaN
        # came from an f16 overflow in z (not from a loss-scaled dz) the batch statistics folded into them are non-finite
        _lib.check(self.lib.od_copy_if_nonzero(self.ctx.handle, self.run_stats.data_ptr(), self.run_stats_saved.data_ptr(),
                                               self.run_stats.numel(), self.nonfinite.data_ptr(), _stream_ptr()),
                   "od_copy_if_nonzero")
        if self.ema_decay is not None:  # behind the restore; a skipped step leaves the averaged statistics alone too
            _lib.check(self.lib.od_ema_update(self.ctx.handle, self.ema_run_stats.data_ptr(), self.run_stats.data_ptr(),
                                              self.run_stats.numel(), omd, self.nonfinite.data_ptr(), _stream_ptr()),
                       "od_ema_update")
            self.ema_updates += 1
        self._repack()  # (a skipped step re-packs unchanged masters: harmless, and keeps the launch sequence fixed)
        self.steps_issued += 1
        host = self._flag_pool.pop() if self._flag_pool else torch.zeros(1, dtype=torch.int32).pin_memory()
        host.copy_(self.nonfinite, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self._ctl.push((ev, host))

    def _poll_nonfinite(self, wait=False):
        """Start of a step: apply the flag of the step LAG steps back (LossScaleControl.begin_step) and no newer one,
        waiting for its device->host copy.  That copy was queued behind a step that ended a whole step ago, so the wait
        does not stall and the host still runs two steps ahead: encode_batch and the first launches of this step overlap
        the previous step's tail.  When a flag is applied therefore depends on the step count alone -- not on timing, not
        on the rank.  A skipped step halves the loss scale; a long clean run doubles it again.
        wait=True applies everything pending, in order (the end of a run, tests)."""
        for entry in (self._ctl.drain() if wait else self._ctl.begin_step()):
            if isinstance(entry, tuple):
                self._flag_pool.append(entry[1])

    def pending_flags(self):
        """The flags of the steps the control has not applied yet, oldest first (waits for their copies, applies none)."""
        return self._ctl.pending_flags()

    def diverged(self):
        """True when the last `max_consecutive_skips` steps were ALL skipped although the loss scale has already been halved
        as far as it can help: the FORWARD pass overflows f16 (the weights themselves are in a bad place -- typically a
        learning rate too high for the batch size), which no loss scale can cure and a skipped step never changes."""
        return self._consecutive_skips >= self.max_consecutive_skips

    def step(self, x_u8, annotations=None, y_target=None):
        """One training step.  annotations: list[ObjectsAnnotation] (encoded on the device) or y_target [B,P,C].
        assigner="tal" assigns from this step's predictions: annotations only, encoded between forward and loss on the
        step's stream.  self.last_npos keeps the positives per image of the encode (device [B]; None after a y_target step)."""
        tal = self.pb.assigner == "tal"
        if tal and (y_target is not None or annotations is None):
            raise ValueError('assigner "tal" assigns from the predictions of the step: step(x, annotations=...) only, '
                             'a ready-made y_target cannot be used')
        self._poll_nonfinite()
        self.last_npos = None
        if y_target is None and not tal:
            y_target, self.last_npos, _ = self.pb.encode_batch(annotations, return_device=True)
        if tal:  # the boxes travel to the device now: nothing but the assigner's launches sits behind the forward pass
            uploaded = self.pb.upload_batch(annotations)
        self.forward(x_u8)
        if tal:
            y_target, self.last_npos, assigned = self.pb.encode_uploaded(uploaded, return_device=True, pred=self.pred)
        self.last_target = y_target
        # objectness "qfl" | "vfl": loss() launches the quality pass in front of the loss, on the step's stream
        self.loss(y_target, (uploaded[2], assigned) if tal else None)
        self.backward()
        self.allreduce()
        self.sgd()
        return self.losses

    def fit(self, batches, steps, lr_schedule=None, log_every=0, log=print, start_step=0, validate_every=None,
            validator=None):
        """Run `steps` training steps from an iterator of (x_u8 [B,H,W,3] device tensor, y_target [B,P,C] device tensor or
        list of annotations) -- what od_gen.Generator(on_device=True).flow(...) yields (the reference's unseen `fit`:
        generator -> encode_truth -> losses, check_assign.py:21-22).  lr_schedule(step) -> learning rate.  Returns the
        per-step losses [steps, 4] (objectness, class, box, total) as a numpy array; losses stay on the device until the
        end, and the loop waits for nothing but the flag copy of the step LAG steps back (_poll_nonfinite), so the host
        runs two steps ahead.  start_step: a continued run (load_state_dict) -- the schedule is asked for start_step + i,
        and the history covers the `steps` steps run here.  The flags of the last LAG steps stay pending when fit()
        returns: a run in several fit() calls is the run in one, and _poll_nonfinite(wait=True) ends a run.
        validate_every=N with validator=v (validate.Validator, or any callable (trainer, step) -> dict or str): v is called
        behind every step whose number start_step + i + 1 is a multiple of N and what it returns goes to `log`.  It reads
        the weights on the device (ObjectDetector.refresh_from) and writes nothing the training reads: the run's weights
        and losses are those of the run without it.  Both or neither (ValueError); the defaults launch nothing."""
        if (validate_every is None) != (validator is None):
            raise ValueError("fit: validate_every and validator go together (got "
                             f"validate_every={validate_every!r}, validator={'None' if validator is None else 'a validator'})")
        if validate_every is not None and (int(validate_every) != validate_every or validate_every < 1):
            raise ValueError(f"fit: validate_every must be a positive step count, got {validate_every!r}")
        hist = torch.zeros((steps, 4), dtype=torch.float32, device=self.device)
        for i, (xb, yb) in zip(range(steps), batches):
            if lr_schedule is not None:
                self.lr = float(lr_schedule(start_step + i))
            if isinstance(yb, torch.Tensor):
                self.step(xb, y_target=yb)
            else:
                self.step(xb, annotations=yb)
            hist[i].copy_(self.losses)
            if self.diverged():
                raise RuntimeError(
                    f"training diverged: {self._consecutive_skips} consecutive steps produced non-finite values (step {i + 1}, loss "
                    f"scale {self.loss_scale:g}); the forward pass itself overflows f16 -- lower the learning rate (it scales "
                    f"with the batch size) or lengthen the warm-up; the weights of the last good step are intact")
            if log_every and (start_step + i + 1) % log_every == 0:
                l = hist[i].cpu().numpy()
                log(f"step {start_step + i + 1}/{start_step + steps} lr {self.lr:.4g} loss {l[3]:.4f} (obj {l[0]:.4f} cls {l[1]:.4f} box {l[2]:.4f}) "
                    f"loss_scale {self.loss_scale:g} skipped {self.skipped_steps}"
                    + (f" grad_norm {float(self.last_grad_norm.item()):.4g}" if self._optim_path else ""))
            if validate_every is not None and (start_step + i + 1) % validate_every == 0:
                from .tk.dl import is_main_process
                res = validator(self, start_step + i + 1)
                if res is not None and is_main_process():  # every rank validates its shard; one of them reports
                    log(res if isinstance(res, str) else validation_line(res))
        return hist.cpu().numpy()

    def export_params(self, ema=False):
        """-> dict in the weights.py format (masters + BatchNorm running statistics) for ObjectDetector(params, ...).
        ema=True: the same keys and shapes from the averaged model (Trainer(ema_decay=...))."""
        if ema and self.ema_decay is None:
            raise ValueError("export_params(ema=True): this trainer keeps no averaged model (ema_decay=None)")
        host = (self.ema if ema else self.params).cpu().numpy()
        out = {}
        for (name, kind), (o, n) in self.seg.items():
            _n, cin, cout, k, _s, _bn = self.specs[name]
            a = host[o:o + n]
            out[f"{name}.{kind}"] = a.reshape(cout, k, k, cin).copy() if kind == "w" else a.copy()
        if not ema:
            for name in self.run_mean:
                out[name + ".mean"] = self.run_mean[name].cpu().numpy()
                out[name + ".var"] = self.run_var[name].cpu().numpy()
            return out
        rhost = self.ema_run_stats.cpu().numpy()
        for name, o in self._run_off.items():
            c = self.specs[name][2]
            cp = desc.pad_to(c, 4)
            out[name + ".mean"] = rhost[o:o + c].copy()
            out[name + ".var"] = rhost[o + cp:o + cp + c].copy()
        return out

    # ---- resumable state ------------------------------------------------------------------------------------------
    _STATE_SCALARS = ("loss_scale", "_good_steps", "skipped_steps", "_consecutive_skips", "ema_updates")

    def _layout(self):
        """What a state's flat buffers mean: the segments of params / mom / ema in buffer order and the BatchNorm layers
        of run_stats, as arrays an .npz can hold."""
        keys = list(self.seg)
        return {"layout.names": np.array([k[0] for k in keys]), "layout.kinds": np.array([k[1] for k in keys]),
                "layout.offsets": np.array([self.seg[k][0] for k in keys], np.int64),
                "layout.counts": np.array([self.seg[k][1] for k in keys], np.int64),
                "layout.run_names": np.array(list(self._run_off)),
                "layout.run_offsets": np.array(list(self._run_off.values()), np.int64),
                "layout.sizes": np.array([self.n_flat, self.run_stats.numel()], np.int64)}

    def state_dict(self):
        """Everything a continued run needs, as host numpy arrays and scalars (weights.save_state writes it): masters,
        momentum, BatchNorm running statistics, the averaged model when there is one, the loss-scale control's counters
        and the layout record that load_state_dict checks.  An observer: it applies no pending flag, it waits for their
        values and stores them as "pending_flags" (int32, oldest first, at most LAG entries in a run of step() calls), so
        that a run goes on as if it had not been called and a resumed run applies them at the same steps."""
        sd = {"params": self.params.cpu().numpy(), "mom": self.mom.cpu().numpy(), "run_stats": self.run_stats.cpu().numpy()}
        if self.ema_decay is not None:
            sd["ema"], sd["ema_run_stats"] = self.ema.cpu().numpy(), self.ema_run_stats.cpu().numpy()
        sd["loss_scale"] = float(self.loss_scale)
        for k in self._STATE_SCALARS[1:]:
            sd[k] = int(getattr(self, k))
        sd["pending_flags"] = np.array(self.pending_flags(), np.int32)
        sd["ema_decay"] = self.ema_decay  # None = no averaged model (weights.save_state leaves a None out of the file)
        sd["optimizer"] = self.optimizer
        if self.mom2 is not None:
            sd["mom2"] = self.mom2.cpu().numpy()
        if self._optim_path:  # what od_optim_prepare carries from step to step; the other fields are rewritten every step
            st = _lib.OptimState.from_buffer_copy(self.optim_state.cpu().numpy().tobytes())
            sd["optim_state"] = np.array((st.step, st.b1pow, st.b2pow), OPTIM_STATE_DTYPE)  # a 0-d record: an .npz holds it
        sd.update(self._layout())
        return sd

    def load_state_dict(self, sd):
        """Continue from a state_dict() of a trainer with the same layout and the same EMA switch (ValueError otherwise):
        uploads every buffer, sets the counters, puts the state's pending flags in place of this trainer's own (a state
        without "pending_flags" is of the older format: none pending), re-packs the f16 weights, and has the next sgd()
        rebuild its table."""
        mine = self._layout()
        for k, v in mine.items():
            if k not in sd or not np.array_equal(np.asarray(sd[k]), v):
                raise ValueError(f"load_state_dict: the state's {k} is not this trainer's (another architecture or class count)")
        has_ema = "ema" in sd
        if has_ema != (self.ema_decay is not None):
            raise ValueError("load_state_dict: the state " + ("has" if has_ema else "has no") + " averaged model, the trainer "
                             + ("has none (ema_decay=None)" if has_ema else "keeps one"))
        theirs = str(np.asarray(sd["optimizer"]).item()) if "optimizer" in sd else "sgd"  # an older state is an SGD one
        if theirs != self.optimizer:
            raise ValueError(f"load_state_dict: the state is of optimizer {theirs!r}, this trainer runs {self.optimizer!r}")
        bufs = [("params", self.params), ("mom", self.mom), ("run_stats", self.run_stats)]
        if self.mom2 is not None:
            bufs += [("mom2", self.mom2)]
        if has_ema:
            bufs += [("ema", self.ema), ("ema_run_stats", self.ema_run_stats)]
        for k, t in bufs:
            if k not in sd:
                raise ValueError(f"load_state_dict: the state has no {k}")
            a = np.ascontiguousarray(sd[k], np.float32)
            if a.shape != tuple(t.shape):
                raise ValueError(f"load_state_dict: {k} has shape {a.shape}, expected {tuple(t.shape)}")
        pending = [int(v) for v in np.asarray(sd["pending_flags"]).reshape(-1)] if "pending_flags" in sd else []
        self._poll_nonfinite(wait=True)  # flags of this trainer's own earlier steps must not touch the loaded counters
        self._flag_queue[:] = pending
        for k, t in bufs:
            t.copy_(torch.from_numpy(np.ascontiguousarray(sd[k], np.float32)))
        self.loss_scale = float(sd["loss_scale"])
        for k in self._STATE_SCALARS[1:]:
            setattr(self, k, int(sd[k]))
        if has_ema:
            self.ema_decay = float(sd["ema_decay"])
        if self._optim_path:  # a state without the record (an SGD run without clipping) starts the count afresh
            ost = np.asarray(sd["optim_state"] if "optim_state" in sd else np.array((0, 1.0, 1.0), OPTIM_STATE_DTYPE))
            st = _lib.OptimState()
            st.step, st.b1pow, st.b2pow = int(ost["step"]), float(ost["b1pow"]), float(ost["b2pow"])
            st.bc1, st.bc2 = float(np.float32(1) - np.float32(st.b1pow)), float(np.float32(1) - np.float32(st.b2pow))
            self.optim_state.copy_(torch.frombuffer(bytearray(bytes(st)), dtype=torch.int32))
        self._repack()
        self._sgd_key = None


def validation_line(entry):
    """The log line of one validation record: its step first, then every scalar of the dict in order."""
    rest = " ".join(f"{k} {v:.4f}" if isinstance(v, float) else f"{k} {v}" for k, v in entry.items()
                    if k != "step" and isinstance(v, (int, float, str, bool)))
    return f"validation at step {entry.get('step', '?')}: {rest}"


# "optim_state" of a state_dict: what od_optim_prepare carries from step to step
OPTIM_STATE_DTYPE = np.dtype([("step", np.int32), ("b1pow", np.float32), ("b2pow", np.float32)])


def check_optimizer_args(optimizer, betas, adam_eps, clip_grad_norm):
    """ValueError for an optimizer setting the trainer cannot run (host-only: no library is loaded).
    -> (optimizer, (beta1, beta2), adam_eps, clip_grad_norm or None) as floats."""
    if optimizer not in _lib.OPTIMIZERS:
        raise ValueError(f"optimizer must be one of {sorted(_lib.OPTIMIZERS)}, got {optimizer!r}")
    try:
        b1, b2 = (float(b) for b in betas)
    except (TypeError, ValueError):
        raise ValueError(f"betas must be (beta1, beta2), got {betas!r}") from None
    if not (0.0 <= b1 < 1.0 and 0.0 <= b2 < 1.0):
        raise ValueError(f"betas must lie in [0, 1), got {betas!r}")
    eps = float(adam_eps)
    if not (math.isfinite(eps) and eps > 0.0):
        raise ValueError(f"adam_eps must be positive and finite, got {adam_eps!r}")
    if clip_grad_norm is not None:
        clip_grad_norm = float(clip_grad_norm)
        if not (math.isfinite(clip_grad_norm) and clip_grad_norm > 0.0):
            raise ValueError(f"clip_grad_norm must be None or positive and finite, got {clip_grad_norm!r}")
    return optimizer, (b1, b2), eps, clip_grad_norm


def check_objectness_args(objectness, quality, assigner):
    """ValueError for an objectness term or a quality target the trainer cannot run (host-only: no library is loaded):
    unknown names, and quality="tal" without assigner="tal" (its inputs are the task-aligned assignment's outputs)."""
    if objectness not in OBJ_MODES:
        raise ValueError(f"objectness must be one of {sorted(OBJ_MODES)}, got {objectness!r}")
    if quality not in QUALITY_MODES:
        raise ValueError(f"quality must be one of {QUALITY_MODES}, got {quality!r}")
    if quality == "tal" and assigner != "tal":
        raise ValueError(f'quality="tal" needs assigner="tal" (it normalises the metric of that assignment), got '
                         f'assigner={assigner!r}')


def make_buckets(layers, n_flat, min_elems):
    """Gradient buckets for the overlapped all-reduce.  layers: [(lo, hi, name)] in buffer (= forward) order, contiguous
    and covering [0, n_flat).  -> [(lo, hi, {layer names})] in the order backward completes them: contiguous ranges cut
    at layer boundaries, walking from the last layer to the first, each at least `min_elems` long (the last one takes
    whatever is left)."""
    buckets, hi, names = [], n_flat, set()
    for lo, _h, name in reversed(layers):
        names.add(name)
        if hi - lo >= min_elems:
            buckets.append((lo, hi, names))
            hi, names = lo, set()
    if names:
        buckets.append((0, hi, names))
    return buckets


def dp_allreduce_(flat: torch.Tensor):
    """In-place sum over the ranks of the default process group (backend "nccl" = RCCL on GPUs, gloo in CPU tests)."""
    torch.distributed.all_reduce(flat, op=torch.distributed.ReduceOp.SUM)
    return flat


def dp_effective_scale(loss_scale: float, world: int) -> float:
    """od_sgd_step's inv_loss_scale: undo the loss scale and average the summed gradients over the ranks."""
    return 1.0 / (loss_scale * world)


def init_comm(ctx: Context):
    """Create the RCCL communicator of this rank through the C ABI; the unique id travels over torch.distributed."""
    rank, world = torch.distributed.get_rank(), torch.distributed.get_world_size()
    nbytes = ctx.lib.od_comm_unique_id_bytes()
    buf = (C.c_ubyte * nbytes)()
    if rank == 0:
        _lib.check(ctx.lib.od_comm_get_unique_id(buf, nbytes), "od_comm_get_unique_id")
    box = [bytes(buf)]
    torch.distributed.broadcast_object_list(box, src=0)
    raw = (C.c_ubyte * nbytes).from_buffer_copy(box[0])
    h = C.c_void_p()
    _lib.check(ctx.lib.od_comm_init(ctx.handle, rank, world, raw, C.byref(h)), "od_comm_init")
    return h, world
