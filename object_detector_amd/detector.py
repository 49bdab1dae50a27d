"""`tk.dl.od.ObjectDetector`: the drop-in boundary of the hot path.

Keeps the call surface the reference scripts use (voc_validate.py:25-27, voc_evaluate.py:25-27, check_assign.py:19):
    ObjectDetector.load_voc(batch_size, input_size=(320,320), keep_aspect=False, strict_nms=False, use_multi_gpu=True)
    od.predict(X, conf_threshold=...) -> list of per-image predictions (.classes, .confs, .bboxes, .plot(x, names))
    od.pb.encode_truth / od.pb.decode_locs
and runs everything below it on MI355X through libodhip.so.  use_multi_gpu shards images by index over the ranks of
an already-initialised torch.distributed job (one process per GPU); inference needs no collective on the data path,
results are gathered on the host.
"""
from __future__ import annotations

import contextlib
import os
import pathlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import slicing
from . import weights as W
from .net import Net
from .pb import ObjectsAnnotation, PriorBoxes
from .postprocess import SOFT_SIGMA, Postprocessor, check_nms_args
from .tta import VOTE_IOU, TtaPostprocessor, normalize_views

DEFAULT_CONF_THRESHOLD = 0.01  # [BUILD-DEFINED]: mAP needs the low-confidence tail (voc_evaluate.py:27 passes 0.6)
PREFETCH_AHEAD = 2  # predict(): batches whose host work is started before the current one is submitted
N_STAGING = PREFETCH_AHEAD + 2  # a staging buffer is busy from the start of its decode until its upload has completed
VOC_WEIGHTS_ENV = "OD_VOC_WEIGHTS"


class ObjectsPrediction:
    """Detections of one image: classes i32 [n], confs f32 [n], bboxes f32 [n,4] (corner form, normalised [0,1] of the
    ORIGINAL image: keep_aspect=False is a plain resize, so normalised coordinates are resize-invariant)."""

    def __init__(self, classes, confs, bboxes, flat_indices=None):
        self.classes = np.asarray(classes, np.int32)
        self.confs = np.asarray(confs, np.float32)
        self.bboxes = np.asarray(bboxes, np.float32).reshape(-1, 4)
        self.flat_indices = None if flat_indices is None else np.asarray(flat_indices, np.int32)

    def plot(self, x, class_names=None):
        from .tk import ml
        return ml.plot_objects(x, self.classes, self.confs, self.bboxes, class_names)

    def __len__(self):
        return len(self.classes)


from .imageio import decode_chunk_into_shm, load_image  # noqa: E402,F401  (host-side decode + resize; re-exported)


def dist_info(use_multi_gpu=True):
    """(rank, world) of the torch.distributed job this process belongs to (one process per GPU), else (0, 1)."""
    if use_multi_gpu and torch.distributed.is_available() and torch.distributed.is_initialized():
        return torch.distributed.get_rank(), torch.distributed.get_world_size()
    return 0, 1


def shard_indices(n, rank, world):
    """Images are independent: rank r takes indices r, r+world, ... -- no collective on the data path."""
    return list(range(rank, n, world))


def gather_results(local: dict, world: int) -> dict:
    """Host-side gather of the per-rank {index: prediction} maps (variable-length results; every rank gets all)."""
    if world <= 1:
        return local
    gathered = [None] * world
    torch.distributed.all_gather_object(gathered, local)
    out = {}
    for d in gathered:
        out.update(d)
    return out


_QUEUE_SETS = {}  # (device index, n) -> [torch.cuda.Stream] that were measured to run concurrently


def _streams_overlap(a, b, spin_cycles):
    """True when a kernel queued on `b` finishes while an earlier, long kernel on `a` is still running (different hardware
    queues); False when `b`'s kernel had to wait for it (same queue)."""
    ea, eb = torch.cuda.Event(), torch.cuda.Event()
    with torch.cuda.stream(a):
        torch.cuda._sleep(spin_cycles)
        ea.record()
    with torch.cuda.stream(b):
        torch.cuda._sleep(1)
        eb.record()
    eb.synchronize()
    free = not ea.query()
    ea.synchronize()
    return free


def stream_queue_sets(device, n, candidates=6, seed_streams=(), beside=None):
    """n streams of `device` that overlap pairwise -- and with the stream `beside`, if given (the trainer's side streams must
    run next to its main stream) -- chosen greedily from `candidates` fresh streams by the probe above (about 2 ms per pair,
    a few dozen ms once per process); cached.  Falls back to creation order when the probe cannot tell streams apart (e.g.
    a runtime that serialises everything)."""
    device = torch.device(device)
    key = (device.index if device.index is not None else torch.cuda.current_device(), n,
           None if beside is None else beside.cuda_stream)
    if key in _QUEUE_SETS:
        return _QUEUE_SETS[key]
    if not hasattr(torch.cuda, "_sleep"):  # no spin kernel to probe with: creation order (what rounds 1-2 started from)
        _QUEUE_SETS[key] = list(seed_streams)[:n] + [torch.cuda.Stream(device=device) for _ in range(n - min(n, len(seed_streams)))]
        return _QUEUE_SETS[key]
    with torch.cuda.device(device):
        cands = list(seed_streams) + [torch.cuda.Stream(device=device) for _ in range(max(candidates, n) - len(seed_streams))]
        for c in cands:  # every stream's first launch (queue creation) happens outside the probes
            with torch.cuda.stream(c):
                torch.cuda._sleep(1000)
        torch.cuda.synchronize(device)
        # spin length: ~2 ms of a kernel that does nothing but read the clock (calibrated, the tick rate is not assumed)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(cands[0]):
            torch.cuda._sleep(1000)  # first launch: module load
            e0.record()
            torch.cuda._sleep(200000)
            e1.record()
        e1.synchronize()
        per_ms = 200000 / max(e0.elapsed_time(e1), 1e-3)
        spin = int(max(1000, 2.0 * per_ms))
        chosen = []
        fixed = [] if beside is None else [beside]
        for c in cands:
            if len(chosen) == n:
                break
            if all(_streams_overlap(q, c, spin) and _streams_overlap(c, q, spin) for q in fixed + chosen):
                chosen.append(c)
        for c in cands:  # not enough distinguishable queues: take the rest in creation order
            if len(chosen) == n:
                break
            if c not in chosen:
                chosen.append(c)
    _QUEUE_SETS[key] = chosen
    return chosen


def _device_key(device):
    d = torch.device(device)
    if d.type == "cuda" and d.index is None:
        return d.type, (torch.cuda.current_device() if torch.cuda.is_available() else 0)
    return d.type, d.index


def check_refresh(device, arch, trainer, ema):
    """ValueError for a (detector, trainer) pair ObjectDetector.refresh_from cannot serve -- a trainer on another device or
    of another architecture ((num_classes, neck_ch, tower) and the layer specs), ema=True without an averaged model.
    Host-only: runs before anything touches the GPU."""
    if _device_key(trainer.device) != _device_key(device):
        raise ValueError(f"refresh_from: the trainer lives on {trainer.device}, the detector on {device}; the refresh is a "
                         f"launch on one device")
    theirs = (trainer.num_classes, trainer.neck_ch, trainer.tower)
    if tuple(arch) != theirs or list(trainer.specs.values()) != W.layer_specs(*arch):
        raise ValueError(f"refresh_from: the trainer's architecture (classes, neck channels, tower) = {theirs} is not the "
                         f"detector's {tuple(arch)}")
    if ema and trainer.ema_decay is None:
        raise ValueError("refresh_from(ema=True): this trainer keeps no averaged model (ema_decay=None)")


class _Pipeline:
    """One batch in flight: its own activation buffers (Net), post-processing buffers and HIP stream."""

    def __init__(self, net, post, stream, tta=None, slc=None):
        self.net, self.post, self.stream = net, post, stream
        self.tta = tta  # TtaPostprocessor beside `post` when the detector runs test-time augmentation
        self.slc = slc  # slicing.SlicePostprocessor beside `post` when the detector runs sliced inference
        self.done = torch.cuda.Event()
        self.decoder = None  # devdecode.BatchDecoder of image_decode="device", made on first use


class ObjectDetector:
    def __init__(self, params, batch_size=16, input_size=(320, 320), keep_aspect=False, strict_nms=False,
                 use_multi_gpu=True, device=None, prior_wh=None, n_inflight=None, precision=None, image_decode="host",
                 tta=None, tta_vote_iou=VOTE_IOU, slices=None, slice_overlap=0.2, slice_full_view=True, slice_edge=0.01,
                 slice_vote_iou=VOTE_IOU, nms="hard", soft_sigma=SOFT_SIGMA, soft_min_conf=None):
        # the suppression stage: "hard" (greedy NMS, the default path, unchanged), "soft-linear" or "soft-gaussian" (Soft-NMS:
        # neighbours' scores decay instead of being deleted; soft_min_conf=None = the call's conf_threshold).  On every
        # route: plain, tta, slices.  Checked before anything touches the GPU.
        self.nms, self.soft_sigma, self.soft_min_conf = check_nms_args(nms, soft_sigma, soft_min_conf)
        # test-time augmentation: None = off (the plain path, unchanged); () = the identity view alone (box voting only);
        # ("flip",) = identity + horizontal mirror, merged on the device (tta.py).  Checked before anything touches the GPU.
        self.tta = normalize_views(tta)
        self.tta_vote_iou = float(tta_vote_iou)
        # sliced inference: None = off (the plain path, unchanged); (ny, nx) = every image is cut into ny x nx overlapping
        # tiles (+ the whole image), T rows of the network batch each, merged on the device (slicing.py).  Also checked here.
        self.slices = slicing.normalize(slices, slice_overlap, slice_full_view, slice_edge, batch_size=batch_size, tta=tta,
                                        keep_aspect=keep_aspect)
        self.slice_vote_iou = float(slice_vote_iou)
        if device is None:  # one process per GPU; the modulo only matters when several ranks rehearse on one GPU
            device = f"cuda:{int(os.environ.get('LOCAL_RANK', 0)) % max(1, torch.cuda.device_count())}"
        if not torch.cuda.is_available():
            from ._lib import OdError
            raise OdError("ObjectDetector needs an MI355X (no GPU visible); there is no CPU path")
        self.device = torch.device(device)
        torch.cuda.set_device(self.device)
        self.batch_size = int(batch_size)
        self.input_size = tuple(int(v) for v in input_size)
        self.keep_aspect, self.strict_nms, self.use_multi_gpu = bool(keep_aspect), bool(strict_nms), bool(use_multi_gpu)
        # predict()'s image route: "host" = PIL decode + resize on the host; "device" = JPEG decode and every resize on
        # the GPU (devdecode.py), byte-identical network input.  decode_stats counts the device route's inputs per route.
        if image_decode not in ("host", "device"):
            raise ValueError(f"image_decode must be 'host' or 'device', got {image_decode!r}")
        self.image_decode = image_decode
        self.decode_stats = {"jpeg": 0, "fallback": 0, "array": 0}
        # after refresh_from() the weights on the device are the trainer's and `params` is STALE: it stays the dict the
        # detector was built from.  refreshed_from: None, or (id(trainer), ema, trainer.steps_issued) of the last refresh
        self.params = params
        self.refreshed_from = None
        self._refresh_ev = None  # recorded behind the last refresh: a pipeline's stream waits for it before its next batch
        self.arch = W.infer_arch(params)
        self.num_classes, _, _ = self.arch
        kw = {} if prior_wh is None else {"prior_wh": prior_wh}
        self.pb = PriorBoxes(self.input_size, self.num_classes, device=self.device, **kw)
        n = int(n_inflight) if n_inflight is not None else int(os.environ.get("OD_INFLIGHT", 3))  # explicit argument wins
        # precision: "f16" (default, the throughput plan) or "mixed" (f32 residual stream + split operands in the last layers:
        # north_star's 1e-3 logit tolerance at any logit scale, net.py); None = $OD_PRECISION or "f16"
        self.net = Net(params, self.batch_size, self.input_size, device=self.device, overlapped=n > 1, precision=precision)
        self.precision = self.net.precision
        assert self.net.P == len(self.pb)
        self.post = Postprocessor(self.batch_size, self.net.P, self.num_classes, self.pb.pb_locs, device=self.device,
                                  strict_nms=self.strict_nms, loc_scale=self.pb.loc_scale, **self._nms_kw())
        # Batches in flight (submit / collect): every pipeline has its own buffers and stream, so the launch ramps, tile
        # tails, epilogue write bursts and the small post-processing kernels of one batch overlap the convolutions of the
        # next (measured +23 % images/s at batch 32 with 2-3 in flight, profiles/r01/inflight_sweep.txt).  Pipeline 0 =
        # (self.net, self.post) on the caller's stream is what predict_batch_device uses.
        self._pipes = [_Pipeline(self.net, self.post, torch.cuda.Stream(device=self.device), self._make_tta(self.post),
                                 self._make_slc(self.net, self.post))]
        for _ in range(max(1, n) - 1):
            net = Net(params, self.batch_size, self.input_size, device=self.device, overlapped=True,
                      share_weights_with=self.net, precision=self.precision, stream_stages=self.net.stream_stages,
                      split=self.net.split, wide_fpn=self.net.wide_fpn)
            post = Postprocessor(self.batch_size, net.P, self.num_classes, self.pb.pb_locs, device=self.device,
                                 strict_nms=self.strict_nms, loc_scale=self.pb.loc_scale, **self._nms_kw())
            self._pipes.append(_Pipeline(net, post, torch.cuda.Stream(device=self.device), self._make_tta(post),
                                         self._make_slc(net, post)))
        self._next = 0
        self._hbufs = None  # predict()'s pinned staging: N_STAGING x [buffer, event of its last upload], made on first use
        self._calibrated = len(self._pipes) < 2 or os.environ.get("OD_INFLIGHT_CALIBRATE", "1") == "0"

    def _nms_kw(self):
        return {"nms": self.nms, "soft_sigma": self.soft_sigma, "soft_min_conf": self.soft_min_conf}

    def _make_tta(self, post):
        if self.tta is None:
            return None
        return TtaPostprocessor(post, self.net.input.shape, self.tta, self.tta_vote_iou)

    def _make_slc(self, net, post):
        if self.slices is None:
            return None
        slc = slicing.SlicePostprocessor(post, self.slices, self.slice_vote_iou)
        net.input[slc.G * slc.T:].zero_()  # rows no image's tile ever lands in: zeroed once, their candidates are never read
        torch.cuda.current_stream(self.device).synchronize()  # the pipelines write this buffer on their own streams
        return slc

    def _no_batch_entry_with_slices(self, what, graph=False):
        if self.slices is not None:
            if graph:
                raise ValueError("graph=True is not available with slices: the sliced step is not one captured plan")
            raise ValueError(f"{what} takes a ready-made batch and a sliced batch needs its tile rectangles: "
                             f"with slices, predict() is the public route")

    @staticmethod
    def _no_graph_with_tta(graph):
        if graph:
            raise ValueError("graph=True is not available with tta: the captured plan replays one view")

    # -- construction -----------------------------------------------------------------------------------------
    @classmethod
    def load_voc(cls, batch_size, input_size=(320, 320), keep_aspect=False, strict_nms=False, use_multi_gpu=True,
                 weights=None, **kw):
        """VOC-trained detector.  The reference pulls an LFS `*.h5` (.gitattributes:5); offline this build reads its own
        .npz from `weights`, $OD_VOC_WEIGHTS, or ./weights/voc07+12_<H>x<W>.npz -- a LOCAL path, never a download."""
        path = weights or os.environ.get(VOC_WEIGHTS_ENV) or \
            pathlib.Path("weights") / f"voc07+12_{input_size[0]}x{input_size[1]}.npz"
        path = pathlib.Path(path)
        if not path.exists():
            raise FileNotFoundError(
                f"VOC weights not found at {path}. Trained weights are not distributable offline; pass weights=<npz>, "
                f"set ${VOC_WEIGHTS_ENV}, or build a synthetic detector with ObjectDetector.synthetic(...).")
        params, meta = W.load(path)
        if "prior_wh" in meta:
            kw.setdefault("prior_wh", meta["prior_wh"])
        return cls(params, batch_size, input_size, keep_aspect, strict_nms, use_multi_gpu, **kw)

    @classmethod
    def synthetic(cls, batch_size, input_size=(320, 320), seed=2, num_classes=20, **kw):
        """Random-init detector of the VOC architecture (benchmarks / parity tests)."""
        return cls(W.random_init(seed, num_classes), batch_size, input_size, **kw)

    @classmethod
    def from_trainer(cls, trainer, batch_size=None, ema=False, **kw):
        """A detector of `trainer`'s architecture, input size, priors and device holding its current weights (ema=True: the
        averaged model): the host route once (export_params, fold, pack, upload), refresh_from(trainer) from then on."""
        kw.setdefault("device", trainer.device)
        kw.setdefault("prior_wh", trainer.pb.prior_wh)
        od = cls(trainer.export_params(ema=ema), trainer.B if batch_size is None else batch_size,
                 (trainer.H0, trainer.W0), **kw)
        od.refreshed_from = (id(trainer), bool(ema), trainer.steps_issued)
        return od

    def refresh_from(self, trainer, ema=False):
        """Rewrite this detector's weights on the device from a live Trainer's flat buffers -- trainer.params / run_stats, or
        with ema=True the averaged model trainer.ema / ema_run_stats -- in one launch (od_net_refresh): the bits of
        ObjectDetector(trainer.export_params(ema), ...) without the host round trip.  In place, so every pipeline, plan and
        captured graph of the detector runs the new weights.  ValueError (before anything touches the GPU) for a trainer
        on another device or of another architecture, and for ema=True without an averaged model.

        Ordering, with no host synchronisation: the launch goes on the CURRENT stream, where the trainer's step was issued;
        it first waits for the `done` event of every pipeline (no batch in flight reads half-written weights), and every
        pipeline's stream waits for an event recorded behind it before its next batch.  self.params is left alone and is
        stale afterwards; self.refreshed_from records (id(trainer), ema, trainer.steps_issued)."""
        check_refresh(self.device, self.arch, trainer, ema)
        cur = torch.cuda.current_stream(self.device)
        for p in self._pipes:
            cur.wait_event(p.done)
        self.net.refresh(trainer, ema)
        ev = torch.cuda.Event()
        ev.record(cur)
        for p in self._pipes:
            p.stream.wait_event(ev)
        self._refresh_ev = ev  # _pick_streams: streams chosen later wait for it too
        self.refreshed_from = (id(trainer), bool(ema), trainer.steps_issued)

    # -- inference --------------------------------------------------------------------------------------------
    def predict_batch_device(self, x_u8: torch.Tensor, conf_threshold=DEFAULT_CONF_THRESHOLD, graph=False):
        """uint8 [B,H,W,3] on device -> (keep_flat [B,max_det], keep_count [B]) on device.  The timed hot path.
        With tta: -> (det f32 [B, 1 + 6*max_det], keep_count [B]) on device; det is od_tta_merge's record block (word 0 =
        keep count, row r = {class (int bits), conf, x1, y1, x2, y2}): a merged detection has no single flat index.
        With slices: ValueError (predict() is the route)."""
        self._no_batch_entry_with_slices("predict_batch_device", graph)
        torch.cuda.current_stream(self.device).wait_stream(self._pipes[0].stream)  # pipeline 0's buffers may be in flight
        if self.tta is not None:
            self._no_graph_with_tta(graph)
            return self._pipes[0].tta.run(self.net, x_u8, conf_threshold)
        pred = self.net.forward(x_u8, graph=graph)
        return self.post.run(pred, conf_threshold)

    # -- batches in flight ------------------------------------------------------------------------------------------
    @property
    def n_inflight(self):
        return len(self._pipes)

    def submit(self, x_u8: torch.Tensor, conf_threshold=DEFAULT_CONF_THRESHOLD, graph=False, gather=False) -> int:
        """Queue one batch on the next pipeline's stream and return its ticket.  Never blocks the host: a pipeline's new
        batch is stream-ordered behind its previous one (whose results it overwrites -- collect() them first).
        With tta every view runs on that stream and the merged record block is always copied to the host (`gather` is moot).
        With slices: ValueError (predict() is the route)."""
        self._no_batch_entry_with_slices("submit", graph)
        if self.tta is not None:
            self._no_graph_with_tta(graph)
        with self._next_pipeline() as (ticket, p):  # x_u8 was produced on the caller's stream
            self._forward_post(p, x_u8, conf_threshold, graph, gather)
        x_u8.record_stream(p.stream)
        return ticket

    @contextlib.contextmanager
    def _next_pipeline(self):
        """What every submit shares: the streams are calibrated on first use, the next pipeline is taken, its stream waits
        for the caller's and is the current one inside the block, and `done` is recorded behind what the block queued.
        -> (ticket, pipeline)"""
        if not self._calibrated:
            self._pick_streams()
        i = self._next
        self._next = (i + 1) % len(self._pipes)
        p = self._pipes[i]
        p.stream.wait_stream(torch.cuda.current_stream(self.device))
        with torch.cuda.stream(p.stream):
            yield i, p
            p.done.record()

    @staticmethod
    def _forward_post(p, x_u8, conf_threshold, graph=False, gather=True):
        """The network and the post-processing of one unsliced batch on the current stream (x_u8 None: p.net.input)."""
        if p.tta is not None:
            p.tta.run(p.net, x_u8, conf_threshold)  # x_u8 None: the mirror is taken from the decoded input
        else:
            pred = p.net.forward(x_u8, graph=graph)
            p.post.run(pred, conf_threshold)
            if gather:
                p.post.gather()  # kept detections -> one record block -> pinned host memory, still on this stream

    def _decoder(self, p):
        """The pipeline's devdecode.BatchDecoder, made on first use."""
        if p.decoder is None:
            from .devdecode import BatchDecoder
            p.decoder = BatchDecoder(self.device)
        return p.decoder

    def _submit_images(self, items, conf_threshold=DEFAULT_CONF_THRESHOLD) -> int:
        """submit() for image_decode="device": the upload and the decode / resize kernels of `items` (devdecode.prepare
        results) write the next pipeline's Net.input on its stream, and the network runs on that input without a copy."""
        with self._next_pipeline() as (ticket, p):
            self._decoder(p).run(items, p.net.input)
            self._forward_post(p, None, conf_threshold)
        for it in items:
            self.decode_stats[it[0]] += 1
        return ticket

    def _pick_streams(self):
        """One stream per pipeline, on DIFFERENT hardware queues.  HIP deals streams onto a few hardware queues (4 by
        default) in creation order, and kernels of two streams that share a queue never overlap: with 1-2 foreign streams
        created first the same code ran at 15.9 k instead of 18.8 k images/s.  Instead of timing real steps on every stream
        combination (rounds 1-2), the queue map is MEASURED once per process and device with a probe that does no real work
        (stream_queue_sets) and cached; every detector of the process takes its streams from that set."""
        self._calibrated = True
        sts = stream_queue_sets(self.device, len(self._pipes), seed_streams=[p.stream for p in self._pipes])
        for p, st in zip(self._pipes, sts):
            if self._refresh_ev is not None:  # the stream it replaces was ordered behind the last refresh_from
                st.wait_event(self._refresh_ev)
            p.stream = st
        self._next = 0

    def collect(self, ticket: int):
        """Wait for the batch submitted with `ticket`; -> (keep_flat [B,max_det], keep_count [B]) on device.
        With tta: -> (det [B, 1 + 6*max_det], keep_count [B]), as predict_batch_device.  With slices: ValueError."""
        self._no_batch_entry_with_slices("collect")
        p = self._pipes[ticket]
        p.done.synchronize()
        if p.tta is not None:
            return p.post.det, p.post.keep_count
        return p.post.keep_flat, p.post.keep_count

    def synchronize(self):
        for p in self._pipes:
            p.stream.synchronize()

    def _collect(self, n_valid, scales=None, post=None):
        """Per-image predictions of a collected batch from its pinned record block (submit(..., gather=True) queued the
        gather kernel and the single device->host copy behind the NMS; no per-image device work or synchronisation)."""
        post = post or self.post
        NC = self.num_classes
        out = []
        for b, (k, confs, bxs) in enumerate(post.detections_host(n_valid)):
            if scales is not None and scales[b] != (1.0, 1.0):  # keep_aspect: canvas coordinates -> image coordinates
                sx, sy = scales[b]
                bxs = np.clip(bxs / np.array([sx, sy, sx, sy], np.float32), 0.0, 1.0)
            if self.tta is not None:  # word 0 of a merged record is the class; there is no flat index
                out.append(ObjectsPrediction(k, confs, bxs, None))
            else:
                out.append(ObjectsPrediction(k % NC, confs, bxs, k))
        return out

    def _decode_procs(self, n, nbytes):
        """Lazily created pool of spawned decode workers + their shared-memory staging block (kept for the detector's life)."""
        import atexit
        import multiprocessing as mp
        from concurrent.futures import ProcessPoolExecutor
        from multiprocessing import shared_memory
        st = getattr(self, "_dproc", None)
        if st is not None and (st[2] != n or st[1].size < nbytes):
            self.close_decode_pool()
            st = None
        if st is None:
            pool = ProcessPoolExecutor(max_workers=n, mp_context=mp.get_context("spawn"))
            shm = shared_memory.SharedMemory(create=True, size=nbytes)
            st = self._dproc = (pool, shm, n)
            atexit.register(self.close_decode_pool)
        return st[0], st[1]

    def close_decode_pool(self):
        st = getattr(self, "_dproc", None)
        self._dproc = None
        if st is not None:
            st[0].shutdown(wait=True, cancel_futures=True)
            st[1].close()
            try:
                st[1].unlink()
            except FileNotFoundError:
                pass

    def predict(self, X, conf_threshold=DEFAULT_CONF_THRESHOLD, verbose=0, image_decode=None):
        """X: sequence of image paths or uint8 arrays -> list[ObjectsPrediction] in input order.
        image_decode: "host" / "device" for this call (None = the detector's setting).
        With slices every image is cut into tiles that share a network batch (_predict_sliced): bboxes are in [0,1]
        coordinates of the whole image and flat_indices is None."""
        X = list(X)
        route = self.image_decode if image_decode is None else image_decode
        if route not in ("host", "device"):
            raise ValueError(f"image_decode must be 'host' or 'device', got {route!r}")
        rank, world = dist_info(self.use_multi_gpu)
        mine = shard_indices(len(X), rank, world)
        run = self._predict_plain if self.slices is None else self._predict_sliced
        results = gather_results(run(X, mine, conf_threshold, route), world)
        return [results[i] for i in range(len(X))]

    def _run_batches(self, batches, start, finish, drain):
        """The look-ahead loop of predict(): start(bi) begins the host work of batch bi and returns its futures -- issued
        PREFETCH_AHEAD batches early, so decode + upload of the next batches overlaps the device work of this one --,
        finish(bi, results) submits the batch and returns what drain(image indices, that) reads its results with.  A
        pipeline's results are drained before it is reused, the rest at the end."""
        pending = []  # (image indices, what finish returned), oldest first
        futs = {bi: start(bi) for bi in range(min(PREFETCH_AHEAD + 1, len(batches)))}
        for bi, idx in enumerate(batches):
            if bi + PREFETCH_AHEAD + 1 < len(batches):
                futs[bi + PREFETCH_AHEAD + 1] = start(bi + PREFETCH_AHEAD + 1)
            res = [f.result() for f in futs.pop(bi)]
            if len(pending) == len(self._pipes):  # the pipeline about to be reused still holds unread results
                drain(*pending.pop(0))
            pending.append((idx, finish(bi, res)))
        for entry in pending:
            drain(*entry)

    @staticmethod
    def _decode_threads():
        """predict()'s pool of decode threads: OD_DECODE_THREADS, or up to 8."""
        nthreads = int(os.environ.get("OD_DECODE_THREADS", "0")) or min(8, os.cpu_count() or 1)
        return ThreadPoolExecutor(max_workers=max(1, nthreads))

    def _stage(self, bi):
        """Pinned staging buffer of batch bi as a numpy array uint8 [B,H,W,3], free to be written."""
        if self._hbufs is None:
            shape = (self.batch_size,) + tuple(self.input_size) + (3,)
            self._hbufs = [[torch.zeros(shape, dtype=torch.uint8).pin_memory(), None] for _ in range(N_STAGING)]
        hb = self._hbufs[bi % N_STAGING]
        if hb[1] is not None:
            hb[1].synchronize()  # the upload that last read this pinned buffer
            hb[1] = None
        return hb[0].numpy()

    def _upload_stage(self, bi):
        """Queue the upload of batch bi's staging buffer on the current stream -> the device tensor."""
        hb = self._hbufs[bi % N_STAGING]
        x = hb[0].to(self.device, non_blocking=True)
        hb[1] = torch.cuda.Event()
        hb[1].record(torch.cuda.current_stream(self.device))
        return x

    def _predict_plain(self, X, mine, conf_threshold, route):
        """predict() without slices for the images `mine` of this rank -> {index: prediction}."""
        results = {}
        B = self.batch_size
        batches = [mine[s:s + B] for s in range(0, len(mine), B)]

        def drain(idx, submitted):
            ticket, scales = submitted
            self.collect(ticket)
            for i, pr in zip(idx, self._collect(len(idx), scales, self._pipes[ticket].post)):
                results[i] = pr

        # Host side: JPEG decode + resize is the slow half of a real predict() (a few ms per image against ~50 us of device
        # time), so the images of the next batches are decoded by a pool while this batch runs.  Default: threads (PIL
        # releases the GIL for decode and resize; ~3x on 4+ cores, then GIL-bound) writing straight into rotating pinned
        # staging buffers that are uploaded asynchronously.  OD_DECODE_PROCS=N: N spawned worker PROCESSES (numpy + PIL
        # only, never the GPU) writing into one shared-memory staging block -- scales with the cores (measured 9.5 k
        # decodes/s on 16); opt-in because spawn re-imports the caller's __main__ (needs the usual __main__ guard).
        nprocs = int(os.environ.get("OD_DECODE_PROCS", "0"))
        own_pool = None
        if route == "device":  # pool threads read files and parse headers; the device decodes and resizes
            from .devdecode import prepare
            own_pool = pool = self._decode_threads()

            def start(bi):
                return [pool.submit(prepare, X[i], tuple(self.input_size), self.keep_aspect) for i in batches[bi]]

            def finish(bi, items):
                return self._submit_images(items, conf_threshold), [it[3] for it in items]
        elif nprocs > 0:
            nb = N_STAGING
            img_bytes = self.input_size[0] * self.input_size[1] * 3
            pool, shm = self._decode_procs(nprocs, nb * B * img_bytes)
            stage = np.ndarray((nb, B) + tuple(self.input_size) + (3,), np.uint8, buffer=shm.buf)

            class _Chunk:  # one future = 4 images; .result() of image j picks its scale out of the chunk's list
                def __init__(self, fut, j):
                    self.fut, self.j = fut, j

                def result(self):
                    return self.fut.result()[self.j]

            def start(bi):
                k = bi % nb  # free: its upload was synchronous
                idxs = batches[bi]
                out = []
                for c0 in range(0, len(idxs), 4):
                    part = idxs[c0:c0 + 4]
                    fut = pool.submit(decode_chunk_into_shm, shm.name, [(k * B + c0 + j) * img_bytes for j in range(len(part))],
                                      [X[i] for i in part], tuple(self.input_size), self.keep_aspect)
                    out += [_Chunk(fut, j) for j in range(len(part))]
                return out

            def finish(bi, scales):
                return self.submit(torch.from_numpy(stage[bi % nb]).to(self.device), conf_threshold, gather=True), scales
        else:
            own_pool = pool = self._decode_threads()

            def load_into(x, dst):  # worker thread: decode + resize, then the (slow, uncached) write into pinned memory
                img, sc = load_image(x, self.input_size, self.keep_aspect, True)
                np.copyto(dst, img)
                return sc

            def start(bi):
                host = self._stage(bi)
                return [pool.submit(load_into, X[i], host[j]) for j, i in enumerate(batches[bi])]

            def finish(bi, scales):
                return self.submit(self._upload_stage(bi), conf_threshold, gather=True), scales
        try:
            self._run_batches(batches, start, finish, drain)
        finally:
            if own_pool is not None:
                own_pool.shutdown(wait=True)
        return results

    # -- sliced inference -------------------------------------------------------------------------------------------
    def _submit_sliced(self, conf_threshold, x_u8=None, sizes=None, images=None, cut_only=False) -> int:
        """Queue one sliced batch (at most G = batch_size // T images) on the next pipeline's stream; -> its ticket.
        Host route: x_u8 uint8 [B,H,W,3] holds the tiles (row g*T + t = tile t of image g), sizes the images' (w, h).
        Device route: images = the uint8 [h,w,3] arrays; one upload, then od_tiles_resize writes the pipeline's Net.input.
        cut_only: the images are the ones the pipeline's decoder uploaded last (scripts/bench_slices.py)."""
        with self._next_pipeline() as (ticket, p):  # x_u8 was produced on the caller's stream
            if images is not None:
                if cut_only:
                    self._decoder(p).cut_tiles(p.net.input)
                else:
                    sizes = self._decoder(p).run_tiles(images, self.slices, p.net.input)
            p.slc.run(p.net, x_u8, sizes, conf_threshold)
        if x_u8 is not None:
            x_u8.record_stream(p.stream)
        return ticket

    def _predict_sliced(self, X, mine, conf_threshold, route):
        """predict() with slices for the images `mine` of this rank -> {index: prediction}: G = batch_size // T images per
        network batch.  Same shape as the plain route: pool threads prepare the next batches while this one runs, a
        pipeline's results are read before it is reused.  Host route: the threads crop and resize every tile with PIL into
        pinned staging.  Device route: the threads decode every image ONCE at its own size (files count as "fallback" in
        decode_stats -- the device JPEG decoder does not feed the tile cutter), the device cuts the tiles.  The pool is
        always threads (OD_DECODE_PROCS is for the plain route)."""
        grid = self.slices
        T = grid.T
        G = self.batch_size // T
        batches = [mine[s:s + G] for s in range(0, len(mine), G)]
        results = {}

        def drain(idx, ticket):
            p = self._pipes[ticket]
            p.done.synchronize()
            for i, (k, confs, bxs) in zip(idx, p.slc.detections_host(len(idx))):
                results[i] = ObjectsPrediction(k, confs, bxs, None)  # word 0 of a merged record is the class

        pool = self._decode_threads()
        if route == "device":
            def start(bi):
                return [pool.submit(slicing.load_native, X[i]) for i in batches[bi]]

            def finish(bi, items):
                ticket = self._submit_sliced(conf_threshold, images=[it[0] for it in items])
                for it in items:
                    self.decode_stats["fallback" if it[1] else "array"] += 1
                return ticket
        else:
            def load_into(x, dst):  # worker thread: decode, then crop + resize every tile into pinned memory
                return slicing.host_tiles(slicing.load_native(x)[0], grid, self.input_size, dst)

            def start(bi):
                host = self._stage(bi)
                return [pool.submit(load_into, X[i], host[j * T:(j + 1) * T]) for j, i in enumerate(batches[bi])]

            def finish(bi, sizes):
                return self._submit_sliced(conf_threshold, x_u8=self._upload_stage(bi), sizes=sizes)
        try:
            self._run_batches(batches, start, finish, drain)
        finally:
            pool.shutdown(wait=True)
        return results
