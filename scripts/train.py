#!/usr/bin/env python3
"""Train the detector and write the weights file `voc_validate.py --weights` / `ObjectDetector.load_voc` read.

The reference trains through the unseen `fit` of tk.dl.od.ObjectDetector (generator -> encode_truth -> losses:
check_assign.py:21-22, docs/MODEL.md:33-52, per-layer learning rates docs/MODEL.md:84-90) and is accepted by the mAP that
voc_validate.py then logs (README.md:17,22).  This is that loop on MI355X: od_gen generator (pixels augmented on the
device) -> Trainer.step (every tensor op a libodhip.so kernel) -> weights.save.

Data: a VOCdevkit directory (--vocdevkit-dir, image set --image-set of VOC<year>), a COCO-format dataset (--coco-json +
--coco-image-dir: the network gets one class per category, and the class names travel in the weights' __meta__), or
--shapes N generated images (_common.shapes_dataset; VOC07+12 cannot be fetched offline).  Under torch.distributed.run every rank trains on its shard of
the images and the gradients are all-reduced through RCCL (od_allreduce)."""
import argparse
import json
import pathlib
import time

import numpy as np

import _common  # noqa: F401
import pytoolkit as tk


def build_parser():
    p = argparse.ArgumentParser()
    p.add_argument("--vocdevkit-dir", default=None, type=pathlib.Path)
    p.add_argument("--image-set", default="trainval")
    p.add_argument("--year", default=2007, type=int)
    p.add_argument("--shapes", default=0, type=int, help="N generated images instead of a VOC directory")
    p.add_argument("--coco-json", default=None, type=pathlib.Path,
                   help="COCO-format instances JSON instead of a VOC directory (with --coco-image-dir)")
    p.add_argument("--coco-image-dir", default=None, type=pathlib.Path, help="the images --coco-json names")
    p.add_argument("--result-dir", default=pathlib.Path("results"), type=pathlib.Path)
    p.add_argument("--out", default=None, type=pathlib.Path, help="weights file to write (default <result-dir>/trained.npz)")
    p.add_argument("--init", default=None, type=pathlib.Path, help="start from this weights file (e.g. an imported Darknet53)")
    p.add_argument("--input-size", default=(320, 320), type=int, nargs=2)
    p.add_argument("--batch-size", default=32, type=int, help="per rank")
    p.add_argument("--steps", default=600, type=int)
    p.add_argument("--lr", default=None, type=float,
                   help="peak learning rate (default 0.02 x global batch / 32: the linear scaling rule; 0.005 x global batch / 32 "
                        "with --assigner tal)")
    p.add_argument("--warmup", default=None, type=int,
                   help="linear warm-up steps (default 50 at a global batch of 32, 200 below it: measured -- 16 x 640^2 from "
                        "scratch diverges with 50 warm-up steps at lr 0.01-0.02 and trains with 200-300)")
    p.add_argument("--momentum", default=0.9, type=float)
    p.add_argument("--weight-decay", default=1e-4, type=float)
    p.add_argument("--from-scratch", action="store_true",
                   help="base network at the full learning rate instead of docs/MODEL.md:84-90's 1/100 (no pre-trained "
                        "Darknet53 is available offline)")
    p.add_argument("--box-loss", default="smooth_l1", choices=("smooth_l1", "mse", "giou", "diou", "ciou"),
                   help="bounding-box loss: smooth-L1 (north_star), the mean squared error docs/MODEL.md:46-52 describes, or "
                        "1 - GIoU / DIoU / CIoU of the decoded boxes")
    p.add_argument("--box-weight", default=1.0, type=float, metavar="W", help="weight of the box loss in the total")
    p.add_argument("--fit-priors", action="store_true",
                   help="prior-box sizes from KMeans over the training boxes in grid-cell units (docs/MODEL.md:29-31) instead of "
                        "the frozen default table; they travel with the weights file")
    p.add_argument("--seed", default=0, type=int)
    p.add_argument("--log-every", default=50, type=int)
    p.add_argument("--no-device-cache", action="store_true",
                   help="decode and upload every image every epoch instead of keeping the decoded dataset in HBM")
    p.add_argument("--mosaic", default=0.0, type=float, metavar="P",
                   help="probability that a training image is a mosaic of four (od_augment_mosaic; off by default)")
    p.add_argument("--affine", default=None, type=float, nargs=4, metavar=("DEG", "TRANSLATE", "SCALE", "SHEAR"),
                   help="random affine warp of every training frame (od_augment_warp): rotation and shear in degrees, "
                        "translation as a share of the frame, zoom in 1 +- SCALE; off by default")
    p.add_argument("--hsv", default=None, type=float, nargs=3, metavar=("H", "S", "V"),
                   help="hue (turns) / saturation / value jitter half-widths, e.g. 0.015 0.7 0.4; off by default")
    p.add_argument("--mixup", default=0.0, type=float, metavar="P",
                   help="probability that a training image is a MixUp of two frames; off by default")
    p.add_argument("--mixup-beta", default=8.0, type=float, metavar="B", help="--mixup: the ratio is Beta(B, B)")
    p.add_argument("--ignore-regions", action="store_true",
                   help="difficult / iscrowd boxes and the slivers a mosaic leaves are ignore regions instead of positives")
    p.add_argument("--assigner", default="max-iou", choices=("max-iou", "atss", "tal"),
                   help="the rule that gives priors to objects: fixed IoU thresholds (0.5 / 0.4) with a forced best match; "
                        "ATSS: the priors nearest to the object's centre on every level, IoU threshold = their mean + std; "
                        "or TAL: the priors whose predicted score and predicted box agree best on the object (assigned behind "
                        "the forward pass of every step)")
    p.add_argument("--atss-topk", default=9, type=int, metavar="K", help="--assigner atss: nearest cells per level (1..32)")
    p.add_argument("--tal-topk", default=13, type=int, metavar="K", help="--assigner tal: positives per object (1..32)")
    p.add_argument("--tal-alpha", default=1.0, type=float, metavar="A", help="--assigner tal: exponent of the score")
    p.add_argument("--tal-beta", default=6.0, type=float, metavar="B", help="--assigner tal: exponent of the predicted box's IoU")
    p.add_argument("--objectness", default="focal", choices=("focal", "qfl", "vfl"),
                   help="objectness term: focal loss on hard targets, or quality focal / varifocal loss towards the quality "
                        "targets of --quality (od_loss_fwd_bwd_quality)")
    p.add_argument("--quality", default="iou", choices=("iou", "tal"),
                   help="--objectness qfl | vfl: the target of an assigned prior: IoU of its predicted box with its object, or "
                        "TOOD's normalised alignment metric (needs --assigner tal)")
    p.add_argument("--shapes-difficult", default=0.0, type=float, help="--shapes: share of objects marked difficult")
    p.add_argument("--shapes-crowd", default=0.0, type=float, help="--shapes: share of images with a crowd region")
    p.add_argument("--prefetch", default=2, type=int, help="batches the generator thread runs ahead (0 = in the training thread)")
    p.add_argument("--ema", default=None, type=float, metavar="D",
                   help="keep an exponential moving average of the weights with decay D (0 < D < 1, warmed up from 0.1) and "
                        "write it to <out stem>_ema.npz beside the usual file")
    p.add_argument("--optimizer", default="sgd", choices=("sgd", "nesterov", "adamw"),
                   help="update rule: momentum SGD, Nesterov momentum (both with --momentum), or AdamW with decoupled "
                        "--weight-decay (--beta1 / --beta2 / --adam-eps; default --lr 0.001 at batch 32)")
    p.add_argument("--beta1", default=0.9, type=float, help="--optimizer adamw: decay of the first moment, in [0, 1)")
    p.add_argument("--beta2", default=0.999, type=float, help="--optimizer adamw: decay of the second moment, in [0, 1)")
    p.add_argument("--adam-eps", default=1e-8, type=float, help="--optimizer adamw: added to the root of the second moment")
    p.add_argument("--clip-norm", default=None, type=float, metavar="X",
                   help="scale a step's gradients down so that their global norm is at most X (computed on the device, "
                        "the same on every rank); the log lines then show the unclipped norm")
    p.add_argument("--save-state-every", default=0, type=int, metavar="N",
                   help="every N steps rank 0 writes <result-dir>/state.npz (masters, momentum, BatchNorm statistics, the "
                        "average, loss scale, step) for --resume")
    p.add_argument("--resume", default=None, type=pathlib.Path, metavar="FILE",
                   help="continue from a state file at the step it recorded, up to --steps in total.  The generator is "
                        "seeded from (seed, rank, that step), so the batches that follow are NOT those an uninterrupted run "
                        "would have drawn")
    p.add_argument("--val-every", default=0, type=int, metavar="N",
                   help="validate every N steps during the run: a detector refreshed on the GPU from the live weights (the "
                        "average under --ema) predicts the validation images, the mAP is logged (needs --val-shapes or --val-set)")
    p.add_argument("--val-shapes", default=0, type=int, metavar="M",
                   help="--val-every: M generated images, drawn with another seed than the --shapes training set")
    p.add_argument("--val-set", default=None, metavar="SET",
                   help="--val-every: this image set of the VOC directory (e.g. test, val)")
    p.add_argument("--val-batch-size", default=None, type=int, help="batch size of the validation detector (default --batch-size)")
    p.add_argument("--val-coco", action="store_true", help="--val-every: also log the twelve COCO AP / AR numbers")
    p.add_argument("--keep-best", action="store_true",
                   help="--val-every: write the weights of the best validation so far (by VOC mAP) to <result-dir>/best.npz")
    # the validation detector's options (absent = off, as in the evaluation scripts)
    _common.add_tta_arguments(p)
    _common.add_nms_arguments(p)
    _common.add_slice_arguments(p)
    return p


def check_validation_args(args):
    """--val-every needs validation data; said right after parsing, before any data is read or a trainer built."""
    if args.val_every > 0 and not args.val_shapes and (args.val_set is None or args.vocdevkit_dir is None):
        raise SystemExit("--val-every needs validation data: --val-shapes M, or --val-set SET with --vocdevkit-dir")


def make_validator(args, tr, class_names=None):
    """--val-every: the Validator of the run (held-out data, a detector built once from the trainer), or None.  Under
    --resume an existing <result-dir>/best.npz keeps its place until a validation scores above the value it recorded."""
    if args.val_every <= 0:
        return None
    from object_detector_amd.detector import ObjectDetector
    from object_detector_amd.validate import Validator
    if args.val_shapes:
        Xv, yv = _common.shapes_dataset(args.val_shapes, seed=args.seed + 1000)  # held out: another seed
    else:
        Xv, yv = tk.data.voc.load_set(args.vocdevkit_dir, args.year, args.val_set)
    od = ObjectDetector.from_trainer(tr, batch_size=args.val_batch_size, **_common.detector_options(args))
    v = Validator(od, Xv, yv, coco=args.val_coco, class_names=class_names,
                  keep_best=args.result_dir / "best.npz" if args.keep_best else None)
    if args.resume is not None and v.resume_best():
        tk.log.get(__name__).info(f"{v.keep_best}: {v.metric} {v.best_value:.4f} of step {v.best_step} stays the best so far")
    return v


def _main():
    tk.better_exceptions()
    args = build_parser().parse_args()
    check_validation_args(args)
    with tk.dl.session():
        tk.log.init(args.result_dir / "train.log")
        _run(args)


def init_for_training(params, prior=0.01):
    """Prediction-conv bias so that every prior starts at objectness `prior` (the focal-loss initialisation of the RetinaNet
    paper docs/MODEL.md:37 cites): logit(not-obj) - logit(obj) = log((1 - prior) / prior); class and box biases zero."""
    from object_detector_amd import weights as W
    params = dict(params)
    nc, _, _ = W.infer_arch(params)
    b = np.zeros((W.NUM_PRIORS, nc + 6), np.float32)
    half = 0.5 * np.log((1.0 - prior) / prior)
    b[:, 0], b[:, 1] = half, -half
    params["h.out.bias"] = b.reshape(-1)
    return params


def cosine_schedule(lr, steps, warmup):
    def f(i):
        if i < warmup:
            return lr * (i + 1) / warmup
        return lr * 0.5 * (1.0 + np.cos(np.pi * (i - warmup) / max(1, steps - warmup)))
    return f


@tk.log.trace()
def _run(args):
    import torch
    from object_detector_amd import od_gen, weights as W
    from object_detector_amd.net import Context
    from object_detector_amd.trainer import LR_MULTIPLIERS, Trainer, init_comm
    log = tk.log.get(__name__)
    rank, _local, world = tk.dl.dist_env()
    if args.lr is None:
        # "tal" assigns from the predictions, and its from-scratch run diverges at the rate the static assigners take; it
        # trains at a quarter of it (DESIGN.md "Task-aligned assignment")
        # AdamW's step is the gradient's sign at first, not its size: 1e-3 at batch 32 (DESIGN.md "Optimizers and gradient
        # clipping")
        base = 0.001 if args.optimizer == "adamw" else (0.005 if args.assigner == "tal" else 0.02)
        args.lr = base * args.batch_size * world / 32.0
    if args.warmup is None:
        args.warmup = 50 if args.batch_size * world >= 32 else 200
    class_names = None
    if args.shapes:
        X, y = _common.shapes_dataset(args.shapes, seed=args.seed, difficult_frac=args.shapes_difficult,
                                      crowd_frac=args.shapes_crowd)
    elif args.coco_json is not None:
        if args.coco_image_dir is None:
            raise SystemExit("--coco-json needs --coco-image-dir")
        X, y, class_names = tk.data.coco.load_od(args.coco_json, args.coco_image_dir)
    else:
        X, y = tk.data.voc.load_set(args.vocdevkit_dir, args.year, args.image_set)
    y_all = y
    X, y = X[rank::world], y[rank::world]  # data-parallel: images sharded by index, no collective on the data path
    n = len(X) // args.batch_size * args.batch_size
    if n == 0:
        raise SystemExit(f"rank {rank}: {len(X)} images < one batch of {args.batch_size}")
    X, y = X[:n], y[:n]
    dev = torch.device("cuda", torch.cuda.current_device())
    if args.init is not None:
        params, _meta = W.load(args.init)
    else:
        nc = 20 if class_names is None else len(class_names)
        params = init_for_training(W.random_init(seed=2 + args.seed, num_classes=nc))
    comm = None
    if world > 1 and torch.distributed.get_backend() == "nccl":
        comm, _ = init_comm(Context.get(dev))
    mult = {k: v for k, v in LR_MULTIPLIERS.items() if not (args.from_scratch and k == "b.")}
    prior_wh = None
    if args.fit_priors:  # from ALL ranks' boxes: every rank must assign against the same priors
        from object_detector_amd import priors as PR
        prior_wh = PR.fit(np.concatenate([a.bboxes for a in y_all if a.num_objects]), tuple(args.input_size), seed=args.seed)
        log.info(f"fitted prior sizes (grid-cell units), level 0: {np.round(prior_wh[0], 2).tolist()}")
    tr = Trainer(params, args.batch_size, tuple(args.input_size), device=dev, lr=args.lr, momentum=args.momentum,
                 weight_decay=args.weight_decay, comm=comm, world_size=world, lr_multipliers=mult, prior_wh=prior_wh, box_mode=args.box_loss,
                 ignore_regions=args.ignore_regions, loss_weights=(1.0, 1.0, args.box_weight), assigner=args.assigner,
                 atss_topk=args.atss_topk, tal_topk=args.tal_topk, tal_alpha=args.tal_alpha, tal_beta=args.tal_beta,
                 objectness=args.objectness, quality=args.quality, optimizer=args.optimizer,
                 betas=(args.beta1, args.beta2), adam_eps=args.adam_eps, clip_grad_norm=args.clip_norm,
                 **({} if args.ema is None else {"ema_decay": args.ema}))
    start, flow_seed = 0, args.seed + rank
    if args.resume is not None:
        sd = W.load_state(args.resume)
        try:
            tr.load_state_dict(sd)
        except ValueError as e:  # another architecture, another EMA switch, another optimizer: the trainer's own message
            raise SystemExit(f"--resume {args.resume}: {e}") from None
        start = int(sd["step"])
        if start >= args.steps:
            raise SystemExit(f"{args.resume} is at step {start}: nothing left of --steps {args.steps}")
        flow_seed = int(np.random.SeedSequence([args.seed, rank, start]).generate_state(1)[0] >> 1)
        log.info(f"resumed from {args.resume}: starting at step {start}, loss scale {tr.loss_scale:g}, "
                 f"ema_updates {tr.ema_updates}")
    validator = make_validator(args, tr, class_names)
    val_kw = {} if validator is None else {"validate_every": args.val_every, "validator": validator}
    positives = {"sum": torch.zeros((), dtype=torch.int64, device=dev), "images": 0}

    def encode_truth(anns):  # tr.pb.encode_truth_device, and the positives it made are counted (on the device: no sync)
        anns = list(anns)
        target, npos, _assigned = tr.pb.encode_batch(anns, return_device=True)
        positives["sum"] += npos.sum()
        positives["images"] += len(anns)
        return target
    # "tal" assigns from the predictions: the generator yields the annotation lists themselves (encode_truth=None) and
    # Trainer.step encodes behind its forward pass; the positives are then counted from tr.last_npos
    tal = args.assigner == "tal"
    gen =od_gen.create_generator(tuple(args.input_size), preprocess_input=None, encode_truth=None if tal else encode_truth,
                                  device=dev, on_device=True, device_cache=not args.no_device_cache, mosaic=args.mosaic,
                                  ignore_regions=args.ignore_regions,
                                  affine=None if args.affine is None else dict(zip(("degrees", "translate", "scale", "shear"),
                                                                                   args.affine)),
                                  hsv=None if args.hsv is None else tuple(args.hsv), mixup=args.mixup,
                                  mixup_beta=args.mixup_beta)
    batches, per_epoch = gen.flow(X, y, batch_size=args.batch_size, data_augmentation=True, shuffle=True, seed=flow_seed,
                                  prefetch=args.prefetch)
    log.info(f"{n} images on rank {rank} of {world}, {per_epoch} steps per epoch, {args.steps} steps, lr {args.lr}, "
             f"multipliers {mult}")
    pending = []  # "tal": batch sizes of issued steps whose tr.last_npos is not counted yet (at most one)

    def count_last_step():
        if pending and tr.last_npos is not None:
            positives["sum"] += tr.last_npos.sum()
            positives["images"] += pending.pop()

    def counted(it):  # fit() asks for the next batch when the step on the last one has been issued
        for xb, anns in it:
            count_last_step()
            pending.append(len(anns))
            yield xb, anns
    feed = counted(batches) if tal else batches
    t0 = time.perf_counter()
    schedule = cosine_schedule(args.lr, args.steps, args.warmup)
    hists, done = [], start
    while done < args.steps:  # one fit() for the whole run, or one per --save-state-every steps
        k = args.steps - done if args.save_state_every <= 0 else min(args.save_state_every, args.steps - done)
        hists.append(tr.fit(feed, k, lr_schedule=schedule, log_every=args.log_every, log=log.info, start_step=done,
                            **val_kw))
        count_last_step()
        done += k
        if args.save_state_every > 0 and tk.dl.is_main_process():
            state = args.result_dir / "state.npz"
            tmp = state.with_name("state.npz.tmp")
            W.save_state(tmp, dict(tr.state_dict(), step=done))
            tmp.replace(state)  # a run killed while writing leaves the previous state file whole
            log.info(f"state of step {done} written to {state}")
    tr._poll_nonfinite(wait=True)  # the run is over: apply the flags of its last steps (fit() and state_dict() leave them pending)
    hist = np.concatenate(hists)
    ran = args.steps - start
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    if args.mosaic > 0 or gen.warp:
        log.info(f"mosaic: {json.dumps(gen.stats)}")
    batches.close()  # ends the generator's prefetch thread (a thread still issuing GPU work at interpreter exit aborts)
    k = max(1, min(20, ran // 10))
    log.info(f"loss first {k} steps {hist[:k, 3].mean():.4f} -> last {k} steps {hist[-k:, 3].mean():.4f}; "
             f"{ran} steps in {dt:.1f} s ({ran * args.batch_size * world / dt:.0f} images/s), "
             f"skipped {tr.skipped_steps}, loss scale {tr.loss_scale:g}")
    torch.cuda.synchronize()  # the generator's thread counted on its own stream
    log.info(f"assigner {tr.pb.assigner}: {int(positives['sum']) / max(1, positives['images']):.2f} positive priors per image "
             f"over {positives['images']} encoded images")
    if tr.ema_decay is not None:
        log.info(f"weight average: decay {tr.ema_decay:g}, ema_updates {tr.ema_updates}")
    if validator is not None and validator.history:
        log.info(f"validation: best {validator.metric} {validator.best_value:.4f} at step {validator.best_step} of "
                 f"{len(validator.history)} validations"
                 + (f", weights in {validator.keep_best}" if validator.keep_best is not None else ""))
    if tk.dl.is_main_process():
        out = args.out or (args.result_dir / "trained.npz")
        out.parent.mkdir(parents=True, exist_ok=True)
        meta = {"prior_wh": np.asarray(tr.pb.prior_wh), "loss_history": hist[:, 3]}
        if class_names is not None:
            meta["class_names"] = np.asarray(class_names)
        if tr.ema_decay is not None:
            meta["ema_decay"] = np.float64(tr.ema_decay)
        W.save(out, tr.export_params(), meta=meta)
        log.info(f"weights written to {out}")
        if tr.ema_decay is not None:
            out_ema = out.with_name(out.stem + "_ema.npz")
            W.save(out_ema, tr.export_params(ema=True), meta=meta)
            log.info(f"weight average written to {out_ema}")


if __name__ == "__main__":
    _main()
