#!/usr/bin/env python3
# Adapted from ak110/object_detector check_generator.py (MIT): the same argparse flags and tk.* call sequence.
"""Visual check of the data generator / augmentation (equivalent of the reference's check_generator.py)."""
import argparse
import pathlib

import _common  # noqa: F401
import pytoolkit as tk


def _main():
    p = argparse.ArgumentParser()
    p.add_argument("--vocdevkit-dir", default=pathlib.Path("data/VOCdevkit"), type=pathlib.Path)
    p.add_argument("--save-dir", default=pathlib.Path("___generator_check"), type=pathlib.Path)
    p.add_argument("--synthetic", default=0, type=int)
    p.add_argument("--batches", default=32, type=int)
    p.add_argument("--mosaic", default=0.0, type=float, metavar="P",
                   help="probability of a four-image mosaic (composed on the GPU: needs one)")
    p.add_argument("--affine", default=None, type=float, nargs=4, metavar=("DEG", "TRANSLATE", "SCALE", "SHEAR"),
                   help="random affine warp (od_augment_warp on the GPU: needs one)")
    p.add_argument("--hsv", default=None, type=float, nargs=3, metavar=("H", "S", "V"), help="hue / saturation / value jitter")
    p.add_argument("--mixup", default=0.0, type=float, metavar="P", help="probability of a MixUp of two frames")
    p.add_argument("--mixup-beta", default=8.0, type=float, metavar="B")
    args = p.parse_args()
    warp = args.affine is not None or args.hsv is not None or args.mixup > 0
    if args.synthetic:
        X_val, y_val = _common.synthetic_dataset(1)
    else:
        X_val, y_val = tk.data.voc.load_07_test(args.vocdevkit_dir)
    if args.mosaic > 0 or args.mixup > 0:  # partners wanted: up to 16 images (4 synthetic ones) instead of the reference's one
        X_val, y_val = _common.synthetic_dataset(4) if args.synthetic else (X_val[:16], y_val[:16])
    else:
        X_val, y_val = X_val[:1], y_val[:1]
    kw = {"mosaic": args.mosaic, "device": "cuda:0", "ignore_regions": True} if args.mosaic > 0 or warp else {}
    if warp:
        kw.update(affine=None if args.affine is None else dict(zip(("degrees", "translate", "scale", "shear"), args.affine)),
                  hsv=None if args.hsv is None else tuple(args.hsv), mixup=args.mixup, mixup_beta=args.mixup_beta)
    gen = tk.dl.od.od_gen.create_generator((512, 512), preprocess_input=lambda x: x, encode_truth=None, **kw)
    g, _ = gen.flow(X_val, y_val, data_augmentation=True)
    for i, (X_batch, y_batch) in zip(tk.tqdm(range(args.batches)), g):
        for rgb, y in zip(X_batch, y_batch):
            ign = y.difficults & bool(kw)  # with ignore_regions: slivers a tile border or the warp left, difficult objects
            img = tk.ml.plot_objects(rgb, y.classes[~ign], None, y.bboxes[~ign], tk.data.voc.CLASS_NAMES)
            if ign.any():  # ... drawn in one grey
                img = tk.ml.plot_objects(img, None, None, y.bboxes[ign], ["ignored"], color=(160, 160, 160))
            tk.ndimage.save(args.save_dir / f"{i}.jpg", img)


if __name__ == "__main__":
    _main()
