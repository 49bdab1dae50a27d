#!/usr/bin/env python3
"""Write N generated "shapes" images (_common.shapes_dataset) as a VOCdevkit-layout directory, so that voc_validate.py /
voc_evaluate.py / train.py can be run end to end without the (offline-unavailable) PASCAL VOC data."""
import argparse
import pathlib

import _common


def _main():
    p = argparse.ArgumentParser()
    p.add_argument("vocdevkit_dir", type=pathlib.Path)
    p.add_argument("-n", default=64, type=int)
    p.add_argument("--seed", default=1000, type=int)
    p.add_argument("--image-set", default="test")
    p.add_argument("--format", default="png", choices=("png", "jpg"))
    p.add_argument("--difficult", default=0.0, type=float, metavar="FRAC",
                   help="mark this share of the objects <difficult>1</difficult> (drawn half faded)")
    p.add_argument("--crowd", default=0.0, type=float, metavar="FRAC",
                   help="give this share of the images a cluster of small shapes under one loose box marked difficult")
    p.add_argument("--image-size", default=(240, 400), type=int, nargs=2, metavar=("LO", "HI"),
                   help="image sides are drawn from LO..HI pixels")
    p.add_argument("--object-scale", default=1.0, type=float,
                   help="multiply the objects' sides (0.15 .. 0.6 of the image) by this: small objects in large images")
    args = p.parse_args()
    X, y = _common.shapes_dataset(args.n, seed=args.seed, size_range=tuple(args.image_size), difficult_frac=args.difficult,
                                  crowd_frac=args.crowd, object_scale=args.object_scale)
    base = _common.write_voc_layout(args.vocdevkit_dir, X, y, image_set=args.image_set, fmt=args.format)
    print(f"{args.n} images -> {base}")


if __name__ == "__main__":
    _main()
