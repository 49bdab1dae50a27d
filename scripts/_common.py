"""Shared bits of the four entry-point scripts: repo root on sys.path, synthetic VOC-shaped data when there is no VOC."""
import pathlib
import sys

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))


def synthetic_dataset(n, size=(375, 500), seed=1):
    """VOC-shaped synthetic images + annotations (SURVEY.md §8d recipe): uint8 arrays, 1..10 boxes per image."""
    from object_detector_amd.pb import ObjectsAnnotation
    rng = np.random.default_rng(seed)
    X, y = [], []
    for _ in range(n):
        X.append(rng.integers(0, 256, size + (3,), dtype=np.uint8))
        k = int(np.clip(1 + rng.poisson(1.5), 1, 10))
        c = rng.uniform(0, 1, (k, 2))
        wh = np.exp(rng.uniform(np.log(0.05), np.log(0.9), (k, 2)))
        b = np.clip(np.concatenate([c - wh / 2, c + wh / 2], 1), 0, 1).astype(np.float32)
        y.append(ObjectsAnnotation(None, size[1], size[0], rng.integers(0, 20, k), b))
    return np.array(X, dtype=object), np.array(y, dtype=object)


def add_tta_arguments(p):
    """--tta [flip] / --vote-iou X of the evaluation scripts (ObjectDetector(tta=..., tta_vote_iou=...))."""
    p.add_argument("--tta", default=None, nargs="*", metavar="VIEW",
                   help="test-time augmentation: `--tta flip` merges the mirrored view on the GPU; `--tta` alone runs the "
                        "identity view with box voting only; absent = off")
    p.add_argument("--vote-iou", default=0.5, type=float, help="box-voting overlap under --tta (<= 0: no voting)")


def add_nms_arguments(p):
    """--nms METHOD / --soft-sigma S / --soft-min-conf C of the evaluation scripts (ObjectDetector(nms=..., ...))."""
    p.add_argument("--nms", default="hard", choices=("hard", "soft-linear", "soft-gaussian"),
                   help="suppression stage: greedy NMS, or Soft-NMS with linear / Gaussian score decay on the GPU")
    p.add_argument("--soft-sigma", default=0.5, type=float, help="sigma of --nms soft-gaussian")
    p.add_argument("--soft-min-conf", default=None, type=float,
                   help="under Soft-NMS a detection whose decayed score is not above this is dropped (default: the "
                        "confidence threshold of the run)")


def add_slice_arguments(p):
    """--slices NY NX [--slice-overlap F] [--no-slice-full-view] of the evaluation scripts (ObjectDetector(slices=...))."""
    p.add_argument("--slices", default=None, type=int, nargs=2, metavar=("NY", "NX"),
                   help="sliced inference: every image is cut into NY x NX overlapping tiles (+ the whole image), each tile "
                        "is one row of the network batch, the tiles' detections are merged on the GPU; absent = off")
    p.add_argument("--slice-overlap", default=0.2, type=float, help="overlap of neighbouring tiles under --slices, 0 .. 0.5")
    p.add_argument("--no-slice-full-view", action="store_true",
                   help="under --slices: leave the whole-image tile out (objects larger than the overlap can then be lost)")


def detector_options(args):
    """The ObjectDetector keywords of --tta / --nms / --slices (add_*_arguments above); an absent option adds nothing."""
    kw = {}
    if getattr(args, "tta", None) is not None:
        kw["tta"], kw["tta_vote_iou"] = tuple(args.tta), args.vote_iou
    if getattr(args, "slices", None) is not None:
        kw["slices"], kw["slice_overlap"] = tuple(args.slices), args.slice_overlap
        kw["slice_full_view"] = not args.no_slice_full_view
    if getattr(args, "nms", "hard") != "hard":
        kw["nms"], kw["soft_sigma"], kw["soft_min_conf"] = args.nms, args.soft_sigma, args.soft_min_conf
    return kw


def make_detector(tk, args, batch_size, input_size=(320, 320), device_decode=False, **kw):
    """device_decode: JPEG decode and resize of predict()'s inputs on the GPU (image_decode="device")."""
    OD = tk.dl.od.ObjectDetector
    kw["image_decode"] = "device" if device_decode else "host"
    kw.update(detector_options(args))
    if args.synthetic:
        return OD.synthetic(batch_size, input_size, **kw)
    return OD.load_voc(batch_size=batch_size, input_size=input_size, weights=args.weights, **kw)


# ---- "shapes": a learnable VOC-shaped detection task that needs no dataset ------------------------------------------
# VOC07+12 cannot be fetched offline, so the train -> export -> voc_validate loop the reference is accepted by
# (README.md:17,22; voc_validate.py:24-31) is closed on generated images instead: 1..3 colour-coded, lightly textured
# rectangles (one fixed colour per class, five VOC class ids) on a smooth random background, VOC-like image sizes.
SHAPE_CLASSES = (1, 6, 7, 11, 14)  # bicycle, car, cat, dog, person
SHAPE_COLOURS = ((220, 40, 40), (40, 200, 60), (50, 80, 230), (230, 210, 40), (200, 60, 210))


def shapes_dataset(n, seed=0, size_range=(240, 400), difficult_frac=0.0, crowd_frac=0.0, object_scale=1.0):
    """-> (X: object array of uint8 [h,w,3] images, y: object array of ObjectsAnnotation).
    size_range: image sides in pixels; object_scale: the objects' sides (0.15 .. 0.6 of the image) are multiplied by it --
    large images with small objects are the test set of sliced inference.  The defaults draw what they always drew.
    difficult_frac: this share of the objects is marked `difficult` and drawn half faded into the background (VOC's hard
    objects); crowd_frac: this share of the images gets a "crowd" -- a cluster of 6-12 small shapes of one class under ONE
    loose box marked difficult, the way COCO annotates iscrowd regions.  Both are drawn from a generator of their own: the
    images and boxes of the default call do not depend on them."""
    from scipy.ndimage import uniform_filter
    from object_detector_amd.pb import ObjectsAnnotation
    rng = np.random.default_rng(seed)
    marks = np.random.default_rng([int(seed), 0x1646]) if (difficult_frac > 0 or crowd_frac > 0) else None
    X, y = [], []
    for _ in range(n):
        h, w = (int(v) for v in rng.integers(size_range[0], size_range[1] + 1, 2))
        gh, gw = h // 32 + 2, w // 32 + 2  # greyish blocks with a mild tint: never as saturated as a class colour
        low = (rng.uniform(70, 180, (gh, gw, 1)) + rng.normal(0, 14, (gh, gw, 3))).astype(np.float32)
        bg = np.repeat(np.repeat(low, 32, 0), 32, 1)[:h, :w]
        bg = uniform_filter(bg, size=(9, 9, 1), mode="nearest")  # smooth blocks: no hard edges in the background
        img = bg + 6.0 * rng.standard_normal((h, w, 3), dtype=np.float32)
        boxes, classes = [], []
        for _obj in range(int(rng.integers(1, 4))):
            for _try in range(20):
                bw, bh = rng.uniform(0.15, 0.6, 2) * object_scale
                x1, y1 = rng.uniform(0.02, 0.98 - bw), rng.uniform(0.02, 0.98 - bh)
                b = np.array([x1, y1, x1 + bw, y1 + bh])
                if all(_iou(b, o) < 0.15 for o in boxes):
                    break
            else:
                continue
            ci = int(rng.integers(0, len(SHAPE_CLASSES)))
            px = (int(round(b[0] * w)), int(round(b[1] * h)), int(round(b[2] * w)), int(round(b[3] * h)))
            col = np.asarray(SHAPE_COLOURS[ci], np.float64) * rng.uniform(0.85, 1.0)
            img[px[1]:px[3], px[0]:px[2]] = col + 10.0 * rng.standard_normal((px[3] - px[1], px[2] - px[0], 3), dtype=np.float32)
            boxes.append(np.array([px[0] / w, px[1] / h, px[2] / w, px[3] / h]))
            classes.append(SHAPE_CLASSES[ci])
        difficults = [False] * len(boxes)
        if marks is not None:
            for k, b in enumerate(boxes):
                if marks.random() < difficult_frac:
                    px = (int(round(b[0] * w)), int(round(b[1] * h)), int(round(b[2] * w)), int(round(b[3] * h)))
                    reg = (slice(px[1], px[3]), slice(px[0], px[2]))
                    img[reg] = 0.5 * img[reg] + 0.5 * bg[reg]
                    difficults[k] = True
            if marks.random() < crowd_frac:
                for _try in range(20):
                    bw, bh = marks.uniform(0.25, 0.45, 2)
                    x1, y1 = marks.uniform(0.02, 0.98 - bw), marks.uniform(0.02, 0.98 - bh)
                    b = np.array([x1, y1, x1 + bw, y1 + bh])
                    if all(_iou(b, o) < 0.05 for o in boxes):
                        break
                else:
                    b = None
                if b is not None:
                    ci = int(marks.integers(0, len(SHAPE_CLASSES)))
                    for _k in range(int(marks.integers(6, 13))):
                        sw, sh = marks.uniform(0.04, 0.08, 2)
                        sx, sy = marks.uniform(b[0], b[2] - sw), marks.uniform(b[1], b[3] - sh)
                        px = (int(round(sx * w)), int(round(sy * h)), int(round((sx + sw) * w)), int(round((sy + sh) * h)))
                        img[px[1]:px[3], px[0]:px[2]] = np.asarray(SHAPE_COLOURS[ci], np.float64) * marks.uniform(0.85, 1.0)
                    boxes.append(b)
                    classes.append(SHAPE_CLASSES[ci])
                    difficults.append(True)
        X.append(np.clip(np.rint(img), 0, 255).astype(np.uint8))
        y.append(ObjectsAnnotation(None, w, h, classes, np.asarray(boxes, np.float32), difficults))
    Xa = np.empty(n, dtype=object)
    Xa[:] = X
    return Xa, np.array(y, dtype=object)


def _iou(a, b):
    iw = max(0.0, min(a[2], b[2]) - max(a[0], b[0]))
    ih = max(0.0, min(a[3], b[3]) - max(a[1], b[1]))
    inter = iw * ih
    return inter / ((a[2] - a[0]) * (a[3] - a[1]) + (b[2] - b[0]) * (b[3] - b[1]) - inter)


def write_voc_layout(vocdevkit_dir, X, y, image_set="test", year=2007, fmt="png"):
    """Write images + annotations as a VOCdevkit directory (JPEGImages / Annotations / ImageSets/Main/<set>.txt) that
    tk.data.voc.load_07_test / load_set read back.  fmt="png" keeps the pixels exact (the files still sit in JPEGImages)."""
    from PIL import Image
    from object_detector_amd.tk.data.voc import CLASS_NAMES
    base = pathlib.Path(vocdevkit_dir) / f"VOC{year}"
    for d in ("Annotations", "JPEGImages", "ImageSets/Main"):
        (base / d).mkdir(parents=True, exist_ok=True)
    ids = []
    for i, (img, a) in enumerate(zip(X, y)):
        name = f"{i:06d}"
        ids.append(name)
        h, w = img.shape[:2]
        Image.fromarray(img).save(base / "JPEGImages" / f"{name}.{fmt}", **({"quality": 95} if fmt == "jpg" else {}))
        objs = ""
        for c, b, d in zip(a.classes, a.bboxes, a.difficults):  # VOC pixels are 1-based inclusive (load_annotation undoes this)
            objs += (f"<object><name>{CLASS_NAMES[int(c)]}</name><difficult>{int(d)}</difficult><bndbox>"
                     f"<xmin>{int(round(b[0] * w)) + 1}</xmin><ymin>{int(round(b[1] * h)) + 1}</ymin>"
                     f"<xmax>{int(round(b[2] * w))}</xmax><ymax>{int(round(b[3] * h))}</ymax></bndbox></object>\n")
        (base / "Annotations" / f"{name}.xml").write_text(
            f"<annotation><filename>{name}.{fmt}</filename><size><width>{w}</width><height>{h}</height><depth>3</depth>"
            f"</size>\n{objs}</annotation>")
    (base / "ImageSets" / "Main" / f"{image_set}.txt").write_text("\n".join(ids))
    return base
