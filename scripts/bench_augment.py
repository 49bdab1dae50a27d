#!/usr/bin/env python3
"""Kernel times of the generator's pixel launches on resident sources: od_augment_mosaic, and od_augment_warp at identity,
with affine + HSV, and with a MixUp of two mosaics (each with affine + HSV), at 32 x 320^2 and 16 x 640^2.

    python scripts/bench_augment.py [--out FILE]        -> one JSON line

Every output image is a four-image mosaic over 128 generated images that live on the device; parameters are drawn once from
a fixed seed, packed and uploaded before the clock starts, so a timed launch is the C entry alone.  Time: device events
around GROUP back-to-back launches on one stream, divided by GROUP; the figure reported is the median over REPEATS such
groups after WARMUP untimed launches (a single launch of a few tens of microseconds is too short for one pair of events).
Bytes: `bytes_min` is the output written once; `bytes_max` adds every byte of every distinct source image the batch shows,
read once, and the parameter block -- a gather reads only the crops it shows, and re-reads come from cache, so the truth
lies between.  `hbm_frac_*` = bytes / time over the 8.0 TB/s HBM3E peak of an MI355X.  The 128 sources (about 38 MB) fit
the 256 MB Infinity Cache, so after warm-up the reads need not come from HBM at all: the share is a roofline position, not
a measured HBM traffic."""
import argparse
import json
import pathlib
import sys

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "scripts"))

HBM_PEAK = 8.0e12
WARMUP, GROUP, REPEATS = 20, 20, 31


def _frames(rng, y, n, hw, od_gen):
    four = [int(j) for j in rng.integers(0, n, 4)]
    mp, _ann = od_gen.sample_mosaic(rng, [y[j] for j in four], hw, random_erasing=False)
    return four, mp


def _cases(B, hw, y, od_gen, seed=0):
    """-> {name: (per image the frames' source indices, list[WarpParams])}; "mosaic" and "warp_identity" share parameters."""
    rng = np.random.default_rng(seed)
    n = len(y)
    out = {"warp_identity": ([], []), "warp_affine_hsv": ([], []), "warp_mixup": ([], [])}
    for _ in range(B):
        fa, fb = _frames(rng, y, n, hw, od_gen), _frames(rng, y, n, hw, od_gen)
        inv = [od_gen.affine_inverse(od_gen.sample_affine(rng, hw, degrees=10, translate=0.1, scale=0.5, shear=2)) for _ in range(2)]
        col = [od_gen.sample_hsv(rng, (0.015, 0.7, 0.4)) for _ in range(2)]
        r = np.float32(rng.beta(8.0, 8.0))
        for name, wp in (("warp_identity", od_gen.WarpParams([fa[1]])),
                         ("warp_affine_hsv", od_gen.WarpParams([fa[1]], inv[:1], col[:1])),
                         ("warp_mixup", od_gen.WarpParams([fa[1], fb[1]], inv, col, (r, np.float32(1.0) - r)))):
            out[name][0].append([fa[0], fb[0]][:len(wp.frames)])
            out[name][1].append(wp)
    return out


def _main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, type=pathlib.Path, help="also write the JSON line to this file")
    args = ap.parse_args()
    import torch

    import _common
    from object_detector_amd import _lib, od_gen
    from object_detector_amd.net import Context, _stream_ptr
    if not torch.cuda.is_available():
        raise SystemExit("bench_augment.py measures on the GPU: none is visible")
    dev = torch.device("cuda:0")
    ctx = Context.get(dev)
    X, y = _common.shapes_dataset(128, seed=0)
    res = [torch.from_numpy(np.ascontiguousarray(x[..., :3], np.uint8)).to(dev) for x in X]
    rec = {"bench": "augment", "hbm_peak_bytes_per_s": HBM_PEAK, "warmup": WARMUP, "group": GROUP, "repeats": REPEATS,
           "sources": len(X), "source_bytes_total": int(sum(t.numel() for t in res)), "shapes": {}}
    for B, S in ((32, 320), (16, 640)):
        hw = (S, S)
        cases = _cases(B, hw, y, od_gen)
        out = torch.empty((B, S, S, 3), dtype=torch.uint8, device=dev)
        launches = {}
        keep = []
        for name, (fours, wps) in cases.items():
            arr, srcs = od_gen._pack_warp([[tuple(res[j] for j in four) for four in f] for f in fours], wps, hw)
            prm = torch.from_numpy(np.frombuffer(bytes(arr), np.uint8).copy()).to(dev)
            keep.append(prm)
            shown = {j for f in fours for four in f for j in four}
            launches[name] = (ctx.lib.od_augment_warp, srcs.base, prm, sum(res[j].numel() for j in shown) + prm.numel())
            if name == "warp_identity":  # the same mosaics through od_augment_mosaic
                marr = (_lib.MosaicParams * B)()
                msrc = od_gen._Sources([res[j] for f in fours for j in f[0]], "bench_augment")
                for i, (f, wp) in enumerate(zip(fours, wps)):
                    od_gen._fill_mosaic(marr[i], tuple(res[j] for j in f[0]), wp.frames[0], hw, i, msrc)
                mprm = torch.from_numpy(np.frombuffer(bytes(marr), np.uint8).copy()).to(dev)
                keep.append(mprm)
                launches["mosaic"] = (ctx.lib.od_augment_mosaic, msrc.base, mprm,
                                      sum(res[j].numel() for j in shown) + mprm.numel())
        shape = {}
        outs = {}
        for name in ("mosaic", "warp_identity", "warp_affine_hsv", "warp_mixup"):
            fn, base, prm, src_bytes = launches[name]

            def launch():
                _lib.check(fn(ctx.handle, base, prm.data_ptr(), out.data_ptr(), B, S, S, _stream_ptr()), name)
            for _ in range(WARMUP):
                launch()
            torch.cuda.synchronize()
            times = []
            for _ in range(REPEATS):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _k in range(GROUP):
                    launch()
                e1.record()
                e1.synchronize()
                times.append(e0.elapsed_time(e1) * 1e-3 / GROUP)
            outs[name] = out.clone()
            t = float(np.median(times))
            bmin, bmax = B * S * S * 3, B * S * S * 3 + src_bytes
            shape[name] = {"median_us": round(t * 1e6, 2), "min_us": round(min(times) * 1e6, 2),
                           "max_us": round(max(times) * 1e6, 2), "bytes_min": bmin, "bytes_max": bmax,
                           "hbm_frac_min": round(bmin / t / HBM_PEAK, 4), "hbm_frac_max": round(bmax / t / HBM_PEAK, 4)}
        assert torch.equal(outs["mosaic"], outs["warp_identity"]), "identity warp differs from od_augment_mosaic"
        rec["shapes"][f"{B}x{S}x{S}"] = shape
    line = json.dumps(rec)
    if args.out is not None:
        args.out.parent.mkdir(parents=True, exist_ok=True)
        args.out.write_text(line + "\n")
    print(line)


if __name__ == "__main__":
    _main()
