#!/usr/bin/env python3
"""Fingerprint of what the Python host layer makes the library do: per inference plan the op list (name, flops, bytes,
shape), the kernel of every op and sha256 of pred; per training configuration sha256 of losses / grads / params /
run_stats and of every f16 weight pack after one step.  Uses only attributes that older trees have too, so one copy of
this file fingerprints any checkout:

  host_fingerprint.py [--tree DIR] [--only infer|train] > a.json      (DIR: the checkout to import, default: this one)
  host_fingerprint.py --compare a.json b.json [--drop drop.json]      (exit 1 when a key outside drop.json differs)
  host_fingerprint.py --compare a.json b.json --write-drop drop.json  (two runs of ONE tree: record what is not repeatable)
"""
import argparse
import hashlib
import itertools
import json
import os
import pathlib
import sys


def sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def infer(out):
    import numpy as np
    import torch
    from object_detector_amd import weights as W
    from object_detector_amd.net import Net
    params = W.random_init(2)
    for (B, S), precision, fuse, overlapped in itertools.product(((2, 96), (1, 96), (3, 160)), ("f16", "mixed"), ("1", "0"),
                                                                 (False, True)):
        os.environ["OD_FUSE_BLOCKS"] = fuse
        x = torch.from_numpy(np.random.default_rng(7).integers(0, 256, (B, S, S, 3), dtype=np.uint8)).to("cuda:0")
        net = Net(params, B, (S, S), device="cuda:0", precision=precision, overlapped=overlapped)
        pred = net.forward(x)
        torch.cuda.synchronize()
        key = f"infer B{B} S{S} {precision} fuse{fuse} overlapped{int(overlapped)}"
        out[key + " ops"] = [[i["name"], i["flops"], i["bytes"], list(i["shape"])] for i in net.op_info]
        out[key + " n_ops"] = len(net.ops)
        out[key + " pred"] = sha(pred)
        out[key + " kernels"] = net.time_ops()[1]
        del net
    os.environ.pop("OD_FUSE_BLOCKS")


def train(out):
    import numpy as np
    import torch
    import bench
    from object_detector_amd import weights as W
    from object_detector_amd.trainer import Trainer
    B, S = 2, 96
    for box_mode, fuse_stats in (("smooth_l1", "0"), ("ciou", "0"), ("smooth_l1", "1")):
        os.environ["OD_TRAIN_FUSE_BN_STATS"] = fuse_stats
        rng = np.random.default_rng(1000)
        x = torch.from_numpy(rng.integers(0, 256, (B, S, S, 3), dtype=np.uint8)).to("cuda:0")
        anns = bench.bench_annotations(B, S, rng)
        tr = Trainer(W.random_init(2), B, (S, S), device="cuda:0", box_mode=box_mode)
        tr.step(x, anns)
        torch.cuda.synchronize()
        key = f"train {box_mode} fuse_bn_stats{fuse_stats}"
        for name in ("losses", "grads", "params", "run_stats"):
            out[f"{key} {name}"] = sha(getattr(tr, name))
        for kind, packs in (("wf", tr.wf), ("wb", tr.wb)):
            for layer, t in packs.items():
                out[f"{key} {kind} {layer}"] = sha(t)
        del tr
    os.environ.pop("OD_TRAIN_FUSE_BN_STATS")


def compare(a, b, drop, write_drop):
    fa, fb = (json.loads(pathlib.Path(p).read_text()) for p in (a, b))
    skip = set(json.loads(pathlib.Path(drop).read_text())) if drop else set()
    differ = sorted(k for k in set(fa) | set(fb) if fa.get(k) != fb.get(k))
    if write_drop:
        pathlib.Path(write_drop).write_text(json.dumps(differ, indent=1))
    bad = [k for k in differ if k not in skip]
    print(json.dumps({"keys": len(set(fa) | set(fb)), "dropped": sorted(skip), "differ": bad}, indent=1))
    return 1 if bad and not write_drop else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=str(pathlib.Path(__file__).resolve().parent.parent.parent))
    ap.add_argument("--only", choices=["infer", "train"])
    ap.add_argument("--compare", nargs=2, metavar="JSON")
    ap.add_argument("--drop")
    ap.add_argument("--write-drop")
    a = ap.parse_args()
    if a.compare:
        sys.exit(compare(*a.compare, a.drop, a.write_drop))
    sys.path.insert(0, str(pathlib.Path(a.tree).resolve()))
    out = {}
    if a.only != "train":
        infer(out)
    if a.only != "infer":
        train(out)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
