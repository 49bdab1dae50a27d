"""usage: rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python scripts/dev/exp_assign_ign.py NC NFLAG TAG H W OUTDIR
then: python scripts/dev/kernel_trace_groups.py OUT 20 5 summary.json   (5 warm-up calls skipped, groups of 20 calls)
Workload for rocprofv3: od_assign_anchors vs od_assign_anchors_ign at B = 32, 12 boxes per image (P = 16800 at 320 x 320); NC and
the flagged boxes per image from argv; 5 repeats x 20 calls, alternating.  Same boxes for both; flags only differ."""
import json, sys, pathlib
ROOT = pathlib.Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))
import numpy as np, torch
from object_detector_amd.pb import ObjectsAnnotation, PriorBoxes

NC, NFLAG, tag = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3]
size = tuple(int(v) for v in sys.argv[4:6])
OUT = pathlib.Path(sys.argv[6] if len(sys.argv) > 6 else "results")
dev = torch.device("cuda:0")
rng = np.random.default_rng(0)
anns = []
for i in range(32):
    n = 12
    c = rng.uniform(0, 1, (n, 2)); wh = np.exp(rng.uniform(np.log(0.05), np.log(0.9), (n, 2)))
    b = np.clip(np.concatenate([c - wh / 2, c + wh / 2], 1), 0, 1).astype(np.float32)
    f = np.zeros(n, bool); f[:NFLAG] = True
    anns.append(ObjectsAnnotation(None, 1, 1, rng.integers(0, NC, n), b, f))
old = PriorBoxes(size, NC, device=dev)
new = PriorBoxes(size, NC, device=dev, ignore_regions=True)
print("P =", len(old))
for _ in range(5):
    old.encode_batch(anns, return_device=True); new.encode_batch(anns, return_device=True)
torch.cuda.synchronize()
for rep in range(6):
    for pb in (old, new):
        for _ in range(20):
            pb.encode_batch(anns, return_device=True)
        torch.cuda.synchronize()
OUT.mkdir(parents=True, exist_ok=True)
(OUT / f"assign_ign_{tag}.json").write_text(json.dumps({"tag": tag, "NC": NC, "flagged_per_image": NFLAG, "B": 32, "P": len(old), "G": 12, "repeats": 6, "calls_per_repeat": 20, "warm_calls": 5}))
