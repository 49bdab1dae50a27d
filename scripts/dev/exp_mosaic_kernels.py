"""usage: rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python scripts/dev/exp_mosaic_kernels.py B S TAG OUTDIR
then: python scripts/dev/kernel_trace_groups.py OUT 5 0 summary.json   (the first group of each kernel is the warm-up)
Workload for rocprofv3: the generator with and without mosaic, same images, same output size; 25 batches each, alternating
blocks of 5.  Prints the bytes each kernel needs (output + the source crop it reads) so that a parser can turn kernel time
into a share of HBM bandwidth."""
import json, sys, pathlib
ROOT = pathlib.Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "scripts"))
import numpy as np, torch
import _common
from object_detector_amd import od_gen

B, S, tag = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3]
OUT = pathlib.Path(sys.argv[4] if len(sys.argv) > 4 else "results")
X, y = _common.shapes_dataset(128, seed=0)
dev = torch.device("cuda:0")
gens = {}
for name, kw in (("plain", {}), ("mosaic", {"mosaic": 1.0, "ignore_regions": True})):
    g = od_gen.create_generator((S, S), device=dev, on_device=True, device_cache=True, **kw)
    gens[name] = g.flow(X, y, batch_size=B, data_augmentation=True, shuffle=True, seed=0)[0]
for name in gens:  # one epoch each: everything resident, code objects loaded
    for _ in range(128 // B + 1):
        next(gens[name])
torch.cuda.synchronize()
n = {"plain": 0, "mosaic": 0}
for rep in range(5):
    for name in ("plain", "mosaic"):
        for _ in range(5):
            next(gens[name]); n[name] += 1
        torch.cuda.synchronize()
src_bytes = float(np.mean([x.size for x in X]))
out_bytes = B * S * S * 3
rec = {"tag": tag, "B": B, "S": S, "batches": n, "warm_batches_each": 128 // B + 1, "out_bytes_per_batch": out_bytes,
       "mean_source_image_bytes": src_bytes,
       # bytes the algorithm needs per batch: every output byte written once + at most every source byte of the images shown read
       # once (plain: B images; mosaic: 4 B images, of which a tile shows a part) -- the upper bounds used for the roofline share
       "need_bytes_plain_max": out_bytes + B * src_bytes, "need_bytes_mosaic_max": out_bytes + 4 * B * src_bytes,
       "need_bytes_min": out_bytes}
OUT.mkdir(parents=True, exist_ok=True)
(OUT / f"mosaic_kernels_{tag}.json").write_text(json.dumps(rec, indent=1))
print(json.dumps(rec))
