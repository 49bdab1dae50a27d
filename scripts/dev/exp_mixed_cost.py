"""Throughput cost of precision="mixed" at the BASELINE sizes, for several (stream_stages, split) choices: the network alone
(no post-processing), 3 or 1 batches in flight, one stream per in-flight plan.
usage: python scripts/dev/exp_mixed_cost.py [B] [S]"""
import pathlib
import sys
import time

ROOT = pathlib.Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))
import torch  # noqa: E402

from object_detector_amd import weights as W  # noqa: E402
from object_detector_amd.net import Net  # noqa: E402

B = int(sys.argv[1]) if len(sys.argv) > 1 else 32
S = int(sys.argv[2]) if len(sys.argv) > 2 else 320
dev = torch.device("cuda:0")
x = torch.randint(0, 256, (B, S, S, 3), dtype=torch.uint8, device=dev)
params = W.random_init(2)


def bench(nets, streams, steps=60, warm=15):
    def run(n):
        for i in range(n):
            with torch.cuda.stream(streams[i % len(nets)]):
                nets[i % len(nets)].forward(x)
        torch.cuda.synchronize()
    run(warm)
    t0 = time.perf_counter()
    run(steps)
    return (time.perf_counter() - t0) / steps * 1e3


plans = [("f16", None, None), ("mixed", (4, 5), ("n.lat4", "n.lat5", "n.out3", "n.out4", "h.t0", "h.out")),
         ("mixed", (3, 4, 5), ("n.out3", "n.out4", "h.t0", "h.out")), ("mixed", (3, 4, 5), ("h.t0", "h.out")),
         ("mixed", (3, 4, 5), ()), ("mixed", (4, 5), ("n.out3", "n.out4", "h.t0", "h.out")), ("mixed", (), ("n.out3", "n.out4", "h.t0", "h.out")),
         ("mixed", (3, 4, 5), ("n.lat3", "n.lat4", "n.lat5", "n.out3", "n.out4", "h.t0", "h.out"))]
for prec, st, sp in plans:
    for nin in (3, 1):
        nets = []
        for _ in range(nin):
            nets.append(Net(params, B, (S, S), device=dev, overlapped=nin > 1, precision=prec, stream_stages=st, split=sp,
                            share_weights_with=nets[0] if nets else None))
        ms = bench(nets, [torch.cuda.Stream(device=dev) for _ in nets])
        print(f"{prec:6s} stream {st} split {sp}: {nin} in flight {ms:.3f} ms/batch = {B / ms * 1e3:.0f} img/s", flush=True)
        del nets
        torch.cuda.empty_cache()
