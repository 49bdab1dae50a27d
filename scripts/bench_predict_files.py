#!/usr/bin/env python3
"""End-to-end predict() on image FILES (JPEG decode + resize on the host, upload, network, NMS, results to host):
synthetic VOC-sized JPEGs.  usage: bench_predict_files.py [--n 512] [--threads 1,4,16] [--decode host,device]
--decode device runs predict(..., image_decode="device") with the default thread pool in the same process: both routes
on the same files, plus the entropy decode's synchronisation rounds."""
import argparse
import os
import pathlib
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent.parent))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--threads", default="1,4,16")
    ap.add_argument("--procs", default="", help="comma list: also run with OD_DECODE_PROCS=N")
    ap.add_argument("--size", type=int, default=320)
    ap.add_argument("--decode", default="host", help="comma list of routes: host (threads / procs runs), device")
    ap.add_argument("--profile", action="store_true", help="cProfile the last run (main thread)")
    a = ap.parse_args()
    from PIL import Image
    from object_detector_amd.detector import ObjectDetector
    d = tempfile.mkdtemp(prefix="od_jpg_")
    rng = np.random.default_rng(0)
    base = rng.integers(0, 256, (24, 32, 3), dtype=np.uint8)
    paths = []
    for i in range(a.n):
        img = Image.fromarray(np.roll(base, i, 1)).resize((500, 375), Image.BILINEAR)  # smooth: JPEG-typical content
        p = os.path.join(d, f"{i}.jpg")
        img.save(p, quality=90)
        paths.append(p)
    od = ObjectDetector.synthetic(32, (a.size, a.size), seed=2, device="cuda:0", use_multi_gpu=False)
    od.predict(paths[:64], conf_threshold=0.3)  # warm-up (stream calibration, first touch)
    routes = [r for r in a.decode.split(",") if r]
    runs = []
    if "host" in routes:
        runs = [("0", t) for t in a.threads.split(",") if t] + [(q, "1") for q in a.procs.split(",") if q]
    if "device" in routes:
        os.environ.pop("OD_DECODE_THREADS", None)
        os.environ["OD_DECODE_PROCS"] = "0"
        od.predict(paths[:64], conf_threshold=0.3, image_decode="device")  # warm-up: buffers, first launches
        if "host" in routes:  # the default host thread pool, next to the device route
            t0 = time.perf_counter()
            od.predict(paths, conf_threshold=0.3)
            host_rate = a.n / (time.perf_counter() - t0)
            print(f"decode host  (default thread pool): {host_rate:8.1f} images/s end to end", flush=True)
        od.decode_stats = dict.fromkeys(od.decode_stats, 0)
        t0 = time.perf_counter()
        r = od.predict(paths, conf_threshold=0.3, image_decode="device")
        dt = time.perf_counter() - t0
        rounds = [x for p in od._pipes if p.decoder is not None for x in p.decoder.sync_rounds()]
        print(f"decode device (default thread pool): {a.n / dt:8.1f} images/s end to end ({dt * 1e3 / a.n:.2f} ms per image, "
              f"{len(r)} results, routes {od.decode_stats}, sync rounds min/mean/max {min(rounds)}/{np.mean(rounds):.2f}/"
              f"{max(rounds)})", flush=True)
        from object_detector_amd import jpeg
        us = [jpeg.parse_file(p).parse_us for p in paths[:64]]
        print(f"host header parse + unstuffing: {np.median(us):.0f} us per image (median, one thread)", flush=True)
    for q, t in runs:
        os.environ["OD_DECODE_PROCS"] = q
        os.environ["OD_DECODE_THREADS"] = t
        if q != "0":
            od.predict(paths[:64], conf_threshold=0.3)  # start the workers
        if a.profile:
            import cProfile
            import pstats
            pr = cProfile.Profile()
            pr.enable()
        t0 = time.perf_counter()
        r = od.predict(paths, conf_threshold=0.3)
        dt = time.perf_counter() - t0
        if a.profile:
            pr.disable()
            pstats.Stats(pr).sort_stats("cumulative").print_stats(18)
        print(f"decode {os.environ.get('OD_DECODE_PROCS', '0')} procs / threads {t:>3s}: {a.n / dt:8.1f} images/s end to end ({dt * 1e3 / a.n:.2f} ms per image, {len(r)} results)", flush=True)


if __name__ == "__main__":
    main()
