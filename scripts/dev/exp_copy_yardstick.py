"""usage: exp_copy_yardstick.py [B P NC]
The yardstick of od_detect_pass1: the time of a plain device-to-device copy that moves the bytes pass 1 moves (pred [B,P,NC+6]
f32 read; boxes [B,P,4] + rowmax [B,P] f32 written).  A copy of n bytes reads n and writes n, so the copy with pass 1's traffic
is one of (read + written) / 2 bytes; the copy of all of pred (which writes as much as it reads) is printed beside it."""
import sys

import torch


def copy_us(nbytes, iters=200):
    n = nbytes // 4
    src = torch.empty(n, dtype=torch.float32, device="cuda").normal_()
    dst = torch.empty_like(src)
    for _ in range(20):
        dst.copy_(src)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    best = []
    for _rep in range(5):
        torch.cuda.synchronize()
        e0.record()
        for _ in range(iters):
            dst.copy_(src)
        e1.record()
        torch.cuda.synchronize()
        best.append(e0.elapsed_time(e1) * 1e3 / iters)
    return sorted(best)[len(best) // 2]


def main():
    B, P, NC = (int(v) for v in sys.argv[1:4]) if len(sys.argv) > 3 else (32, 16800, 20)
    rd, wr = B * P * (NC + 6) * 4, B * P * 5 * 4
    t_same = copy_us((rd + wr) // 2)
    t_pred = copy_us(rd)
    print(f"pass 1 at B={B} P={P} NC={NC}: reads {rd / 1e6:.1f} MB, writes {wr / 1e6:.1f} MB")
    print(f"copy of {(rd + wr) / 2e6:.1f} MB (the same traffic, {(rd + wr) / 1e6:.1f} MB): {t_same:.1f} us "
          f"= {(rd + wr) / t_same / 1e3:.0f} GB/s")
    print(f"copy of {rd / 1e6:.1f} MB (all of pred, traffic {2 * rd / 1e6:.1f} MB): {t_pred:.1f} us = {2 * rd / t_pred / 1e3:.0f} GB/s")


if __name__ == "__main__":
    main()
