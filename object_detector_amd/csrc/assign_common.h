// Device helpers shared by the prior-box assigners (assign.hip: max-IoU rule; assign_atss.hip: ATSS rule; assign_tal.hip:
// task-aligned rule): the f32 IoU and cover, the flag staging, the target row, and the claim key and encode pass of the two
// claim-table assigners.  Every f32 sequence here is mirrored op for op by oracle/assign.py and
// tests/assign_ign_ref.py, so these TUs are compiled with -ffp-contract=off.
#pragma once
#include "common.h"

namespace {

typedef unsigned long long u64;
constexpr int GMAX = 128;

__device__ __forceinline__ float iou_f32(const f32x4 a, const f32x4 c) {
  const float ix1 = fmaxf(a[0], c[0]), iy1 = fmaxf(a[1], c[1]);
  const float ix2 = fminf(a[2], c[2]), iy2 = fminf(a[3], c[3]);
  const float iw = fmaxf(ix2 - ix1, 0.f), ih = fmaxf(iy2 - iy1, 0.f);
  const float inter = iw * ih;
  const float area_a = (a[2] - a[0]) * (a[3] - a[1]);
  const float area_c = (c[2] - c[0]) * (c[3] - c[1]);
  const float uni = (area_a + area_c) - inter;
  return uni > 0.f ? inter / uni : 0.f;
}

// share of prior c that lies inside region a: intersection over the PRIOR's area (>= IoU)
__device__ __forceinline__ float cover_f32(const f32x4 a, const f32x4 c) {
  const float ix1 = fmaxf(a[0], c[0]), iy1 = fmaxf(a[1], c[1]);
  const float ix2 = fminf(a[2], c[2]), iy2 = fminf(a[3], c[3]);
  const float iw = fmaxf(ix2 - ix1, 0.f), ih = fmaxf(iy2 - iy1, 0.f);
  const float inter = iw * ih;
  const float area_c = (c[2] - c[0]) * (c[3] - c[1]);
  return area_c > 0.f ? inter / area_c : 0.f;
}

// IGN: bit g of smask[g >> 6] <- bit 0 of flags[g] for g < G (G <= 128: waves 0 and 1 of the block, one ballot each)
__device__ __forceinline__ void stage_flags(const int* __restrict__ flags, int G, int tid, u64* smask) {
  if (tid < GMAX) {
    const bool f = tid < G && (flags[tid] & 1);
    const u64 m = __ballot(f);
    if ((tid & 63) == 0) smask[tid >> 6] = m;
  }
}

// rule 3: does any flagged box of image boxes[Gmax,4] (bits of smask) hold at least ign_thr of prior pr's area?
__device__ __forceinline__ bool region_covers(const float* __restrict__ boxes, const u64* smask, const f32x4 pr,
                                              float ign_thr) {
  bool region = false;
  for (int w = 0; w < GMAX / 64; ++w)
    for (u64 m = smask[w]; m; m &= m - 1) {  // the flagged boxes only; the address is the same for the whole block
      const int r = w * 64 + __builtin_ctzll(m);
      region |= cover_f32(*(const f32x4*)(boxes + (long long)r * 4), pr) >= ign_thr;
    }
  return region;
}

// the row of an owned prior (row is all zero on entry): objectness, one-hot class, corner offsets / loc_scale
__device__ __forceinline__ void write_owned_row(float* row, int NC, const f32x4 pr, const f32x4 gb, int cls,
                                                float loc_scale) {
  const float pw = pr[2] - pr[0], ph = pr[3] - pr[1];
  row[1] = 1.f;
  if (cls >= 0 && cls < NC) row[2 + cls] = 1.f;
  row[2 + NC + 0] = ((gb[0] - pr[0]) / pw) / loc_scale;
  row[2 + NC + 1] = ((gb[1] - pr[1]) / ph) / loc_scale;
  row[2 + NC + 2] = ((gb[2] - pr[2]) / pw) / loc_scale;
  row[2 + NC + 3] = ((gb[3] - pr[3]) / ph) / loc_scale;
}

// claim key: forced | IoU bits | 255 - g.  IoU >= 0, so its bits order like its value; 255 - g >= 128 keeps a key nonzero.
__device__ __forceinline__ u64 claim_key(bool forced, float v, int g) {
  return ((u64)forced << 40) | ((u64)__float_as_uint(v) << 8) | (u64)(255 - g);
}

// encode pass of the claim-table assigners (assign_atss.hip, assign_tal.hip): one thread per prior reads its claim and writes
// the row, assigned_gt and npos
template <bool IGN>
__global__ __launch_bounds__(256) void od_claim_encode(const float* __restrict__ priors, const float* __restrict__ gt_boxes,
                                                       const int* __restrict__ gt_classes,
                                                       const int* __restrict__ gt_counts, const int* __restrict__ gt_flags,
                                                       int P, int Gmax, int NC, float ign_thr, float loc_scale,
                                                       const u64* __restrict__ claim, float* __restrict__ y,
                                                       int* __restrict__ assigned_gt, int* __restrict__ npos) {
  __shared__ int scount;
  __shared__ u64 smask[GMAX / 64];
  const int b = blockIdx.y, tid = threadIdx.x;
  const int G = min(gt_counts[b], Gmax);
  if (IGN) stage_flags(gt_flags + (long long)b * Gmax, G, tid, smask);
  if (tid == 0) scount = 0;
  __syncthreads();
  const int p = blockIdx.x * 256 + tid;
  if (p < P) {
    const int C = NC + 6;
    const u64 k = claim[(long long)b * P + p];
    const int g = k ? 255 - (int)(k & 255ull) : -1;
    const f32x4 pr = *(const f32x4*)(priors + (long long)p * 4);
    bool region = false;
    if (IGN && g < 0 && (smask[0] | smask[1]))  // background prior of an image that has regions
      region = region_covers(gt_boxes + (long long)b * Gmax * 4, smask, pr, ign_thr);
    float* row = y + ((long long)b * P + p) * C;
    for (int c = 0; c < C; ++c) row[c] = 0.f;
    if (g >= 0) {
      const f32x4 gb = *(const f32x4*)(gt_boxes + ((long long)b * Gmax + g) * 4);
      write_owned_row(row, NC, pr, gb, gt_classes[(long long)b * Gmax + g], loc_scale);
      atomicAdd(&scount, 1);
    } else if (!region) {
      row[0] = 1.f;
    }
    if (assigned_gt) assigned_gt[(long long)b * P + p] = g >= 0 ? g : (region ? -3 : -1);
  }
  __syncthreads();
  if (tid == 0 && scount) atomicAdd(&npos[b], scount);
}

}  // namespace
