// Device helpers shared by the prior-box assigners (assign.hip: max-IoU rule; assign_atss.hip: ATSS rule): the f32 IoU and
// cover, the flag staging and the target row.  Every f32 sequence here is mirrored op for op by oracle/assign.py and
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

}  // namespace
