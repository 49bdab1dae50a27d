// Pillow's fixed-point BILINEAR pass (22 fraction bits), shared by jpeg.hip (od_img_hpass_k / od_img_vpass_k) and slice.hip
// (od_tiles_resize): out = clip8((2^21 + sum(in * w)) >> 22) per channel, over the taps of one row of a
// object_detector_amd/resample.py table (first source index, tap count, weights...).
#pragma once
#include "common.h"

__device__ __forceinline__ uint8_t clip8(int64_t acc) {
  return (uint8_t)min(max(acc >> 22, (int64_t)0), (int64_t)255);
}

// one output pixel of a pass: taps of table row t over source pixels `step` bytes apart
__device__ __forceinline__ void resample_px(const uint8_t* s, int64_t step, const int* t, uint8_t* o) {
  const int nt = t[1];
  int64_t a0 = 1 << 21, a1 = 1 << 21, a2 = 1 << 21;
  for (int k = 0; k < nt; ++k) {
    const int64_t w = t[2 + k];
    a0 += s[k * step] * w;
    a1 += s[k * step + 1] * w;
    a2 += s[k * step + 2] * w;
  }
  o[0] = clip8(a0);
  o[1] = clip8(a1);
  o[2] = clip8(a2);
}
