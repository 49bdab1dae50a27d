// Test-time augmentation: the mirror of the network input (od_hflip_u8).  The merge of the per-view candidate lists into ONE
// NMS + box voting (od_tta_merge) is merge.hip's, with the views as its list source.  DESIGN.md "Flip test-time augmentation"
// freezes the semantics; tests/test_gpu_tta.py compares the mirror with numpy byte for byte.
#include "common.h"

namespace {

// ---- od_hflip_u8 ----------------------------------------------------------------------------------------------------
// 16 pixels = 48 bytes = three 16-byte words per thread: group gx of a row is read from group (W/16 - 1 - gx) and its
// pixels are reversed in registers (every byte index below is a compile-time constant).  Needs W % 16 == 0 and 16-byte
// aligned tensors (then every row, 3 * W bytes, starts 16-byte aligned too).
__global__ __launch_bounds__(256) void od_hflip_u8_x16(const uint4* __restrict__ src, uint4* __restrict__ dst, int gpr,
                                                       long long ngroups) {
  for (long long g = (long long)blockIdx.x * 256 + threadIdx.x; g < ngroups; g += (long long)gridDim.x * 256) {
    const long long row = g / gpr;
    const int gx = (int)(g - row * gpr);
    const long long sg = row * gpr + (gpr - 1 - gx);
    const uint4 a = src[sg * 3], b = src[sg * 3 + 1], c = src[sg * 3 + 2];
    const unsigned in[12] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, c.x, c.y, c.z, c.w};
    unsigned o[12];
#pragma unroll
    for (int w = 0; w < 12; ++w) {
      unsigned acc = 0;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int k = 4 * w + e, q = k / 3, ch = k - 3 * q;
        const int sb = (15 - q) * 3 + ch;
        acc |= ((in[sb >> 2] >> ((sb & 3) * 8)) & 0xFFu) << (e * 8);
      }
      o[w] = acc;
    }
    dst[g * 3] = make_uint4(o[0], o[1], o[2], o[3]);
    dst[g * 3 + 1] = make_uint4(o[4], o[5], o[6], o[7]);
    dst[g * 3 + 2] = make_uint4(o[8], o[9], o[10], o[11]);
  }
}

// any width / alignment: one pixel per thread
__global__ __launch_bounds__(256) void od_hflip_u8_px(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int W,
                                                      long long npix) {
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < npix; i += (long long)gridDim.x * 256) {
    const long long row = i / W;
    const int x = (int)(i - row * W);
    const uint8_t* s = src + (row * W + (W - 1 - x)) * 3;
    uint8_t* d = dst + i * 3;
    d[0] = s[0];
    d[1] = s[1];
    d[2] = s[2];
  }
}

}  // namespace

extern "C" int od_hflip_u8(od_ctx* ctx, const uint8_t* src, uint8_t* dst, int B, int H, int W, void* stream) {
  OD_REQUIRE(ctx && src && dst, "od_hflip_u8: null argument");
  OD_REQUIRE(B > 0 && H > 0 && W > 0, "od_hflip_u8: bad dims");
  const long long npix = (long long)B * H * W;
  const uintptr_t s0 = (uintptr_t)src, d0 = (uintptr_t)dst, bytes = (uintptr_t)npix * 3;
  OD_REQUIRE(s0 + bytes <= d0 || d0 + bytes <= s0, "od_hflip_u8: src and dst overlap");
  hipStream_t s = (hipStream_t)stream;
  if (W % 16 == 0 && s0 % 16 == 0 && d0 % 16 == 0) {
    const long long ngroups = npix / 16;
    const unsigned grid = (unsigned)((ngroups + 255) / 256 < 4096 ? (ngroups + 255) / 256 : 4096);
    hipLaunchKernelGGL(od_hflip_u8_x16, dim3(grid), dim3(256), 0, s, (const uint4*)src, (uint4*)dst, W / 16, ngroups);
  } else {
    const unsigned grid = (unsigned)((npix + 255) / 256 < 4096 ? (npix + 255) / 256 : 4096);
    hipLaunchKernelGGL(od_hflip_u8_px, dim3(grid), dim3(256), 0, s, src, dst, W, npix);
  }
  OD_CHECK_LAUNCH();
  return OD_OK;
}
