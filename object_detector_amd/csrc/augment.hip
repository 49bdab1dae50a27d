// K14: device-side pixel augmentation of the training generator (reference check_generator.py:17-18,
// docs/MODEL.md:60-64: Random Erasing "and anything else at hand").  Augmentation PARAMETERS are sampled on the host
// (od_gen.sample_params); this kernel does the pixel work for a whole batch: crop + resize (bilinear, half-pixel
// centres) + horizontal flip + saturation / contrast / brightness + Random Erasing rectangles, uint8 in -> uint8 NHWC out.
// HBM-bound elementwise; one thread per output pixel.  f32 arithmetic in a fixed order (-ffp-contract=off), mirrored
// op for op by oracle/augment.py => bit-exact.
// od_augment_mosaic composes four sources into one output image: the frame is cut at (split_x, split_y), each of the four
// tiles is an od_augment_k image of its own extent (same per-pixel body: aug_sample), and one erase list acts on the whole
// frame.  With split = (W, H) the TL tile is the frame and the output is od_augment_batch's, byte for byte.
#include "common.h"

namespace {

// colour of one output pixel at normalised position (u, v) of the image / tile p describes: crop -> half-pixel bilinear ->
// flip -> saturation -> contrast -> brightness -> round half up -> clamp.  Shared by both kernels, op for op.
__device__ __forceinline__ void aug_sample(const uint8_t* __restrict__ src, const od_aug_params& p, float u, float v,
                                           float c[3]) {
  const uint8_t* img = src + p.src_offset;
  if (p.flip) u = 1.0f - u;
  // source position in pixel units (half-pixel centres), clamped to the crop rectangle's pixel range
  float sx = (p.crop_x1 + u * (p.crop_x2 - p.crop_x1)) * (float)p.src_w - 0.5f;
  float sy = (p.crop_y1 + v * (p.crop_y2 - p.crop_y1)) * (float)p.src_h - 0.5f;
  sx = fminf(fmaxf(sx, 0.f), (float)(p.src_w - 1));
  sy = fminf(fmaxf(sy, 0.f), (float)(p.src_h - 1));
  const int x0 = (int)floorf(sx), y0 = (int)floorf(sy);
  const int x1 = min(x0 + 1, p.src_w - 1), y1 = min(y0 + 1, p.src_h - 1);
  const float fx = sx - (float)x0, fy = sy - (float)y0;
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    const float p00 = (float)img[((long long)y0 * p.src_w + x0) * 3 + ch];
    const float p01 = (float)img[((long long)y0 * p.src_w + x1) * 3 + ch];
    const float p10 = (float)img[((long long)y1 * p.src_w + x0) * 3 + ch];
    const float p11 = (float)img[((long long)y1 * p.src_w + x1) * 3 + ch];
    const float top = p00 + (p01 - p00) * fx;
    const float bot = p10 + (p11 - p10) * fx;
    c[ch] = top + (bot - top) * fy;
  }
  const float gray = (c[0] * 0.299f + c[1] * 0.587f) + c[2] * 0.114f;
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    float t = gray + (c[ch] - gray) * p.saturation;
    t = (t - 127.5f) * p.contrast + 127.5f;
    t = t + p.brightness;
    c[ch] = fminf(fmaxf(floorf(t + 0.5f), 0.f), 255.f);
  }
}

// Random-Erasing rectangles, on normalised OUTPUT coordinates of the whole frame; then the 3-byte store
__device__ __forceinline__ void aug_erase_store(int n_erase, const float (*erase)[4], const uint8_t (*erase_rgb)[4], int x,
                                                int y, int H, int W, float c[3], uint8_t* __restrict__ o) {
  const float cu = ((float)x + 0.5f) / (float)W, cv = ((float)y + 0.5f) / (float)H;
  for (int e = 0; e < n_erase; ++e) {
    if (cu >= erase[e][0] && cu < erase[e][2] && cv >= erase[e][1] && cv < erase[e][3]) {
      c[0] = (float)erase_rgb[e][0];
      c[1] = (float)erase_rgb[e][1];
      c[2] = (float)erase_rgb[e][2];
    }
  }
  o[0] = (uint8_t)c[0];
  o[1] = (uint8_t)c[1];
  o[2] = (uint8_t)c[2];
}

__global__ __launch_bounds__(256) void od_augment_k(const uint8_t* __restrict__ src, const od_aug_params* __restrict__ prm,
                                                    uint8_t* __restrict__ out, int H, int W) {
  const int b = blockIdx.y;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= H * W) return;
  const int y = i / W, x = i - y * W;
  const od_aug_params& p = prm[b];  // read through the pointer: a by-value copy of the 112-byte block lived in scratch
  float c[3];
  aug_sample(src, p, ((float)x + 0.5f) / (float)W, ((float)y + 0.5f) / (float)H, c);
  aug_erase_store(p.n_erase, p.erase, p.erase_rgb, x, y, H, W, c, out + (((long long)b * H + y) * W + x) * 3);
}

__global__ __launch_bounds__(256) void od_augment_mosaic_k(const uint8_t* __restrict__ src,
                                                           const od_mosaic_params* __restrict__ prm,
                                                           uint8_t* __restrict__ out, int H, int W) {
  const int b = blockIdx.y;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= H * W) return;
  const int y = i / W, x = i - y * W;
  const od_mosaic_params& m = prm[b];
  const int sx = m.split_x, sy = m.split_y;
  const int right = x >= sx, low = y >= sy;  // an empty tile (split_x == W / split_y == H) is never chosen
  const int t = low * 2 + right;             // TL, TR, BL, BR
  const int X0 = right ? sx : 0, Wt = right ? W - sx : sx;
  const int Y0 = low ? sy : 0, Ht = low ? H - sy : sy;
  const float u = ((float)(x - X0) + 0.5f) / (float)Wt, v = ((float)(y - Y0) + 0.5f) / (float)Ht;
  float c[3];
  // The tile is the same for a whole wavefront except on the two split lines.  Uniform wave: ITS tile's parameters come
  // through a wave-uniform index (scalar loads of one tile, not four).  A wave on a split line takes the first active
  // lane's tile, serves the lanes that want it, and repeats (at most four rounds).
  const int t0 = __builtin_amdgcn_readfirstlane(t);
  if (__all(t == t0)) {
    aug_sample(src, m.tile[t0], u, v, c);
  } else {
    for (bool done = false; !done;) {
      const int tu = __builtin_amdgcn_readfirstlane(t);
      if (t == tu) {
        aug_sample(src, m.tile[tu], u, v, c);
        done = true;
      }
    }
  }
  aug_erase_store(m.n_erase, m.erase, m.erase_rgb, x, y, H, W, c, out + (((long long)b * H + y) * W + x) * 3);
}

// round half up, clamp to a byte's range (aug_sample's last step)
__device__ __forceinline__ float aug_round_u8(float t) { return fminf(fmaxf(floorf(t + 0.5f), 0.f), 255.f); }

// K14b: affine warp + colour matrix + MixUp of one or two mosaic frames.  Per output pixel (x, y), all f32, in this order:
//  1. px = (float)x + 0.5f, py = (float)y + 0.5f
//  2. frame f: fx = (a0*px + a1*py) + a2, fy = (a3*px + a4*py) + a5   (frame coordinates in OUTPUT-PIXEL units, so the
//     identity matrix gives fx = px, fy = py exactly)
//  3. fx < 0 || fx >= W || fy < 0 || fy >= H: the frame's colour is fill_rgb (no colour matrix)
//  4. else right = fx >= split_x, low = fy >= split_y pick the tile (X0, Y0, Wt, Ht) as od_augment_mosaic_k does;
//     u = (fx - X0) / Wt, v = (fy - Y0) / Ht; c = aug_sample(tile, u, v) (whole numbers in [0, 255]);
//     t[ch] = ((k[ch][0]*c0 + k[ch][1]*c1) + k[ch][2]*c2) + k[ch][3], round half up, clamp to [0, 255]
//  5. two frames: t = A*mix_a + B*mix_b of the two finished colours, round half up, clamp
//  6. the erase list on normalised output coordinates and the 3-byte store (aug_erase_store)
// One frame's colour at (px, py).  The tile is wave-uniform except where a wavefront crosses a split line -- under
// rotation most waves near one do -- so the mosaic kernel's scheme is kept: take the first unserved lane's tile through a
// wave-uniform index (scalar loads of that tile's parameters), serve the lanes that want it, at most four rounds.  Lanes
// outside the frame take the fill colour and never enter the loop.
__device__ __forceinline__ void warp_frame(const uint8_t* __restrict__ src, const od_warp_params& w, int f, float px,
                                           float py, int H, int W, float c[3]) {
  const float* a = w.a[f];
  const od_mosaic_params& m = w.frame[f];
  const float fx = (a[0] * px + a[1] * py) + a[2];
  const float fy = (a[3] * px + a[4] * py) + a[5];
  const bool outside = fx < 0.f || fx >= (float)W || fy < 0.f || fy >= (float)H;
  const int sx = m.split_x, sy = m.split_y;
  const int right = fx >= (float)sx, low = fy >= (float)sy;
  const int t = low * 2 + right;  // TL, TR, BL, BR
  const int X0 = right ? sx : 0, Wt = right ? W - sx : sx;
  const int Y0 = low ? sy : 0, Ht = low ? H - sy : sy;
  const float u = (fx - (float)X0) / (float)Wt, v = (fy - (float)Y0) / (float)Ht;
  c[0] = (float)w.fill_rgb[0];
  c[1] = (float)w.fill_rgb[1];
  c[2] = (float)w.fill_rgb[2];
  for (bool done = outside; !done;) {
    const int tu = __builtin_amdgcn_readfirstlane(t);
    if (t == tu) {
      float s[3];
      aug_sample(src, m.tile[tu], u, v, s);
      const float(*k)[4] = w.k[f];
#pragma unroll
      for (int ch = 0; ch < 3; ++ch)
        c[ch] = aug_round_u8(((k[ch][0] * s[0] + k[ch][1] * s[1]) + k[ch][2] * s[2]) + k[ch][3]);
      done = true;
    }
  }
}

__global__ __launch_bounds__(256) void od_augment_warp_k(const uint8_t* __restrict__ src,
                                                         const od_warp_params* __restrict__ prm,
                                                         uint8_t* __restrict__ out, int H, int W) {
  const int b = blockIdx.y;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= H * W) return;
  const int y = i / W, x = i - y * W;
  const od_warp_params& w = prm[b];
  const float px = (float)x + 0.5f, py = (float)y + 0.5f;
  float c[3];
  warp_frame(src, w, 0, px, py, H, W, c);
  if (w.n_frames == 2) {  // wave-uniform: one image per blockIdx.y
    float d[3];
    warp_frame(src, w, 1, px, py, H, W, d);
    const float ma = w.mix_a, mb = w.mix_b;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) c[ch] = aug_round_u8(c[ch] * ma + d[ch] * mb);
  }
  aug_erase_store(w.n_erase, w.erase, w.erase_rgb, x, y, H, W, c, out + (((long long)b * H + y) * W + x) * 3);
}

}  // namespace

extern "C" int od_aug_params_bytes(void) { return (int)sizeof(od_aug_params); }
extern "C" int od_mosaic_params_bytes(void) { return (int)sizeof(od_mosaic_params); }
extern "C" int od_warp_params_bytes(void) { return (int)sizeof(od_warp_params); }

extern "C" int od_augment_batch(od_ctx* ctx, const uint8_t* src, const void* params, uint8_t* out, int B, int H, int W,
                                void* stream) {
  OD_REQUIRE(ctx && src && params && out && B > 0 && B <= 65535 && H > 0 && W > 0, "od_augment_batch: bad argument");
  hipLaunchKernelGGL(od_augment_k, dim3(od_ceil_div(H * W, 256), B), dim3(256), 0, (hipStream_t)stream, src,
                     (const od_aug_params*)params, out, H, W);
  OD_CHECK_LAUNCH();
  return OD_OK;
}

extern "C" int od_augment_mosaic(od_ctx* ctx, const uint8_t* src, const void* params, uint8_t* out, int B, int H, int W,
                                 void* stream) {
  OD_REQUIRE(ctx && src && params && out && B > 0 && B <= 65535 && H > 0 && W > 0, "od_augment_mosaic: bad argument");
  hipLaunchKernelGGL(od_augment_mosaic_k, dim3(od_ceil_div(H * W, 256), B), dim3(256), 0, (hipStream_t)stream, src,
                     (const od_mosaic_params*)params, out, H, W);
  OD_CHECK_LAUNCH();
  return OD_OK;
}

extern "C" int od_augment_warp(od_ctx* ctx, const uint8_t* src, const void* params, uint8_t* out, int B, int H, int W,
                               void* stream) {
  OD_REQUIRE(ctx && src && params && out && B > 0 && B <= 65535 && H > 0 && W > 0, "od_augment_warp: bad argument");
  hipLaunchKernelGGL(od_augment_warp_k, dim3(od_ceil_div(H * W, 256), B), dim3(256), 0, (hipStream_t)stream, src,
                     (const od_warp_params*)params, out, H, W);
  OD_CHECK_LAUNCH();
  return OD_OK;
}
