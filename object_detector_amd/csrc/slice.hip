// Sliced inference: tiles of a full-resolution image cut and resized into the network batch (od_tiles_resize).  The merge of
// the per-tile candidate lists of every image into ONE NMS + box voting (od_slice_merge) is merge.hip's, with the batch rows as
// its list source.  DESIGN.md "Sliced inference" freezes the semantics; tests/slice_ref.py is their numpy restatement and
// tests/test_gpu_slice_tiles.py compares bit for bit.
//
// od_tiles_resize: Pillow's crop + resize(BILINEAR) of one rectangle per network row, the two passes of resample_common.h in
// Image.resize's order, each rounded to 8 bits; a pass whose length does not change is skipped.  HBM-bound: a pass reads
// the rows of its source once (the taps of neighbouring outputs overlap in L1 / L2).
//   od_tiles_pass1_k   rectangle -> tmp [th, W] (horizontal), or -> tmp [H, tw] when the tile takes the vertical pass first
//   od_tiles_pass2_k   tmp (or the rectangle itself, when pass 1 was skipped) -> row n of the output
// Every source read is inside the rectangle: a tap row is clamped to the pass's source length, whatever the table holds.
#include "post_common.h"
#include "resample_common.h"

#include <algorithm>

namespace {

// ---- od_tiles_resize --------------------------------------------------------------------------------------------------
// Image.resize's pass order for the crop: vertical first for a very tall, narrow tile that shrinks vertically
__host__ __device__ __forceinline__ bool tile_vfirst(int tw, int th, int H) { return th > (int64_t)100 * tw && H < th; }

// one output pixel of a pass over a source axis of n_in pixels `step` bytes apart starting at s
__device__ __forceinline__ void tile_px(const uint8_t* s, int64_t step, const int* t, int n_in, uint8_t* o) {
  const int first = min(max(t[0], 0), n_in - 1), nt = min(t[1], n_in - first);
  s += first * step;
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

__device__ __forceinline__ const uint8_t* tile_src(const uint8_t* blob, const od_tile_desc& d) {
  return blob + d.src_off + (int64_t)d.y0 * d.pitch + 3LL * d.x0;
}

__global__ __launch_bounds__(256) void od_tiles_pass1_k(const uint8_t* __restrict__ blob, const od_tile_desc* __restrict__ descs,
                                                        uint8_t* __restrict__ ws, int H, int W) {
  const od_tile_desc d = descs[blockIdx.y];
  const int tw = d.x1 - d.x0, th = d.y1 - d.y0;
  const uint8_t* src = tile_src(blob, d);
  uint8_t* tmp = ws + d.tmp_ws;
  if (tile_vfirst(tw, th, H)) {  // rectangle -> tmp [H, tw]
    const int* tb = (const int*)(blob + d.vcoef_off);
    for (int i = blockIdx.x * 256 + threadIdx.x; i < H * tw; i += gridDim.x * 256) {
      const int y = i / tw, x = i - y * tw;
      tile_px(src + 3LL * x, d.pitch, tb + (int64_t)y * (2 + d.vk), th, tmp + (int64_t)i * 3);
    }
    return;
  }
  if (W == tw) return;
  const int* tb = (const int*)(blob + d.hcoef_off);  // rectangle -> tmp [th, W]
  for (int i = blockIdx.x * 256 + threadIdx.x; i < th * W; i += gridDim.x * 256) {
    const int y = i / W, x = i - y * W;
    tile_px(src + (int64_t)y * d.pitch, 3, tb + (int64_t)x * (2 + d.hk), tw, tmp + (int64_t)i * 3);
  }
}

__global__ __launch_bounds__(256) void od_tiles_pass2_k(const uint8_t* __restrict__ blob, const od_tile_desc* __restrict__ descs,
                                                        const uint8_t* __restrict__ ws, uint8_t* __restrict__ out, int H, int W) {
  const od_tile_desc d = descs[blockIdx.y];
  const int tw = d.x1 - d.x0, th = d.y1 - d.y0;
  const uint8_t* tmp = ws + d.tmp_ws;
  uint8_t* dst = out + (int64_t)blockIdx.y * H * W * 3;
  const bool vfirst = tile_vfirst(tw, th, H);
  // the second pass's source: tmp, or the rectangle itself when the first pass was skipped
  const bool direct = !vfirst && W == tw;
  const uint8_t* src = direct ? tile_src(blob, d) : tmp;
  const int64_t pitch = direct ? d.pitch : 3LL * (vfirst ? tw : W);
  const int* htb = (const int*)(blob + d.hcoef_off);
  const int* vtb = (const int*)(blob + d.vcoef_off);
  for (int i = blockIdx.x * 256 + threadIdx.x; i < H * W; i += gridDim.x * 256) {
    const int y = i / W, x = i - y * W;
    uint8_t* o = dst + (int64_t)i * 3;
    if (vfirst ? W == tw : H == th) {  // this pass is skipped too: copy
      const uint8_t* s = src + (int64_t)y * pitch + 3LL * x;
      o[0] = s[0];
      o[1] = s[1];
      o[2] = s[2];
    } else if (vfirst) {
      tile_px(src + (int64_t)y * pitch, 3, htb + (int64_t)x * (2 + d.hk), tw, o);
    } else {
      tile_px(src + 3LL * x, pitch, vtb + (int64_t)y * (2 + d.vk), th, o);
    }
  }
}

int64_t align256(int64_t v) { return (v + 255) & ~(int64_t)255; }

// pixels of the intermediate image between the passes (0: the first pass is skipped)
int64_t tile_tmp_pixels(const od_tile_desc& d, int H, int W) {
  const int tw = d.x1 - d.x0, th = d.y1 - d.y0;
  if (tile_vfirst(tw, th, H)) return (int64_t)H * tw;
  return W == tw ? 0 : (int64_t)th * W;
}

bool tile_rect_ok(const od_tile_desc& d) {
  return d.src_w > 0 && d.src_h > 0 && d.src_w <= 65535 && d.src_h <= 65535 && d.x0 >= 0 && d.y0 >= 0 && d.x0 < d.x1 &&
         d.y0 < d.y1 && d.x1 <= d.src_w && d.y1 <= d.src_h;
}

int grid_x(int64_t n) { return (int)std::min<int64_t>(std::max<int64_t>((n + 255) / 256, 1), 512); }

}  // namespace

extern "C" int od_tiles_workspace_plan(od_tile_desc* descs_host, int N, int H, int W, long long* workspace_bytes) {
  OD_REQUIRE(descs_host && workspace_bytes && N > 0 && H > 0 && W > 0, "od_tiles_workspace_plan: bad argument");
  int64_t off = 0, end = 0;  // the size returned is the end of the last intermediate image, not rounded up
  for (int n = 0; n < N; ++n) {
    od_tile_desc& d = descs_host[n];
    OD_REQUIRE(tile_rect_ok(d), "od_tiles_workspace_plan: tile %d: rectangle outside the source", n);
    const int64_t nb = 3 * tile_tmp_pixels(d, H, W);
    d.tmp_ws = off;
    if (nb) end = off + nb;
    off = align256(off + nb);
  }
  *workspace_bytes = end;
  return OD_OK;
}

extern "C" int od_tiles_resize(od_ctx* ctx, const od_tile_desc* descs_host, const od_tile_desc* descs, int N,
                               const uint8_t* blob, long long blob_bytes, void* workspace, long long ws_bytes, uint8_t* out,
                               int H, int W, void* stream) {
  OD_REQUIRE(ctx && descs_host && descs && blob && workspace && out, "od_tiles_resize: null argument");
  OD_REQUIRE(N > 0 && N <= 65535 && H > 0 && W > 0 && H <= 65535 && W <= 65535 && (int64_t)H * W <= (1 << 28),
             "od_tiles_resize: bad dims");
  int64_t max_tmp = 0;
  for (int n = 0; n < N; ++n) {
    const od_tile_desc& d = descs_host[n];
    auto in_blob = [&](int64_t off, int64_t nb, int al) { return off >= 0 && nb >= 0 && off % al == 0 && off + nb <= blob_bytes; };
    OD_REQUIRE(tile_rect_ok(d), "od_tiles_resize: tile %d: rectangle outside the source", n);
    OD_REQUIRE(d.pitch >= 3LL * d.src_w && in_blob(d.src_off, (int64_t)(d.src_h - 1) * d.pitch + 3LL * d.src_w, 1),
               "od_tiles_resize: tile %d: source out of bounds", n);
    OD_REQUIRE(d.hk >= 0 && d.vk >= 0 && in_blob(d.hcoef_off, 4LL * W * (2 + d.hk), 4) &&
                   in_blob(d.vcoef_off, 4LL * H * (2 + d.vk), 4),
               "od_tiles_resize: tile %d: resample tables out of bounds", n);
    const int64_t tp = tile_tmp_pixels(d, H, W);
    OD_REQUIRE(tp <= (1 << 28), "od_tiles_resize: tile %d: too large", n);
    if (tp > 0 && (d.tmp_ws < 0 || d.tmp_ws + 3 * tp > ws_bytes)) {  // tmp_ws of a tile without a first pass is never used
      od_set_error("od_tiles_resize: tile %d: workspace too small (%lld bytes)", n, ws_bytes);
      return OD_ERR_WORKSPACE;
    }
    max_tmp = std::max(max_tmp, tp);
  }
  hipStream_t s = (hipStream_t)stream;
  uint8_t* ws = (uint8_t*)workspace;
  if (max_tmp > 0) {
    hipLaunchKernelGGL(od_tiles_pass1_k, dim3(grid_x(max_tmp), N), dim3(256), 0, s, blob, descs, ws, H, W);
    OD_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(od_tiles_pass2_k, dim3(grid_x((int64_t)H * W), N), dim3(256), 0, s, blob, descs, ws, out, H, W);
  OD_CHECK_LAUNCH();
  return OD_OK;
}
