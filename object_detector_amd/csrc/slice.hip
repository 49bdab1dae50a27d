// Sliced inference: tiles of a full-resolution image cut and resized into the network batch (od_tiles_resize), and the merge
// of the per-tile candidate lists of every image into ONE NMS + box voting (od_slice_merge).  DESIGN.md "Sliced inference"
// freezes the semantics; tests/slice_ref.py is their numpy restatement and tests/test_gpu_slice_*.py compare bit for bit.
//
// od_tiles_resize: Pillow's crop + resize(BILINEAR) of one rectangle per network row, the two passes of resample_common.h in
// Image.resize's order, each rounded to 8 bits; a pass whose length does not change is skipped.  HBM-bound: a pass reads
// the rows of its source once (the taps of neighbouring outputs overlap in L1 / L2).
//   od_tiles_pass1_k   rectangle -> tmp [th, W] (horizontal), or -> tmp [H, tw] when the tile takes the vertical pass first
//   od_tiles_pass2_k   tmp (or the rectangle itself, when pass 1 was skipped) -> row n of the output
// Every source read is inside the rectangle: a tap row is clamped to the pass's source length, whatever the table holds.
//
// od_slice_merge is od_tta_merge with batch rows as the "views": three launches,
//   rank  (od_slice_rank)  one workgroup of 1024 threads per image, thread r owns entry r of every tile's list.  The
//         interior-edge rule drops candidates cut at a seam; the survivors of each list are compacted in order (ballot +
//         prefix over the 16 waves), so the lists stay sorted and a survivor's merged rank (conf bits desc, tile asc, flat
//         asc) is its compacted position plus a binary-searched count per other list -- a dropped entry is in no list and
//         cannot disturb a rank.  The first Km = min(K, survivors) are written as od_nms_sort leaves a table behind.
//   od_nms_greedy_k, then od_tta_vote_gather (tta.hip), unchanged, through od_merge_nms_vote_launch
//   (od_slice_merge_soft: the soft scan of soft_nms.hip in place of od_nms_greedy_k).
// Compiled with -ffp-contract=off: the map to image coordinates is one rounding per op, as numpy's.
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

// ---- od_slice_merge ---------------------------------------------------------------------------------------------------
constexpr int SL_MAX_T = 16;
constexpr int SL_MAX_K = 1024;
constexpr int SL_LEFT = 1, SL_TOP = 2, SL_RIGHT = 4, SL_BOTTOM = 8;  // interior sides of a tile (slicing.edges)

// grid G, 1024 threads: thread r owns entry r of every tile's list (K <= 1024).  What a thread knows about its 16 entries
// lives in LDS (one byte each: the survivors of its wave before it, or SL_DROPPED), not in registers: the loops over the
// tiles stay rolled, and the keys are read again where they are needed (they sit in L2).
constexpr unsigned char SL_DROPPED = 0xFF;

__global__ __launch_bounds__(1024) void od_slice_rank(const u64* __restrict__ keys, const int* __restrict__ counts,
                                                      const float* __restrict__ boxes, const float* __restrict__ tiles,
                                                      const int* __restrict__ edges, int T, int P, int NC, int K, int KP,
                                                      float edge_lo, float edge_hi, u64* __restrict__ skeys,
                                                      f32x4* __restrict__ sbox, int* __restrict__ scls,
                                                      int* __restrict__ msrc, int* __restrict__ mcount) {
  __shared__ unsigned lconf[SL_MAX_T * SL_MAX_K];      // conf bits of every compacted list, descending
  __shared__ unsigned char lpre[SL_MAX_T * SL_MAX_K];  // per entry: survivors of its wave before it, or SL_DROPPED
  __shared__ int wtot[SL_MAX_T * 16];                  // survivors per (tile, wave)
  __shared__ int wpre[SL_MAX_T * 16];                  // survivors of the tile in the waves before this one
  __shared__ int lcnt[SL_MAX_T];
  const int g = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const bool rule = edge_lo >= 0.f;
  for (int t = 0; t < T; ++t) {
    const long long row = (long long)g * T + t;
    const int cnt = min(max(counts[row], 0), K);
    bool keep = tid < cnt;
    const int e = rule ? edges[row] : 0;
    if (keep && e) {  // cut at a seam: the box touches an interior side of its tile
      const unsigned p = min(od_key_flat(keys[row * K + tid]) / (unsigned)NC, (unsigned)(P - 1));
      const f32x4 bx = *(const f32x4*)(boxes + (row * P + p) * 4);
      keep = !(((e & SL_LEFT) && bx[0] <= edge_lo) || ((e & SL_TOP) && bx[1] <= edge_lo) ||
               ((e & SL_RIGHT) && bx[2] >= edge_hi) || ((e & SL_BOTTOM) && bx[3] >= edge_hi));
    }
    const u64 m = __ballot(keep);
    lpre[t * SL_MAX_K + tid] = keep ? (unsigned char)__popcll(m & ((1ull << lane) - 1ull)) : SL_DROPPED;
    if (lane == 0) wtot[t * 16 + wv] = __popcll(m);
  }
  __syncthreads();
  if (tid < T * 16) {  // (tile, wave) = (tid / 16, tid % 16)
    const int base = tid & ~15;
    int pre = 0;
    for (int w = 0; w < (tid & 15); ++w) pre += wtot[base + w];
    wpre[tid] = pre;
    if ((tid & 15) == 15) lcnt[tid >> 4] = pre + wtot[tid];
  }
  __syncthreads();
  for (int t = 0; t < T; ++t) {  // the compacted lists: order kept, so still sorted
    const unsigned char v = lpre[t * SL_MAX_K + tid];
    if (v != SL_DROPPED)
      lconf[t * SL_MAX_K + wpre[t * 16 + wv] + v] = od_key_score_bits(keys[((long long)g * T + t) * K + tid]);
  }
  __syncthreads();
  if (tid == 0) {
    int total = 0;
    for (int t = 0; t < T; ++t) total += lcnt[t];
    mcount[g] = min(K, total);
  }
  for (int t = 0; t < T; ++t) {
    const unsigned char v = lpre[t * SL_MAX_K + tid];
    if (v == SL_DROPPED) continue;
    const int pos = wpre[t * 16 + wv] + v;  // position in the compacted list
    const unsigned cb = lconf[t * SL_MAX_K + pos];
    int rank = pos;
    for (int u = 0; u < T; ++u) {
      if (u == t) continue;
      // entries of list u that precede (cb, t): conf > cb, and conf == cb too when u < t
      const unsigned* lu = lconf + u * SL_MAX_K;
      int lo = 0, hi = lcnt[u];
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        const unsigned x = lu[mid];
        if (u < t ? x >= cb : x > cb) lo = mid + 1; else hi = mid;
      }
      rank += lo;
    }
    if (rank >= K) continue;
    const long long row = (long long)g * T + t;
    const unsigned flat = od_key_flat(keys[row * K + tid]);
    unsigned p = flat / (unsigned)NC;
    const unsigned c = flat - p * (unsigned)NC;
    p = min(p, (unsigned)(P - 1));  // a malformed key must not read outside the row's box table
    const f32x4 bx = *(const f32x4*)(boxes + (row * P + p) * 4);
    const f32x4 a = *(const f32x4*)(tiles + row * 4);  // (ox, oy, sx, sy)
    f32x4 m;
    m[0] = fminf(fmaxf(a[0] + a[2] * bx[0], 0.f), 1.f);
    m[1] = fminf(fmaxf(a[1] + a[3] * bx[1], 0.f), 1.f);
    m[2] = fminf(fmaxf(a[0] + a[2] * bx[2], 0.f), 1.f);
    m[3] = fminf(fmaxf(a[1] + a[3] * bx[3], 0.f), 1.f);
    const long long o = (long long)g * KP + rank;
    skeys[o] = od_make_key(cb, (unsigned)(rank * NC + (int)c));
    sbox[o] = m;
    scls[o] = (int)c;
    msrc[o * 2] = t;
    msrc[o * 2 + 1] = (int)flat;
  }
}

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

extern "C" size_t od_slice_merge_workspace_bytes(int G, int T, int K) {
  if (G <= 0 || T < 1 || T > SL_MAX_T || K <= 0 || K > SL_MAX_K) return 0;
  return od_merge_workspace_bytes(G, K);  // the merged table holds K candidates however many tiles feed it
}

// od_slice_merge (soft null) and od_slice_merge_soft: the rank kernel, then the greedy or the soft scan, then vote-and-gather
static int slice_merge(const char* who, od_ctx* ctx, const uint64_t* keys, const int32_t* counts, const float* boxes,
                       const float* tiles, const int32_t* edges, int G, int T, int P, int NC, int K, float edge_lo, float edge_hi,
                       float iou_threshold, int strict, int max_det, const od_soft_nms_cfg* soft, float vote_iou, float* out,
                       int32_t* src, int32_t* keep_count, void* workspace, size_t workspace_bytes, void* stream) {
  OD_REQUIRE(ctx && keys && counts && boxes && tiles && edges && out && keep_count && workspace, "%s: null argument", who);
  OD_REQUIRE(T >= 1 && T <= SL_MAX_T, "%s: T = %d outside 1..%d", who, T, SL_MAX_T);
  OD_REQUIRE(NC >= 1 && NC <= OD_MAX_NC, "%s: NC = %d outside the supported class counts 1..%d", who, NC, OD_MAX_NC);
  OD_REQUIRE(G > 0 && G <= 65535 && K > 0 && K <= SL_MAX_K && max_det > 0, "%s: bad dims (K <= 1024)", who);
  OD_REQUIRE(P > 0 && (long long)P * NC < (1LL << 31), "%s: P * NC must fit 31 bits", who);
  const size_t need = od_merge_workspace_bytes(G, K);
  if (workspace_bytes < need) {
    od_set_error("%s: workspace %zu < %zu bytes", who, workspace_bytes, need);
    return OD_ERR_WORKSPACE;
  }
  const OdMergeWs w = od_merge_workspace(workspace, G, K);
  u64* skeys;
  f32x4* sbox;
  int* scls;
  int KP;
  od_nms_sorted_buffers(w.nms, G, K, &skeys, &sbox, &scls, &KP);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(od_slice_rank, dim3(G), dim3(1024), 0, s, (const u64*)keys, counts, boxes, tiles, edges, T, P, NC, K, KP,
                     edge_lo, edge_hi, skeys, sbox, scls, w.msrc, w.mcount);
  OD_CHECK_LAUNCH();
  return od_merge_nms_vote_launch(w, G, NC, K, iou_threshold, strict, max_det, vote_iou, out, src, keep_count, s, soft);
}

extern "C" int od_slice_merge(od_ctx* ctx, const uint64_t* keys, const int32_t* counts, const float* boxes, const float* tiles,
                              const int32_t* edges, int G, int T, int P, int NC, int K, float edge_lo, float edge_hi,
                              float iou_threshold, int strict, int max_det, float vote_iou, float* out, int32_t* src,
                              int32_t* keep_count, void* workspace, size_t workspace_bytes, void* stream) {
  return slice_merge("od_slice_merge", ctx, keys, counts, boxes, tiles, edges, G, T, P, NC, K, edge_lo, edge_hi, iou_threshold,
                     strict, max_det, nullptr, vote_iou, out, src, keep_count, workspace, workspace_bytes, stream);
}

extern "C" int od_slice_merge_soft(od_ctx* ctx, const uint64_t* keys, const int32_t* counts, const float* boxes,
                                   const float* tiles, const int32_t* edges, int G, int T, int P, int NC, int K, float edge_lo,
                                   float edge_hi, const od_soft_nms_cfg* cfg, float vote_iou, float* out, int32_t* src,
                                   int32_t* keep_count, void* workspace, size_t workspace_bytes, void* stream) {
  if (int rc = od_soft_cfg_check("od_slice_merge_soft", cfg, K)) return rc;
  return slice_merge("od_slice_merge_soft", ctx, keys, counts, boxes, tiles, edges, G, T, P, NC, K, edge_lo, edge_hi,
                     cfg->iou_threshold, cfg->strict, cfg->max_det, cfg, vote_iou, out, src, keep_count, workspace,
                     workspace_bytes, stream);
}
