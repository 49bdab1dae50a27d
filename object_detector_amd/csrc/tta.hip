// Test-time augmentation: the mirror of the network input (od_hflip_u8) and the merge of the per-view candidate lists into
// ONE NMS + box voting (od_tta_merge).  DESIGN.md "Flip test-time augmentation" freezes the semantics; tests/tta_ref.py is
// their numpy restatement and tests/test_gpu_tta.py compares the two bit for bit.
//
// od_tta_merge is latency-bound (one workgroup of work per image, like od_detect_refine_sort) and takes three launches:
//   rank   (od_tta_merge_rank)  one workgroup per image.  Every view's list arrives sorted, so a candidate's place in the
//          merged order (conf bits desc, view asc, flat asc) is its own position plus, per other view, a binary-searched
//          count of the entries that precede it (merge path; no sort).  The first Km = min(K, sum counts) are written in
//          rank order as exactly what od_nms_sort leaves behind: box (un-mirrored), class, and the key re-made with the
//          flat index rank * NC + class, so the order is preserved and the scan's keep_flat / NC is the merged rank
//   od_nms_greedy_k   the suppression launch of od_nms, unchanged (nms.hip), on that table
//   vote   (od_tta_vote_gather)  one workgroup per image, the merged table in LDS: the waves ballot every kept candidate's
//          member set, then one thread per kept candidate accumulates conf_j and conf_j * box_j over its members in ascending
//          rank; writes the record block, the (view, flat) sources and the padding
// od_tta_merge_soft is the same three launches with the soft scan (od_soft_scan_k, soft_nms.hip) in the middle: the vote kernel
// then reports the scan's rescored confidence for every kept row (its votes still weigh the original confidences).
// Nothing in the workspace carries over from call to call (every word that is read was written by this call).
// Compiled with -ffp-contract=off: the mirror, the IoU predicate and the voting sums are one rounding per op, as numpy's.
#include "post_common.h"

namespace {

constexpr int TTA_MAX_VIEWS = 8;
constexpr int TTA_MAX_K = 1024;

struct TtaViews {
  const u64* keys[TTA_MAX_VIEWS];
  const int* counts[TTA_MAX_VIEWS];
  const float* boxes[TTA_MAX_VIEWS];
  int P[TTA_MAX_VIEWS];
  int flip[TTA_MAX_VIEWS];
  int V;
};

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

// ---- od_tta_merge ---------------------------------------------------------------------------------------------------
// grid B, 1024 threads: thread r owns entry r of every view's list (K <= 1024).
__global__ __launch_bounds__(1024) void od_tta_merge_rank(TtaViews vw, int NC, int K, int KP, u64* __restrict__ skeys,
                                                          f32x4* __restrict__ sbox, int* __restrict__ scls,
                                                          int* __restrict__ msrc, int* __restrict__ mcount) {
  __shared__ unsigned lconf[TTA_MAX_VIEWS * TTA_MAX_K];  // conf bits of every list, descending
  __shared__ int lcnt[TTA_MAX_VIEWS];
  const int b = blockIdx.x, tid = threadIdx.x, V = vw.V;
  if (tid < TTA_MAX_VIEWS) lcnt[tid] = tid < V ? min(max(vw.counts[tid][b], 0), K) : 0;
  __syncthreads();
  u64 mykey[TTA_MAX_VIEWS];
#pragma unroll
  for (int v = 0; v < TTA_MAX_VIEWS; ++v) {
    mykey[v] = 0ull;
    if (v < V && tid < lcnt[v]) {
      mykey[v] = vw.keys[v][(long long)b * K + tid];
      lconf[v * TTA_MAX_K + tid] = od_key_score_bits(mykey[v]);
    }
  }
  __syncthreads();
  if (tid == 0) {
    int total = 0;
    for (int v = 0; v < V; ++v) total += lcnt[v];
    mcount[b] = min(K, total);
  }
#pragma unroll
  for (int v = 0; v < TTA_MAX_VIEWS; ++v) {
    if (v >= V || tid >= lcnt[v]) continue;
    const unsigned cb = od_key_score_bits(mykey[v]);
    int rank = tid;
    for (int u = 0; u < V; ++u) {
      if (u == v) continue;
      // entries of list u that precede (cb, v): conf > cb, and conf == cb too when u < v
      const unsigned* lu = lconf + u * TTA_MAX_K;
      int lo = 0, hi = lcnt[u];
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        const unsigned x = lu[mid];
        if (u < v ? x >= cb : x > cb) lo = mid + 1; else hi = mid;
      }
      rank += lo;
    }
    if (rank >= K) continue;
    const unsigned flat = od_key_flat(mykey[v]);
    unsigned p = flat / (unsigned)NC;
    const unsigned c = flat - p * (unsigned)NC;
    p = min(p, (unsigned)(vw.P[v] - 1));  // a malformed key must not read outside the view's box table
    f32x4 bx = *(const f32x4*)(vw.boxes[v] + ((long long)b * vw.P[v] + p) * 4);
    if (vw.flip[v]) {
      const float x1 = 1.f - bx[2], x2 = 1.f - bx[0];
      bx[0] = x1;
      bx[2] = x2;
    }
    const long long o = (long long)b * KP + rank;
    skeys[o] = od_make_key(cb, (unsigned)(rank * NC + (int)c));
    sbox[o] = bx;
    scls[o] = (int)c;
    msrc[o * 2] = v;
    msrc[o * 2 + 1] = (int)flat;
  }
}

// grid B, 1024 threads.  Kept detections are taken 256 at a time (max_det <= 256: one round).  Phase 1, voting only: the 16
// waves share the round's kept detections; a wave tests 64 merged candidates per step against its detection and ballots the
// membership word, so the 1024 predicates of a detection are 16 steps instead of a serial loop.  Phase 2: one kept detection
// per thread walks ONLY its members, in ascending rank (the order that fixes the rounding), and writes record, source, padding.
// keep_conf (optional) [B, keep_stride]: the confidence to report for every kept row instead of its key's (the soft scan's
// rescored one); the votes are weighted by the keys' confidences either way.
constexpr int TTA_ROUND = 256;
constexpr int TTA_MW = TTA_MAX_K / 64 + 1;  // mask row pitch in words: 17 spreads a column of rows over the LDS banks

__global__ __launch_bounds__(1024) void od_tta_vote_gather(const u64* __restrict__ skeys, const f32x4* __restrict__ sbox,
                                                           const int* __restrict__ scls, const int* __restrict__ msrc,
                                                           const int* __restrict__ mcount, const int* __restrict__ keepf,
                                                           const int* __restrict__ keep_count,
                                                           const float* __restrict__ keep_conf, int NC, int KP, int keep_stride,
                                                           int max_det, float vote_iou, float* __restrict__ out,
                                                           int* __restrict__ src) {
  __shared__ f32x4 lb[TTA_MAX_K];
  __shared__ int lc[TTA_MAX_K];
  __shared__ float lw[TTA_MAX_K];
  __shared__ int lrank[TTA_ROUND];
  __shared__ u64 lmask[TTA_ROUND * TTA_MW];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int n = min(mcount[b], KP), nk = min(keep_count[b], max_det);
  const int W = (n + 63) >> 6;
  for (int i = tid; i < n; i += 1024) {
    lb[i] = sbox[(long long)b * KP + i];
    lc[i] = scls[(long long)b * KP + i];
    lw[i] = __uint_as_float(od_key_score_bits(skeys[(long long)b * KP + i]));
  }
  float* o = out + (size_t)b * (1 + 6 * (size_t)max_det);
  if (tid == 0) o[0] = __int_as_float(nk);
  for (int r0 = 0; r0 < max_det; r0 += TTA_ROUND) {
    const int nr = min(TTA_ROUND, nk - r0);  // kept detections of this round (<= 0: padding only)
    if (tid < nr)  // merged rank of kept detection r0 + tid
      lrank[tid] = min(max(keepf[(long long)b * keep_stride + r0 + tid] / NC, 0), n - 1);
    __syncthreads();  // (first round: also the table above)
    if (vote_iou > 0.f) {
      for (int q = wv; q < nr; q += 16) {  // wave-uniform
        const int i = lrank[q];
        const f32x4 a = lb[i];
        const int ci = lc[i];
        const float area_a = (a[2] - a[0]) * (a[3] - a[1]);
        for (int w = 0; w < W; ++w) {
          const int j = w * 64 + lane;
          const bool hit = j < n && (j == i || (lc[j] == ci && od_iou_exceeds(a, area_a, lb[j], vote_iou)));
          const u64 m = __ballot(hit);
          if (lane == 0) lmask[q * TTA_MW + w] = m;
        }
      }
      __syncthreads();
    }
    const int r = r0 + tid;
    if (tid < TTA_ROUND && r < max_det) {
      float* rec = o + 1 + 6 * (size_t)r;
      int sv = -1, sf = -1;
      if (r < nk) {
        const int i = lrank[tid];
        f32x4 bx = lb[i];
        if (vote_iou > 0.f) {
          float sw = 0.f, s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
          for (int w = 0; w < W; ++w) {
            u64 m = lmask[tid * TTA_MW + w];
            while (m) {  // members in ascending rank
              const int j = w * 64 + __builtin_ctzll(m);
              m &= m - 1ull;
              const f32x4 c = lb[j];
              const float cw = lw[j];
              sw += cw;
              s0 += cw * c[0];
              s1 += cw * c[1];
              s2 += cw * c[2];
              s3 += cw * c[3];
            }
          }
          bx = f32x4{s0 / sw, s1 / sw, s2 / sw, s3 / sw};
        }
        rec[0] = __int_as_float(lc[i]);
        rec[1] = keep_conf ? keep_conf[(long long)b * keep_stride + r] : lw[i];  // the soft scan's rescored confidence
        rec[2] = bx[0];
        rec[3] = bx[1];
        rec[4] = bx[2];
        rec[5] = bx[3];
        sv = msrc[((long long)b * KP + i) * 2];
        sf = msrc[((long long)b * KP + i) * 2 + 1];
      } else {
        rec[0] = __int_as_float(-1);
        rec[1] = rec[2] = rec[3] = rec[4] = rec[5] = 0.f;
      }
      if (src) {
        src[((size_t)b * max_det + r) * 2] = sv;
        src[((size_t)b * max_det + r) * 2 + 1] = sf;
      }
    }
    __syncthreads();  // the next round overwrites lrank / lmask
  }
}

int tta_kp(int K) {
  int p = 64;
  while (p < K) p <<= 1;
  return p;
}

struct TtaLayout {
  size_t nms, mcount, msrc, keepf, total;
};
TtaLayout tta_layout(int B, int K) {
  const size_t a = 255;
  TtaLayout l;
  size_t o = 0;
  l.nms = o;
  o += (od_nms_workspace_bytes(B, K) + a) & ~a;
  l.mcount = o;
  o += ((size_t)B * 4 + a) & ~a;
  l.msrc = o;
  o += ((size_t)B * tta_kp(K) * 8 + a) & ~a;
  l.keepf = o;
  o += ((size_t)B * K * 4 + a) & ~a;
  l.total = o;
  return l;
}

}  // namespace

size_t od_merge_workspace_bytes(int B, int K) { return tta_layout(B, K).total; }

OdMergeWs od_merge_workspace(void* workspace, int B, int K) {
  const TtaLayout l = tta_layout(B, K);
  char* ws = (char*)workspace;
  return OdMergeWs{ws + l.nms, (int*)(ws + l.mcount), (int*)(ws + l.msrc), (int*)(ws + l.keepf)};
}

int od_merge_nms_vote_launch(const OdMergeWs& w, int B, int NC, int K, float iou_threshold, int strict, int max_det,
                             float vote_iou, float* out, int32_t* src, int32_t* keep_count, hipStream_t s,
                             const od_soft_nms_cfg* soft) {
  u64* skeys;
  f32x4* sbox;
  int* scls;
  int KP;
  od_nms_sorted_buffers(w.nms, B, K, &skeys, &sbox, &scls, &KP);
  const int md = max_det < K ? max_det : K;  // at most Km <= K are ever kept: the scan's list needs no more slots
  const float* keep_conf = nullptr;
  if (soft) {
    od_soft_nms_cfg cfg = *soft;
    cfg.max_det = md;
    float* kc = od_nms_scratch(w.nms, B, K);  // [B, md]
    if (int rc = od_soft_scan_launch(w.nms, w.mcount, B, K, cfg, w.keepf, kc, keep_count, nullptr, s)) return rc;
    keep_conf = kc;
  } else if (int rc = od_nms_greedy_launch(w.nms, w.mcount, B, K, iou_threshold, strict, md, w.keepf, keep_count, s)) {
    return rc;
  }
  hipLaunchKernelGGL(od_tta_vote_gather, dim3(B), dim3(1024), 0, s, skeys, sbox, scls, w.msrc, w.mcount, w.keepf, keep_count,
                     keep_conf, NC, KP, md, max_det, vote_iou, out, src);
  OD_CHECK_LAUNCH();
  return OD_OK;
}

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

extern "C" size_t od_tta_merge_workspace_bytes(int B, int V, int K) {
  if (B <= 0 || V < 1 || V > TTA_MAX_VIEWS || K <= 0 || K > TTA_MAX_K) return 0;
  return od_merge_workspace_bytes(B, K);  // the merged table holds K candidates however many views feed it
}

// od_tta_merge (soft null) and od_tta_merge_soft: the rank kernel, then the greedy or the soft scan, then vote-and-gather
static int tta_merge(const char* who, od_ctx* ctx, const od_tta_view* views, int V, int B, int NC, int K, float iou_threshold,
                     int strict, int max_det, const od_soft_nms_cfg* soft, float vote_iou, float* out, int32_t* src,
                     int32_t* keep_count, void* workspace, size_t workspace_bytes, void* stream) {
  OD_REQUIRE(ctx && views && out && keep_count && workspace, "%s: null argument", who);
  OD_REQUIRE(V >= 1 && V <= TTA_MAX_VIEWS, "%s: V = %d outside 1..%d", who, V, TTA_MAX_VIEWS);
  OD_REQUIRE(NC >= 1 && NC <= OD_MAX_NC, "%s: NC = %d outside the supported class counts 1..%d", who, NC, OD_MAX_NC);
  OD_REQUIRE(B > 0 && B <= 65535 && K > 0 && K <= TTA_MAX_K && max_det > 0, "%s: bad dims (K <= 1024)", who);
  TtaViews vw = {};
  vw.V = V;
  for (int v = 0; v < V; ++v) {
    OD_REQUIRE(views[v].keys && views[v].counts && views[v].boxes, "%s: view %d has a null pointer", who, v);
    OD_REQUIRE(views[v].P > 0 && (long long)views[v].P * NC < (1LL << 31), "%s: view %d: P * NC must fit 31 bits", who, v);
    vw.keys[v] = (const u64*)views[v].keys;
    vw.counts[v] = views[v].counts;
    vw.boxes[v] = views[v].boxes;
    vw.P[v] = views[v].P;
    vw.flip[v] = views[v].flip != 0;
  }
  const size_t need = od_merge_workspace_bytes(B, K);
  if (workspace_bytes < need) {
    od_set_error("%s: workspace %zu < %zu bytes", who, workspace_bytes, need);
    return OD_ERR_WORKSPACE;
  }
  const OdMergeWs w = od_merge_workspace(workspace, B, K);
  u64* skeys;
  f32x4* sbox;
  int* scls;
  int KP;
  od_nms_sorted_buffers(w.nms, B, K, &skeys, &sbox, &scls, &KP);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(od_tta_merge_rank, dim3(B), dim3(1024), 0, s, vw, NC, K, KP, skeys, sbox, scls, w.msrc, w.mcount);
  OD_CHECK_LAUNCH();
  return od_merge_nms_vote_launch(w, B, NC, K, iou_threshold, strict, max_det, vote_iou, out, src, keep_count, s, soft);
}

extern "C" int od_tta_merge(od_ctx* ctx, const od_tta_view* views, int V, int B, int NC, int K, float iou_threshold,
                            int strict, int max_det, float vote_iou, float* out, int32_t* src, int32_t* keep_count,
                            void* workspace, size_t workspace_bytes, void* stream) {
  return tta_merge("od_tta_merge", ctx, views, V, B, NC, K, iou_threshold, strict, max_det, nullptr, vote_iou, out, src,
                   keep_count, workspace, workspace_bytes, stream);
}

extern "C" int od_tta_merge_soft(od_ctx* ctx, const od_tta_view* views, int V, int B, int NC, int K, const od_soft_nms_cfg* cfg,
                                 float vote_iou, float* out, int32_t* src, int32_t* keep_count, void* workspace,
                                 size_t workspace_bytes, void* stream) {
  if (int rc = od_soft_cfg_check("od_tta_merge_soft", cfg, K)) return rc;
  return tta_merge("od_tta_merge_soft", ctx, views, V, B, NC, K, cfg->iou_threshold, cfg->strict, cfg->max_det, cfg, vote_iou,
                   out, src, keep_count, workspace, workspace_bytes, stream);
}
