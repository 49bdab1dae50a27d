// The merged candidate table: the sorted top-K lists of several passes over one image -- the views of test-time
// augmentation (od_tta_merge) or the tiles of sliced inference (od_slice_merge) -- merged into ONE NMS + box voting.
// DESIGN.md "Flip test-time augmentation" and "Sliced inference" freeze the semantics; tests/tta_ref.py and
// tests/slice_ref.py are their numpy restatements and tests/test_gpu_tta.py / test_gpu_slice_merge.py compare bit for bit.
//
// A merge is latency-bound (one workgroup of work per image, like od_detect_refine_sort) and takes three launches:
//   rank   (od_merge_rank<Src>)  one workgroup of 1024 threads per image, thread r owns entry r of every list.  A source may
//          drop entries (the tiles' interior-edge rule); the survivors of each list are compacted in order (ballot + prefix
//          over the 16 waves), so the lists stay sorted and a survivor's place in the merged order (conf bits desc, list asc,
//          flat asc) is its compacted position plus, per other list, a binary-searched count of the entries that precede it
//          (merge path; no sort) -- a dropped entry is in no list and cannot disturb a rank.  The first Km = min(K, survivors)
//          are written in rank order as exactly what od_nms_sort leaves behind: box (mapped to image coordinates), class, and
//          the key re-made with the flat index rank * NC + class, so the order is preserved and the scan's keep_flat / NC is
//          the merged rank
//   od_nms_greedy_k   the suppression launch of od_nms, unchanged (nms.hip), on that table
//   vote   (od_tta_vote_gather)  one workgroup per image, the merged table in LDS: the waves ballot every kept candidate's
//          member set, then one thread per kept candidate accumulates conf_j and conf_j * box_j over its members in ascending
//          rank; writes the record block, the (list, flat) sources and the padding
// The _soft entries are the same three launches with the soft scan (od_soft_scan_k, soft_nms.hip) in the middle: the vote
// kernel then reports the scan's rescored confidence for every kept row (its votes still weigh the original confidences).
// Nothing in the workspace carries over from call to call (every word that is read was written by this call).
// Compiled with -ffp-contract=off: the box maps, the IoU predicate and the voting sums are one rounding per op, as numpy's.
#include "post_common.h"

namespace {

// ---- list sources -----------------------------------------------------------------------------------------------------
// What od_merge_rank<Src> asks of a source: MAX_LISTS (its LDS is sized by it), lists(), list(b, l, K) -> a List with the
// list's count, keys, box table and P (plus whatever the next two need), survives(list, i, NC): whether entry i is ranked
// at all, and map(list, box) -> the box in image coordinates.

// the box entry `flat` of a list points at; a malformed key must not read outside the list's box table
template <class List>
__device__ __forceinline__ f32x4 merge_box(const List& li, unsigned flat, int NC) {
  return li.boxes[min(flat / (unsigned)NC, (unsigned)(li.P - 1))];
}

// the views of od_tta_merge: every view has its own buffers and its own P; nothing is dropped; a flipped view is mirrored
struct ViewSrc {
  static constexpr int MAX_LISTS = 8;
  struct List {
    int count, P;
    const u64* keys;
    const f32x4* boxes;
    int flip;
  };
  const u64* keys[MAX_LISTS];
  const int* counts[MAX_LISTS];
  const float* boxes[MAX_LISTS];
  int P[MAX_LISTS];
  int flip[MAX_LISTS];
  int V;

  __device__ int lists() const { return V; }
  __device__ List list(int b, int l, int K) const {
    return List{counts[l][b], P[l], keys[l] + (long long)b * K, (const f32x4*)boxes[l] + (long long)b * P[l], flip[l]};
  }
  __device__ bool survives(const List&, int, int) const { return true; }
  __device__ f32x4 map(const List& li, f32x4 bx) const {
    if (li.flip) {  // the mirror itself, not an affine map: 1 - x is one rounding
      const float x1 = 1.f - bx[2], x2 = 1.f - bx[0];
      bx[0] = x1;
      bx[2] = x2;
    }
    return bx;
  }
};

// the tiles of od_slice_merge: list t of image g is batch row g * T + t; a candidate cut at a seam (its box touches an
// interior side of its tile) is dropped, edge_lo < 0 disables that; tile coordinates map to the image by (ox, oy, sx, sy)
constexpr int SL_LEFT = 1, SL_TOP = 2, SL_RIGHT = 4, SL_BOTTOM = 8;  // interior sides of a tile (slicing.edges)

struct TileSrc {
  static constexpr int MAX_LISTS = 16;
  struct List {
    int count, P;
    const u64* keys;
    const f32x4* boxes;
    int edges;
    const f32x4* affine;
  };
  const u64* keys;
  const int* counts;
  const float* boxes;
  const float* tiles;
  const int* edges;
  int T, P;
  float edge_lo, edge_hi;

  __device__ int lists() const { return T; }
  __device__ List list(int g, int l, int K) const {
    const long long row = (long long)g * T + l;
    return List{counts[row], P, keys + row * K, (const f32x4*)boxes + row * P, edge_lo >= 0.f ? edges[row] : 0,
                (const f32x4*)tiles + row};
  }
  __device__ bool survives(const List& li, int i, int NC) const {
    const int e = li.edges;
    if (!e) return true;
    const f32x4 bx = merge_box(li, od_key_flat(li.keys[i]), NC);
    return !(((e & SL_LEFT) && bx[0] <= edge_lo) || ((e & SL_TOP) && bx[1] <= edge_lo) ||
             ((e & SL_RIGHT) && bx[2] >= edge_hi) || ((e & SL_BOTTOM) && bx[3] >= edge_hi));
  }
  __device__ f32x4 map(const List& li, const f32x4& bx) const {
    const f32x4 a = *li.affine;
    f32x4 m;
    m[0] = fminf(fmaxf(a[0] + a[2] * bx[0], 0.f), 1.f);
    m[1] = fminf(fmaxf(a[1] + a[3] * bx[1], 0.f), 1.f);
    m[2] = fminf(fmaxf(a[0] + a[2] * bx[2], 0.f), 1.f);
    m[3] = fminf(fmaxf(a[1] + a[3] * bx[3], 0.f), 1.f);
    return m;
  }
};

// ---- rank ---------------------------------------------------------------------------------------------------------------
// grid B, 1024 threads: thread r owns entry r of every list (K <= OD_MERGE_MAX_K).  What a thread knows about its entries
// lives in LDS (one byte each: the survivors of its wave before it, or MERGE_DROPPED), not in registers: the loops over the
// lists stay rolled, and the keys are read again where they are needed (they sit in L2).
constexpr unsigned char MERGE_DROPPED = 0xFF;

template <class Src>
__global__ __launch_bounds__(1024) void od_merge_rank(const Src src, int NC, int K, int KP, u64* __restrict__ skeys,
                                                      f32x4* __restrict__ sbox, int* __restrict__ scls,
                                                      int* __restrict__ msrc, int* __restrict__ mcount) {
  constexpr int ML = Src::MAX_LISTS;
  __shared__ unsigned lconf[ML * OD_MERGE_MAX_K];      // conf bits of every compacted list, descending
  __shared__ unsigned char lpre[ML * OD_MERGE_MAX_K];  // per entry: survivors of its wave before it, or MERGE_DROPPED
  __shared__ int wtot[ML * 16];                        // survivors per (list, wave)
  __shared__ int wpre[ML * 16];                        // survivors of the list in the waves before this one
  __shared__ int lcnt[ML];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int L = src.lists();
  for (int l = 0; l < L; ++l) {
    const typename Src::List li = src.list(b, l, K);
    const bool keep = tid < min(max(li.count, 0), K) && src.survives(li, tid, NC);
    const u64 m = __ballot(keep);
    lpre[l * OD_MERGE_MAX_K + tid] = keep ? (unsigned char)__popcll(m & ((1ull << lane) - 1ull)) : MERGE_DROPPED;
    if (lane == 0) wtot[l * 16 + wv] = __popcll(m);
  }
  __syncthreads();
  if (tid < L * 16) {  // (list, wave) = (tid / 16, tid % 16)
    const int base = tid & ~15;
    int pre = 0;
    for (int w = 0; w < (tid & 15); ++w) pre += wtot[base + w];
    wpre[tid] = pre;
    if ((tid & 15) == 15) lcnt[tid >> 4] = pre + wtot[tid];
  }
  __syncthreads();
  for (int l = 0; l < L; ++l) {  // the compacted lists: order kept, so still sorted
    const unsigned char v = lpre[l * OD_MERGE_MAX_K + tid];
    if (v != MERGE_DROPPED)
      lconf[l * OD_MERGE_MAX_K + wpre[l * 16 + wv] + v] = od_key_score_bits(src.list(b, l, K).keys[tid]);
  }
  __syncthreads();
  if (tid == 0) {
    int total = 0;
    for (int l = 0; l < L; ++l) total += lcnt[l];
    mcount[b] = min(K, total);
  }
  for (int l = 0; l < L; ++l) {
    const unsigned char v = lpre[l * OD_MERGE_MAX_K + tid];
    if (v == MERGE_DROPPED) continue;
    const int pos = wpre[l * 16 + wv] + v;  // position in the compacted list
    const unsigned cb = lconf[l * OD_MERGE_MAX_K + pos];
    int rank = pos;
    for (int u = 0; u < L; ++u) {
      if (u == l) continue;
      // entries of list u that precede (cb, l): conf > cb, and conf == cb too when u < l
      const unsigned* lu = lconf + u * OD_MERGE_MAX_K;
      int lo = 0, hi = lcnt[u];
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        const unsigned x = lu[mid];
        if (u < l ? x >= cb : x > cb) lo = mid + 1; else hi = mid;
      }
      rank += lo;
    }
    if (rank >= K) continue;
    const typename Src::List li = src.list(b, l, K);
    const unsigned flat = od_key_flat(li.keys[tid]);
    const unsigned c = flat % (unsigned)NC;
    const long long o = (long long)b * KP + rank;
    skeys[o] = od_make_key(cb, (unsigned)(rank * NC + (int)c));
    sbox[o] = src.map(li, merge_box(li, flat, NC));
    scls[o] = (int)c;
    msrc[o * 2] = l;
    msrc[o * 2 + 1] = (int)flat;
  }
}

// ---- vote and gather ------------------------------------------------------------------------------------------------------
// grid B, 1024 threads.  Kept detections are taken 256 at a time (max_det <= 256: one round).  Phase 1, voting only: the 16
// waves share the round's kept detections; a wave tests 64 merged candidates per step against its detection and ballots the
// membership word, so the 1024 predicates of a detection are 16 steps instead of a serial loop.  Phase 2: one kept detection
// per thread walks ONLY its members, in ascending rank (the order that fixes the rounding), and writes record, source, padding.
// keep_conf (optional) [B, keep_stride]: the confidence to report for every kept row instead of its key's (the soft scan's
// rescored one); the votes are weighted by the keys' confidences either way.
constexpr int TTA_ROUND = 256;
constexpr int TTA_MW = OD_MERGE_MAX_K / 64 + 1;  // mask row pitch in words: 17 spreads a column of rows over the LDS banks

__global__ __launch_bounds__(1024) void od_tta_vote_gather(const u64* __restrict__ skeys, const f32x4* __restrict__ sbox,
                                                           const int* __restrict__ scls, const int* __restrict__ msrc,
                                                           const int* __restrict__ mcount, const int* __restrict__ keepf,
                                                           const int* __restrict__ keep_count,
                                                           const float* __restrict__ keep_conf, int NC, int KP, int keep_stride,
                                                           int max_det, float vote_iou, float* __restrict__ out,
                                                           int* __restrict__ src) {
  __shared__ f32x4 lb[OD_MERGE_MAX_K];
  __shared__ int lc[OD_MERGE_MAX_K];
  __shared__ float lw[OD_MERGE_MAX_K];
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

// ---- workspace --------------------------------------------------------------------------------------------------------
// od_nms's workspace, the merged count [B], the (list, flat) source of every merged rank [B,KP,2] and the scan's kept list
// [B,K], each 256-byte aligned.  The merged table holds K candidates however many lists feed it.
struct OdMergeWs {
  void* nms;
  int* mcount;
  int* msrc;
  int* keepf;
  size_t bytes;
};

OdMergeWs od_merge_workspace(void* workspace, int B, int K) {
  const size_t a = 255;
  int KP = 64;  // od_nms's row pitch: the next power of two >= K
  while (KP < K) KP <<= 1;
  const uintptr_t ws = (uintptr_t)workspace;
  OdMergeWs w;
  size_t o = 0;
  w.nms = (void*)(ws + o);
  o += (od_nms_workspace_bytes(B, K) + a) & ~a;
  w.mcount = (int*)(ws + o);
  o += ((size_t)B * 4 + a) & ~a;
  w.msrc = (int*)(ws + o);
  o += ((size_t)B * KP * 8 + a) & ~a;
  w.keepf = (int*)(ws + o);
  o += ((size_t)B * K * 4 + a) & ~a;
  w.bytes = o;
  return w;
}

size_t od_merge_workspace_bytes(int B, int lists, int max_lists, int K) {
  if (B <= 0 || lists < 1 || lists > max_lists || K <= 0 || K > OD_MERGE_MAX_K) return 0;
  return od_merge_workspace(nullptr, B, K).bytes;
}

// what follows the rank kernel: the greedy scan, or with soft non-null the soft scan (cfg->iou_threshold / strict / max_det in
// place of the three scalars) and its rescored confidences; then vote-and-gather
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

// every merge entry behind its own checks of `src` (soft null: the greedy scan): the rank kernel, the scan, vote-and-gather
template <class Src>
int merge_run(const char* who, od_ctx* ctx, const Src& src, int B, int NC, int K, float iou_threshold, int strict, int max_det,
              const od_soft_nms_cfg* soft, float vote_iou, float* out, int32_t* out_src, int32_t* keep_count, void* workspace,
              size_t workspace_bytes, void* stream) {
  OD_REQUIRE(ctx && out && keep_count && workspace, "%s: null argument", who);
  OD_REQUIRE(NC >= 1 && NC <= OD_MAX_NC, "%s: NC = %d outside the supported class counts 1..%d", who, NC, OD_MAX_NC);
  OD_REQUIRE(B > 0 && B <= 65535 && K > 0 && K <= OD_MERGE_MAX_K && max_det > 0, "%s: bad dims (K <= %d)", who, OD_MERGE_MAX_K);
  const OdMergeWs w = od_merge_workspace(workspace, B, K);
  if (workspace_bytes < w.bytes) {
    od_set_error("%s: workspace %zu < %zu bytes", who, workspace_bytes, w.bytes);
    return OD_ERR_WORKSPACE;
  }
  u64* skeys;
  f32x4* sbox;
  int* scls;
  int KP;
  od_nms_sorted_buffers(w.nms, B, K, &skeys, &sbox, &scls, &KP);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(od_merge_rank<Src>, dim3(B), dim3(1024), 0, s, src, NC, K, KP, skeys, sbox, scls, w.msrc, w.mcount);
  OD_CHECK_LAUNCH();
  return od_merge_nms_vote_launch(w, B, NC, K, iou_threshold, strict, max_det, vote_iou, out, out_src, keep_count, s, soft);
}

int tta_merge(const char* who, od_ctx* ctx, const od_tta_view* views, int V, int B, int NC, int K, float iou_threshold,
              int strict, int max_det, const od_soft_nms_cfg* soft, float vote_iou, float* out, int32_t* src,
              int32_t* keep_count, void* workspace, size_t workspace_bytes, void* stream) {
  OD_REQUIRE(views, "%s: null argument", who);
  OD_REQUIRE(V >= 1 && V <= ViewSrc::MAX_LISTS, "%s: V = %d outside 1..%d", who, V, ViewSrc::MAX_LISTS);
  ViewSrc vs = {};
  vs.V = V;
  for (int v = 0; v < V; ++v) {
    OD_REQUIRE(views[v].keys && views[v].counts && views[v].boxes, "%s: view %d has a null pointer", who, v);
    OD_REQUIRE(views[v].P > 0 && (long long)views[v].P * NC < (1LL << 31), "%s: view %d: P * NC must fit 31 bits", who, v);
    vs.keys[v] = (const u64*)views[v].keys;
    vs.counts[v] = views[v].counts;
    vs.boxes[v] = views[v].boxes;
    vs.P[v] = views[v].P;
    vs.flip[v] = views[v].flip != 0;
  }
  return merge_run(who, ctx, vs, B, NC, K, iou_threshold, strict, max_det, soft, vote_iou, out, src, keep_count, workspace,
                   workspace_bytes, stream);
}

int slice_merge(const char* who, od_ctx* ctx, const uint64_t* keys, const int32_t* counts, const float* boxes,
                const float* tiles, const int32_t* edges, int G, int T, int P, int NC, int K, float edge_lo, float edge_hi,
                float iou_threshold, int strict, int max_det, const od_soft_nms_cfg* soft, float vote_iou, float* out,
                int32_t* src, int32_t* keep_count, void* workspace, size_t workspace_bytes, void* stream) {
  OD_REQUIRE(keys && counts && boxes && tiles && edges, "%s: null argument", who);
  OD_REQUIRE(T >= 1 && T <= TileSrc::MAX_LISTS, "%s: T = %d outside 1..%d", who, T, TileSrc::MAX_LISTS);
  OD_REQUIRE(P > 0 && (long long)P * NC < (1LL << 31), "%s: P * NC must fit 31 bits", who);
  const TileSrc ts = {(const u64*)keys, counts, boxes, tiles, edges, T, P, edge_lo, edge_hi};
  return merge_run(who, ctx, ts, G, NC, K, iou_threshold, strict, max_det, soft, vote_iou, out, src, keep_count, workspace,
                   workspace_bytes, stream);
}

}  // namespace

extern "C" size_t od_tta_merge_workspace_bytes(int B, int V, int K) {
  return od_merge_workspace_bytes(B, V, ViewSrc::MAX_LISTS, K);
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

extern "C" size_t od_slice_merge_workspace_bytes(int G, int T, int K) {
  return od_merge_workspace_bytes(G, T, TileSrc::MAX_LISTS, K);
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
