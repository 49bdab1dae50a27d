// The product path of K5-K8 as ONE call (od_detect): pred -> boxes + exact top-K + NMS kept indices in three launches, without
// materialising the confidence tensor.
//
// Round 2 ran od_head_postprocess (writes conf f32 [B,P,NC]: 43 MB at 32 x 320^2), od_topk_scores (two full passes over conf:
// histogram, partition) and od_nms -- 9 kernels + 2 memsets and 194 MB of HBM traffic per batch.  Here:
//   pass 1  (od_detect_pass1)  reads pred once: 256 rows in LDS at an odd pitch, one thread per row; decoded boxes out, the
//           4096-bin first-digit histogram of all scores (LDS atomics -> global), and ONE float per prior: its largest
//           confidence (rowmax)
//   pass 2  (od_detect_pass2)  finds the first digit d0 of the K-th key from the histogram, then reads rowmax and recomputes
//           (od_row_conf again: bit-identical) the confidences of ONLY the priors whose best score reaches the d0 bin -- a
//           fraction of a percent of them -- and partitions those into winners (digit > d0) and the d0-bin candidate list, as
//           64-bit keys
//   tail    (od_detect_tail)  one workgroup per image: od_radix_refine inside the d0 bin on the remaining <= 51 key bits,
//           od_bitonic_sort_desc of the K winners in LDS, od_rank_gather of their boxes / classes, counts; re-zeroes the
//           histogram; then od_nms_greedy on the candidates still in LDS.  All four are topk_common.h's, shared with topk.hip,
//           nms.hip and detect_wide.hip.  od_detect_refine_sort is the same kernel without the last step
// Same total order, same exact selection, same kept indices as the three-call path (tests compare them bit for bit).
// od_detect_candidates is the same call with od_detect_refine_sort for a tail (boxes, sorted keys, counts): one view of
// od_tta_merge (merge.hip).
// Compiled with -ffp-contract=off like post.hip / topk.hip / nms.hip.  NC <= 76 (256 whole rows in LDS); larger class counts
// take the streamed kernels of detect_wide.hip through the same entry points, and od_nms's suppression launch after them.
#include <string.h>

#include "post_common.h"

namespace {

constexpr int NB = OD_TOPK_NB;
constexpr int DT_ROWS = OD_DT_ROWS, DT2_RPT = OD_DT2_RPT;  // priors per workgroup in pass 1 / per thread in pass 2
constexpr int DT_CAND_CAP = 1024; // d0-bin candidates a workgroup compacts in LDS before falling back to global atomics

constexpr int dt_row_pitch(int C) { return C | 1; }  // LDS row pitch in floats, odd: a thread walking its own row meets no other

// The workgroup's nel = nrows * C contiguous floats at src go to rows [nrows][CS] in LDS, V floats per global load (V = 4, 2:
// src is V * 4-byte aligned; 1: it is not), eight loads in flight per thread before the first LDS store: one round trip to
// memory for rows of up to 32 floats instead of one per load.  A load past the last whole vector is clamped onto it (and not
// stored), so no load sits under a branch.  (r, c) walk along with the element index instead of being divided out of it.
template <int V>
__device__ __forceinline__ void dt_stage_rows(const float* __restrict__ src, int nel, int C, int CS, float* rows) {
  typedef float vec __attribute__((ext_vector_type(V)));
  constexpr int U = 8;
  const int nfull = nel & ~(V - 1);  // >= V: a workgroup has at least two rows of at least 7 floats
  const int step = 256 * V, dr = step / C, dc = step - dr * C;
  int i = threadIdx.x * V, r = i / C, c = i - r * C;
  for (; i < nfull; i += U * step) {
    vec t[U];
#pragma unroll
    for (int u = 0; u < U; ++u) t[u] = *(const vec*)(src + min(i + u * step, nfull - V));
#pragma unroll
    for (int u = 0; u < U; ++u) {
      int rr = r, cc = c;
#pragma unroll
      for (int e = 0; e < V; ++e) {
        if (i + u * step < nfull) rows[rr * CS + cc] = t[u][e];
        if (++cc == C) cc = 0, ++rr;
      }
      r += dr, c += dc;
      if (c >= C) c -= C, ++r;
    }
  }
  const int e = nfull + threadIdx.x;  // the last nel % V floats
  if (e < nel) rows[(e / C) * CS + (e - (e / C) * C)] = src[e];
}

// grid (ceil(P / 256), B).  LDS: rows [256][C | 1] f32 + hist[4096].  NCT: the class count at compile time (the loops over
// classes unroll and the confidences stay in registers), or 0 = NC_rt at run time (computed in place over the class logits in
// LDS).  Either way od_row_conf's operations in od_row_conf's order: the same bits as pass 2's and od_gather_det_pred's.
template <int NCT>
__global__ __launch_bounds__(256) void od_detect_pass1(const float* __restrict__ pred, const float* __restrict__ priors,
                                                       float* __restrict__ boxes, float* __restrict__ rowmax,
                                                       float* __restrict__ conf_out, int* __restrict__ hist,
                                                       TopkState* __restrict__ st, int P, int NC_rt, float loc_scale, int clip,
                                                       float thr, unsigned dbase, int dshift) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int NC = NCT ? NCT : NC_rt;
  const int C = NC + 6, CS = dt_row_pitch(C), tid = threadIdx.x, b = blockIdx.y;
  float* rows = sm;                        // [DT_ROWS][CS]
  int* lh = (int*)(sm + DT_ROWS * CS);     // [NB]
  const int p0 = blockIdx.x * DT_ROWS;
  const int nrows = min(DT_ROWS, P - p0);
  for (int i = tid; i < NB; i += 256) lh[i] = 0;
  if (blockIdx.x == 0 && tid == 0) {  // pass 2 counts into these with atomics
    TopkState z = {0, 0, 0, 0};
    st[b] = z;
  }
  const long long r0 = (long long)b * P + p0;
  // the block's first element sits at float (b * P + p0) * C of pred: a multiple of 4 for even C (P is even, p0 a multiple of
  // 256), but only of 2 for odd C when b * P is 2 mod 4 -- so the load width follows the address
  const float* src = pred + r0 * C;
  const int nel = nrows * C;
  const unsigned mis = (unsigned)(uintptr_t)src & 15u;
  if (mis == 0) {
    dt_stage_rows<4>(src, nel, C, CS, rows);
  } else if ((mis & 7u) == 0) {
    dt_stage_rows<2>(src, nel, C, CS, rows);
  } else {
    dt_stage_rows<1>(src, nel, C, CS, rows);
  }
  __syncthreads();
  if (tid < nrows) {
    float* row = rows + tid * CS;
    const f32x4 loc = {row[2 + NC], row[3 + NC], row[4 + NC], row[5 + NC]};
    float mx = 0.f;
    const auto score = [&](float v) {
      mx = fmaxf(mx, v);
      const unsigned sb = od_score_bits(v, thr);
      if (sb) atomicAdd(&lh[od_digit0(sb, dbase, dshift)], 1);
    };
    if constexpr (NCT > 0) {
      float cf[NCT];
      od_row_conf(row, NCT, cf);
#pragma unroll
      for (int c = 0; c < NCT; ++c) score(cf[c]);
      if (conf_out) {
#pragma unroll
        for (int c = 0; c < NCT; ++c) row[2 + c] = cf[c];
      }
    } else {
      od_row_conf(row, NC, row + 2);
      for (int c = 0; c < NC; ++c) score(row[2 + c]);
    }
    rowmax[r0 + tid] = mx;
    const f32x4 pr = *(const f32x4*)(priors + (long long)(p0 + tid) * 4);
    *(f32x4*)(boxes + (r0 + tid) * 4) = od_decode_one(loc, pr, loc_scale, clip);
  }
  __syncthreads();
  int* gh = hist + (long long)b * NB;
  for (int i = tid; i < NB; i += 256)
    if (lh[i]) atomicAdd(&gh[i], lh[i]);
  if (conf_out) {  // optional dense confidences (API parity with od_head_postprocess; the product path passes NULL)
    float* dst = conf_out + r0 * NC;
    for (int i = tid; i < nrows * NC; i += 256) {
      const int r = i / NC, c = i - r * NC;
      dst[i] = rows[r * CS + 2 + c];
    }
  }
}

// grid (ceil(P / 1024), B).  LDS: per-thread row scratch [256][C] + l_out [K] + l_cand [DT_CAND_CAP] keys.
__global__ __launch_bounds__(256) void od_detect_pass2(const float* __restrict__ pred, const float* __restrict__ rowmax,
                                                       const int* __restrict__ hist, TopkState* __restrict__ st,
                                                       u64* __restrict__ keys, u64* __restrict__ cand, int P, int NC, int K,
                                                       float thr, long long cand_stride, unsigned dbase, int dshift) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int C = NC + 6, tid = threadIdx.x, b = blockIdx.y;
  float* rows = sm;                          // [DT_ROWS][C]
  u64* l_out = (u64*)(sm + DT_ROWS * C);     // [K]   (DT_ROWS * C * 4 bytes is a multiple of 8)
  u64* l_cand = l_out + K;                   // [DT_CAND_CAP]
  __shared__ int n_out, n_cand, n_hot, base_out, base_cand, sh_fd[8];
  __shared__ int hot_list[DT_ROWS * DT2_RPT];
  if (tid == 0) {
    n_out = 0;
    n_cand = 0;
    n_hot = 0;
  }
  int d0, above;
  od_find_digit_256(hist + (long long)b * NB, K, sh_fd, &d0, &above);  // (its barriers also publish n_out / n_cand)
  if (blockIdx.x == 0 && tid == 0) {
    st[b].d0 = d0;  // -1: fewer than K candidates in the whole image -> every candidate is a winner
    st[b].krem = d0 < 0 ? 0 : K - above;
  }
  const int p_base = blockIdx.x * (DT_ROWS * DT2_RPT);
  const int nh = od_compact_hot_priors(rowmax + (long long)b * P, P, p_base, thr, dbase, dshift, d0, hot_list, &n_hot);
  for (int e = tid; e < nh; e += 256) {
    const int p = hot_list[e];
    float* row = rows + tid * C;
    const float* src = pred + ((long long)b * P + p) * C;
    for (int c = 0; c < 2 + NC; ++c) row[c] = src[c];
    od_row_conf(row, NC, row + 2);  // as in pass 1: bit-identical confidences
    for (int c = 0; c < NC; ++c) {
      const unsigned sbc = od_score_bits(row[2 + c], thr);
      if (!sbc) continue;
      const int dg = od_digit0(sbc, dbase, dshift);
      if (dg < d0) continue;
      const unsigned flat = (unsigned)(p * NC + c);
      const u64 key = od_make_key(sbc, flat);
      if (dg > d0) {  // fewer than K of these in the whole image
        l_out[atomicAdd(&n_out, 1)] = key;
      } else {
        const int slot = atomicAdd(&n_cand, 1);
        if (slot < DT_CAND_CAP) {
          l_cand[slot] = key;
        } else {  // a degenerate image (e.g. all scores equal): straight to the global list
          cand[(long long)b * cand_stride + atomicAdd(&st[b].ncand, 1)] = key;
        }
      }
    }
  }
  __syncthreads();
  const int nc = min(n_cand, DT_CAND_CAP);
  if (tid == 0) base_cand = nc ? atomicAdd(&st[b].ncand, nc) : 0;
  od_block_copy_out(l_out, n_out, &st[b].nout, keys + (long long)b * K, &base_out);  // (its barrier publishes base_cand too)
  u64* oc = cand + (long long)b * cand_stride + base_cand;
  for (int j = tid; j < nc; j += 256) oc[j] = l_cand[j];
}

// what one image's refine / sort / gather reads and writes (od_detect_refine_sort and od_detect_tail)
struct RefineArgs {
  const float* boxes;
  TopkState* st;
  u64* keys;
  const u64* cand;
  int *hist, *counts;
  int P, NC, K, KP;
  long long cand_stride;
  u64* skeys;
  f32x4* sbox;
  int* scls;
  unsigned dbase;
  int dshift;
};

// One workgroup (1024 threads) for image blockIdx.x: the winners pass 2 wrote straight to the output, plus the krem best of the
// d0-bin candidate list (od_radix_refine), then sort (s [1024], LDS) + gather for the NMS.  Returns the number of candidates n;
// s[0..n) are their keys in rank order, lbox / lcls (LDS, optional) their boxes / classes, not yet published by a barrier.
__device__ __forceinline__ int dt_refine_sort_gather(const RefineArgs& a, u64* s, f32x4* lbox, int* lcls) {
  __shared__ int n_win;
  const int b = blockIdx.x, tid = threadIdx.x, K = a.K;
  const TopkState t = a.st[b];
  const int nout0 = min(t.nout, K);
  if (tid == 0) n_win = 0;
  // winners that pass 2 wrote straight to the output; the rest of the sort array is empty (key 0 sorts last)
  s[tid] = tid < nout0 ? a.keys[(long long)b * K + tid] : 0ull;
  __syncthreads();
  if (t.d0 >= 0 && t.krem > 0) {
    const u64* ic = a.cand + (long long)b * a.cand_stride;
    od_radix_refine(
        t.ncand, t.ncand, t.krem, a.dbase, a.dshift, [&](int i) { return ic[i]; },
        [&](u64 key) {
          const int slot = nout0 + atomicAdd(&n_win, 1);
          if (slot < K) s[slot] = key;
        });
    __syncthreads();
  }
  od_bitonic_sort_desc(s, a.KP);
  const int n = min(nout0 + n_win, K);
  od_rank_gather(s, n, b, a.boxes, a.P, a.NC, K, a.KP, a.skeys, a.sbox, a.scls, a.keys, a.counts, a.hist, lbox, lcls);
  return n;
}

__global__ __launch_bounds__(1024) void od_detect_refine_sort(const RefineArgs a) {
  __shared__ u64 s[1024];
  dt_refine_sort_gather(a, s, nullptr, nullptr);
}

// The per-image tail of od_detect in one launch, one workgroup (1024 threads) per image: od_detect_refine_sort, then od_nms's
// greedy suppression (od_nms_greedy of topk_common.h: the code od_nms_greedy_k runs) on the n candidates while their keys, boxes
// and classes are still in LDS.  Dynamic LDS: s [1024] keys | boxes [KP] | classes [KP].
__global__ __launch_bounds__(1024) void od_detect_tail(const RefineArgs a, float iou_thr, int strict, int max_det,
                                                       int* __restrict__ keep_flat, int* __restrict__ keep_count) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  u64* s = (u64*)smem;
  f32x4* lb = (f32x4*)(smem + 1024 * 8);
  int* lc = (int*)(lb + a.KP);
  const int b = blockIdx.x;
  const int n = dt_refine_sort_gather(a, s, lb, lc);
  __syncthreads();
  od_nms_greedy(lb, lc, s, n, iou_thr, strict, max_det, keep_flat + (long long)b * max_det, keep_count + b);
}

// one workgroup per image: row r of out[b] = {flat index (int bits), conf, x1, y1, x2, y2} of kept detection r, the
// confidence recomputed from pred by the same code as pass 1
__global__ __launch_bounds__(256) void od_gather_det_pred(const float* __restrict__ pred, const float* __restrict__ boxes,
                                                          const int32_t* __restrict__ keep_flat,
                                                          const int32_t* __restrict__ keep_count, int P, int NC, int max_det,
                                                          float* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int b = blockIdx.x, C = NC + 6;
  const int n = keep_count[b];
  float* o = out + (size_t)b * (1 + 6 * (size_t)max_det);
  if (threadIdx.x == 0) o[0] = __int_as_float(n);
  float* row = sm + threadIdx.x * C;
  for (int r = threadIdx.x; r < max_det; r += 256) {
    float* rec = o + 1 + 6 * (size_t)r;
    if (r < n) {
      const int flat = keep_flat[(size_t)b * max_det + r];
      const int p = flat / NC, c = flat - p * NC;
      const float* src = pred + ((size_t)b * P + p) * C;
      for (int e = 0; e < 2 + NC; ++e) row[e] = src[e];
      od_row_conf(row, NC, row + 2);
      const float* bx = boxes + ((size_t)b * P + p) * 4;
      rec[0] = __int_as_float(flat);
      rec[1] = row[2 + c];
      rec[2] = bx[0];
      rec[3] = bx[1];
      rec[4] = bx[2];
      rec[5] = bx[3];
    } else {
      rec[0] = __int_as_float(-1);
      rec[1] = rec[2] = rec[3] = rec[4] = rec[5] = 0.f;
    }
  }
}

struct DetLayout {
  size_t hist, state, rowmax, cand, total;
  long long cand_stride;
  size_t nhot, hot;  // NC > 76 only (then cand / cand_stride are unused)
};
DetLayout det_layout(int B, int P, int NC) {
  DetLayout l;
  size_t o = 0;
  l.hist = o;
  o += (size_t)B * NB * sizeof(int);
  l.state = o;
  o += ((size_t)B * sizeof(TopkState) + 255) & ~(size_t)255;
  l.rowmax = o;
  o += (((size_t)B * P * sizeof(float)) + 255) & ~(size_t)255;
  if (NC > OD_MAX_LDS_NC) {
    l.cand = 0;
    l.cand_stride = 0;
    l.nhot = o;
    o += ((size_t)B * sizeof(int) + 255) & ~(size_t)255;
    l.hot = o;
    o += (size_t)B * P * sizeof(HotRow);
    l.total = o;
    return l;
  }
  l.nhot = l.hot = 0;
  l.cand = o;
  l.cand_stride = (long long)P * NC;  // worst case: every score of an image sits in the d0 bin
  o += (size_t)B * (size_t)l.cand_stride * sizeof(u64);
  l.total = o;
  return l;
}

}  // namespace

extern "C" size_t od_detect_workspace_bytes(int B, int P, int NC, int K) {
  (void)K;
  if (B <= 0 || P <= 0 || NC <= 0) return 0;
  return det_layout(B, P, NC).total;
}

extern "C" int od_detect_workspace_init(od_ctx* ctx, void* workspace, size_t workspace_bytes, int B, int P, int NC, void* stream) {
  OD_REQUIRE(ctx && workspace && B > 0 && P > 0 && NC > 0, "od_detect_workspace_init: bad argument");
  const DetLayout l = det_layout(B, P, NC);
  if (workspace_bytes < l.total) {
    od_set_error("od_detect_workspace_init: workspace %zu < %zu bytes", workspace_bytes, l.total);
    return OD_ERR_WORKSPACE;
  }
  OD_CHECK_HIP(hipMemsetAsync(workspace, 0, l.rowmax, (hipStream_t)stream));  // histograms + state
  return OD_OK;
}

namespace {
struct NmsArgs {  // what od_detect adds to od_detect_candidates
  float iou_threshold;
  int strict, max_det;
  int32_t *keep_flat, *keep_count;
};

template <int NCT>
int launch_pass1(od_ctx* ctx, dim3 grid, size_t lds, hipStream_t s, const float* pred, const float* priors, float* boxes,
                 float* rowmax, float* conf, int* hist, TopkState* st, int P, int NC, float loc_scale, int clip, float thr,
                 unsigned dbase, int dshift) {
  if (int rc = od_ensure_lds(ctx, (const void*)&od_detect_pass1<NCT>, lds)) return rc;
  hipLaunchKernelGGL(od_detect_pass1<NCT>, grid, dim3(256), lds, s, pred, priors, boxes, rowmax, conf, hist, st, P, NC, loc_scale,
                     clip, thr, dbase, dshift);
  OD_CHECK_LAUNCH();
  return OD_OK;
}

// od_detect (nms given) and od_detect_candidates (nms null), either dispatch: pred -> boxes, sorted keys, counts, the
// rank-ordered keys / boxes / classes in the NMS workspace, and for od_detect the kept indices.  NC <= 76: pass 1, pass 2 and
// od_detect_tail (od_detect) or od_detect_refine_sort (od_detect_candidates).  NC > 76: the three streamed launches of
// detect_wide.hip, whose refine kernel is another one, and for od_detect od_nms's suppression launch behind them.
int detect_launch(od_ctx* ctx, const char* who, const float* pred, const float* priors, int B, int P, int NC, float loc_scale,
                  int clip, float conf_threshold, int K, float* boxes, float* conf, uint64_t* keys, int32_t* counts,
                  void* workspace, size_t workspace_bytes, void* nms_workspace, size_t nms_workspace_bytes, const NmsArgs* nms,
                  hipStream_t s) {
  OD_REQUIRE(NC >= 1 && NC <= OD_MAX_NC, "%s: NC = %d outside the supported class counts 1..%d", who, NC, OD_MAX_NC);
  OD_REQUIRE(B > 0 && B <= 65535 && P > 0 && P % 2 == 0 && K > 0 && K <= OD_MERGE_MAX_K,
             "%s: bad dims (P even, K <= %d)", who, OD_MERGE_MAX_K);
  OD_REQUIRE((long long)P * NC < (1LL << 31), "%s: P * NC must fit 31 bits", who);
  OD_REQUIRE(conf_threshold >= 0.f, "%s: conf_threshold must be >= 0 (scores are probabilities)", who);
  const DetLayout l = det_layout(B, P, NC);
  if (workspace_bytes < l.total) {
    od_set_error("%s: workspace %zu < %zu bytes", who, workspace_bytes, l.total);
    return OD_ERR_WORKSPACE;
  }
  if (nms_workspace_bytes < od_nms_workspace_bytes(B, K)) {
    od_set_error("%s: NMS workspace %zu < %zu bytes", who, nms_workspace_bytes, od_nms_workspace_bytes(B, K));
    return OD_ERR_WORKSPACE;
  }
  char* ws = (char*)workspace;
  int* hist = (int*)(ws + l.hist);
  TopkState* st = (TopkState*)(ws + l.state);
  float* rowmax = (float*)(ws + l.rowmax);
  u64* cand = (u64*)(ws + l.cand);
  const int C = NC + 6;
  // first-digit mapping: 4096 bins over (bits(thr), bits(1.0)]
  unsigned dbase;
  memcpy(&dbase, &conf_threshold, 4);
  int dshift = 0;
  while (((0x3F800000u - dbase) >> dshift) >= (unsigned)NB) ++dshift;
  const dim3 grid((unsigned)od_ceil_div(P, DT_ROWS), (unsigned)B);
  const dim3 grid2((unsigned)od_ceil_div(P, DT_ROWS * DT2_RPT), (unsigned)B);
  u64* skeys;
  f32x4* sbox;
  int* scls;
  int KP;
  od_nms_sorted_buffers(nms_workspace, B, K, &skeys, &sbox, &scls, &KP);
  if (NC > OD_MAX_LDS_NC) {
    if (int rc = od_detect_wide_launch(pred, priors, B, P, NC, loc_scale, clip, conf_threshold, dbase, dshift, K, KP, boxes, conf,
                                       (u64*)keys, counts, hist, st, rowmax, (int*)(ws + l.nhot), (HotRow*)(ws + l.hot), skeys,
                                       sbox, scls, s))
      return rc;
    if (!nms) return OD_OK;
    return od_nms_greedy_launch(nms_workspace, counts, B, K, nms->iou_threshold, nms->strict, nms->max_det, nms->keep_flat,
                                nms->keep_count, s);
  }
  // the class counts with a compile-time pass 1: VOC's 20 (every other count up to 76 runs the same kernel with NC at run time)
  const size_t lds1 = (size_t)DT_ROWS * dt_row_pitch(C) * 4 + (size_t)NB * 4;
  const auto pass1 = NC == 20 ? launch_pass1<20> : launch_pass1<0>;
  if (int rc = pass1(ctx, grid, lds1, s, pred, priors, boxes, rowmax, conf, hist, st, P, NC, loc_scale, clip, conf_threshold,
                     dbase, dshift))
    return rc;
  const size_t lds2 = (size_t)DT_ROWS * C * 4 + ((size_t)K + DT_CAND_CAP) * 8;
  if (int rc = od_ensure_lds(ctx, (const void*)&od_detect_pass2, lds2)) return rc;
  hipLaunchKernelGGL(od_detect_pass2, grid2, dim3(256), lds2, s, pred, rowmax, hist, st, (u64*)keys, cand, P, NC, K,
                     conf_threshold, l.cand_stride, dbase, dshift);
  OD_CHECK_LAUNCH();
  const RefineArgs ra = {boxes, st, (u64*)keys, cand, hist, counts, P, NC, K, KP, l.cand_stride, skeys, sbox, scls, dbase, dshift};
  if (!nms) {
    hipLaunchKernelGGL(od_detect_refine_sort, dim3(B), dim3(1024), 0, s, ra);
    OD_CHECK_LAUNCH();
    return OD_OK;
  }
  hipLaunchKernelGGL(od_detect_tail, dim3(B), dim3(1024), (size_t)1024 * 8 + (size_t)KP * 20, s, ra, nms->iou_threshold,
                     nms->strict, nms->max_det, nms->keep_flat, nms->keep_count);
  OD_CHECK_LAUNCH();
  return OD_OK;
}
}  // namespace

extern "C" int od_detect(od_ctx* ctx, const float* pred, const float* priors, int B, int P, int NC, float loc_scale, int clip,
                         float conf_threshold, int K, float iou_threshold, int strict, int max_det, float* boxes, float* conf,
                         uint64_t* keys, int32_t* counts, int32_t* keep_flat, int32_t* keep_count, void* workspace,
                         size_t workspace_bytes, void* nms_workspace, size_t nms_workspace_bytes, void* stream) {
  OD_REQUIRE(ctx && pred && priors && boxes && keys && counts && keep_flat && keep_count && workspace && nms_workspace,
             "od_detect: null argument");
  OD_REQUIRE(max_det > 0, "od_detect: bad dims (P even, K <= 1024)");
  const NmsArgs nms = {iou_threshold, strict, max_det, keep_flat, keep_count};
  return detect_launch(ctx, "od_detect", pred, priors, B, P, NC, loc_scale, clip, conf_threshold, K, boxes, conf, keys, counts,
                       workspace, workspace_bytes, nms_workspace, nms_workspace_bytes, &nms, (hipStream_t)stream);
}

extern "C" int od_detect_candidates(od_ctx* ctx, const float* pred, const float* priors, int B, int P, int NC, float loc_scale,
                                    int clip, float conf_threshold, int K, float* boxes, float* conf, uint64_t* keys,
                                    int32_t* counts, void* workspace, size_t workspace_bytes, void* nms_workspace,
                                    size_t nms_workspace_bytes, void* stream) {
  OD_REQUIRE(ctx && pred && priors && boxes && keys && counts && workspace && nms_workspace, "od_detect_candidates: null argument");
  return detect_launch(ctx, "od_detect_candidates", pred, priors, B, P, NC, loc_scale, clip, conf_threshold, K, boxes, conf, keys,
                       counts, workspace, workspace_bytes, nms_workspace, nms_workspace_bytes, nullptr, (hipStream_t)stream);
}

extern "C" int od_gather_detections_pred(od_ctx* ctx, const float* pred, const float* boxes, const int32_t* keep_flat,
                                         const int32_t* keep_count, int B, int P, int NC, int max_det, float* out, void* stream) {
  OD_REQUIRE(ctx && pred && boxes && keep_flat && keep_count && out, "od_gather_detections_pred: null argument");
  OD_REQUIRE(NC >= 1 && NC <= OD_MAX_NC, "od_gather_detections_pred: NC = %d outside the supported class counts 1..%d", NC,
             OD_MAX_NC);
  OD_REQUIRE(B > 0 && P > 0 && max_det > 0, "od_gather_detections_pred: bad dims");
  if (NC > OD_MAX_LDS_NC) {
    return od_gather_det_pred_wide_launch(pred, boxes, keep_flat, keep_count, B, P, NC, max_det, out, (hipStream_t)stream);
  }
  hipLaunchKernelGGL(od_gather_det_pred, dim3(B), dim3(256), (size_t)256 * (NC + 6) * 4, (hipStream_t)stream, pred, boxes,
                     keep_flat, keep_count, P, NC, max_det, out);
  OD_CHECK_LAUNCH();
  return OD_OK;
}
