// od_detect / od_gather_detections_pred for class counts whose rows no longer fit the LDS kernels of detect.hip
// (NC > 76, up to OD_MAX_NC): the same five-launch pipeline, the same total order and exact selection, the same kept indices
// as the three-call path.  The class columns are streamed instead of held:
//   pass 1  (od_detect_pass1_wide)  reads a workgroup's 256 rows three times through an LDS column tile (max, sum of expf,
//           confidences; sweeps 2-3 mostly hit L2): decoded boxes, the first-digit histogram, one rowmax per prior
//   pass 2  (od_detect_pass2_wide)  winners (digit > d0) straight to the output as in od_detect_pass2; the d0-bin candidates
//           are only counted, and every prior that may hold one is recorded as a HotRow (index + row stats, <= P per image)
//           instead of listing the d0-bin keys themselves (up to P * NC per image)
//   refine  (od_detect_refine_rows)  one workgroup per image: od_detect_refine_sort with the d0-bin keys re-derived from the
//           HotRows for every radix pass
// Pass 2's compaction and copy-out, the radix refine, the sort and the gather are topk_common.h's: one copy for both dispatches.
// The workspace is O(B * P) for any NC (det_layout in detect.hip).  Compiled with -ffp-contract=off like detect.hip.
#include "post_common.h"

namespace {

constexpr int NB = OD_TOPK_NB;
constexpr int DT_ROWS = OD_DT_ROWS, DT2_RPT = OD_DT2_RPT;  // priors per workgroup in pass 1 / per thread in pass 2

// grid (ceil(P / 256), B).  Static LDS: the column tile + hist[4096].  conf_out: optional dense [B,P,NC] confidences.
__global__ __launch_bounds__(256) void od_detect_pass1_wide(const float* __restrict__ pred, const float* __restrict__ priors,
                                                            float* __restrict__ boxes, float* __restrict__ rowmax,
                                                            float* __restrict__ conf_out, int* __restrict__ hist,
                                                            TopkState* __restrict__ st, int* __restrict__ nhot, int P, int NC,
                                                            float loc_scale, int clip, float thr, unsigned dbase, int dshift) {
  __shared__ float tile[DT_ROWS * OD_WIDE_LD];
  __shared__ int lh[NB];
  const int C = NC + 6, tid = threadIdx.x, b = blockIdx.y;
  const int p0 = blockIdx.x * DT_ROWS;
  const int nrows = min(DT_ROWS, P - p0);
  for (int i = tid; i < NB; i += 256) lh[i] = 0;
  if (blockIdx.x == 0 && tid == 0) {  // pass 2 counts into these with atomics
    TopkState z = {0, 0, 0, 0};
    st[b] = z;
    nhot[b] = 0;
  }
  const long long r0 = (long long)b * P + p0;
  const float* src = pred + r0 * C;
  const OdRowStats rs = od_wide_stats(src, C, NC, nrows, tile);  // (its barriers also publish the zeroed lh)
  float mx = 0.f;
  for (int c0 = 0; c0 < NC; c0 += OD_WIDE_CW) {  // sweep 3: confidences, histogram, rowmax
    const int w = min(OD_WIDE_CW, NC - c0);
    od_wide_stage(src, C, nrows, 2 + c0, w, tile);
    __syncthreads();
    if (tid < nrows) {
      float* t = tile + tid * OD_WIDE_LD;
      for (int c = 0; c < w; ++c) {
        const float v = od_wide_conf(t[c], rs);
        t[c] = v;
        mx = fmaxf(mx, v);
        const unsigned sb = od_score_bits(v, thr);
        if (sb) atomicAdd(&lh[od_digit0(sb, dbase, dshift)], 1);
      }
    }
    __syncthreads();
    if (conf_out) {
      for (int i = tid; i < nrows * OD_WIDE_CW; i += 256) {
        const int r = i / OD_WIDE_CW, c = i % OD_WIDE_CW;
        if (c < w) conf_out[(r0 + r) * NC + c0 + c] = tile[r * OD_WIDE_LD + c];
      }
      __syncthreads();
    }
  }
  if (tid < nrows) {
    rowmax[r0 + tid] = mx;
    const float* row = src + (long long)tid * C;
    const f32x4 loc = {row[2 + NC], row[3 + NC], row[4 + NC], row[5 + NC]};
    const f32x4 pr = *(const f32x4*)(priors + (long long)(p0 + tid) * 4);
    *(f32x4*)(boxes + (r0 + tid) * 4) = od_decode_one(loc, pr, loc_scale, clip);
  }
  int* gh = hist + (long long)b * NB;
  for (int i = tid; i < NB; i += 256)
    if (lh[i]) atomicAdd(&gh[i], lh[i]);
}

// grid (ceil(P / 1024), B).  Dynamic LDS: l_out [K] keys.  Winners (digit > d0) go to the output as in od_detect_pass2; the
// d0-bin candidates are only counted (st.ncand), and every prior that may hold one is appended to the image's HotRow list.
__global__ __launch_bounds__(256) void od_detect_pass2_wide(const float* __restrict__ pred, const float* __restrict__ rowmax,
                                                            const int* __restrict__ hist, TopkState* __restrict__ st,
                                                            u64* __restrict__ keys, HotRow* __restrict__ hot,
                                                            int* __restrict__ nhot, int P, int NC, int K, float thr,
                                                            unsigned dbase, int dshift) {
  extern __shared__ __attribute__((aligned(16))) u64 l_out[];  // [K]
  const int C = NC + 6, tid = threadIdx.x, b = blockIdx.y;
  __shared__ int n_out, n_cand, n_hot, base_out, base_hot, sh_fd[8];
  __shared__ int hot_list[DT_ROWS * DT2_RPT];
  if (tid == 0) {
    n_out = 0;
    n_cand = 0;
    n_hot = 0;
  }
  int d0, above;
  od_find_digit_256(hist + (long long)b * NB, K, sh_fd, &d0, &above);  // (its barriers also publish the counters)
  if (blockIdx.x == 0 && tid == 0) {
    st[b].d0 = d0;
    st[b].krem = d0 < 0 ? 0 : K - above;
  }
  const int p_base = blockIdx.x * (DT_ROWS * DT2_RPT);
  const int nh = od_compact_hot_priors(rowmax + (long long)b * P, P, p_base, thr, dbase, dshift, d0, hot_list, &n_hot);
  if (tid == 0) base_hot = nh ? atomicAdd(&nhot[b], nh) : 0;
  __syncthreads();
  HotRow* hb = hot + (long long)b * P + base_hot;
  int my_cand = 0;
  for (int e = tid; e < nh; e += 256) {
    const int p = hot_list[e];
    const float* row = pred + ((long long)b * P + p) * C;
    const OdRowStats rs = od_row_stats(row, NC);
    hb[e] = HotRow{p, rs};
    for (int c = 0; c < NC; ++c) {
      const unsigned sbc = od_score_bits(od_wide_conf(row[2 + c], rs), thr);
      if (!sbc) continue;
      const int dg = od_digit0(sbc, dbase, dshift);
      if (dg > d0) {
        l_out[atomicAdd(&n_out, 1)] = od_make_key(sbc, (unsigned)(p * NC + c));
      } else if (dg == d0) {
        ++my_cand;
      }
    }
  }
  if (my_cand) atomicAdd(&n_cand, my_cand);
  __syncthreads();
  if (tid == 0 && n_cand) atomicAdd(&st[b].ncand, n_cand);
  od_block_copy_out(l_out, n_out, &st[b].nout, keys + (long long)b * K, &base_out);
}

// One workgroup (1024 threads) per image: od_detect_refine_sort with the d0-bin candidates re-derived from the HotRows
// (one (row, class) pair per thread and step; the confidence from the recorded row stats is the same bits as pass 1's).
__global__ __launch_bounds__(1024) void od_detect_refine_rows(const float* __restrict__ pred, const float* __restrict__ boxes,
                                                              TopkState* __restrict__ st, u64* __restrict__ keys,
                                                              const HotRow* __restrict__ hot, const int* __restrict__ nhot,
                                                              int* __restrict__ hist, int* __restrict__ counts, int P, int NC,
                                                              int K, int KP, u64* __restrict__ skeys, f32x4* __restrict__ sbox,
                                                              int* __restrict__ scls, float thr, unsigned dbase, int dshift) {
  __shared__ u64 s[1024];
  __shared__ int n_win;
  const int b = blockIdx.x, tid = threadIdx.x, C = NC + 6;
  const TopkState t = st[b];
  const int nout0 = min(t.nout, K);
  if (tid == 0) n_win = 0;
  s[tid] = tid < nout0 ? keys[(long long)b * K + tid] : 0ull;
  __syncthreads();
  if (t.d0 >= 0 && t.krem > 0) {
    const HotRow* hr = hot + (long long)b * P;
    const float* pb = pred + (long long)b * P * C;
    const int nel = nhot[b] * NC;  // < 2^31: P * NC is
    od_radix_refine(
        nel, t.ncand, t.krem, dbase, dshift,
        [&](int i) -> u64 {  // the key of (row h, class c) if it lies in the d0 bin, else 0
          const int h = i / NC, c = i - h * NC;
          const HotRow r = hr[h];
          const unsigned sb = od_score_bits(od_wide_conf(pb[(long long)r.p * C + 2 + c], r.r), thr);
          if (!sb || od_digit0(sb, dbase, dshift) != t.d0) return 0ull;
          return od_make_key(sb, (unsigned)(r.p * NC + c));
        },
        [&](u64 key) {
          const int slot = nout0 + atomicAdd(&n_win, 1);
          if (slot < K) s[slot] = key;
        });
    __syncthreads();
  }
  od_bitonic_sort_desc(s, KP);
  od_rank_gather(s, min(nout0 + n_win, K), b, boxes, P, NC, K, KP, skeys, sbox, scls, keys, counts, hist);
}

// od_gather_det_pred for NC > 76: the kept row's stats read straight from pred (one detection per thread)
__global__ __launch_bounds__(256) void od_gather_det_pred_wide(const float* __restrict__ pred, const float* __restrict__ boxes,
                                                               const int32_t* __restrict__ keep_flat,
                                                               const int32_t* __restrict__ keep_count, int P, int NC,
                                                               int max_det, float* __restrict__ out) {
  const int b = blockIdx.x, C = NC + 6;
  const int n = keep_count[b];
  float* o = out + (size_t)b * (1 + 6 * (size_t)max_det);
  if (threadIdx.x == 0) o[0] = __int_as_float(n);
  for (int r = threadIdx.x; r < max_det; r += 256) {
    float* rec = o + 1 + 6 * (size_t)r;
    if (r < n) {
      const int flat = keep_flat[(size_t)b * max_det + r];
      const int p = flat / NC, c = flat - p * NC;
      const float* src = pred + ((size_t)b * P + p) * C;
      const float* bx = boxes + ((size_t)b * P + p) * 4;
      rec[0] = __int_as_float(flat);
      rec[1] = od_wide_conf(src[2 + c], od_row_stats(src, NC));
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

}  // namespace

int od_detect_wide_launch(const float* pred, const float* priors, int B, int P, int NC, float loc_scale, int clip, float thr,
                          unsigned dbase, int dshift, int K, int KP, float* boxes, float* conf, u64* keys, int* counts,
                          int* hist, TopkState* st, float* rowmax, int* nhot, HotRow* hot, u64* skeys, f32x4* sbox, int* scls,
                          hipStream_t s) {
  const dim3 grid((unsigned)od_ceil_div(P, DT_ROWS), (unsigned)B);
  const dim3 grid2((unsigned)od_ceil_div(P, DT_ROWS * DT2_RPT), (unsigned)B);
  hipLaunchKernelGGL(od_detect_pass1_wide, grid, dim3(256), 0, s, pred, priors, boxes, rowmax, conf, hist, st, nhot, P, NC,
                     loc_scale, clip, thr, dbase, dshift);
  OD_CHECK_LAUNCH();
  hipLaunchKernelGGL(od_detect_pass2_wide, grid2, dim3(256), (size_t)K * 8, s, pred, rowmax, hist, st, keys, hot, nhot, P, NC,
                     K, thr, dbase, dshift);
  OD_CHECK_LAUNCH();
  hipLaunchKernelGGL(od_detect_refine_rows, dim3(B), dim3(1024), 0, s, pred, boxes, st, keys, hot, nhot, hist, counts, P, NC, K,
                     KP, skeys, sbox, scls, thr, dbase, dshift);
  OD_CHECK_LAUNCH();
  return OD_OK;
}

int od_gather_det_pred_wide_launch(const float* pred, const float* boxes, const int32_t* keep_flat, const int32_t* keep_count,
                                   int B, int P, int NC, int max_det, float* out, hipStream_t s) {
  hipLaunchKernelGGL(od_gather_det_pred_wide, dim3(B), dim3(256), 0, s, pred, boxes, keep_flat, keep_count, P, NC, max_det,
                     out);
  OD_CHECK_LAUNCH();
  return OD_OK;
}
