// K16: COCO bbox evaluation (AP@[.50:.95], AR) -- the greedy matching and the precision / recall accumulation of
// pycocotools' COCOeval with default parameters, in f64.  The protocol is stated in object_detector_amd/cocoeval.py; the
// host there sorts, packs and uploads, these kernels do the O(dets x GTs x thresholds) work.
//
// Built with -ffp-contract=off (not in the Makefile's CONTRACT_ON list): every IoU, precision and recall value is the
// exact op sequence of the numpy statement of the protocol, so results are bit-identical to it.  No float atomics: the
// only atomics are integer ORs on match words and integer MAXes on the bit patterns of non-negative doubles, whose result
// does not depend on their order.
#include <climits>

#include "common.h"

namespace {

constexpr int T = OD_COCO_T, A = OD_COCO_A, R = OD_COCO_R, M = OD_COCO_M;
constexpr int WAVES = 4;         // waves (independent work units) per workgroup of both kernels
constexpr int MATCH_LDS_GT = 256;  // match words of a group with at most this many GTs live in LDS, others in the workspace
static_assert(T * A <= 64, "one lane per (threshold, area range)");

// Order between lanes of one wave: the compiler keeps memory accesses on either side, and the hardware waits for the
// LDS / global accesses before the fence (a wave's lanes exchange data through memory here, never across waves).
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
  __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ int popc(uint64_t v) { return __popcll(v); }

// index of the k-th (1-based) set bit of v; v holds at least k set bits
__device__ __forceinline__ int select_bit(uint64_t v, int k) {
  int pos = 0;
#pragma unroll
  for (int w = 32; w >= 1; w >>= 1) {
    const int c = popc((v >> pos) & ((1ull << w) - 1));
    if (c < k) {
      k -= c;
      pos += w;
    }
  }
  return pos;
}

// One wave per group (image, category).  Lane l < T*A walks the group's GTs for threshold t = l / A, area range a = l % A;
// the IoU of (detection, GT) is the same for every lane and computed once per visit.  A single walk in file order keeps
// two candidates per lane: the best non-ignored GT (pycocotools' pass over the non-ignored GTs) and the best ignored GT
// (its pass over the ignored ones, which only counts when the first found nothing and starts from the same threshold).
// Match state: one u64 per GT, bit l = matched for lane l, in LDS or (large groups) in the caller's workspace.
__global__ __launch_bounds__(64 * WAVES) void od_coco_match_k(
    const int32_t* __restrict__ gt_off, const int32_t* __restrict__ det_off, int n_groups,
    const double* __restrict__ gt_box, const double* __restrict__ gt_area, const int32_t* __restrict__ gt_crowd,
    const double* __restrict__ det_box, const int32_t* __restrict__ det_out,
    const double* __restrict__ iou_thrs, const double* __restrict__ area_rng, uint64_t* __restrict__ matched_out,
    uint64_t* __restrict__ ignored_out, uint64_t* __restrict__ ws) {
  __shared__ uint64_t lds_words[WAVES][MATCH_LDS_GT];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int g = blockIdx.x * WAVES + wave;
  if (g >= n_groups) return;
  const int d0 = det_off[g], d1 = det_off[g + 1];
  if (d1 == d0) return;  // GT-only group: no detection to label
  const int g0 = gt_off[g], ng = gt_off[g + 1] - g0;
  const bool active = lane < T * A;
  const int ln = active ? lane : 0;
  const double thr = fmin(iou_thrs[ln / A], 1.0 - 1e-10);
  const double lo = area_rng[2 * (ln % A)], hi = area_rng[2 * (ln % A) + 1];
  const uint64_t me = 1ull << lane;
  uint64_t* words = ng <= MATCH_LDS_GT ? &lds_words[wave][0] : ws + g0;
  for (int j = lane; j < ng; j += 64) __hip_atomic_store(words + j, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  wave_sync();
  for (int d = d0; d < d1; ++d) {
    const double dx = det_box[4 * d], dy = det_box[4 * d + 1], dw = det_box[4 * d + 2], dh = det_box[4 * d + 3];
    const double da = dw * dh;
    double best1 = thr, best2 = thr;
    int m1 = -1, m2 = -1;
    for (int j = 0; j < ng; ++j) {
      const int gi = g0 + j;
      const double gx = gt_box[4 * gi], gy = gt_box[4 * gi + 1], gw = gt_box[4 * gi + 2], gh = gt_box[4 * gi + 3];
      const bool crowd = gt_crowd[gi] != 0;
      const double garea = gt_area[gi];
      // pycocotools bbIou: w, h, i = w*h, u = crowd ? da : (da + ga) - i
      double iou = 0.0;
      const double w = fmin(dx + dw, gx + gw) - fmax(dx, gx);
      if (w > 0.0) {
        const double h = fmin(dy + dh, gy + gh) - fmax(dy, gy);
        if (h > 0.0) {
          const double i = w * h;
          const double u = crowd ? da : (da + gw * gh) - i;
          iou = i / u;
        }
      }
      const bool ign = crowd || garea < lo || garea > hi;
      const bool taken = !crowd && (__hip_atomic_load(words + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & me);
      if (!taken && !(iou < (ign ? best2 : best1))) {
        if (ign) {
          best2 = iou;
          m2 = j;
        } else {
          best1 = iou;
          m1 = j;
        }
      }
    }
    const int m = m1 >= 0 ? m1 : m2;
    const bool dt_out_of_range = da < lo || da > hi;
    const uint64_t mt = __ballot(active && m >= 0);
    const uint64_t ig = __ballot(active && (m >= 0 ? m1 < 0 : dt_out_of_range));
    if (active && m >= 0) __hip_atomic_fetch_or(words + m, me, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (lane == 0) {
      const int o = det_out[d];
      matched_out[o] = mt;
      ignored_out[o] = ig;
    }
    wave_sync();
  }
}

// smallest c in [0, npig] with (double)c / npig >= thr (thr <= 1): the c-th true positive is where rc first reaches thr
__device__ int min_count(double thr, int npig) {
  const double n = (double)npig;
  int c = (int)ceil(thr * n);
  c = c < 0 ? 0 : (c > npig ? npig : c);
  while (c > 0 && (double)(c - 1) / n >= thr) --c;
  while (c < npig && (double)c / n < thr) ++c;
  return c;
}

// One wave per (t, k, a, m) over category k's detections in accumulation order (descending score, then image, then rank;
// those of rank >= max_dets[m] are skipped, ignored ones stay in the sequence).  Lane l owns recall thresholds r = l and
// r = l + 64.  Pass 1: the position i_r of the c_r-th true positive (= np.searchsorted(rc, rec_thrs[r], 'left')).
// Pass 2: every position p's precision goes into bucket b = last r with i_r <= p (integer max on the f64 bits, exact and
// order-free); the suffix maximum over buckets is precision[r] = max(pr[i_r:]).
__global__ __launch_bounds__(64 * WAVES) void od_coco_accumulate_k(
    const int32_t* __restrict__ cat_off, int K, const int32_t* __restrict__ rank, const double* __restrict__ score,
    const uint64_t* __restrict__ matched, const uint64_t* __restrict__ ignored, const int32_t* __restrict__ npig_ka,
    const double* __restrict__ rec_thrs, const int32_t* __restrict__ max_dets, double* __restrict__ precision,
    double* __restrict__ recall, double* __restrict__ scores) {
  __shared__ int lds_pos[WAVES][R];
  __shared__ uint64_t lds_bucket[WAVES][R];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int u = blockIdx.x * WAVES + wave;
  if (u >= K * T * A * M) return;
  const int m = u % M, a = (u / M) % A, t = (u / (M * A)) % T, k = u / (M * A * T);
  const int bit = t * A + a;
  const int npig = npig_ka[k * A + a];
  const int max_det = max_dets[m];
  const int r0 = lane, r1 = lane + 64;
  const bool has1 = r1 < R;
  auto pidx = [&](int r) { return ((((int64_t)t * R + r) * K + k) * A + a) * M + m; };
  const int64_t ridx = (((int64_t)t * K + k) * A + a) * M + m;
  if (npig == 0) {
    precision[pidx(r0)] = -1.0;
    scores[pidx(r0)] = -1.0;
    if (has1) {
      precision[pidx(r1)] = -1.0;
      scores[pidx(r1)] = -1.0;
    }
    if (lane == 0) recall[ridx] = -1.0;
    return;
  }
  const int c0 = min_count(rec_thrs[r0], npig), c1 = has1 ? min_count(rec_thrs[r1], npig) : 0;
  const int cmax = min_count(rec_thrs[R - 1], npig);
  const int s0 = cat_off[k], s1 = cat_off[k + 1];
  const uint64_t le = (2ull << lane) - 1;  // lanes <= this one (wraps to all ones for lane 63)
  // pass 1: positions (among included detections) and sequence indices of the c_r-th true positive
  int pos0 = INT_MAX, pos1 = INT_MAX, seq0 = -1, seq1 = -1;
  int inc_n = 0, tp_n = 0;
  for (int base = s0; base < s1 && tp_n < cmax; base += 64) {
    const int j = base + lane;
    const bool inc = j < s1 && rank[j] < max_det;
    const uint64_t mt = inc ? matched[j] : 0, ig = inc ? ignored[j] : 0;
    const bool tp = inc && ((mt >> bit) & 1) && !((ig >> bit) & 1);
    const uint64_t inc_mask = __ballot(inc), tp_mask = __ballot(tp);
    const int ntp = popc(tp_mask);
    auto find = [&](int c, int& pos, int& seq) {
      if (c == 0 && seq < 0 && inc_mask) {  // rec_thrs = 0: the first included detection
        pos = inc_n;
        seq = base + __builtin_ctzll(inc_mask);
      } else if (c > tp_n && c <= tp_n + ntp) {
        const int l = select_bit(tp_mask, c - tp_n);
        pos = inc_n + popc(inc_mask & ((2ull << l) - 1)) - 1;
        seq = base + l;
      }
    };
    find(c0, pos0, seq0);
    if (has1) find(c1, pos1, seq1);
    inc_n += popc(inc_mask);
    tp_n += ntp;
  }
  int* pos_l = lds_pos[wave];
  uint64_t* bucket = lds_bucket[wave];
  pos_l[r0] = pos0;
  bucket[r0] = 0;
  if (has1) {
    pos_l[r1] = pos1;
    bucket[r1] = 0;
  }
  wave_sync();
  // pass 2: precision of every included position into its bucket; totals
  inc_n = 0;
  tp_n = 0;
  int fp_n = 0;
  for (int base = s0; base < s1; base += 64) {
    const int j = base + lane;
    const bool inc = j < s1 && rank[j] < max_det;
    const uint64_t mt = inc ? matched[j] : 0, ig = inc ? ignored[j] : 0;
    const bool valid = inc && !((ig >> bit) & 1);
    const bool tp = valid && ((mt >> bit) & 1), fp = valid && !((mt >> bit) & 1);
    const uint64_t inc_mask = __ballot(inc), tp_mask = __ballot(tp), fp_mask = __ballot(fp);
    if (inc) {
      const int tpj = tp_n + popc(tp_mask & le), fpj = fp_n + popc(fp_mask & le);
      const int p = inc_n + popc(inc_mask & le) - 1;
      const double pr = (double)tpj / (((double)fpj + (double)tpj) + 0x1p-52);
      int lo = 0, hi = R;  // first r with pos > p; i_0 = 0 <= p, so b >= 0
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (pos_l[mid] <= p) lo = mid + 1;
        else hi = mid;
      }
      atomicMax((unsigned long long*)&bucket[lo - 1], (unsigned long long)__double_as_longlong(pr));
    }
    inc_n += popc(inc_mask);
    tp_n += popc(tp_mask);
    fp_n += popc(fp_mask);
  }
  wave_sync();
  const int nd = inc_n;
  auto emit = [&](int r, int pos, int seq) {
    double q = 0.0, ss = 0.0;
    if (pos < nd) {
      uint64_t mx = 0;
      for (int b = r; b < R; ++b) mx = bucket[b] > mx ? bucket[b] : mx;
      q = __longlong_as_double((long long)mx);
      ss = score[seq];
    }
    precision[pidx(r)] = q;
    scores[pidx(r)] = ss;
  };
  emit(r0, pos0, seq0);
  if (has1) emit(r1, pos1, seq1);
  if (lane == 0) recall[ridx] = nd ? (double)tp_n / (double)npig : 0.0;
}

}  // namespace

extern "C" size_t od_coco_match_workspace_bytes(long long n_gt) { return (size_t)(n_gt > 0 ? n_gt : 0) * 8; }

extern "C" int od_coco_match(od_ctx* ctx, const int32_t* gt_off, const int32_t* det_off, int n_groups,
                             const double* gt_box, const double* gt_area, const int32_t* gt_crowd, long long n_gt,
                             const double* det_box, const int32_t* det_out,
                             const double* iou_thrs, const double* area_rng, uint64_t* matched, uint64_t* ignored,
                             void* workspace, size_t workspace_bytes, void* stream) {
  OD_REQUIRE(ctx && n_groups >= 0 && n_gt >= 0, "od_coco_match: bad argument");
  if (n_groups == 0) return OD_OK;
  OD_REQUIRE(gt_off && det_off && det_box && det_out && iou_thrs && area_rng && matched && ignored &&
                 (n_gt == 0 || (gt_box && gt_area && gt_crowd)),
             "od_coco_match: null pointer");
  OD_REQUIRE(workspace_bytes >= od_coco_match_workspace_bytes(n_gt) && (n_gt == 0 || workspace),
             "od_coco_match: workspace %zu B < %zu B", workspace_bytes, od_coco_match_workspace_bytes(n_gt));
  hipLaunchKernelGGL(od_coco_match_k, dim3(od_ceil_div(n_groups, WAVES)), dim3(64 * WAVES), 0, (hipStream_t)stream,
                     gt_off, det_off, n_groups, gt_box, gt_area, gt_crowd, det_box, det_out, iou_thrs, area_rng,
                     matched, ignored, (uint64_t*)workspace);
  OD_CHECK_LAUNCH();
  return OD_OK;
}

extern "C" int od_coco_accumulate(od_ctx* ctx, const int32_t* cat_off, int K, const int32_t* rank, const double* score,
                                  const uint64_t* matched, const uint64_t* ignored, const int32_t* npig,
                                  const double* rec_thrs, const int32_t* max_dets, double* precision, double* recall,
                                  double* scores, void* stream) {
  OD_REQUIRE(ctx && K > 0 && K <= (1 << 20) && cat_off && npig && rec_thrs && max_dets && precision && recall && scores,
             "od_coco_accumulate: bad argument");
  const int units = K * T * A * M;
  hipLaunchKernelGGL(od_coco_accumulate_k, dim3(od_ceil_div(units, WAVES)), dim3(64 * WAVES), 0, (hipStream_t)stream,
                     cat_off, K, rank, score, matched, ignored, npig, rec_thrs, max_dets, precision, recall, scores);
  OD_CHECK_LAUNCH();
  return OD_OK;
}
