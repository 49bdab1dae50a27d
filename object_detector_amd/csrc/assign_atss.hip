// K9b: ATSS prior-box assignment (Zhang et al., CVPR 2020) + target encoding: the opt-in assigner of od.pb.encode_truth
// (PriorBoxes(assigner="atss")).  [BUILD-DEFINED] rule, frozen so that every step is integer arithmetic or one stated f32
// sequence and mirrored op for op by tests/atss_ref.py (this TU is built with -ffp-contract=off):
//   1. per unflagged box g and pyramid level l (gh x gw cells, A priors per cell, prior row order (level, y, x, prior)):
//        gx = (x1 + x2) * 0.5f, gy likewise;  cx = ((float)x + 0.5f) / (float)gw, cy likewise (the GRID's centres);
//        d2 = dx*dx + dy*dy;  the min(k, gh*gw) cells with the smallest key (d2 bits as u32, cell index y*gw + x) are
//        chosen, and all A priors of a chosen cell are candidates (n of them over the levels)
//   2. v_c = iou_f32(box, prior_c); q_c = (int)rintf(v_c * 1048576.0f); S1 = sum q, S2 = sum q^2, D = n*S2 - S1^2,
//      L_c = n*q_c - S1.  Candidate c PASSES when L_c >= 0, L_c^2 >= D (q_c >= mean + population std, exactly) and its
//      cell centre lies strictly inside the box
//   3. a box without a passing candidate FORCES its candidate of the largest v_c > 0 (ties: lowest prior index)
//   4. a prior claimed more than once goes to a forced claim first, then to the larger v (f32 bits), then to the lower g
//   5. owned priors get the row od_assign_encode writes; every other prior is background (no IoU ignore band, assigned_gt is
//      never -2); flagged boxes (gt_flags bit 0) take no part in 1-4 and turn background priors they cover into all-zero
//      rows (assigned_gt -3): rule 3 of assign.hip
// Nothing depends on the order of a reduction: the sums are integers and a claim is one u64 key resolved by atomicMax.
#include "assign_common.h"

namespace {

constexpr int ATSS_MAX_LEVELS = 4, ATSS_MAX_TOPK = 32, ATSS_MAX_A = 8;
constexpr int ATSS_MAX_CAND = ATSS_MAX_LEVELS * ATSS_MAX_TOPK * ATSS_MAX_A;  // 1024 = 4 per thread of a 256-thread block
// with n <= 1024 and q <= 2^20: S1 <= 2^30, S2 <= 2^50, n*S2 and L_c^2 <= 2^60: everything fits a signed 64-bit integer

struct AtssLevels {
  int n;
  int gh[ATSS_MAX_LEVELS], gw[ATSS_MAX_LEVELS], base[ATSS_MAX_LEVELS];  // base: index of the level's first prior
};

__device__ __forceinline__ u64 wave_min_u64(u64 v) {
  for (int o = 32; o; o >>= 1) {
    const u64 t = __shfl_xor(v, o, 64);
    v = t < v ? t : v;
  }
  return v;
}
__device__ __forceinline__ u64 wave_max_u64(u64 v) {
  for (int o = 32; o; o >>= 1) {
    const u64 t = __shfl_xor(v, o, 64);
    v = t > v ? t : v;
  }
  return v;
}
__device__ __forceinline__ long long wave_sum_i64(long long v) {
  for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// select pass: one workgroup per (box, image).  The k nearest cells of a level are found by k rounds of a block-wide
// minimum over ALL the level's cells (each thread rescans its cells for the smallest key above the last one chosen), so the
// choice is the rule's for every input, a box far outside the image or with non-finite corners included: no window to prove.
__global__ __launch_bounds__(256) void od_atss_select(const float* __restrict__ priors, const float* __restrict__ gt_boxes,
                                                      const int* __restrict__ gt_counts, const int* __restrict__ gt_flags,
                                                      AtssLevels lv, int A, int topk, int P, int Gmax,
                                                      u64* __restrict__ claim) {
  __shared__ u64 swave[2][4];                                // per-wave partial of a round, double-buffered
  __shared__ unsigned ssel[ATSS_MAX_LEVELS * ATSS_MAX_TOPK];  // chosen cells, level by level, ascending key
  __shared__ long long ssum[2];
  __shared__ u64 sforced;
  __shared__ int spass;
  const int g = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, wave = tid >> 6;
  if (g >= min(gt_counts[b], Gmax)) return;  // a padding slot is never read as a box
  if (gt_flags && (gt_flags[(long long)b * Gmax + g] & 1)) return;
  const f32x4 box = *(const f32x4*)(gt_boxes + ((long long)b * Gmax + g) * 4);
  const float gx = (box[0] + box[2]) * 0.5f, gy = (box[1] + box[3]) * 0.5f;
  if (tid == 0) {
    ssum[0] = ssum[1] = 0;
    sforced = 0ull;
    spass = 0;
  }

  // 1. candidate cells
  int off[ATSS_MAX_LEVELS + 1];  // off[l]: chosen cells in the levels before l
  off[0] = 0;
  int round = 0;
#pragma unroll
  for (int l = 0; l < ATSS_MAX_LEVELS; ++l) {
    int nsel = 0;
    if (l < lv.n) {
      const int gw = lv.gw[l], cells = lv.gh[l] * gw;
      const float fgw = (float)gw, fgh = (float)lv.gh[l];
      nsel = min(topk, cells);
      u64 lo = 0ull;  // keys below lo are already chosen
      for (int r = 0; r < nsel; ++r, ++round) {
        u64 best = ~0ull;  // no key: a cell index never reaches 2^32 - 1
        for (int c = tid; c < cells; c += 256) {
          const int yy = c / gw, xx = c - yy * gw;
          const float dx = ((float)xx + 0.5f) / fgw - gx, dy = ((float)yy + 0.5f) / fgh - gy;
          const float d2 = dx * dx + dy * dy;
          const u64 key = ((u64)__float_as_uint(d2) << 32) | (u64)(unsigned)c;
          if (key >= lo && key < best) best = key;
        }
        best = wave_min_u64(best);
        if ((tid & 63) == 0) swave[round & 1][wave] = best;
        __syncthreads();  // round r + 2 rewrites this buffer only after every wave has passed round r + 1's barrier
        const u64* w = swave[round & 1];
        best = min(min(w[0], w[1]), min(w[2], w[3]));
        if (tid == 0) ssel[l * ATSS_MAX_TOPK + r] = (unsigned)best;
        lo = best + 1ull;
      }
    }
    off[l + 1] = off[l] + nsel;
  }
  __syncthreads();

  // 2. the candidates' IoUs on the 2^-20 lattice and their integer sums; a thread keeps its (at most 4) candidates in registers
  const int n = off[ATSS_MAX_LEVELS] * A;
  float v[4];
  int q[4], pi[4];
  bool inside[4];
  long long s1 = 0, s2 = 0;
#pragma unroll
  for (int i = 0; i < ATSS_MAX_CAND / 256; ++i) {
    const int c = tid + i * 256;
    v[i] = 0.f, q[i] = 0, pi[i] = -1, inside[i] = false;
    if (c < n) {  // every chosen cell is a real one: nsel <= cells keys are distinct, so each round finds a key
      const int s = c / A, a = c - s * A;
      int l = 0;
#pragma unroll
      for (int j = 1; j < ATSS_MAX_LEVELS; ++j) l += s >= off[j];  // beyond the last level off[j] is the total, above every s
      int gw = lv.gw[0], gh = lv.gh[0], base = lv.base[0], o = 0;
#pragma unroll
      for (int j = 1; j < ATSS_MAX_LEVELS; ++j)
        if (l == j) gw = lv.gw[j], gh = lv.gh[j], base = lv.base[j], o = off[j];
      const int cell = (int)ssel[l * ATSS_MAX_TOPK + (s - o)];
      const int yy = cell / gw, xx = cell - yy * gw;
      const float cx = ((float)xx + 0.5f) / (float)gw, cy = ((float)yy + 0.5f) / (float)gh;
      pi[i] = base + cell * A + a;  // < P: cell < gh*gw, and the host checked sum gh*gw*A == P
      v[i] = iou_f32(box, *(const f32x4*)(priors + (long long)pi[i] * 4));
      q[i] = (int)rintf(v[i] * 1048576.0f);
      inside[i] = cx > box[0] && cx < box[2] && cy > box[1] && cy < box[3];
      s1 += q[i];
      s2 += (long long)q[i] * q[i];
    }
  }
  s1 = wave_sum_i64(s1);
  s2 = wave_sum_i64(s2);
  if ((tid & 63) == 0) {
    atomicAdd((u64*)&ssum[0], (u64)s1);
    atomicAdd((u64*)&ssum[1], (u64)s2);
  }
  __syncthreads();
  const long long S1 = ssum[0], S2 = ssum[1];
  const long long D = (long long)n * S2 - S1 * S1;

  // 2./3. pass test; the box's best candidate in case nothing passes
  bool pass[4];
  bool any = false;
  u64 fbest = 0ull;
#pragma unroll
  for (int i = 0; i < ATSS_MAX_CAND / 256; ++i) {
    const long long Lc = (long long)n * q[i] - S1;
    pass[i] = pi[i] >= 0 && Lc >= 0 && Lc * Lc >= D && inside[i];
    any |= pass[i];
    if (pi[i] >= 0 && v[i] > 0.f) {
      const u64 k = ((u64)__float_as_uint(v[i]) << 32) | (u64)(0xFFFFFFFFu - (unsigned)pi[i]);
      fbest = k > fbest ? k : fbest;
    }
  }
  const bool wany = __ballot(any) != 0ull;
  fbest = wave_max_u64(fbest);
  if ((tid & 63) == 0) {
    if (wany) atomicOr(&spass, 1);
    if (fbest) atomicMax(&sforced, fbest);
  }
  __syncthreads();

  // 4. claims
  u64* cl = claim + (long long)b * P;
  if (spass) {
#pragma unroll
    for (int i = 0; i < ATSS_MAX_CAND / 256; ++i)
      if (pass[i]) atomicMax(&cl[pi[i]], claim_key(false, v[i], g));
  } else if (tid == 0 && sforced) {
    const unsigned p = 0xFFFFFFFFu - (unsigned)(sforced & 0xFFFFFFFFull);
    atomicMax(&cl[p], claim_key(true, __uint_as_float((unsigned)(sforced >> 32)), g));
  }
}

}  // namespace

extern "C" size_t od_assign_atss_workspace_bytes(int B, int P, int Gmax) {
  if (B <= 0 || P <= 0 || Gmax <= 0) return 0;
  return (size_t)B * P * sizeof(u64);  // one claim per prior
}

extern "C" int od_assign_atss(od_ctx* ctx, const float* priors, const int32_t* grid_hw, int n_levels, int priors_per_cell,
                              const float* gt_boxes, const int32_t* gt_classes, const int32_t* gt_counts,
                              const int32_t* gt_flags, float ign_thr, int topk, int B, int P, int Gmax, int NC,
                              float loc_scale, float* y, int32_t* assigned_gt, int32_t* npos, void* workspace,
                              size_t workspace_bytes, void* stream) {
  const char* who = "od_assign_atss";
  OD_REQUIRE(ctx && priors && grid_hw && gt_boxes && gt_classes && gt_counts && y && npos && workspace, "%s: null argument",
             who);
  OD_REQUIRE(B > 0 && B <= 65535 && P > 0 && NC > 0 && Gmax > 0 && Gmax <= GMAX, "%s: bad dims (Gmax <= %d)", who, GMAX);
  OD_REQUIRE(n_levels >= 1 && n_levels <= ATSS_MAX_LEVELS, "%s: n_levels %d outside 1..%d", who, n_levels, ATSS_MAX_LEVELS);
  OD_REQUIRE(topk >= 1 && topk <= ATSS_MAX_TOPK, "%s: topk %d outside 1..%d", who, topk, ATSS_MAX_TOPK);
  OD_REQUIRE(priors_per_cell >= 1 && priors_per_cell <= ATSS_MAX_A, "%s: priors_per_cell %d outside 1..%d", who,
             priors_per_cell, ATSS_MAX_A);
  OD_REQUIRE(loc_scale > 0.f && (!gt_flags || ign_thr > 0.f), "%s: bad thresholds", who);
  AtssLevels lv = {};
  lv.n = n_levels;
  long long total = 0;
  for (int l = 0; l < n_levels; ++l) {
    const int gh = grid_hw[2 * l], gw = grid_hw[2 * l + 1];
    OD_REQUIRE(gh > 0 && gw > 0 && (long long)gh * gw * priors_per_cell <= P, "%s: level %d: bad grid %d x %d", who, l, gh,
               gw);
    lv.gh[l] = gh, lv.gw[l] = gw, lv.base[l] = (int)total;
    total += (long long)gh * gw * priors_per_cell;
  }
  OD_REQUIRE(total == P, "%s: the levels hold %lld priors, P = %d", who, total, P);
  const size_t need = (size_t)B * P * sizeof(u64);
  if (workspace_bytes < need) {
    od_set_error("%s: workspace %zu < %zu bytes", who, workspace_bytes, need);
    return OD_ERR_WORKSPACE;
  }
  hipStream_t s = (hipStream_t)stream;
  OD_CHECK_HIP(hipMemsetAsync(workspace, 0, need, s));
  OD_CHECK_HIP(hipMemsetAsync(npos, 0, (size_t)B * 4, s));
  hipLaunchKernelGGL(od_atss_select, dim3(Gmax, B), dim3(256), 0, s, priors, gt_boxes, gt_counts, gt_flags, lv,
                     priors_per_cell, topk, P, Gmax, (u64*)workspace);
  OD_CHECK_LAUNCH();
  dim3 grid(od_ceil_div(P, 256), B);
  if (gt_flags)
    hipLaunchKernelGGL(od_claim_encode<true>, grid, dim3(256), 0, s, priors, gt_boxes, gt_classes, gt_counts, gt_flags, P,
                       Gmax, NC, ign_thr, loc_scale, (const u64*)workspace, y, assigned_gt, npos);
  else
    hipLaunchKernelGGL(od_claim_encode<false>, grid, dim3(256), 0, s, priors, gt_boxes, gt_classes, gt_counts, gt_flags, P,
                       Gmax, NC, ign_thr, loc_scale, (const u64*)workspace, y, assigned_gt, npos);
  OD_CHECK_LAUNCH();
  return OD_OK;
}
