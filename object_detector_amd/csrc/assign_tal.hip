// K9c: task-aligned prior-box assignment (TOOD, Feng et al., ICCV 2021) + target encoding: the prediction-aware opt-in
// assigner (PriorBoxes(assigner="tal"), Trainer.step(x, annotations=...)).  [BUILD-DEFINED] rule, frozen; tests/tal_ref.py
// restates it (this TU is built with -ffp-contract=off, every f32 sequence below is evaluated as written):
//   1. per prior p of image b, from its pred row (z0, z1 objectness logits, z_c NC class logits, 4 offsets), computed once:
//        m = fmaxf(z0, z1);  la = (z1 - m) - logf(expf(z0 - m) + expf(z1 - m))            (log P(object))
//        mc = max_c z_c;     lse = mc + logf(sum_c expf(z_c - mc))
//        d = od_decode_one(offsets, prior, loc_scale, no clip);  pbox = (min(d0, d2), min(d1, d3), max(d0, d2), max(d1, d3)):
//        the decode and the corner sort of od_loss_fwd_bwd_iou.
//      A prior with a non-finite pbox coordinate, la or lse is no candidate for any box.
//   2. per unflagged box g, a prior is a candidate when its cell centre ((x + .5f) / gw, (y + .5f) / gh) lies strictly inside
//      the box and u = iou_f32(box, pbox) > 0.  Its metric, in the log domain (no underflow at NC = 1024, beta = 6):
//        l = alpha * ((la + z_cls(g)) - lse) + beta * logf(u);   a class outside 0..NC-1 drops the class term: l = alpha * la + ...
//      The box claims its min(topk, #candidates) candidates of the largest l (ties: lower prior index).
//   3. a box without a candidate FORCES the prior of the largest static v = iou_f32(box, prior) > 0 over all P priors (ties:
//      lowest index); without such a prior it owns nothing
//   4. a prior claimed more than once goes to a forced claim first, then to the larger v (f32 bits; v = u for a normal claim),
//      then to the lower g: the claim key of assign_atss.hip
//   5. rows, ignore regions, assigned_gt (never -2) and npos: step 5 of assign_atss.hip, the same encode kernel
//      (od_claim_encode, assign_common.h).  metric [B,P] = l of the winning NORMAL claim, 0 for every other prior.
// u, v and every comparison on them are exact f32 sequences.  l holds logf / expf, so only the cut at rank topk can depend on
// the device's libm; the order of the additions in lse is fixed (per-lane stride, then a butterfly), and claims are resolved
// by atomicMax on one u64 key: two calls on the same inputs give the same bytes.
#include "assign_common.h"
#include "post_common.h"  // od_decode_one

namespace {

constexpr int TAL_MAX_LEVELS = 4, TAL_MAX_TOPK = 32, TAL_MAX_A = 8, TAL_MAX_NC = 1024;
constexpr int TAL_TILE = 4 * (TAL_MAX_NC + 6);  // floats of pred one block of the per-prior pass stages: >= (256 / L) * C
constexpr int TAL_CACHE = 4;                    // best keys a thread of the select pass keeps between rounds

struct TalLevels {
  int n;
  int gh[TAL_MAX_LEVELS], gw[TAL_MAX_LEVELS], base[TAL_MAX_LEVELS];  // base: index of the level's first prior
};

struct TalPrior {  // what the per-prior pass leaves for the select pass: 24 bytes per prior
  f32x4* pbox;     // [B*P]
  float2* ll;      // [B*P] (la, lse); la = NaN marks a prior that is no candidate
};

__device__ __forceinline__ u64 tal_wave_max_u64(u64 v) {
  for (int o = 32; o; o >>= 1) {
    const u64 t = __shfl_xor(v, o, 64);
    v = t > v ? t : v;
  }
  return v;
}

// total order of the non-NaN floats as unsigned: larger value, larger key; never 0 for a finite value or -inf
__device__ __forceinline__ unsigned tal_ordered(float v) {
  const unsigned b = __float_as_uint(v);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

__device__ __forceinline__ float tal_metric(float la, float lse, bool has_cls, float zc, float u, float alpha, float beta) {
  const float t = has_cls ? (la + zc) - lse : la;
  return alpha * t + beta * logf(u);
}

// per-prior pass: a block stages R = 256 / L consecutive rows of pred ([B*P, C] is one contiguous array, so the tile is one
// contiguous, 16-byte aligned span: R * C * 4 is a multiple of 16 for R >= 4) in LDS, then L lanes share a row.  pred is read
// exactly once, in whole 16-byte words; 24 bytes per prior are written.
__global__ __launch_bounds__(256) void od_tal_prior(const float* __restrict__ pred, const float* __restrict__ priors,
                                                    long long rows, int P, int NC, int L, float loc_scale, TalPrior out) {
  __shared__ __attribute__((aligned(16))) float tile[TAL_TILE];
  const int tid = threadIdx.x, C = NC + 6, R = 256 / L;
  const long long row0 = (long long)blockIdx.x * R;
  const int nrow = (int)min((long long)R, rows - row0);
  const int n = nrow * C;  // <= TAL_TILE (the host chose L)
  const float* src = pred + row0 * C;
  const int n4 = n >> 2;
  for (int i = tid; i < n4; i += 256) ((f32x4*)tile)[i] = ((const f32x4*)src)[i];
  for (int i = (n4 << 2) + tid; i < n; i += 256) tile[i] = src[i];
  __syncthreads();
  const int r = tid / L, j = tid - r * L;
  // every lane of a row's group runs the shuffles, a group beyond the last row included (it reads row 0 and writes nothing)
  const float* row = tile + (r < nrow ? r : 0) * C;
  float mc = -INFINITY;
  for (int i = 2 + j; i < 2 + NC; i += L) mc = fmaxf(mc, row[i]);  // fmaxf drops a NaN here; the sum below keeps it
  for (int o = L >> 1; o; o >>= 1) mc = fmaxf(mc, __shfl_xor(mc, o, 64));
  float sum = 0.f;
  for (int i = 2 + j; i < 2 + NC; i += L) sum += expf(row[i] - mc);
  for (int o = L >> 1; o; o >>= 1) sum += __shfl_xor(sum, o, 64);
  if (j != 0 || r >= nrow) return;
  const float lse = mc + logf(sum);
  const float z0 = row[0], z1 = row[1], m = fmaxf(z0, z1);
  const float la = (z1 - m) - logf(expf(z0 - m) + expf(z1 - m));
  const long long idx = row0 + r;
  const f32x4 pr = *(const f32x4*)(priors + (idx % P) * 4);
  const f32x4 loc = {row[2 + NC], row[3 + NC], row[4 + NC], row[5 + NC]};
  const f32x4 d = od_decode_one(loc, pr, loc_scale, 0);
  const bool sx = d[0] <= d[2], sy = d[1] <= d[3];
  const f32x4 pb = {sx ? d[0] : d[2], sy ? d[1] : d[3], sx ? d[2] : d[0], sy ? d[3] : d[1]};
  const bool ok = isfinite(pb[0]) && isfinite(pb[1]) && isfinite(pb[2]) && isfinite(pb[3]) && isfinite(la) && isfinite(lse);
  out.pbox[idx] = pb;
  out.ll[idx] = make_float2(ok ? la : __uint_as_float(0x7FC00000u), lse);
}

// One thread's share of a box's candidates: items tid, tid + 256, ... of the box's cell rectangles (level by level, cell by
// cell, A priors per cell).  Keeps the TAL_CACHE largest keys below `bound` (descending in c, their u in cu) and tells
// whether the thread has more below them.  key = (ordered l << 32) | (2^32 - 1 - prior): largest l, then lowest prior.
struct TalBox {
  f32x4 box;
  int cls;     // -1: no class term
  int x0[TAL_MAX_LEVELS], y0[TAL_MAX_LEVELS], nx[TAL_MAX_LEVELS], ny[TAL_MAX_LEVELS];  // the rectangle a level is scanned on
};

__device__ __forceinline__ bool tal_scan(const TalBox& tb, const TalLevels& lv, int A, int tid, const float* __restrict__ predb,
                                         const f32x4* __restrict__ pbox, const float2* __restrict__ ll, int C, float alpha,
                                         float beta, u64 bound, u64 c[TAL_CACHE], float cu[TAL_CACHE]) {
#pragma unroll
  for (int i = 0; i < TAL_CACHE; ++i) c[i] = 0ull, cu[i] = 0.f;
  int below = 0;
#pragma unroll
  for (int l = 0; l < TAL_MAX_LEVELS; ++l) {
    if (l >= lv.n) break;
    const int gw = lv.gw[l], nx = tb.nx[l], items = nx * tb.ny[l] * A;
    const float fgw = (float)gw, fgh = (float)lv.gh[l];
    for (int i = tid; i < items; i += 256) {
      const int cell = i / A, a = i - cell * A;
      const int ry = cell / nx, xx = tb.x0[l] + (cell - ry * nx), yy = tb.y0[l] + ry;
      const float cx = ((float)xx + 0.5f) / fgw, cy = ((float)yy + 0.5f) / fgh;
      if (!(cx > tb.box[0] && cx < tb.box[2] && cy > tb.box[1] && cy < tb.box[3])) continue;
      const int p = lv.base[l] + (yy * gw + xx) * A + a;  // < P: the rectangle lies inside the grid, sum gh*gw*A == P
      const float2 q = ll[p];
      if (!(q.x == q.x)) continue;  // a non-finite row
      const float u = iou_f32(tb.box, pbox[p]);
      if (!(u > 0.f)) continue;
      const bool has = tb.cls >= 0;
      const float zc = has ? predb[(long long)p * C + 2 + tb.cls] : 0.f;
      const float lm = tal_metric(q.x, q.y, has, zc, u, alpha, beta);
      u64 k = ((u64)tal_ordered(lm) << 32) | (u64)(0xFFFFFFFFu - (unsigned)p);
      if (k >= bound) continue;
      ++below;
      if (k > c[TAL_CACHE - 1]) {
        float ku = u;
        c[TAL_CACHE - 1] = k, cu[TAL_CACHE - 1] = ku;
#pragma unroll
        for (int s = TAL_CACHE - 1; s > 0; --s)
          if (c[s] > c[s - 1]) {
            k = c[s], c[s] = c[s - 1], c[s - 1] = k;
            ku = cu[s], cu[s] = cu[s - 1], cu[s - 1] = ku;
          }
      }
    }
  }
  return below > TAL_CACHE;
}

// select pass: one workgroup per (box, image).  Every thread evaluates its candidates once and keeps its best few keys; a
// round is one block-wide maximum over the threads' heads, the owner of the winner claims the prior and moves on to its next
// key (a thread that runs out of kept keys while it has more rescans its share below its last winner).  The maximum does not
// depend on which thread holds which candidate, so the choice is the rule's.
__global__ __launch_bounds__(256) void od_tal_select(const float* __restrict__ priors, const float* __restrict__ pred,
                                                     const float* __restrict__ gt_boxes, const int* __restrict__ gt_classes,
                                                     const int* __restrict__ gt_counts, const int* __restrict__ gt_flags,
                                                     TalLevels lv, int A, int topk, int P, int Gmax, int NC, float alpha,
                                                     float beta, TalPrior pp, u64* __restrict__ claim) {
  __shared__ u64 swave[2][4];  // per-wave partial of a round, double-buffered
  const int g = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, wave = tid >> 6;
  if (g >= min(gt_counts[b], Gmax)) return;  // a padding slot is never read as a box
  if (gt_flags && (gt_flags[(long long)b * Gmax + g] & 1)) return;
  TalBox tb;
  tb.box = *(const f32x4*)(gt_boxes + ((long long)b * Gmax + g) * 4);
  const int cls = gt_classes[(long long)b * Gmax + g];
  tb.cls = cls >= 0 && cls < NC ? cls : -1;
#pragma unroll
  for (int l = 0; l < TAL_MAX_LEVELS; ++l) {
    tb.x0[l] = tb.y0[l] = tb.nx[l] = tb.ny[l] = 0;
    if (l < lv.n) {
      // cells whose centre can lie inside the box, one cell of margin on each side (the strict f32 test decides per cell);
      // fmaxf / fminf turn a NaN bound into the grid's edge, and the clamps happen before the conversion to int
      const float fgw = (float)lv.gw[l], fgh = (float)lv.gh[l];
      const int x0 = (int)fminf(fmaxf(floorf(tb.box[0] * fgw - 0.5f) - 1.f, 0.f), fgw);
      const int y0 = (int)fminf(fmaxf(floorf(tb.box[1] * fgh - 0.5f) - 1.f, 0.f), fgh);
      const int x1 = (int)fmaxf(fminf(ceilf(tb.box[2] * fgw - 0.5f) + 1.f, fgw - 1.f), -1.f);
      const int y1 = (int)fmaxf(fminf(ceilf(tb.box[3] * fgh - 0.5f) + 1.f, fgh - 1.f), -1.f);
      tb.x0[l] = x0, tb.y0[l] = y0, tb.nx[l] = max(x1 - x0 + 1, 0), tb.ny[l] = max(y1 - y0 + 1, 0);
    }
  }
  const int C = NC + 6;
  const float* predb = pred + (long long)b * P * C;
  const f32x4* pbox = pp.pbox + (long long)b * P;
  const float2* ll = pp.ll + (long long)b * P;
  u64* cl = claim + (long long)b * P;

  u64 c[TAL_CACHE], last = ~0ull;
  float cu[TAL_CACHE];
  bool more = tal_scan(tb, lv, A, tid, predb, pbox, ll, C, alpha, beta, last, c, cu);
  int round = 0;
  for (; round < topk; ++round) {
    if (c[0] == 0ull && more) more = tal_scan(tb, lv, A, tid, predb, pbox, ll, C, alpha, beta, last, c, cu);
    u64 best = tal_wave_max_u64(c[0]);
    if ((tid & 63) == 0) swave[round & 1][wave] = best;
    __syncthreads();  // round r + 2 rewrites this buffer only after every wave has passed round r + 1's barrier
    const u64* w = swave[round & 1];
    best = max(max(w[0], w[1]), max(w[2], w[3]));
    if (best == 0ull) break;  // the same value in every thread: fewer candidates than topk
    if (c[0] == best) {       // keys are distinct (the prior index is part of them): one owner
      const unsigned p = 0xFFFFFFFFu - (unsigned)(best & 0xFFFFFFFFull);
      atomicMax(&cl[p], claim_key(false, cu[0], g));
      last = best;
#pragma unroll
      for (int s = 0; s < TAL_CACHE - 1; ++s) c[s] = c[s + 1], cu[s] = cu[s + 1];
      c[TAL_CACHE - 1] = 0ull, cu[TAL_CACHE - 1] = 0.f;
    }
  }
  if (round > 0) return;

  // 3. no candidate at all: the prior of the largest static IoU over all P priors
  u64 fbest = 0ull;
  for (int p = tid; p < P; p += 256) {
    const float v = iou_f32(tb.box, *(const f32x4*)(priors + (long long)p * 4));
    if (v > 0.f) {
      const u64 k = ((u64)__float_as_uint(v) << 32) | (u64)(0xFFFFFFFFu - (unsigned)p);
      fbest = k > fbest ? k : fbest;
    }
  }
  fbest = tal_wave_max_u64(fbest);
  if ((tid & 63) == 0) swave[1][wave] = fbest;  // round 0 used swave[0]
  __syncthreads();
  if (tid == 0) {
    const u64* w = swave[1];
    fbest = max(max(w[0], w[1]), max(w[2], w[3]));
    if (fbest) {
      const unsigned p = 0xFFFFFFFFu - (unsigned)(fbest & 0xFFFFFFFFull);
      atomicMax(&cl[p], claim_key(true, __uint_as_float((unsigned)(fbest >> 32)), g));
    }
  }
}

// metric pass: l of the winning normal claim, recomputed from the claim's u with the select pass's own sequence
__global__ __launch_bounds__(256) void od_tal_metric(const float* __restrict__ pred, const int* __restrict__ gt_classes,
                                                     const u64* __restrict__ claim, TalPrior pp, int P, int Gmax, int NC,
                                                     float alpha, float beta, float* __restrict__ metric) {
  const int b = blockIdx.y, p = blockIdx.x * 256 + threadIdx.x;
  if (p >= P) return;
  const long long idx = (long long)b * P + p;
  const u64 k = claim[idx];
  float lm = 0.f;
  if (k && !((k >> 40) & 1ull)) {
    const int g = 255 - (int)(k & 255ull);
    const int cls = gt_classes[(long long)b * Gmax + g];
    const bool has = cls >= 0 && cls < NC;
    const float2 q = pp.ll[idx];
    const float zc = has ? pred[idx * (NC + 6) + 2 + cls] : 0.f;
    lm = tal_metric(q.x, q.y, has, zc, __uint_as_float((unsigned)(k >> 8)), alpha, beta);
  }
  metric[idx] = lm;
}

// workspace: pbox f32x4 [B*P] | claim u64 [B*P] | (la, lse) [B*P]
constexpr size_t TAL_BYTES_PER_PRIOR = sizeof(f32x4) + sizeof(u64) + sizeof(float2);

}  // namespace

extern "C" size_t od_assign_tal_workspace_bytes(int B, int P, int Gmax) {
  if (B <= 0 || P <= 0 || Gmax <= 0) return 0;
  return (size_t)B * P * TAL_BYTES_PER_PRIOR;  // grows with B*P only
}

extern "C" int od_assign_tal(od_ctx* ctx, const float* priors, const int32_t* grid_hw, int n_levels, int priors_per_cell,
                             const float* pred, const float* gt_boxes, const int32_t* gt_classes, const int32_t* gt_counts,
                             const int32_t* gt_flags, float ign_thr, float alpha, float beta, int topk, int B, int P, int Gmax,
                             int NC, float loc_scale, float* y, int32_t* assigned_gt, int32_t* npos, float* metric,
                             void* workspace, size_t workspace_bytes, void* stream) {
  const char* who = "od_assign_tal";
  OD_REQUIRE(ctx && priors && grid_hw && pred && gt_boxes && gt_classes && gt_counts && y && npos && workspace,
             "%s: null argument", who);
  OD_REQUIRE(B > 0 && B <= 65535 && P > 0 && Gmax > 0 && Gmax <= GMAX, "%s: bad dims (Gmax <= %d)", who, GMAX);
  OD_REQUIRE(NC >= 1 && NC <= TAL_MAX_NC, "%s: NC %d outside 1..%d", who, NC, TAL_MAX_NC);
  OD_REQUIRE(n_levels >= 1 && n_levels <= TAL_MAX_LEVELS, "%s: n_levels %d outside 1..%d", who, n_levels, TAL_MAX_LEVELS);
  OD_REQUIRE(topk >= 1 && topk <= TAL_MAX_TOPK, "%s: topk %d outside 1..%d", who, topk, TAL_MAX_TOPK);
  OD_REQUIRE(priors_per_cell >= 1 && priors_per_cell <= TAL_MAX_A, "%s: priors_per_cell %d outside 1..%d", who,
             priors_per_cell, TAL_MAX_A);
  OD_REQUIRE(loc_scale > 0.f && (!gt_flags || ign_thr > 0.f), "%s: bad thresholds", who);
  OD_REQUIRE(std::isfinite(alpha) && alpha > 0.f && std::isfinite(beta) && beta > 0.f,
             "%s: alpha %g and beta %g must be finite and > 0", who, (double)alpha, (double)beta);
  OD_REQUIRE(((uintptr_t)pred & 15) == 0 && ((uintptr_t)workspace & 15) == 0, "%s: pred and workspace must be 16-byte aligned",
             who);
  TalLevels lv = {};
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
  const size_t rows = (size_t)B * P, need = rows * TAL_BYTES_PER_PRIOR;
  if (workspace_bytes < need) {
    od_set_error("%s: workspace %zu < %zu bytes", who, workspace_bytes, need);
    return OD_ERR_WORKSPACE;
  }
  TalPrior pp;
  pp.pbox = (f32x4*)workspace;
  u64* claim = (u64*)(pp.pbox + rows);
  pp.ll = (float2*)(claim + rows);
  const int C = NC + 6;
  int L = 1;  // lanes per row of the per-prior pass: at most 8 columns per lane up to L = 64; (256 / L) * C <= TAL_TILE
  while (L < 64 && C > 8 * L) L *= 2;
  const int R = 256 / L;
  const long long blocks = ((long long)rows + R - 1) / R;
  OD_REQUIRE(blocks <= 0x7FFFFFFFll, "%s: B * P too large", who);
  hipStream_t s = (hipStream_t)stream;
  OD_CHECK_HIP(hipMemsetAsync(claim, 0, rows * sizeof(u64), s));
  OD_CHECK_HIP(hipMemsetAsync(npos, 0, (size_t)B * 4, s));
  hipLaunchKernelGGL(od_tal_prior, dim3((unsigned)blocks), dim3(256), 0, s, pred, priors, (long long)rows, P, NC, L, loc_scale,
                     pp);
  OD_CHECK_LAUNCH();
  hipLaunchKernelGGL(od_tal_select, dim3(Gmax, B), dim3(256), 0, s, priors, pred, gt_boxes, gt_classes, gt_counts, gt_flags,
                     lv, priors_per_cell, topk, P, Gmax, NC, alpha, beta, pp, claim);
  OD_CHECK_LAUNCH();
  dim3 grid(od_ceil_div(P, 256), B);
  if (gt_flags)
    hipLaunchKernelGGL(od_claim_encode<true>, grid, dim3(256), 0, s, priors, gt_boxes, gt_classes, gt_counts, gt_flags, P,
                       Gmax, NC, ign_thr, loc_scale, (const u64*)claim, y, assigned_gt, npos);
  else
    hipLaunchKernelGGL(od_claim_encode<false>, grid, dim3(256), 0, s, priors, gt_boxes, gt_classes, gt_counts, gt_flags, P,
                       Gmax, NC, ign_thr, loc_scale, (const u64*)claim, y, assigned_gt, npos);
  OD_CHECK_LAUNCH();
  if (metric) {
    hipLaunchKernelGGL(od_tal_metric, grid, dim3(256), 0, s, pred, gt_classes, (const u64*)claim, pp, P, Gmax, NC, alpha, beta,
                       metric);
    OD_CHECK_LAUNCH();
  }
  return OD_OK;
}
