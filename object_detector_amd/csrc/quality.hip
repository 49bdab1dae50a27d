// K10b: quality targets q f32 [B,P] for the quality-aware objectness terms of od_loss_fwd_bwd_quality (loss.hip): one number
// in [0,1] per ASSIGNED prior (y[..., 1] > 0.5), 0 on every other row (background, ignore, region-ignored).  [BUILD-DEFINED]
// rules, frozen; tests/quality_ref.py restates them (this TU is built with -ffp-contract=off, every f32 sequence below is
// evaluated as written).  Common to both entries, per assigned row r of image b = r / P with prior pr = priors[r % P]:
//   d = od_decode_one(pred loc columns, pr, loc_scale, no clip);  pbox = (min(d0, d2), min(d1, d3), max(d0, d2), max(d1, d3)):
//   the decode and the corner sort of od_loss_fwd_bwd_iou / od_tal_prior.  A non-finite pbox coordinate makes the row's
//   predicted IoU 0.
// od_quality_iou (any assigner, or a ready-made target):
//   g = od_decode_one(y loc columns, pr, loc_scale, no clip);  q = clamp(iou_f32(g, pbox), 0, 1).   Exact f32.
// od_quality_tal (TOOD's normalised metric, behind od_assign_tal), in the log domain (beta = 6 at NC = 1024 cannot underflow):
//   g = assigned_gt[r] (a row whose g lies outside 0..Gmax-1 gets q = 0);  u = iou_f32(gt_boxes[b, g], pbox).
//   The row is ALIGNED iff metric[r] < 0 (the l of a normal claim; forced claims carry exactly 0).
//   Per object: lmax = max l, umax = max u over its aligned rows (atomicMax on an order-preserving integer image of the float:
//   the result does not depend on the order of the rows).
//   aligned row: q = expf(l - lmax) * umax (the object's best-aligned positive gets the object's best predicted IoU);
//   assigned, not aligned (a forced claim): q = fmaxf(u, iou_f32(gt_boxes[b, g], pr));  both clamped to [0,1].
//   u, umax and the forced rows are exact f32 sequences; expf is the device's.  Two calls on the same inputs give the same bytes.
// Rows are tested on y[..., 1] before any other column of the row is touched; all row indices are 64-bit.
#include "assign_common.h"
#include "post_common.h"  // od_decode_one

namespace {

// total order of the non-NaN floats as unsigned: larger value, larger key; never 0 (0 = "no row yet" in the tables)
__device__ __forceinline__ unsigned q_ordered(float v) {
  const unsigned b = __float_as_uint(v);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float q_unordered(unsigned k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k);
}

__device__ __forceinline__ f32x4 q_loc(const float* __restrict__ row, int NC) {
  const f32x4 l = {row[2 + NC], row[3 + NC], row[4 + NC], row[5 + NC]};
  return l;
}

// the predicted box of a row, corners sorted; ok = every coordinate finite
__device__ __forceinline__ f32x4 q_pbox(const float* __restrict__ prow, int NC, f32x4 pr, float loc_scale, bool& ok) {
  const f32x4 d = od_decode_one(q_loc(prow, NC), pr, loc_scale, 0);
  const bool sx = d[0] <= d[2], sy = d[1] <= d[3];
  const f32x4 pb = {sx ? d[0] : d[2], sy ? d[1] : d[3], sx ? d[2] : d[0], sy ? d[3] : d[1]};
  ok = isfinite(pb[0]) && isfinite(pb[1]) && isfinite(pb[2]) && isfinite(pb[3]);
  return pb;
}

__device__ __forceinline__ float q_clamp(float q) { return fminf(fmaxf(q, 0.f), 1.f); }  // NaN -> 0

__global__ __launch_bounds__(256) void od_quality_iou_rows(const float* __restrict__ pred, const float* __restrict__ y,
                                                           const float* __restrict__ priors, long long rows, int P, int NC,
                                                           float loc_scale, float* __restrict__ q) {
  const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
  if (r >= rows) return;
  const int C = NC + 6;
  const float* yrow = y + r * C;
  float v = 0.f;
  if (yrow[1] > 0.5f) {
    const f32x4 pr = *(const f32x4*)(priors + (r % P) * 4);
    bool ok;
    const f32x4 pb = q_pbox(pred + r * C, NC, pr, loc_scale, ok);
    const f32x4 g = od_decode_one(q_loc(yrow, NC), pr, loc_scale, 0);
    v = ok ? q_clamp(iou_f32(g, pb)) : 0.f;
  }
  q[r] = v;
}

struct QTal {
  const float* pred;
  const float* y;
  const float* priors;
  const float* gt_boxes;
  const int* assigned_gt;
  const float* metric;
  long long rows;
  int P, Gmax, NC;
  float loc_scale;
  unsigned* lmax;  // [B*Gmax] ordered images, 0 = no aligned row
  unsigned* umax;  // [B*Gmax]
};

// -> is row r assigned to an object of its image?  slot = b * Gmax + g, u = its predicted IoU, pr = its prior
__device__ __forceinline__ bool q_tal_row(const QTal& a, long long r, long long& slot, float& u, f32x4& gb, f32x4& pr) {
  const int C = a.NC + 6;
  if (!(a.y[r * C + 1] > 0.5f)) return false;
  const int g = a.assigned_gt[r];
  if (g < 0 || g >= a.Gmax) return false;
  slot = (r / a.P) * a.Gmax + g;
  gb = *(const f32x4*)(a.gt_boxes + slot * 4);
  pr = *(const f32x4*)(a.priors + (r % a.P) * 4);
  bool ok;
  const f32x4 pb = q_pbox(a.pred + r * C, a.NC, pr, a.loc_scale, ok);
  u = ok ? iou_f32(gb, pb) : 0.f;
  return true;
}

__global__ __launch_bounds__(256) void od_quality_tal_max(QTal a) {
  const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
  if (r >= a.rows) return;
  long long slot;
  float u;
  f32x4 gb, pr;
  if (!q_tal_row(a, r, slot, u, gb, pr)) return;
  const float l = a.metric[r];
  if (!(l < 0.f)) return;
  atomicMax(&a.lmax[slot], q_ordered(l));
  atomicMax(&a.umax[slot], q_ordered(u));  // u >= 0, never NaN (iou_f32 returns 0 where the union is not > 0)
}

__global__ __launch_bounds__(256) void od_quality_tal_write(QTal a, float* __restrict__ q) {
  const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
  if (r >= a.rows) return;
  long long slot;
  float u, v = 0.f;
  f32x4 gb, pr;
  if (q_tal_row(a, r, slot, u, gb, pr)) {
    const float l = a.metric[r];
    if (l < 0.f)  // its own l and u went into the maxima: neither table entry is 0
      v = expf(l - q_unordered(a.lmax[slot])) * q_unordered(a.umax[slot]);
    else
      v = fmaxf(u, iou_f32(gb, pr));
    v = q_clamp(v);
  }
  q[r] = v;
}

int q_common(const char* who, od_ctx* ctx, const float* pred, const float* y, const float* priors, float loc_scale, int B,
             int P, int NC, const float* q, unsigned* blocks) {
  OD_REQUIRE(ctx && pred && y && priors && q, "%s: null argument", who);
  OD_REQUIRE(NC >= 1 && NC <= 1024, "%s: NC = %d outside the supported class counts 1..1024", who, NC);
  OD_REQUIRE(B > 0 && P > 0, "%s: bad dims", who);
  OD_REQUIRE(loc_scale > 0.f, "%s: loc_scale must be > 0", who);
  OD_REQUIRE(((uintptr_t)pred & 15) == 0 && ((uintptr_t)priors & 15) == 0, "%s: pred and priors must be 16-byte aligned", who);
  const long long nb = ((long long)B * P + 255) / 256;
  OD_REQUIRE(nb <= 0x7FFFFFFFll, "%s: B * P too large", who);
  *blocks = (unsigned)nb;
  return OD_OK;
}

}  // namespace

extern "C" int od_quality_iou(od_ctx* ctx, const float* pred, const float* y, const float* priors, float loc_scale, int B,
                              int P, int NC, float* q, void* stream) {
  unsigned blocks;
  if (int rc = q_common("od_quality_iou", ctx, pred, y, priors, loc_scale, B, P, NC, q, &blocks)) return rc;
  hipLaunchKernelGGL(od_quality_iou_rows, dim3(blocks), dim3(256), 0, (hipStream_t)stream, pred, y, priors, (long long)B * P, P,
                     NC, loc_scale, q);
  OD_CHECK_LAUNCH();
  return OD_OK;
}

extern "C" size_t od_quality_tal_workspace_bytes(int B, int Gmax) {
  if (B <= 0 || Gmax <= 0) return 0;
  return (size_t)B * Gmax * 2 * sizeof(unsigned);
}

extern "C" int od_quality_tal(od_ctx* ctx, const float* pred, const float* y, const float* priors, float loc_scale,
                              const float* gt_boxes, const int32_t* assigned_gt, const float* metric, int B, int P, int Gmax,
                              int NC, float* q, void* workspace, size_t workspace_bytes, void* stream) {
  const char* who = "od_quality_tal";
  unsigned blocks;
  if (int rc = q_common(who, ctx, pred, y, priors, loc_scale, B, P, NC, q, &blocks)) return rc;
  OD_REQUIRE(gt_boxes && assigned_gt && metric && workspace, "%s: null argument", who);
  OD_REQUIRE(Gmax > 0 && Gmax <= GMAX, "%s: bad dims (Gmax <= %d)", who, GMAX);
  OD_REQUIRE(((uintptr_t)gt_boxes & 15) == 0 && ((uintptr_t)workspace & 3) == 0,
             "%s: gt_boxes must be 16-byte and workspace 4-byte aligned", who);
  const size_t slots = (size_t)B * Gmax, need = slots * 2 * sizeof(unsigned);
  if (workspace_bytes < need) {
    od_set_error("%s: workspace %zu < %zu bytes", who, workspace_bytes, need);
    return OD_ERR_WORKSPACE;
  }
  QTal a;
  a.pred = pred, a.y = y, a.priors = priors, a.gt_boxes = gt_boxes, a.assigned_gt = assigned_gt, a.metric = metric;
  a.rows = (long long)B * P, a.P = P, a.Gmax = Gmax, a.NC = NC, a.loc_scale = loc_scale;
  a.lmax = (unsigned*)workspace;
  a.umax = a.lmax + slots;
  hipStream_t s = (hipStream_t)stream;
  OD_CHECK_HIP(hipMemsetAsync(workspace, 0, need, s));  // the workspace may arrive dirty
  hipLaunchKernelGGL(od_quality_tal_max, dim3(blocks), dim3(256), 0, s, a);
  OD_CHECK_LAUNCH();
  hipLaunchKernelGGL(od_quality_tal_write, dim3(blocks), dim3(256), 0, s, a, q);
  OD_CHECK_LAUNCH();
  return OD_OK;
}
