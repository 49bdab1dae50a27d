// K10: detection loss, forward + gradient w.r.t. the prediction tensor, in one elementwise pass (HBM-bound).
// reference docs/MODEL.md:33-52:
//   objectness : 2-class focal loss (alpha_t, gamma)                    [:33-37];
//                through od_loss_fwd_bwd_quality also quality focal / varifocal loss towards soft targets (od_loss_obj_box)
//   class      : softmax + categorical cross-entropy on assigned priors [:39-44]
//   box        : MSE (doc mode) or smooth-L1 (north_star mode) on the corner-form offsets, assigned priors only [:46-52];
//                through od_loss_fwd_bwd_iou also 1 - GIoU / DIoU / CIoU of the DECODED boxes (od_iou_box below)
// Rows: pred/y f32 [R, 2+NC+4] (R = B*P); y as written by od_assign_anchors (row all-zero = ignore).
// total = (sum_obj + sum_cls + sum_box) / max(1, #assigned rows); grad is d total / d pred.
// Reduction is deterministic: per-workgroup partials, then one workgroup sums them in a fixed order.
//
// Arithmetic (f32, restated in f64 by oracle/loss.py): no term is a difference of nearly equal numbers, so a prior whose
// probability has saturated keeps a gradient with full relative precision, for every gamma >= 0 (0 = plain cross-entropy).
//   objectness, x = l_other - l_t, e = exp(-|x|):
//     log p_t = -max(x, 0) - log1p(e);   p_t, om = 1 - p_t = {e, 1} / (1 + e) in the order the sign of x says;
//     d loss / d log p_t = -a * om^g * (1 - g * p_t * (log p_t / om)), the ratio replaced by its limit -1 for om < 2^-24;
//     d log p_t / d l_t = om = -d log p_t / d l_other   (the gradient never forms 1 - p).
//   class:  s = sum over c != first argmax of exp(l_c - max);  log q_c = (l_c - max) - log1p(s);  at the argmax
//     q = 1 / (1 + s) and q - 1 = -s / (1 + s), elsewhere q_c = exp(log q_c) <= 1/2.
// Both row kernels call the same device functions for all of it; they differ only in how the columns reach the thread.
//
// Non-finite input stays visible, because the trainer skips a step by looking at the gradient: a NaN / +-Inf objectness
// logit of a non-ignored row, or a NaN / +-Inf class or box column of an assigned row, makes that row's gradient in those
// columns and the loss component (hence losses[3]) non-finite.  The stable forms alone would turn x = -Inf, a class logit of
// -Inf or a box offset of +-Inf into finite values, so each group adds `value * 0` (0, or NaN for a non-finite value).
// Rows whose target is all zero (ignore) get an exactly zero gradient and add nothing, whatever the prediction holds.
#include "common.h"
#include "post_common.h"  // od_decode_one: the loss is taken on the boxes inference will output

namespace {

constexpr int LROWS = 256;
constexpr int LMAX_LDS_NC = 74;  // od_loss_rows holds 2 x [256][NC+6] f32: 160 KiB of LDS at NC = 74

__global__ __launch_bounds__(256) void od_loss_count(const float* __restrict__ y, long long R, int C, int* __restrict__ npos) {
  __shared__ int sc;
  if (threadIdx.x == 0) sc = 0;
  __syncthreads();
  int c = 0;
  for (long long r = (long long)blockIdx.x * 256 + threadIdx.x; r < R; r += (long long)gridDim.x * 256)
    c += y[r * C + 1] == 1.f;
  if (c) atomicAdd(&sc, c);
  __syncthreads();
  if (threadIdx.x == 0 && sc) atomicAdd(npos, sc);
}

// log(1 + e) for 0 <= e <= 1.  u = fl(1 + e) has lost the low bits of e, and u - 1 is exactly the part it kept, so
// log(u) * e / (u - 1) puts them back; where u == 1 the answer is e.  A tenth of log1pf's instructions (which runs in
// double-float arithmetic), on the dependent chain every row's thread walks.
__device__ __forceinline__ float od_log1p_unit(float e) {
  const float u = 1.f + e, d = u - 1.f;
  return d > 0.f ? logf(u) * (e * __builtin_amdgcn_rcpf(d)) : e;  // NaN stays NaN
}

// Box modes 2 = giou, 3 = diou, 4 = ciou (od_loss_fwd_bwd_iou): 1 - m of the decoded predicted box b and target box g of one
// ASSIGNED row, and its gradient w.r.t. the four loc columns.  [BUILD-DEFINED] placement of eps = 1e-9 (normalised image
// units; real boxes have areas >= 2e-6), restated in f64 with an autograd gradient by tests/iou_loss_ref.py:
//   b, g = od_decode_one(pred loc | target loc, prior, loc_scale, no clip);  x1, x2 = min / max (bx1, bx2), y likewise: a
//   predicted box with crossed corners is made well-formed as in Algorithm 2 of the GIoU paper, the derivative follows the
//   selection;  iw = max(0, min(x2, gx2) - max(x1, gx1)), inter = iw * ih, U = ((wb * hb + wg * hg) - inter) + eps,
//   IoU = inter / U;  cw, ch = sides of the enclosing box;
//   giou: C = cw * ch + eps,          m = IoU - (C - U) / C
//   diou: D = (cw^2 + ch^2) + eps,    m = IoU - rho2 / D     (rho2 = squared centre distance)
//   ciou: v = (4 / pi^2) * (atan2(wg, hg + eps) - atan2(wb, hb + eps))^2,  a = v / (((1 - IoU) + v) + eps),  m = diou - a * v,
//         a held constant in the gradient, as published.
// Every denominator stays positive for a zero-size predicted box: U >= wg * hg, C and D are at least those of g, and
// atan2's derivative divides by wb^2 + (hb + eps)^2 >= eps^2.  At an exact tie of a min / max the derivative is the one of
// the branch `<=` / `>` / `<` below picks (a convention).  v_rcp_f32 (1 ulp) for the quotients, as in the objectness term.
struct od_iou_args {
  const float* priors;  // f32 [P,4]; row r of pred belongs to prior r % P
  int P;
  float loc_scale;
  const float* quality;  // f32 [B*P]: read by assigned rows of a QUAL instantiation only (od_loss_fwd_bwd_quality)
  int obj_mode;          // 1 = quality focal loss, 2 = varifocal loss (QUAL instantiations)
};

constexpr float OD_IOU_EPS = 1e-9f;

// p, t -> the four loc columns of the row.  -> loss; gl[k] = d loss / d p[k] (unscaled).
__device__ __forceinline__ float od_iou_box(const float* p, const float* t, f32x4 pr, float loc_scale, int box_mode,
                                            float gl[4]) {
  const f32x4 lp = {p[0], p[1], p[2], p[3]}, lt = {t[0], t[1], t[2], t[3]};
  const f32x4 b = od_decode_one(lp, pr, loc_scale, 0), g = od_decode_one(lt, pr, loc_scale, 0);
  const bool sx = b[0] <= b[2], sy = b[1] <= b[3];
  const float x1 = sx ? b[0] : b[2], x2 = sx ? b[2] : b[0], y1 = sy ? b[1] : b[3], y2 = sy ? b[3] : b[1];
  const float wb = x2 - x1, hb = y2 - y1, wg = g[2] - g[0], hg = g[3] - g[1];
  const float iwr = fminf(x2, g[2]) - fmaxf(x1, g[0]), ihr = fminf(y2, g[3]) - fmaxf(y1, g[1]);
  const float iw = fmaxf(iwr, 0.f), ih = fmaxf(ihr, 0.f);
  const float inter = iw * ih;
  const float uni = ((wb * hb + wg * hg) - inter) + OD_IOU_EPS;
  const float ru = __builtin_amdgcn_rcpf(uni);
  const float iou = inter * ru;
  const float cw = fmaxf(x2, g[2]) - fminf(x1, g[0]), ch = fmaxf(y2, g[3]) - fminf(y1, g[1]);
  // derivatives w.r.t. (x1, y1, x2, y2) of the well-formed box: inter, then U, then IoU = inter / U
  const float di[4] = {iwr > 0.f && x1 > g[0] ? -ih : 0.f, ihr > 0.f && y1 > g[1] ? -iw : 0.f,
                       iwr > 0.f && x2 < g[2] ? ih : 0.f, ihr > 0.f && y2 < g[3] ? iw : 0.f};
  const float du[4] = {-hb - di[0], -wb - di[1], hb - di[2], wb - di[3]};
  // d cw / d x1, d ch / d y1, d cw / d x2, d ch / d y2
  const float de[4] = {x1 < g[0] ? -1.f : 0.f, y1 < g[1] ? -1.f : 0.f, x2 > g[2] ? 1.f : 0.f, y2 > g[3] ? 1.f : 0.f};
  float m, dm[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) dm[k] = (di[k] - iou * du[k]) * ru;
  if (box_mode == 2) {
    const float c = cw * ch + OD_IOU_EPS;
    const float rc = __builtin_amdgcn_rcpf(c);
    const float uc = uni * rc;  // m = IoU - 1 + U / C
    m = iou - (c - uni) * rc;
#pragma unroll
    for (int k = 0; k < 4; ++k) dm[k] += (du[k] - uc * (de[k] * ((k & 1) ? cw : ch))) * rc;
  } else {
    const float dx = ((x1 + x2) - (g[0] + g[2])) * 0.5f, dy = ((y1 + y2) - (g[1] + g[3])) * 0.5f;
    const float rd = __builtin_amdgcn_rcpf((cw * cw + ch * ch) + OD_IOU_EPS);
    const float pen = (dx * dx + dy * dy) * rd;
    m = iou - pen;
#pragma unroll
    for (int k = 0; k < 4; ++k) dm[k] -= (((k & 1) ? dy : dx) - pen * (2.f * ((k & 1) ? ch : cw) * de[k])) * rd;
    if (box_mode == 4) {
      const float kv = 0.40528473456935109f;  // 4 / pi^2
      const float hbe = hb + OD_IOU_EPS;
      const float da = atan2f(wg, hg + OD_IOU_EPS) - atan2f(wb, hbe);
      const float v = kv * (da * da);
      const float a = v * __builtin_amdgcn_rcpf(((1.f - iou) + v) + OD_IOU_EPS);
      m -= a * v;
      // d v / d wb = -2 kv da * hbe / (wb^2 + hbe^2),  d v / d hb = 2 kv da * wb / (wb^2 + hbe^2)
      const float q = a * (2.f * kv * da) * __builtin_amdgcn_rcpf(wb * wb + hbe * hbe);
      const float avw = -q * hbe, avh = q * wb;  // a * d v / d wb, a * d v / d hb;  wb = x2 - x1, hb = y2 - y1
      dm[0] += avw, dm[2] -= avw, dm[1] += avh, dm[3] -= avh;
    }
  }
  // loss = 1 - m;  back through the corner selection and the decode: d b_k / d loc_k = loc_scale * (pw | ph)
  const float sw = (pr[2] - pr[0]) * loc_scale, sh = (pr[3] - pr[1]) * loc_scale;
  gl[0] = -(sx ? dm[0] : dm[2]) * sw;
  gl[2] = -(sx ? dm[2] : dm[0]) * sw;
  gl[1] = -(sy ? dm[1] : dm[3]) * sh;
  gl[3] = -(sy ? dm[3] : dm[1]) * sh;
  return 1.f - m;
}

// Objectness (focal loss over softmax(l0, l1)) and box columns of one row: p = prediction row, t = target row, g = gradient
// row (g may be p: every column is read before it is written).  Writes g[0], g[1] and g[2+NC .. 2+NC+3], sets l_obj, adds the
// four box terms to l_box.  The one copy of this arithmetic, for od_loss_rows and od_loss_rows_wide.  IOU (box modes 2..4) is
// a compile-time property, so that the smooth-L1 / MSE instantiations keep their code and registers; `row` = the row's
// index in [0, B*P), `ia` the prior table: both are looked at by assigned rows of an IOU or QUAL instantiation only.
//
// QUAL (od_loss_fwd_bwd_quality, obj_mode 1 | 2) is a compile-time property as well: the assigned rows' objectness target is
// the row's quality q = clamp(quality[row], 0, 1) (NaN -> 0), a constant in the gradient.  z = l1 - l0, p = sigmoid(z),
// sp(t) = log(1 + e^t), CE = q * sp(-z) + (1 - q) * sp(z) (both terms >= 0):
//   1 (QFL, Li et al. 2020):      L = alpha * |q - p|^gamma * CE,  gamma >= 1;
//                                 dL/dz = alpha * (gamma * d^(gamma-1) * sgn(p - q) * p * (1 - p) * CE + d^gamma * (p - q)), d = |p - q|
//   2 (varifocal, Zhang et al. 2021): q > 0: L = q * CE, dL/dz = q * (p - q);  q == 0: focal's background term (1 - alpha included)
// p, 1 - p and the two sp come from e = exp(-|z|) as in the focal term; p - q is the one difference the definition forces, taken
// as (1 - q) - (1 - p) where p > 1/2, so that q = 1 on a saturated row gives -(1 - p) exactly.  Background rows run the focal
// arithmetic below unchanged, in every mode.
template <bool IOU, bool QUAL = false>
__device__ __forceinline__ void od_loss_obj_box(const float* p, const float* t, float* g, int NC, float alpha, float gamma,
                                                int box_mode, float w_obj, float w_box, float invn, long long row,
                                                const od_iou_args& ia, float& l_obj, float& l_box) {
  const float t0 = t[0], t1 = t[1];
  const float l0 = p[0], l1 = p[1];  // read beside the targets, not behind the branch on them: one load latency, not two
  const bool pos = t1 > 0.5f;
  float g1 = 0.f;
  bool soft = false;  // an assigned row of a QUAL instantiation that takes a quality term
  float q = 0.f;
  if constexpr (QUAL) {
    if (pos) {
      q = fminf(fmaxf(ia.quality[row], 0.f), 1.f);  // fmaxf drops a NaN
      soft = ia.obj_mode == 1 || q > 0.f;
    }
  }
  // the focal term's view of the row: an assigned row of a QUAL instantiation that is not soft (varifocal, q == 0) is background
  const bool fpos = QUAL ? false : pos;
  if (soft) {
    const float x = l0 - l1;   // -z
    const float nf = x * 0.f;  // 0, or NaN for a non-finite logit
    const float e = expf(-fabsf(x));
    const float inv = __builtin_amdgcn_rcpf(1.f + e);
    const float pp = (x > 0.f ? e : 1.f) * inv;  // p
    const float om = (x > 0.f ? 1.f : e) * inv;  // 1 - p, without the subtraction
    const float l1p = od_log1p_unit(e);
    const float ce = q * (fmaxf(x, 0.f) + l1p) + (1.f - q) * (fmaxf(-x, 0.f) + l1p);  // q * sp(-z) + (1 - q) * sp(z)
    const float pmq = x > 0.f ? pp - q : (1.f - q) - om;
    if (ia.obj_mode == 1) {
      const float d = fabsf(pmq);
      const float dg = gamma == 2.f ? d * d : powf(d, gamma);
      const float dg1 = gamma == 2.f ? d : powf(d, gamma - 1.f);  // powf(0, 0) = 1, and sgn(0) = 0 beside it
      const float sg = pmq > 0.f ? 1.f : (pmq < 0.f ? -1.f : 0.f);
      l_obj = alpha * dg * ce + nf;
      g1 = alpha * (gamma * dg1 * sg * (pp * om) * ce + dg * pmq) + nf;
    } else {
      l_obj = q * ce + nf;
      g1 = q * pmq + nf;
    }
  } else if (t0 + t1 > 0.f) {
    const float x = fpos ? l0 - l1 : l1 - l0;  // l_other - l_t: p_t = 1 / (1 + exp(x))
    const float nf = x * 0.f;                 // 0, or NaN for a non-finite logit
    const float e = expf(-fabsf(x));
    // v_rcp_f32 (1 ulp) for the two quotients: the thread's dependent chain, not the HBM traffic, is what this kernel waits
    // for at 3 waves per SIMD, and a correctly rounded division is ten dependent instructions
    const float inv = __builtin_amdgcn_rcpf(1.f + e);
    const float pt = (x > 0.f ? e : 1.f) * inv;
    const float om = (x > 0.f ? 1.f : e) * inv;  // 1 - p_t, without the subtraction
    const float lpt = -(fmaxf(x, 0.f) + od_log1p_unit(e));
    const float a = fpos ? alpha : 1.f - alpha;
    const float mod = gamma == 2.f ? om * om : powf(om, gamma);  // powf(0, 0) = 1
    // log p_t / (1 - p_t) = -(1 + om/2 + om^2/3 + ...): -1 to the last bit below 2^-24 (and 1 / om stays finite above it)
    const float ratio = om > 0x1p-24f ? lpt * __builtin_amdgcn_rcpf(om) : -1.f;
    l_obj = -a * mod * lpt + nf;
    // d loss / d log p_t = -a * mod * (1 - gamma * pt * ratio);  d log p_t / d l_t = om, d log p_t / d l_other = -om
    const float gt = -a * mod * (1.f - gamma * pt * ratio) * om + nf;
    g1 = fpos ? gt : -gt;
  }
  g[0] = -g1 * w_obj * invn;
  g[1] = g1 * w_obj * invn;
  if constexpr (IOU) {
    float gl[4] = {0.f, 0.f, 0.f, 0.f};
    if (pos) {
      const float* pl = p + 2 + NC;
      const float* tl = t + 2 + NC;
      // 0, or NaN for a non-finite loc column: fminf / fmaxf and the clamps would hide one
      const float nf = (((pl[0] + pl[1]) + (pl[2] + pl[3])) + ((tl[0] + tl[1]) + (tl[2] + tl[3]))) * 0.f;
      const f32x4 pr = *(const f32x4*)(ia.priors + 4 * (row % ia.P));
      l_box += od_iou_box(pl, tl, pr, ia.loc_scale, box_mode, gl) + nf;
#pragma unroll
      for (int k = 0; k < 4; ++k) gl[k] = (gl[k] + nf) * w_box * invn;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) g[2 + NC + k] = gl[k];
    return;
  }
  for (int k = 0; k < 4; ++k) {
    float gg = 0.f;
    if (pos) {
      const float d = p[2 + NC + k] - t[2 + NC + k];
      float l;
      if (box_mode == 0) {  // smooth-L1, beta = 1
        const float ad = fabsf(d);
        l = ad < 1.f ? 0.5f * d * d : ad - 0.5f;
        gg = ad < 1.f ? d : (d > 0.f ? 1.f : -1.f);
      } else {  // MSE over the 4 coordinates (docs/MODEL.md:46-48)
        l = 0.25f * d * d;
        gg = 0.5f * d;
      }
      l_box += l;
      gg = (gg + d * 0.f) * w_box * invn;  // d * 0: the clamped smooth-L1 slope would hide a non-finite offset
    }
    g[2 + NC + k] = gg;
  }
}

// Class softmax cross-entropy of one assigned row, as three passes over its logits in ascending class order (the caller
// stages them): od_cls_max over every logit, od_cls_sum over every logit, od_cls_finish once, od_cls_grad per (logit, target).
struct od_cls_row {
  float mx, mn, s;
  int imax;            // first maximum: its term exp(0) = 1 is the `1` of log1p, not part of s
  float lse, q1, q1m1; // log sum_c exp(l_c - mx);  q and q - 1 of class imax = 1 / (1 + s) and -s / (1 + s)
};

__device__ __forceinline__ void od_cls_max(od_cls_row& r, int c, float v) {
  if (c == 0) {
    r.mx = r.mn = v;
    r.imax = 0;
    r.s = 0.f;
  } else {
    if (v > r.mx) {
      r.mx = v;
      r.imax = c;
    }
    r.mn = fminf(r.mn, v);
  }
}

__device__ __forceinline__ void od_cls_sum(od_cls_row& r, int c, float v) {
  if (c != r.imax) r.s += expf(v - r.mx);
}

__device__ __forceinline__ void od_cls_finish(od_cls_row& r) {
  const float nf = (r.mx + r.mn) * 0.f;  // NaN where a logit is +-Inf (a NaN logit has already made s NaN)
  const float inv = 1.f / (1.f + r.s);
  r.lse = log1pf(r.s) + nf;
  r.q1 = inv + nf;
  r.q1m1 = -r.s * inv + nf;
}

// -> d l_cls / d l_c = q_c - t_c (unscaled); subtracts t_c * log q_c from l_cls.  Only class imax can have q near 1, and
// there q - 1 = -s / (1 + s) has no cancellation; every other class has q <= 1/2.
__device__ __forceinline__ float od_cls_grad(const od_cls_row& r, int c, float v, float t, float& l_cls) {
  const float lq = (v - r.mx) - r.lse;
  l_cls -= t * lq;
  return c == r.imax ? (t == 1.f ? r.q1m1 : r.q1 - t) : expf(lq) - t;
}

template <bool IOU, bool QUAL>
__global__ __launch_bounds__(256) void od_loss_rows(const float* __restrict__ pred, const float* __restrict__ y,
                                                    float* __restrict__ grad, long long R, int NC, float alpha,
                                                    float gamma, int box_mode, float w_obj, float w_cls, float w_box,
                                                    const int* __restrict__ npos, float* __restrict__ partials,
                                                    od_iou_args ia) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int C = NC + 6, tid = threadIdx.x;
  float* sp = sm;                // [LROWS][C] pred -> grad
  float* sy = sm + LROWS * C;    // [LROWS][C]; its first 12 floats hold the wave partials once the rows are done with y
  float (*red)[4] = (float (*)[4])sy;  // no static LDS: at NC = 74 the two row blocks are the whole 160 KiB
  const long long r0 = (long long)blockIdx.x * LROWS;
  const int nrows = (int)((R - r0) < LROWS ? (R - r0) : LROWS);
  const int nel = nrows * C;
  for (int i = tid * 4; i < nel; i += 256 * 4) {
    if (i + 3 < nel) {
      *(f32x4*)(sp + i) = *(const f32x4*)(pred + r0 * C + i);
      *(f32x4*)(sy + i) = *(const f32x4*)(y + r0 * C + i);
    } else {
      for (int e = i; e < nel; ++e) {
        sp[e] = pred[r0 * C + e];
        sy[e] = y[r0 * C + e];
      }
    }
  }
  __syncthreads();
  const float invn = 1.f / (float)max(1, *npos);
  float l_obj = 0.f, l_cls = 0.f, l_box = 0.f;
  if (tid < nrows) {
    float* p = sp + tid * C;
    const float* t = sy + tid * C;
    od_loss_obj_box<IOU, QUAL>(p, t, p, NC, alpha, gamma, box_mode, w_obj, w_box, invn, r0 + tid, ia, l_obj, l_box);
    if (t[1] > 0.5f) {
      od_cls_row cr;
      for (int c = 0; c < NC; ++c) od_cls_max(cr, c, p[2 + c]);
      for (int c = 0; c < NC; ++c) od_cls_sum(cr, c, p[2 + c]);
      od_cls_finish(cr);
      for (int c = 0; c < NC; ++c) p[2 + c] = od_cls_grad(cr, c, p[2 + c], t[2 + c], l_cls) * w_cls * invn;
    } else {
      for (int c = 0; c < NC; ++c) p[2 + c] = 0.f;
    }
  }
  __syncthreads();
  for (int i = tid * 4; i < nel; i += 256 * 4) {
    if (i + 3 < nel) {
      *(f32x4*)(grad + r0 * C + i) = *(const f32x4*)(sp + i);
    } else {
      for (int e = i; e < nel; ++e) grad[r0 * C + e] = sp[e];
    }
  }
  // deterministic block reduction: wave shuffle tree, then 4 wave partials added in order (red = sy: every read of y
  // lies before the barrier above, and the copy-out reads sp only)
  float v[3] = {l_obj, l_cls, l_box};
#pragma unroll
  for (int k = 0; k < 3; ++k) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v[k] += __shfl_down(v[k], off);
    if ((tid & 63) == 0) red[k][tid >> 6] = v[k];
  }
  __syncthreads();
  if (tid < 3) partials[(long long)blockIdx.x * 3 + tid] = ((red[tid][0] + red[tid][1]) + red[tid][2]) + red[tid][3];
}

// od_loss_rows for NC > 74, where two [256][NC+6] row blocks no longer fit the LDS: the same rows per workgroup and the same
// device functions called in the same order, the class columns streamed through two LDS tiles [256][33] (pred, y) in three
// sweeps (max, sum of expf, gradient + loss).  Objectness and box columns are read and written by the row's thread directly.
constexpr int LW_CW = 32, LW_LD = LW_CW + 1;

__device__ __forceinline__ void od_loss_stage(const float* __restrict__ src, int C, int nrows, int col0, int ncols,
                                              float* tile) {
  for (int i = threadIdx.x; i < nrows * LW_CW; i += 256) {
    const int r = i / LW_CW, c = i % LW_CW;
    if (c < ncols) tile[r * LW_LD + c] = src[(long long)r * C + col0 + c];
  }
}

template <bool IOU, bool QUAL>
__global__ __launch_bounds__(256) void od_loss_rows_wide(const float* __restrict__ pred, const float* __restrict__ y,
                                                         float* __restrict__ grad, long long R, int NC, float alpha,
                                                         float gamma, int box_mode, float w_obj, float w_cls, float w_box,
                                                         const int* __restrict__ npos, float* __restrict__ partials,
                                                         od_iou_args ia) {
  __shared__ float tp[LROWS * LW_LD], ty[LROWS * LW_LD];
  __shared__ float red[3][4];
  const int C = NC + 6, tid = threadIdx.x;
  const long long r0 = (long long)blockIdx.x * LROWS;
  const int nrows = (int)((R - r0) < LROWS ? (R - r0) : LROWS);
  const float* pb = pred + r0 * C;
  const float* yb = y + r0 * C;
  float* gb = grad + r0 * C;
  const float invn = 1.f / (float)max(1, *npos);
  float l_obj = 0.f, l_cls = 0.f, l_box = 0.f;
  bool pos = false;
  if (tid < nrows) {
    const float* t = yb + (long long)tid * C;
    pos = t[1] > 0.5f;
    od_loss_obj_box<IOU, QUAL>(pb + (long long)tid * C, t, gb + (long long)tid * C, NC, alpha, gamma, box_mode, w_obj, w_box,
                         invn, r0 + tid, ia, l_obj, l_box);
  }
  // ---- class: softmax cross-entropy on assigned rows; zero gradient elsewhere ----
  const bool any_pos = __syncthreads_or(pos);
  od_cls_row cr = {};
  for (int sweep = 0; sweep < (any_pos ? 2 : 0); ++sweep) {
    for (int c0 = 0; c0 < NC; c0 += LW_CW) {
      const int w = min(LW_CW, NC - c0);
      od_loss_stage(pb, C, nrows, 2 + c0, w, tp);
      __syncthreads();
      if (pos) {
        const float* q = tp + tid * LW_LD;
        if (sweep == 0) {
          for (int c = 0; c < w; ++c) od_cls_max(cr, c0 + c, q[c]);
        } else {
          for (int c = 0; c < w; ++c) od_cls_sum(cr, c0 + c, q[c]);
        }
      }
      __syncthreads();
    }
  }
  od_cls_finish(cr);
  for (int c0 = 0; c0 < NC; c0 += LW_CW) {
    const int w = min(LW_CW, NC - c0);
    if (any_pos) {
      od_loss_stage(pb, C, nrows, 2 + c0, w, tp);
      od_loss_stage(yb, C, nrows, 2 + c0, w, ty);
      __syncthreads();
      if (pos) {
        float* q = tp + tid * LW_LD;
        const float* t = ty + tid * LW_LD;
        for (int c = 0; c < w; ++c) q[c] = od_cls_grad(cr, c0 + c, q[c], t[c], l_cls) * w_cls * invn;
      } else if (tid < nrows) {
        float* q = tp + tid * LW_LD;
        for (int c = 0; c < w; ++c) q[c] = 0.f;
      }
      __syncthreads();
    }
    for (int i = tid; i < nrows * LW_CW; i += 256) {
      const int r = i / LW_CW, c = i % LW_CW;
      if (c < w) gb[(long long)r * C + 2 + c0 + c] = any_pos ? tp[r * LW_LD + c] : 0.f;
    }
    __syncthreads();
  }
  float v[3] = {l_obj, l_cls, l_box};
#pragma unroll
  for (int k = 0; k < 3; ++k) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v[k] += __shfl_down(v[k], off);
    if ((tid & 63) == 0) red[k][tid >> 6] = v[k];
  }
  __syncthreads();
  if (tid < 3) partials[(long long)blockIdx.x * 3 + tid] = ((red[tid][0] + red[tid][1]) + red[tid][2]) + red[tid][3];
}

__global__ __launch_bounds__(256) void od_loss_final(const float* __restrict__ partials, int nblocks,
                                                     const int* __restrict__ npos, float w_obj, float w_cls, float w_box,
                                                     float* __restrict__ losses) {
  __shared__ float red[3][256];
  const int tid = threadIdx.x;
  float a[3] = {0.f, 0.f, 0.f};
  for (int i = tid; i < nblocks; i += 256)
    for (int k = 0; k < 3; ++k) a[k] += partials[(long long)i * 3 + k];
  for (int k = 0; k < 3; ++k) red[k][tid] = a[k];
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (tid < s)
      for (int k = 0; k < 3; ++k) red[k][tid] += red[k][tid + s];
    __syncthreads();
  }
  if (tid == 0) {
    const float invn = 1.f / (float)max(1, *npos);
    losses[0] = red[0][0] * w_obj * invn;
    losses[1] = red[1][0] * w_cls * invn;
    losses[2] = red[2][0] * w_box * invn;
    losses[3] = (losses[0] + losses[1]) + losses[2];
  }
}

}  // namespace

extern "C" size_t od_loss_workspace_bytes(int B, int P) {
  if (B <= 0 || P <= 0) return 0;
  const long long R = (long long)B * P;
  return 256 + (size_t)((R + LROWS - 1) / LROWS) * 3 * sizeof(float);
}

namespace {

template <bool IOU, bool QUAL>
int od_loss_launch(od_ctx* ctx, const float* pred, const float* y, float* grad, float* losses, long long R, int NC,
                   float focal_alpha, float focal_gamma, int box_mode, float w_obj, float w_cls, float w_box, int* npos,
                   float* partials, od_iou_args ia, hipStream_t s) {
  const int nblocks = (int)((R + LROWS - 1) / LROWS);
  if (NC > LMAX_LDS_NC) {
    hipLaunchKernelGGL((od_loss_rows_wide<IOU, QUAL>), dim3(nblocks), dim3(256), 0, s, pred, y, grad, R, NC, focal_alpha,
                       focal_gamma, box_mode, w_obj, w_cls, w_box, npos, partials, ia);
    OD_CHECK_LAUNCH();
  } else {
    const size_t lds = (size_t)2 * LROWS * (NC + 6) * sizeof(float);
    if (int rc = od_ensure_lds(ctx, (const void*)&od_loss_rows<IOU, QUAL>, lds)) return rc;
    hipLaunchKernelGGL((od_loss_rows<IOU, QUAL>), dim3(nblocks), dim3(256), lds, s, pred, y, grad, R, NC, focal_alpha, focal_gamma,
                       box_mode, w_obj, w_cls, w_box, npos, partials, ia);
    OD_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(od_loss_final, dim3(1), dim3(256), 0, s, partials, nblocks, npos, w_obj, w_cls, w_box, losses);
  OD_CHECK_LAUNCH();
  return OD_OK;
}

// All entry points: `fn` names the caller in error messages.  obj_mode 0 (focal) never looks at `quality`.
int od_loss_run(const char* fn, od_ctx* ctx, const float* pred, const float* y, const float* priors, float* grad,
                float* losses, int B, int P, int NC, float focal_alpha, float focal_gamma, int box_mode, float loc_scale,
                float w_obj, float w_cls, float w_box, void* workspace, size_t workspace_bytes, void* stream,
                const float* quality = nullptr, int obj_mode = 0) {
  OD_REQUIRE(ctx && pred && y && grad && losses && workspace, "%s: null argument", fn);
  OD_REQUIRE(NC >= 1 && NC <= 1024, "%s: NC = %d outside the supported class counts 1..1024", fn, NC);
  OD_REQUIRE(B > 0 && P > 0, "%s: bad dims", fn);
  OD_REQUIRE(box_mode >= 0 && box_mode <= 4, "%s: box_mode 0 = smooth-L1, 1 = MSE, 2 = giou, 3 = diou, 4 = ciou", fn);
  const bool iou = box_mode >= 2;
  OD_REQUIRE(!iou || priors, "%s: box modes 2..4 need the prior table", fn);
  OD_REQUIRE(!iou || ((uintptr_t)priors & 15) == 0, "%s: priors must be 16-byte aligned", fn);
  const long long R = (long long)B * P;
  const int nblocks = (int)((R + LROWS - 1) / LROWS);
  const size_t need = 256 + (size_t)nblocks * 3 * sizeof(float);
  if (workspace_bytes < need) {
    od_set_error("%s: workspace %zu < %zu bytes", fn, workspace_bytes, need);
    return OD_ERR_WORKSPACE;
  }
  hipStream_t s = (hipStream_t)stream;
  int* npos = (int*)workspace;
  float* partials = (float*)((char*)workspace + 256);
  OD_CHECK_HIP(hipMemsetAsync(npos, 0, 4, s));
  int cb = (int)((R + 255) / 256);
  if (cb > 2048) cb = 2048;
  hipLaunchKernelGGL(od_loss_count, dim3(cb), dim3(256), 0, s, y, R, NC + 6, npos);
  OD_CHECK_LAUNCH();
  const bool qual = obj_mode != 0;
  const od_iou_args ia = {iou ? priors : nullptr, P, loc_scale, qual ? quality : nullptr, obj_mode};
#define OD_LOSS_LAUNCH(IOU_, QUAL_)                                                                                     \
  od_loss_launch<IOU_, QUAL_>(ctx, pred, y, grad, losses, R, NC, focal_alpha, focal_gamma, box_mode, w_obj, w_cls, w_box, \
                              npos, partials, ia, s)
  if (qual) return iou ? OD_LOSS_LAUNCH(true, true) : OD_LOSS_LAUNCH(false, true);
  return iou ? OD_LOSS_LAUNCH(true, false) : OD_LOSS_LAUNCH(false, false);
#undef OD_LOSS_LAUNCH
}

}  // namespace

extern "C" int od_loss_fwd_bwd_iou(od_ctx* ctx, const float* pred, const float* y, const float* priors, float* grad,
                                   float* losses, int B, int P, int NC, float focal_alpha, float focal_gamma, int box_mode,
                                   float loc_scale, float w_obj, float w_cls, float w_box, void* workspace,
                                   size_t workspace_bytes, void* stream) {
  return od_loss_run("od_loss_fwd_bwd_iou", ctx, pred, y, priors, grad, losses, B, P, NC, focal_alpha, focal_gamma, box_mode,
                     loc_scale, w_obj, w_cls, w_box, workspace, workspace_bytes, stream);
}

extern "C" int od_loss_fwd_bwd(od_ctx* ctx, const float* pred, const float* y, float* grad, float* losses, int B, int P,
                               int NC, float focal_alpha, float focal_gamma, int box_mode, float w_obj, float w_cls,
                               float w_box, void* workspace, size_t workspace_bytes, void* stream) {
  OD_REQUIRE(box_mode == 0 || box_mode == 1, "od_loss_fwd_bwd: box_mode 0 = smooth-L1, 1 = MSE");
  return od_loss_run("od_loss_fwd_bwd", ctx, pred, y, nullptr, grad, losses, B, P, NC, focal_alpha, focal_gamma, box_mode, 0.f,
                     w_obj, w_cls, w_box, workspace, workspace_bytes, stream);
}

extern "C" int od_loss_fwd_bwd_quality(od_ctx* ctx, const float* pred, const float* y, const float* priors, float* grad,
                                       float* losses, int B, int P, int NC, float focal_alpha, float focal_gamma,
                                       int box_mode, float loc_scale, float w_obj, float w_cls, float w_box,
                                       const float* quality, int obj_mode, void* workspace, size_t workspace_bytes,
                                       void* stream) {
  const char* fn = "od_loss_fwd_bwd_quality";
  OD_REQUIRE(obj_mode >= 0 && obj_mode <= 2, "%s: obj_mode 0 = focal, 1 = quality focal (qfl), 2 = varifocal (vfl)", fn);
  OD_REQUIRE(obj_mode == 0 || quality, "%s: obj_mode %d needs the quality targets", fn, obj_mode);
  OD_REQUIRE(obj_mode != 1 || focal_gamma >= 1.f,
             "%s: qfl needs focal_gamma >= 1 (got %g): below 1 the gradient is unbounded at p = q", fn, (double)focal_gamma);
  return od_loss_run(fn, ctx, pred, y, priors, grad, losses, B, P, NC, focal_alpha, focal_gamma, box_mode, loc_scale, w_obj,
                     w_cls, w_box, workspace, workspace_bytes, stream, quality, obj_mode);
}
