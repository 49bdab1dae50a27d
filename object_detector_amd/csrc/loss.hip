// K10: detection loss, forward + gradient w.r.t. the prediction tensor, in one elementwise pass (HBM-bound).
// reference docs/MODEL.md:33-52:
//   objectness : 2-class focal loss (alpha_t, gamma)                    [:33-37]
//   class      : softmax + categorical cross-entropy on assigned priors [:39-44]
//   box        : MSE (doc mode) or smooth-L1 (north_star mode) on the corner-form offsets, assigned priors only [:46-52]
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

// Objectness (focal loss over softmax(l0, l1)) and box columns of one row: p = prediction row, t = target row, g = gradient
// row (g may be p: every column is read before it is written).  Writes g[0], g[1] and g[2+NC .. 2+NC+3], sets l_obj, adds the
// four box terms to l_box.  The one copy of this arithmetic, for od_loss_rows and od_loss_rows_wide.
__device__ __forceinline__ void od_loss_obj_box(const float* p, const float* t, float* g, int NC, float alpha, float gamma,
                                                int box_mode, float w_obj, float w_box, float invn, float& l_obj,
                                                float& l_box) {
  const float t0 = t[0], t1 = t[1];
  const float l0 = p[0], l1 = p[1];  // read beside the targets, not behind the branch on them: one load latency, not two
  const bool pos = t1 > 0.5f;
  float g1 = 0.f;
  if (t0 + t1 > 0.f) {
    const float x = pos ? l0 - l1 : l1 - l0;  // l_other - l_t: p_t = 1 / (1 + exp(x))
    const float nf = x * 0.f;                 // 0, or NaN for a non-finite logit
    const float e = expf(-fabsf(x));
    // v_rcp_f32 (1 ulp) for the two quotients: the thread's dependent chain, not the HBM traffic, is what this kernel waits
    // for at 3 waves per SIMD, and a correctly rounded division is ten dependent instructions
    const float inv = __builtin_amdgcn_rcpf(1.f + e);
    const float pt = (x > 0.f ? e : 1.f) * inv;
    const float om = (x > 0.f ? 1.f : e) * inv;  // 1 - p_t, without the subtraction
    const float lpt = -(fmaxf(x, 0.f) + od_log1p_unit(e));
    const float a = pos ? alpha : 1.f - alpha;
    const float mod = gamma == 2.f ? om * om : powf(om, gamma);  // powf(0, 0) = 1
    // log p_t / (1 - p_t) = -(1 + om/2 + om^2/3 + ...): -1 to the last bit below 2^-24 (and 1 / om stays finite above it)
    const float ratio = om > 0x1p-24f ? lpt * __builtin_amdgcn_rcpf(om) : -1.f;
    l_obj = -a * mod * lpt + nf;
    // d loss / d log p_t = -a * mod * (1 - gamma * pt * ratio);  d log p_t / d l_t = om, d log p_t / d l_other = -om
    const float gt = -a * mod * (1.f - gamma * pt * ratio) * om + nf;
    g1 = pos ? gt : -gt;
  }
  g[0] = -g1 * w_obj * invn;
  g[1] = g1 * w_obj * invn;
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

__global__ __launch_bounds__(256) void od_loss_rows(const float* __restrict__ pred, const float* __restrict__ y,
                                                    float* __restrict__ grad, long long R, int NC, float alpha,
                                                    float gamma, int box_mode, float w_obj, float w_cls, float w_box,
                                                    const int* __restrict__ npos, float* __restrict__ partials) {
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
    od_loss_obj_box(p, t, p, NC, alpha, gamma, box_mode, w_obj, w_box, invn, l_obj, l_box);
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

__global__ __launch_bounds__(256) void od_loss_rows_wide(const float* __restrict__ pred, const float* __restrict__ y,
                                                         float* __restrict__ grad, long long R, int NC, float alpha,
                                                         float gamma, int box_mode, float w_obj, float w_cls, float w_box,
                                                         const int* __restrict__ npos, float* __restrict__ partials) {
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
    od_loss_obj_box(pb + (long long)tid * C, t, gb + (long long)tid * C, NC, alpha, gamma, box_mode, w_obj, w_box, invn,
                    l_obj, l_box);
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

extern "C" int od_loss_fwd_bwd(od_ctx* ctx, const float* pred, const float* y, float* grad, float* losses, int B, int P,
                               int NC, float focal_alpha, float focal_gamma, int box_mode, float w_obj, float w_cls,
                               float w_box, void* workspace, size_t workspace_bytes, void* stream) {
  OD_REQUIRE(ctx && pred && y && grad && losses && workspace, "od_loss_fwd_bwd: null argument");
  OD_REQUIRE(NC >= 1 && NC <= 1024, "od_loss_fwd_bwd: NC = %d outside the supported class counts 1..1024", NC);
  OD_REQUIRE(B > 0 && P > 0, "od_loss_fwd_bwd: bad dims");
  OD_REQUIRE(box_mode == 0 || box_mode == 1, "od_loss_fwd_bwd: box_mode 0 = smooth-L1, 1 = MSE");
  const long long R = (long long)B * P;
  const int nblocks = (int)((R + LROWS - 1) / LROWS);
  const size_t need = 256 + (size_t)nblocks * 3 * sizeof(float);
  if (workspace_bytes < need) {
    od_set_error("od_loss_fwd_bwd: workspace %zu < %zu bytes", workspace_bytes, need);
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
  if (NC > LMAX_LDS_NC) {
    hipLaunchKernelGGL(od_loss_rows_wide, dim3(nblocks), dim3(256), 0, s, pred, y, grad, R, NC, focal_alpha, focal_gamma,
                       box_mode, w_obj, w_cls, w_box, npos, partials);
    OD_CHECK_LAUNCH();
    hipLaunchKernelGGL(od_loss_final, dim3(1), dim3(256), 0, s, partials, nblocks, npos, w_obj, w_cls, w_box, losses);
    OD_CHECK_LAUNCH();
    return OD_OK;
  }
  const size_t lds = (size_t)2 * LROWS * (NC + 6) * sizeof(float);
  if (int rc = od_ensure_lds(ctx, (const void*)&od_loss_rows, lds)) return rc;
  hipLaunchKernelGGL(od_loss_rows, dim3(nblocks), dim3(256), lds, s, pred, y, grad, R, NC, focal_alpha, focal_gamma,
                     box_mode, w_obj, w_cls, w_box, npos, partials);
  OD_CHECK_LAUNCH();
  hipLaunchKernelGGL(od_loss_final, dim3(1), dim3(256), 0, s, partials, nblocks, npos, w_obj, w_cls, w_box, losses);
  OD_CHECK_LAUNCH();
  return OD_OK;
}
