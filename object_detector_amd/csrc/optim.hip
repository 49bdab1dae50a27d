// K12 (update part): what turns the flat f32 gradient buffer into the next step's master weights.  All HBM-bound, all f32;
// this TU is built with -ffp-contract=off (it must stay out of the Makefile's CONTRACT_ON): every f32 expression is a
// sequence of separately rounded operations in the order written, which tests/optim_ref.py, ema_ref.py and optim2_ref.py
// restate in numpy bit for bit.
//
//   od_sgd_step[_multi][_ema]  SGD + momentum + weight decay on f32 masters: one flat segment, or one launch over a device
//                      table of segments (each with its own learning rate: the trainer folds the per-layer multipliers of
//                      docs/MODEL.md:84-90 into it), optionally with an exponential moving average of the masters updated
//                      in the same pass; od_ema_update is the average alone over a flat buffer (BatchNorm running statistics)
//   od_optim_step_multi  the same launch for OD_OPT_SGD / NESTEROV / ADAMW with the step's scalars read from od_optim_state
//   od_grad_nonfinite / od_grad_stats / od_optim_prepare   the gradient scan (flag, sum of squares) and the step's scalars
//   od_copy_if_nonzero   guards the BatchNorm running statistics of a step that overflowed
//
// One segment walk (walk16), one update body (optim_segment<KIND, EMA>) behind two __global__ wrappers, one scan
// (od_grad_scan_k<SUMSQ>).  Every legacy entry runs an instantiation of the same body, so a fix lands once.
//
// reference: the Keras optimizer machinery behind the (unseen) `fit` of tk.dl.od.ObjectDetector; specified here by
// docs/MODEL.md:84-90.
#include "common.h"

namespace {

// w -= lr * (m = momentum * m + g * inv_scale + wd * w)
__device__ __forceinline__ void sgd_update(float& w, float& m, float g, float lr, float momentum, float wd, float inv_scale) {
  const float grad = g * inv_scale + wd * w;
  const float mv = momentum * m + grad;
  m = mv;
  w -= lr * mv;
}

// e += omd * (x - e): three separately rounded f32 operations, so that e stays bitwise where x == e -- decay * e + omd * x
// would not
__device__ __forceinline__ void ema_update(float& e, float x, float omd) {
  const float d = x - e;
  const float p = omd * d;
  e = e + p;
}

// Elements in front of the first 16-byte boundary of a run of `count` floats at `p` (0..3, at most count)
__device__ __forceinline__ long long head_to_16(const float* p, long long count) {
  const long long h = (4 - (long long)(((uintptr_t)p >> 2) & 3)) & 3;
  return h < count ? h : count;
}

__device__ __forceinline__ unsigned phase16(const void* p) { return (unsigned)((uintptr_t)p & 15); }

// THE segment walk: a grid-stride pass (blockIdx.x, 256 threads) over `count` elements of buffers that start at p0.
// same_phase = every buffer of the segment sits at p0's distance from a 16-byte boundary (the trainer's always do: offsets
// are multiples of 4 floats in 16-byte-aligned buffers): the aligned body goes as four(i), i = index of the first of four
// elements at a 16-byte boundary, and only the head (< 4 elements) and the tail (< 4) go through one(i), on lanes 0..3 and
// 4..7 of workgroup 0.  Otherwise every element goes through one(i).  Each element is visited exactly once either way, so
// where four() does what one() does per element the bits do not depend on the path.
template <class One, class Four>
__device__ __forceinline__ void walk16(const float* p0, long long count, bool same_phase, One one, Four four) {
  const long long first = (long long)blockIdx.x * 256 + threadIdx.x, stride = (long long)gridDim.x * 256;
  if (!same_phase) {
    for (long long i = first; i < count; i += stride) one(i);
    return;
  }
  const long long head = head_to_16(p0, count);
  const long long nvec = (count - head) >> 2;
  const long long tail0 = head + 4 * nvec;  // first element behind the aligned body
  for (long long i = first; i < nvec; i += stride) four(head + 4 * i);
  if (blockIdx.x == 0 && threadIdx.x < 8) {  // lanes 0..3: the head, lanes 4..7: the tail
    const long long i = threadIdx.x < 4 ? (long long)threadIdx.x : tail0 + (threadIdx.x - 4);
    if (threadIdx.x < 4 ? i < head : i < count) one(i);
  }
}

// ema[i] += omd * (x[i] - ema[i]) over a flat buffer, unless *skip != 0
__global__ __launch_bounds__(256) void od_ema_k(float* __restrict__ ema, const float* __restrict__ x, long long n, float omd,
                                                const int32_t* __restrict__ skip) {
  if (skip && *skip) return;
  walk16(
      ema, n, phase16(x) == phase16(ema), [&](long long i) { ema_update(ema[i], x[i], omd); },
      [&](long long i) {
        f32x4 ev = *(f32x4*)(ema + i);
        const f32x4 xv = *(const f32x4*)(x + i);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          float ek = ev[k];
          ema_update(ek, xv[k], omd);
          ev[k] = ek;
        }
        *(f32x4*)(ema + i) = ev;
      });
}

// What the host resolves once per launch: the constants every element's update reads (1 - beta computed in f32 on the host:
// one rounded subtraction, as the header writes it)
struct optim_hp {
  float momentum;  // beta1 for AdamW
  float beta2, omb1, omb2, eps;
  float omd;  // the average's 1 - decay
  float inv;  // what g is multiplied by where no od_optim_state is given (the od_sgd_step* entries)
};

// One element's update, each line one rounded f32 operation or two as the header splits them.  `v` is touched by AdamW alone.
template <int KIND>
__device__ __forceinline__ void optim_update(float& w, float& m, float& v, float g, float lr, float wd, const optim_hp& hp,
                                             float inv, float bc1, float bc2) {
  if (KIND == OD_OPT_SGD) {
    sgd_update(w, m, g, lr, hp.momentum, wd, inv);
  } else if (KIND == OD_OPT_NESTEROV) {
    const float grad = g * inv + wd * w;
    const float mv = hp.momentum * m + grad;
    m = mv;
    const float u = grad + hp.momentum * mv;
    w = w - lr * u;
  } else {
    const float gh = g * inv;
    m = hp.momentum * m + hp.omb1 * gh;
    v = hp.beta2 * v + hp.omb2 * (gh * gh);
    const float mh = m / bc1;
    const float vh = v / bc2;
    const float den = sqrtf(vh) + hp.eps;
    const float u = mh / den;
    w = w - lr * (u + wd * w);
  }
}

// THE update body: walk16 over one segment around optim_update<KIND>, then ema_update when EMA (4 loads and 3 stores of 4 B
// per parameter where a separate EMA launch would read w a third time).  v is NULL unless KIND == OD_OPT_ADAMW, ema is NULL
// unless EMA: neither is then formed into an address that is read.
template <int KIND, bool EMA>
__device__ __forceinline__ void optim_segment(const od_sgd_seg sg, float* __restrict__ w, float* __restrict__ m,
                                              float* __restrict__ v, const float* __restrict__ g, float* __restrict__ ema,
                                              const optim_hp& hp, float inv, float bc1, float bc2) {
  constexpr bool ADAM = KIND == OD_OPT_ADAMW;
  float* ws = w + sg.offset;
  float* ms = m + sg.offset;
  float* vs = ADAM ? v + sg.offset : nullptr;
  const float* gs = g + sg.offset;
  float* es = EMA ? ema + sg.offset : nullptr;
  const unsigned a = phase16(ws);
  // the 20 B / parameter kinds (SGD, Nesterov without the average) go one by one whatever the phase: measured 1 % faster
  // than their 16-byte body (DESIGN.md "Optimizers and gradient clipping"); same bits either way
  constexpr bool BODY16 = EMA || ADAM;
  const bool same_phase = BODY16 && phase16(ms) == a && phase16(gs) == a && (!ADAM || phase16(vs) == a) && (!EMA || phase16(es) == a);
  walk16(
      ws, sg.count, same_phase,
      [&](long long i) {
        float dummy = 0.f;
        optim_update<KIND>(ws[i], ms[i], ADAM ? vs[i] : dummy, gs[i], sg.lr, sg.weight_decay, hp, inv, bc1, bc2);
        if (EMA) ema_update(es[i], ws[i], hp.omd);
      },
      [&](long long i) {
        f32x4 wv = *(f32x4*)(ws + i), mv = *(f32x4*)(ms + i), vv = {0.f, 0.f, 0.f, 0.f}, ev = {0.f, 0.f, 0.f, 0.f};
        const f32x4 gv = *(const f32x4*)(gs + i);
        if (ADAM) vv = *(f32x4*)(vs + i);
        if (EMA) ev = *(f32x4*)(es + i);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          float wk = wv[k], mk = mv[k], vk = vv[k], ek = ev[k];
          optim_update<KIND>(wk, mk, vk, gv[k], sg.lr, sg.weight_decay, hp, inv, bc1, bc2);
          if (EMA) ema_update(ek, wk, hp.omd);
          wv[k] = wk, mv[k] = mk, vv[k] = vk, ev[k] = ek;
        }
        *(f32x4*)(ws + i) = wv;
        *(f32x4*)(ms + i) = mv;
        if (ADAM) *(f32x4*)(vs + i) = vv;
        if (EMA) *(f32x4*)(es + i) = ev;
      });
}

// multi-tensor form: blockIdx.y = segment of the device table, blockIdx.x strides over its elements.  The step's scalars
// come from *state where it is given (od_optim_step_multi), else g is multiplied by hp.inv (od_sgd_step_multi[_ema]).
template <int KIND, bool EMA>
__global__ __launch_bounds__(256) void od_optim_multi_k(float* __restrict__ w, float* __restrict__ m, float* __restrict__ v,
                                                        const float* __restrict__ g, float* __restrict__ ema,
                                                        const od_sgd_seg* __restrict__ segs, optim_hp hp,
                                                        const od_optim_state* __restrict__ state,
                                                        const int32_t* __restrict__ skip) {
  if (skip && *skip) return;  // a non-finite gradient was found: leave weights, both moments and the average untouched
  float inv = hp.inv, bc1 = 1.f, bc2 = 1.f;
  if (state) inv = state->inv_scale_eff, bc1 = state->bc1, bc2 = state->bc2;
  optim_segment<KIND, EMA>(segs[blockIdx.y], w, m, v, g, ema, hp, inv, bc1, bc2);
}
// one flat segment from by-value arguments (od_sgd_step)
__global__ __launch_bounds__(256) void od_sgd_one_k(float* __restrict__ w, float* __restrict__ m, const float* __restrict__ g,
                                                    long long n, float lr, float wd, optim_hp hp) {
  optim_segment<OD_OPT_SGD, false>(od_sgd_seg{0, n, lr, wd}, w, m, nullptr, g, nullptr, hp, hp.inv, 1.f, 1.f);
}

// ---- the gradient scan: od_grad_nonfinite / od_grad_stats, and od_optim_prepare behind the latter ------------------------
// Workgroups of the scan: a function of n alone, one tile of 1024 vectors per workgroup before the grid starts to stride.
// With the sum of squares at most 1024 (4 per CU: enough 16-byte loads in flight to stream from HBM) so that
// od_optim_prepare_k's ordered sum of the partials stays a few microseconds; the flag alone has no partials and takes up
// to 4096 (measured 0.3 us faster over 43 M floats).
#define OD_STATS_MAX_GROUPS 1024
#define OD_FLAG_MAX_GROUPS 4096
static unsigned grad_scan_groups(long long n, long long max_groups) {
  const long long b = (n / 4 + 1023) / 1024;
  return (unsigned)(b > max_groups ? max_groups : (b < 1 ? 1 : b));
}
static unsigned grad_stats_groups(long long n) { return grad_scan_groups(n, OD_STATS_MAX_GROUPS); }

// exponent field all ones <=> Inf or NaN
__device__ __forceinline__ bool nonfinite_bits(float x) { return (__float_as_uint(x) & 0x7f800000u) == 0x7f800000u; }

// flag |= 1 when any of g[0..n) is Inf or NaN; SUMSQ: plus the sum of squares.  Lane order: each lane adds its vectors tile
// by tile (below), the four elements of a vector in index order, then (workgroup 0, lanes 0..2) its tail element; the 256
// lane sums are folded in LDS by halving (lane t += lane t + s for s = 128 .. 1).  All of it in f64, nothing atomic but the
// integer flag.  Without SUMSQ the result is the flag alone and the order means nothing.
template <bool SUMSQ>
__global__ __launch_bounds__(256) void od_grad_scan_k(const float* __restrict__ g, long long n4, long long n,
                                                      int32_t* __restrict__ flag, double* __restrict__ partials) {
  bool bad = false;
  double acc = 0.0;
  const f32x4* g4 = (const f32x4*)g;
  auto add1 = [&](float x) {
    bad = bad || nonfinite_bits(x);
    if (SUMSQ) acc = acc + (double)x * (double)x;
  };
  auto add = [&](const f32x4 v) { add1(v.x), add1(v.y), add1(v.z), add1(v.w); };
  // a workgroup walks tiles of 1024 consecutive vectors (16 KiB) in grid-stride order; a lane takes vectors t, t + 256,
  // t + 512, t + 768 of the tile: four loads in flight, added in that order
  for (long long base = (long long)blockIdx.x * 1024 + threadIdx.x; base < n4; base += (long long)gridDim.x * 1024) {
    if (base + 768 < n4) {
      const f32x4 a = g4[base], b = g4[base + 256], c = g4[base + 512], d = g4[base + 768];
      add(a), add(b), add(c), add(d);
    } else {
      for (long long i = base; i < n4 && i < base + 1024; i += 256) add(g4[i]);
    }
  }
  if (blockIdx.x == 0 && threadIdx.x < (int)(n - 4 * n4)) add1(g[4 * n4 + threadIdx.x]);
  if (__any(bad) && (threadIdx.x & 63) == 0) atomicOr(flag, 1);
  if constexpr (SUMSQ) {
    __shared__ double red[256];
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
      if ((int)threadIdx.x < s) red[threadIdx.x] = red[threadIdx.x] + red[threadIdx.x + s];
      __syncthreads();
    }
    if (threadIdx.x == 0) partials[blockIdx.x] = red[0];
  }
}

// One workgroup: the partials travel to LDS side by side, lane 0 adds them in ascending order and writes the scalars
__global__ __launch_bounds__(256) void od_optim_prepare_k(const double* __restrict__ partials, int npart, float momentum,
                                                          float beta2, float inv_loss_scale, float max_grad_norm,
                                                          const int32_t* __restrict__ flag, od_optim_state* __restrict__ st) {
  __shared__ double p[OD_STATS_MAX_GROUPS];
  double r[OD_STATS_MAX_GROUPS / 256];  // all of a lane's loads in flight before the first is waited for
#pragma unroll
  for (int k = 0; k < OD_STATS_MAX_GROUPS / 256; ++k) {
    const int i = 256 * k + (int)threadIdx.x;
    r[k] = i < npart ? partials[i] : 0.0;
  }
#pragma unroll
  for (int k = 0; k < OD_STATS_MAX_GROUPS / 256; ++k) p[256 * k + threadIdx.x] = r[k];
  __syncthreads();
  if (threadIdx.x != 0) return;
  double s = 0.0;
  for (int i = 0; i < npart; ++i) s = s + p[i];
  const float norm_raw = sqrtf((float)s);
  const float grad_norm = norm_raw * inv_loss_scale;
  const float clip_coef = max_grad_norm > 0.f ? fminf(1.0f, max_grad_norm / (grad_norm + 1e-6f)) : 1.0f;
  st->grad_norm = grad_norm;
  st->clip_coef = clip_coef;
  st->inv_scale_eff = inv_loss_scale * clip_coef;
  if (*flag == 0) {
    const float b1pow = st->b1pow * momentum, b2pow = st->b2pow * beta2;
    st->step = st->step + 1;
    st->b1pow = b1pow;
    st->b2pow = b2pow;
    st->bc1 = 1.0f - b1pow;
    st->bc2 = 1.0f - b2pow;
  }
}

__global__ void od_flag_clear_k(int32_t* flag) { *flag = 0; }

// dst[0..n) = src[0..n) when *flag != 0 (no-op otherwise): the trainer restores the BatchNorm running statistics of a
// step whose update was skipped (the forward pass that overflowed has already folded its batch statistics into them)
__global__ __launch_bounds__(256) void od_copy_if_k(float* __restrict__ dst, const float* __restrict__ src, long long n,
                                                    const int32_t* __restrict__ flag) {
  if (*flag == 0) return;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) dst[i] = src[i];
}

// ---- host side ---------------------------------------------------------------------------------------------------------
// beta in [0, 1) (false for NaN)
bool unit_half_open(float b) { return b >= 0.f && b < 1.f; }

// the checks every entry that keeps an average shares
int check_ema(const char* who, float omd, const float* ema, const float* a, const float* b, const float* c, const float* d) {
  OD_REQUIRE(omd >= 0.f && omd <= 1.f, "%s: ema_one_minus_decay must be in [0, 1]", who);  // (false for NaN)
  OD_REQUIRE(ema != a && ema != b && ema != c && ema != d, "%s: ema must be a buffer of its own", who);
  return OD_OK;
}

// The table form of the update: the instantiation for (kind, ema != NULL), 256 workgroups per segment
int launch_optim_step(int kind, float* w, float* m, float* v, const float* g, float* ema, const od_sgd_seg* segs, int nseg,
                      const optim_hp& hp, const od_optim_state* state, const int32_t* skip, void* stream) {
  using kernel = void (*)(float*, float*, float*, const float*, float*, const od_sgd_seg*, optim_hp, const od_optim_state*,
                          const int32_t*);
  static const kernel table[3][2] = {
      {od_optim_multi_k<OD_OPT_SGD, false>, od_optim_multi_k<OD_OPT_SGD, true>},
      {od_optim_multi_k<OD_OPT_NESTEROV, false>, od_optim_multi_k<OD_OPT_NESTEROV, true>},
      {od_optim_multi_k<OD_OPT_ADAMW, false>, od_optim_multi_k<OD_OPT_ADAMW, true>}};
  static_assert(OD_OPT_SGD == 0 && OD_OPT_NESTEROV == 1 && OD_OPT_ADAMW == 2, "table order");
  hipLaunchKernelGGL(table[kind][ema != nullptr], dim3(256, nseg), dim3(256), 0, (hipStream_t)stream, w, m, v, g, ema, segs,
                     hp, state, skip);
  OD_CHECK_LAUNCH();
  return OD_OK;
}

// flag[0] = 1 when any of g[0..n) is Inf or NaN, else 0 (cleared by the first launch, set by the second); with `partials`
// the scan leaves the sums of squares there as well
int launch_grad_scan(const char* who, const float* g, long long n, int32_t* flag, double* partials, void* stream) {
  OD_REQUIRE(((uintptr_t)g & 15) == 0, "%s: g must be 16-byte aligned", who);
  hipLaunchKernelGGL(od_flag_clear_k, dim3(1), dim3(1), 0, (hipStream_t)stream, flag);
  OD_CHECK_LAUNCH();
  if (partials)
    hipLaunchKernelGGL(od_grad_scan_k<true>, dim3(grad_stats_groups(n)), dim3(256), 0, (hipStream_t)stream, g, n / 4, n, flag,
                       partials);
  else
    hipLaunchKernelGGL(od_grad_scan_k<false>, dim3(grad_scan_groups(n, OD_FLAG_MAX_GROUPS)), dim3(256), 0, (hipStream_t)stream,
                       g, n / 4, n, flag, partials);
  OD_CHECK_LAUNCH();
  return OD_OK;
}

}  // namespace

extern "C" int od_sgd_step(od_ctx* ctx, float* w, float* m, const float* g, long long n, float lr, float momentum,
                           float weight_decay, float inv_loss_scale, void* stream) {
  OD_REQUIRE(ctx && w && m && g && n > 0, "od_sgd_step: bad argument");
  const optim_hp hp = {momentum, 0.f, 0.f, 0.f, 0.f, 0.f, inv_loss_scale};
  hipLaunchKernelGGL(od_sgd_one_k, dim3(od_grid_for((n + 7) / 8)), dim3(256), 0, (hipStream_t)stream, w, m, g, n, lr,
                     weight_decay, hp);
  OD_CHECK_LAUNCH();
  return OD_OK;
}

extern "C" int od_sgd_step_multi(od_ctx* ctx, float* w, float* m, const float* g, const od_sgd_seg* segs, int nseg,
                                 float momentum, float inv_loss_scale, const int32_t* skip_if_nonzero, void* stream) {
  OD_REQUIRE(ctx && w && m && g && segs && nseg > 0 && nseg <= 65535, "od_sgd_step_multi: bad argument");
  const optim_hp hp = {momentum, 0.f, 0.f, 0.f, 0.f, 0.f, inv_loss_scale};
  return launch_optim_step(OD_OPT_SGD, w, m, nullptr, g, nullptr, segs, nseg, hp, nullptr, skip_if_nonzero, stream);
}

extern "C" int od_sgd_step_multi_ema(od_ctx* ctx, float* w, float* m, const float* g, float* ema, const od_sgd_seg* segs,
                                     int nseg, float momentum, float inv_loss_scale, float ema_one_minus_decay,
                                     const int32_t* skip_if_nonzero, void* stream) {
  OD_REQUIRE(ctx && w && m && g && ema && segs && nseg > 0 && nseg <= 65535, "od_sgd_step_multi_ema: bad argument");
  if (const int rc = check_ema("od_sgd_step_multi_ema", ema_one_minus_decay, ema, w, m, g, nullptr)) return rc;
  const optim_hp hp = {momentum, 0.f, 0.f, 0.f, 0.f, ema_one_minus_decay, inv_loss_scale};
  return launch_optim_step(OD_OPT_SGD, w, m, nullptr, g, ema, segs, nseg, hp, nullptr, skip_if_nonzero, stream);
}

extern "C" int od_ema_update(od_ctx* ctx, float* ema, const float* x, long long n, float one_minus_decay,
                             const int32_t* skip_if_nonzero, void* stream) {
  OD_REQUIRE(ctx && ema && x && n > 0, "od_ema_update: bad argument");
  if (const int rc = check_ema("od_ema_update", one_minus_decay, ema, x, nullptr, nullptr, nullptr)) return rc;
  hipLaunchKernelGGL(od_ema_k, dim3(od_grid_for((n + 3) / 4)), dim3(256), 0, (hipStream_t)stream, ema, x, n, one_minus_decay,
                     skip_if_nonzero);
  OD_CHECK_LAUNCH();
  return OD_OK;
}

extern "C" int od_grad_nonfinite(od_ctx* ctx, const float* g, long long n, int32_t* flag, void* stream) {
  OD_REQUIRE(ctx && g && flag && n > 0, "od_grad_nonfinite: bad argument");
  return launch_grad_scan("od_grad_nonfinite", g, n, flag, nullptr, stream);
}

extern "C" size_t od_grad_stats_workspace_bytes(long long n) {
  return n > 0 ? (size_t)grad_stats_groups(n) * sizeof(double) : 0;
}

extern "C" int od_grad_stats(od_ctx* ctx, const float* g, long long n, int32_t* flag, void* workspace, void* stream) {
  OD_REQUIRE(ctx && g && flag && workspace && n > 0, "od_grad_stats: bad argument");
  OD_REQUIRE(((uintptr_t)workspace & 7) == 0, "od_grad_stats: workspace must be 8-byte aligned");
  return launch_grad_scan("od_grad_stats", g, n, flag, (double*)workspace, stream);
}

extern "C" int od_optim_prepare(od_ctx* ctx, const od_optim_cfg* cfg, const void* workspace, long long n,
                                const int32_t* flag, od_optim_state* state, void* stream) {
  OD_REQUIRE(ctx && cfg && workspace && flag && state && n > 0, "od_optim_prepare: bad argument");
  OD_REQUIRE(((uintptr_t)workspace & 7) == 0, "od_optim_prepare: workspace must be 8-byte aligned");
  OD_REQUIRE(cfg->kind == OD_OPT_SGD || cfg->kind == OD_OPT_NESTEROV || cfg->kind == OD_OPT_ADAMW,
             "od_optim_prepare: unknown optimizer kind %d", cfg->kind);
  OD_REQUIRE(unit_half_open(cfg->momentum) && (cfg->kind != OD_OPT_ADAMW || unit_half_open(cfg->beta2)),
             "od_optim_prepare: momentum / beta must be in [0, 1)");
  hipLaunchKernelGGL(od_optim_prepare_k, dim3(1), dim3(256), 0, (hipStream_t)stream, (const double*)workspace,
                     (int)grad_stats_groups(n), cfg->momentum, cfg->beta2, cfg->inv_loss_scale, cfg->max_grad_norm, flag,
                     state);
  OD_CHECK_LAUNCH();
  return OD_OK;
}

extern "C" int od_optim_step_multi(od_ctx* ctx, const od_optim_cfg* cfg, float* w, float* m, float* v, const float* g,
                                   float* ema, const od_sgd_seg* segs, int nseg, const od_optim_state* state,
                                   const int32_t* skip_if_nonzero, void* stream) {
  OD_REQUIRE(ctx && cfg && w && m && g && segs && state, "od_optim_step_multi: bad argument");
  OD_REQUIRE(nseg > 0 && nseg <= 65535, "od_optim_step_multi: nseg must be in 1..65535");
  OD_REQUIRE(cfg->kind == OD_OPT_SGD || cfg->kind == OD_OPT_NESTEROV || cfg->kind == OD_OPT_ADAMW,
             "od_optim_step_multi: unknown optimizer kind %d", cfg->kind);
  const bool adam = cfg->kind == OD_OPT_ADAMW;
  OD_REQUIRE(adam == (v != nullptr), "od_optim_step_multi: v is the second moment of OD_OPT_ADAMW: required there, NULL otherwise");
  OD_REQUIRE(unit_half_open(cfg->momentum), "od_optim_step_multi: momentum (beta1) must be in [0, 1)");
  OD_REQUIRE(!adam || (unit_half_open(cfg->beta2) && cfg->eps > 0.f), "od_optim_step_multi: beta2 must be in [0, 1) and eps > 0");
  if (ema)
    if (const int rc = check_ema("od_optim_step_multi", cfg->ema_one_minus_decay, ema, w, m, g, v)) return rc;
  const optim_hp hp = {cfg->momentum, cfg->beta2, 1.0f - cfg->momentum, 1.0f - cfg->beta2, cfg->eps, cfg->ema_one_minus_decay,
                       0.f};
  return launch_optim_step(cfg->kind, w, m, v, g, ema, segs, nseg, hp, state, skip_if_nonzero, stream);
}

extern "C" int od_copy_if_nonzero(od_ctx* ctx, float* dst, const float* src, long long n, const int32_t* flag, void* stream) {
  OD_REQUIRE(ctx && dst && src && flag && n > 0, "od_copy_if_nonzero: bad argument");
  hipLaunchKernelGGL(od_copy_if_k, dim3(od_grid_for((n + 3) / 4)), dim3(256), 0, (hipStream_t)stream, dst, src, n, flag);
  OD_CHECK_LAUNCH();
  return OD_OK;
}
