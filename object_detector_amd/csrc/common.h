// Internal helpers shared by every translation unit of libodhip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <unordered_map>

#include "../../include/odhip.h"

struct od_ctx {
  int device;
  void* zero_page;  // 8 KiB of zeros: source for padded / out-of-range lanes of LDS-DMA gathers; a zero bias vector
  float* ones;      // 2048 x 1.0f: identity scale vector of od_conv2d_bwd_data
  int num_cu;
  // largest dynamic-LDS size already granted to each kernel ON THIS DEVICE (hipFuncAttributeMaxDynamicSharedMemorySize is
  // per device, and one process may hold a context per GPU): see od_ensure_lds
  std::unordered_map<const void*, size_t> lds_attr;
};

// Raise the kernel's dynamic-LDS limit to `lds` bytes on ctx's device unless that was already done through this context.
int od_ensure_lds(od_ctx* ctx, const void* fn, size_t lds);

void od_set_error(const char* fmt, ...);

#define OD_CHECK_HIP(expr)                                                                   \
  do {                                                                                       \
    hipError_t e_ = (expr);                                                                  \
    if (e_ != hipSuccess) {                                                                  \
      od_set_error("%s:%d: %s -> %s", __FILE__, __LINE__, #expr, hipGetErrorString(e_));     \
      return OD_ERR_HIP;                                                                     \
    }                                                                                        \
  } while (0)

#define OD_CHECK_LAUNCH()                                                                    \
  do {                                                                                       \
    hipError_t e_ = hipGetLastError();                                                       \
    if (e_ != hipSuccess) {                                                                  \
      od_set_error("%s:%d: kernel launch -> %s", __FILE__, __LINE__, hipGetErrorString(e_)); \
      return OD_ERR_HIP;                                                                     \
    }                                                                                        \
  } while (0)

#define OD_REQUIRE(cond, ...)   \
  do {                          \
    if (!(cond)) {              \
      od_set_error(__VA_ARGS__); \
      return OD_ERR_INVALID;    \
    }                           \
  } while (0)

typedef _Float16 f16;
typedef f16 f16x8 __attribute__((ext_vector_type(8)));
typedef f16 f16x4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

static inline int od_ceil_div(int a, int b) { return (a + b - 1) / b; }
static inline int od_round_up(int a, int b) { return od_ceil_div(a, b) * b; }
// workgroups of 256 threads for a grid-stride loop over nvec items: one item per thread up to 4096 workgroups
static inline unsigned od_grid_for(long long nvec) {
  const long long b = (nvec + 255) / 256;
  return (unsigned)(b > 256 * 16 ? 256 * 16 : (b < 1 ? 1 : b));
}

// ---- launch records.  The forward entry points of the conv families and od_wide_add PREPARE an op (validate it, select
//      the kernel, fill its parameter struct, raise its LDS limit) into launch records, then issue them.  A forward plan
//      prepares each op once, at od_plan_create.
struct od_launch {
  const char* name;                                      // the kernel launched (od_plan_op_kernel_name)
  int (*issue)(const od_launch& l, hipStream_t stream);  // the family's launch call
  const void* fn;
  dim3 grid, block;
  size_t lds;
  alignas(16) unsigned char args[352];  // the kernel's arguments (their structs are private to the family's source file)
  template <class T> const T& arg() const { return *reinterpret_cast<const T*>(args); }
};
struct od_launches {  // one op: six cover a grouped conv issued segment by segment, each with a split-K finish
  int n = 0;
  od_launch l[6];
};

template <class T>
int od_add_launch(od_launches* L, od_launch l, const T& args) {
  static_assert(sizeof(T) <= sizeof(l.args) && alignof(T) <= 16, "kernel arguments do not fit an od_launch");
  OD_REQUIRE(L->n < 6, "%s: more than 6 launches in one op", l.name);
  memcpy(l.args, &args, sizeof(T));
  L->l[L->n++] = l;
  return OD_OK;
}
static inline int od_issue(const od_launches& L, hipStream_t stream) {
  for (int i = 0; i < L.n; ++i)
    if (int rc = L.l[i].issue(L.l[i], stream)) return rc;
  return OD_OK;
}

// the direct entry points: prepare(args..., &L), then issue on the caller's stream
template <class F, class... A>
int od_prepare_issue(void* stream, F prepare, A... args) {
  od_launches L;
  if (int rc = prepare(args..., &L)) return rc;
  return od_issue(L, (hipStream_t)stream);
}
// issue functions of the kernels that take one parameter struct, and of those that take (parameter struct, int)
static inline int od_issue_kp(const od_launch& l, hipStream_t stream) {
  void* args[] = {(void*)l.args};
  OD_CHECK_HIP(hipLaunchKernel(l.fn, l.grid, l.block, args, l.lds, stream));
  return OD_OK;
}
template <class KP>
struct od_kp_int {
  KP p;
  int n;
};
template <class KP>
int od_issue_kp_int(const od_launch& l, hipStream_t stream) {
  const od_kp_int<KP>& a = l.arg<od_kp_int<KP>>();
  void* args[] = {(void*)&a.p, (void*)&a.n};
  OD_CHECK_HIP(hipLaunchKernel(l.fn, l.grid, l.block, args, l.lds, stream));
  return OD_OK;
}

int od_conv_prepare(od_ctx* ctx, const od_conv_desc* d, od_launches* L);
int od_conv_first_prepare(od_ctx* ctx, const uint8_t* x, const void* w, const float* scale, const float* bias, void* out,
                          int B, int H, int W, int Cout, int act, float alpha, od_launches* L);
int od_bottleneck_prepare(od_ctx* ctx, const od_bneck_desc* d, od_launches* L);
int od_stem_prepare(od_ctx* ctx, const od_stem_desc* d, od_launches* L);
int od_wide_prepare(od_ctx* ctx, const od_wide_desc* d, od_launches* L);

// weight gradient (conv_wgrad.hip): wgrad_plan validates a layer and decides, once, which kernel it takes and how its pixels
// are split; the launchers fill the kernel's parameters from the plan and decide nothing.
struct WgradPlan {
  enum Kind { T128, W8, THIN } kind;  // od_conv_wgrad / od_conv_wgrad_w8 / od_conv_wgrad_thin<stride>
  const void* fn;
  const char* name;
  int threads;
  size_t lds;  // dynamic LDS
  int grid;
  int split, chunks_per_split;  // slabs written / 32-pixel chunks per workgroup (thin: one slab per workgroup)
  int rtiles, ctiles;
  int Ho, Wo, M;
  int B, H, W, Cin, Cout, ksize, stride;  // the layer it was made for
};
int wgrad_plan(od_ctx* ctx, int B, int H, int W, int Cin, int Cout, int ksize, int stride, int slabs, WgradPlan* pl);
// launches the plan's kernel (a plan made with slabs = 1) into per-split f32 slabs [pl.split][Cout][k*k*Cin]
int od_wgrad_slabs_impl(od_ctx* ctx, const WgradPlan& pl, const void* x, const void* dz, float* slabs, void* stream);
