// Trainer -> detector weight refresh (od_net_refresh): the inference tensors of a live network -- per layer an f16 pack
// [Cout_pad][Kpad] and the folded f32 scale / bias [Cout_pad] -- rewritten in ONE launch from the trainer's flat f32
// parameter and running-statistics buffers.  Plans, extra pipelines and captured graphs hold raw pointers to those
// tensors, so rewriting them in place keeps all of them valid.
//
// Built with -ffp-contract=off like every file that is not a convolution: the fold is the expression of od_bn_fold_k
// (weights.fold_bn on the host), one correctly rounded f32 operation each, and numpy float32 reproduces it bit for bit.
// hipcc's default kernel mode keeps f32 and f16 subnormals and rounds to nearest even, so the (f16) conversion is numpy's
// astype(np.float16): overflow to Inf, subnormals kept, -0 stays -0.
#include "common.h"

namespace {

// One layer of the table.  The launch is DESTINATION-driven: a thread owns 8 consecutive f16 of the pack (one 16-byte
// store), padding included, so every destination element is written exactly once and nothing is assumed about what the
// buffer held.  The 8 sources of a chunk are consecutive f32 of one master row whenever Cin is a multiple of 8 (every
// layer but the image layer): two 16-byte loads when that address is 16-byte aligned, element by element otherwise
// (ragged Cin, the row tail, an offset that is only 4-byte aligned).  Adjacent lanes read adjacent 32 bytes and write
// adjacent 16 bytes.
__device__ __forceinline__ void refresh_layer(const od_refresh_layer L, const float* __restrict__ params,
                                              const float* __restrict__ stats, float eps) {
  const int tid = threadIdx.x;
  // ---- per-channel fold: the first workgroups of the layer (a grid stride covers any Cout_pad) ----
  if (L.scale_dst && L.bias_dst) {
    float* __restrict__ sc_dst = (float*)L.scale_dst;
    float* __restrict__ bi_dst = (float*)L.bias_dst;
    for (int c = blockIdx.x * 256 + tid; c < L.Cout_pad; c += gridDim.x * 256) {
      float sc = 0.f, bi = 0.f;
      if (c < L.Cout) {
        if (L.has_bn) {
          const float g = params[L.gamma_offset + c], b = params[L.beta_offset + c];
          const float m = stats[L.mean_offset + c], v = stats[L.var_offset + c];
          sc = g / sqrtf(v + eps);  // correctly rounded divide / sqrt, no contraction: = numpy f32
          bi = b - m * sc;
          if (L.first) sc = sc / 255.0f;  // the uint8 input's normalisation, folded in behind the bias
        } else {
          sc = 1.f;
          bi = params[L.beta_offset + c];
        }
      }
      sc_dst[c] = sc;
      bi_dst[c] = bi;
    }
  }
  // ---- pack ----
  const int taps = L.ksize * L.ksize;
  const int Ksrc = taps * L.Cin;              // one master row
  const int Klive = Ksrc * L.cin_repeat;      // live columns of a pack row
  const int cpr = L.Kpad >> 3;                // 8-element chunks per pack row (Kpad is a multiple of 8)
  const long long nchunks = (long long)L.Cout_pad * cpr;
  const float* __restrict__ w = params + L.w_offset;
  f16* __restrict__ dst = (f16*)L.w_dst;
  const bool dst_vec = ((uintptr_t)dst & 15) == 0;
  const int rc = L.cin_repeat * L.Cin;  // pack columns of one tap
  // master-row index of pack column c, and how many sources from there on are consecutive (cin_repeat == 1: the pack row
  // IS the master row, column for column; 2: a run ends with its Cin channels)
  auto source = [&](int c, int& run) {
    if (L.cin_repeat == 1) {
      run = Ksrc - c;
      return c;
    }
    const int tap = c / rc;
    int ci = c - tap * rc;
    if (ci >= L.Cin) ci -= L.Cin;
    run = L.Cin - ci;
    return tap * L.Cin + ci;
  };
  for (long long t = (long long)blockIdx.x * 256 + tid; t < nchunks; t += (long long)gridDim.x * 256) {
    const int row = (int)(t / cpr), col = (int)(t - (long long)row * cpr) * 8;
    f16x8 o = {0, 0, 0, 0, 0, 0, 0, 0};
    if (row < L.Cout && col < Klive) {
      const float* wr = w + (long long)row * Ksrc;
      int run;
      const float* src = wr + source(col, run);
      if (run >= 8 && ((uintptr_t)src & 15) == 0) {
        const f32x4 a = *(const f32x4*)src, b = *(const f32x4*)(src + 4);
        o = f16x8{(f16)a[0], (f16)a[1], (f16)a[2], (f16)a[3], (f16)b[0], (f16)b[1], (f16)b[2], (f16)b[3]};
      } else if (run >= 8) {
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = (f16)src[e];
      } else {  // the scalar tail: every live column finds its own source
#pragma unroll
        for (int e = 0; e < 8; ++e)
          if (col + e < Klive) o[e] = (f16)wr[source(col + e, run)];
      }
    }
    f16* d = dst + t * 8;
    if (dst_vec) {
      *(f16x8*)d = o;
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) d[e] = o[e];
    }
  }
}

// blockIdx.y = entry of the device table, blockIdx.x strides over its 8-element chunks
__global__ __launch_bounds__(256) void od_net_refresh_k(const float* __restrict__ params, const float* __restrict__ stats,
                                                        const od_refresh_layer* __restrict__ layers, float eps) {
  refresh_layer(layers[blockIdx.y], params, stats, eps);
}

}  // namespace

extern "C" int od_net_refresh(od_ctx* ctx, const float* params_flat, const float* run_stats_flat,
                              const od_refresh_layer* layers, int nlayers, float eps, void* stream) {
  OD_REQUIRE(ctx && params_flat && run_stats_flat && layers, "od_net_refresh: null argument");
  OD_REQUIRE(nlayers > 0 && nlayers <= 65535, "od_net_refresh: nlayers outside 1..65535");
  // 288 workgroups per entry, od_pack_weights_multi's grid: the largest layers (4.7 M weights = 2304 trips of 256 chunks)
  // need the parallelism; the workgroups of small layers leave after one test
  hipLaunchKernelGGL(od_net_refresh_k, dim3(288, nlayers), dim3(256), 0, (hipStream_t)stream, params_flat, run_stats_flat,
                     layers, eps);
  OD_CHECK_LAUNCH();
  return OD_OK;
}
