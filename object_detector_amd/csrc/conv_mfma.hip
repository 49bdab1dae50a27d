// K1/K2: im2col-free implicit-GEMM convolution (3x3 / 1x1, stride 1 / 2, NHWC f16, f32 accumulate) on CDNA4 MFMA.
//
//   C[n, m] = sum_k W[n, k] * X[m, k]      m = (b, ho, wo) output pixel, n = output channel,
//                                          k = (dy*KS + dx)*Cin + cin  (never materialised)
//
// One workgroup (4 or 8 waves) owns a BM x BN output tile.  Per BK-deep K step it gathers the BM x BK activation
// slice and the BN x BK weight slice straight into LDS with global_load_lds_dwordx4 (LDS-DMA, 16 B per lane, per-lane
// SOURCE address = the shifted input pixel, or the context's zero page for padding / tails).  The LDS is a ring of
// STAGES buffers; loads run STAGES-1 steps ahead of the MFMAs and are retired with a COUNTED s_waitcnt vmcnt(N) + one
// raw s_barrier per step (never vmcnt(0) in the steady state), so the HBM/L2 latency of the gather is covered by
// STAGES-2 whole K steps of matrix work.  LDS images are bank-conflict free for ds_read_b128 fragment reads:
//   BK = 64: 128-B rows, 16-B chunk c of row r at chunk c ^ (r & 7)      (swizzle applied on the DMA source side)
//   BK = 32: per 16-row piece, chunk-major [chunk][row]                  (the DMA lane picks (row, chunk) to match)
// v_mfma_f32_16x16x32_f16 runs with the WEIGHTS as the A operand so that each lane ends up with 4 consecutive output
// channels of one pixel; the epilogue applies scale/bias/activation in f32, stages the tile through LDS and writes full
// NHWC lines (16 B per lane) with the residual added in f32 and ONE rounding to f16.
//
// Replaces the Conv2D + BatchNormalization + LeakyReLU/ELU (+ Add) layers executed inside
// `ObjectDetector.predict` (reference voc_validate.py:27; docs/MODEL.md:5-21).
#include <stdlib.h>
#include <string.h>

#include "conv_common.h"

namespace {

template <int BM, int BN, int BK, int STAGES, int WM, int WN, int SPEC = 0>
struct ConvCfg {
  static constexpr int NT = WM * WN * 64;            // threads of one role (consumers; = loaders when SPEC)
  static constexpr int NTHREADS = NT * (SPEC ? 2 : 1);
  static constexpr int CPR = BK / 8;    // 16-B chunks per row
  static constexpr int RPR = NT / CPR;  // rows covered by one DMA round of the whole workgroup
  static constexpr int AR = BM / RPR, BR = BN / RPR;
  static constexpr int ROWB = BK * 2;
  static constexpr int A_BYTES = BM * ROWB, B_BYTES = BN * ROWB, STAGE_BYTES = A_BYTES + B_BYTES;
  static constexpr int WTM = BM / WM, WTN = BN / WN;
  static constexpr int MT = WTM / 16, NTL = WTN / 16;
  static constexpr int SLD = BN + 4;  // epilogue staging row stride (floats)
  static constexpr int PIPE_BYTES = STAGES * STAGE_BYTES;
  static constexpr int EPI_BYTES = WTM * SLD * 4;
  static constexpr int LDS_BYTES = PIPE_BYTES > EPI_BYTES ? PIPE_BYTES : EPI_BYTES;
  static constexpr int LOADS = AR + BR;  // LDS-DMA instructions per wave per K step
  static_assert(BM % RPR == 0 && BN % RPR == 0, "tile must be a whole number of DMA rounds");
  static_assert(BK == 32 || BK == 64, "BK");
  static_assert(LOADS * (STAGES - 2 > 0 ? STAGES - 2 : 0) <= 63, "vmcnt field");
};

// UNI: every BK-deep K step lies inside ONE filter tap (Cin % BK == 0; always true for KS == 1 with Cin % BK == 0):
// the tap walk is then wave-uniform scalar state advanced incrementally, and per-row padding validity is a 9-bit mask
// computed once.  UNI = false keeps a per-lane k -> (tap, cin) decomposition for odd channel counts.
// SPEC: wave specialisation.  The workgroup has 2 x WM*WN waves: the first half only runs MFMAs (consumers), the second
// half only issues the LDS-DMA (loaders) -- an LDS-DMA instruction costs its issuing wave ~70 cycles, which otherwise
// comes straight out of the MFMA stream.  Both halves meet at the same per-step barrier.
// EPI: the epilogue policy (conv_common.h), the last template argument.
template <int BM, int BN, int BK, int STAGES, int WM, int WN, int KS, int MINW, bool UNI, int SPEC, bool STATS = false,
          int EPI = OD_EPI_RT>
__global__ __launch_bounds__(WM* WN * 64 * (SPEC ? 2 : 1), MINW) void od_conv_igemm(ConvKP p) {
  using Cf = ConvCfg<BM, BN, BK, STAGES, WM, WN, SPEC>;
  constexpr int NT = Cf::NT, AR = Cf::AR, BR = Cf::BR, RPR = Cf::RPR, ROWB = Cf::ROWB;
  constexpr int WTM = Cf::WTM, WTN = Cf::WTN, MT = Cf::MT, NTL = Cf::NTL;

  extern __shared__ __attribute__((aligned(16))) char smem[];

  const int tid_all = threadIdx.x;
  const int lane = tid_all & 63;
  const int wave_all = __builtin_amdgcn_readfirstlane(tid_all >> 6);
  const bool is_loader = SPEC ? (wave_all >= WM * WN) : true;
  const bool is_consumer = SPEC ? (wave_all < WM * WN) : true;
  const int tid = SPEC ? (tid_all & (NT - 1)) : tid_all;   // index inside the role
  const int wave = SPEC ? (wave_all >= WM * WN ? wave_all - WM * WN : wave_all) : wave_all;
  const int l15 = lane & 15, lq = lane >> 4;

  // XCD-aware tile order: blocks b and b+8 share an XCD (and its L2); give each XCD a contiguous run of logical tiles,
  // n fastest, so the tiles that re-read the same activation rows / halos hit the same L2.
  int logical;
  {
    const int nt = p.mtiles * p.ntiles;
    const int pid = p.splitk > 1 ? (int)blockIdx.x / p.splitk : (int)blockIdx.x;
    const int q = nt >> 3, r = nt & 7, xcd = pid & 7, loc = pid >> 3;
    logical = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + loc;
  }
  const int tm = logical / p.ntiles, tn = logical - tm * p.ntiles;
  const int m0 = tm * BM, n0 = tn * BN;
  // split-K: this workgroup's K-step range
  const int nk_all = (p.Ktot + BK - 1) / BK;
  const int ks0 = p.splitk > 1 ? ((int)blockIdx.x % p.splitk) * p.steps_per_split : 0;
  int nk = p.splitk > 1 ? min(p.steps_per_split, nk_all - ks0) : nk_all;
  if (nk <= 0) return;  // uniform for the whole workgroup

  // ---- per-lane gather state --------------------------------------------------------------------------------
  int rr, lc, piece_off;  // row inside a DMA round, logical 16-B chunk fetched, LDS byte offset of this wave's piece
  if (BK == 64) {
    rr = tid >> 3;
    lc = (tid & 7) ^ (rr & 7);
    piece_off = wave * 8 * ROWB;
  } else {
    rr = wave * 16 + (lane & 15);
    lc = lane >> 4;
    piece_off = wave * 16 * ROWB;
  }
  int a_base[AR], a_hi0[AR], a_wi0[AR], a_b[AR];
  unsigned a_vmask[AR];  // UNI: bit t = tap t reads inside the image for this row
#pragma unroll
  for (int rd = 0; rd < AR; ++rd) {
    int m = m0 + rd * RPR + rr;
    a_vmask[rd] = 0u;
    if (p.tconv && m < p.M) m = od_tconv_pixel(p, (unsigned)m, BM);  // rows are grouped by output parity class (see below)
    if (m >= 0 && m < p.M) {
      const unsigned b = (unsigned)m / (unsigned)p.HoWo;
      const unsigned pix = (unsigned)m - b * (unsigned)p.HoWo;
      const unsigned ho = pix / (unsigned)p.Wo;
      const unsigned wo = pix - ho * (unsigned)p.Wo;
      a_hi0[rd] = (int)ho * p.stride - p.pad;
      a_wi0[rd] = (int)wo * p.stride - p.pad;
      a_base[rd] = (((int)b * p.H + a_hi0[rd]) * p.W + a_wi0[rd]) * p.Cin + lc * 8;
      a_b[rd] = (int)b;
#pragma unroll
      for (int t = 0; t < KS * KS; ++t) {
        const int hi = a_hi0[rd] + t / KS, wi = a_wi0[rd] + t % KS;
        bool ok = (unsigned)hi < (unsigned)p.H && (unsigned)wi < (unsigned)p.W;
        if (p.tconv) ok = ok && !((hi | wi) & 1);  // only the even positions of the zero-upsampled view carry data
        if (ok) a_vmask[rd] |= 1u << t;
      }
    } else {
      a_hi0[rd] = -(1 << 24);
      a_wi0[rd] = 0;
      a_base[rd] = 0;
      a_b[rd] = 0;
    }
  }
  const f16* wrow = p.w + (long long)(n0 + rr) * p.Kstride + lc * 8;

  // Transposed mode (backward-data of a stride-2 conv): an output pixel only receives the taps whose source position in
  // the zero-upsampled view is even -- 1, 2, 2 or 4 of the 9, by the parity of (y, x).  The rows of the GEMM are ordered
  // tile by tile in parity classes (od_tconv_pixel), so a tile's rows share their class and the taps that
  // are zero for EVERY row of the tile are skipped as whole K steps: 2.25 instead of 9 taps on average.  Skipped steps
  // only add exact zeros, so the result is bit-identical to the un-skipped walk.
  unsigned tmask = 0x1FFu;
  if (UNI && KS == 3 && p.tconv && p.splitk <= 1) {
    unsigned um = 0u;
#pragma unroll
    for (int rd = 0; rd < AR; ++rd) um |= a_vmask[rd];
    for (int off = 32; off; off >>= 1) um |= (unsigned)__shfl_xor((int)um, off, 64);
    unsigned* sh = (unsigned*)smem;
    if (tid_all == 0) *sh = 0u;
    __syncthreads();
    if (lane == 0) atomicOr(sh, um);
    __syncthreads();
    tmask = (unsigned)__builtin_amdgcn_readfirstlane((int)*sh);
    __syncthreads();  // smem[0] is part of the ring from here on
    nk = __builtin_popcount(tmask) * (p.Cin / BK);
  }

  // loader state: the NEXT step to stage (steps are staged strictly in order) -- all wave-uniform scalars
  int ld_k0 = ks0 * BK, ld_c0 = ld_k0, ld_tap = 0, ld_tapoff = 0, ld_dx = 0, ld_dy = 0;
  if (UNI && KS == 3) {
    ld_tap = ld_k0 / p.Cin;
    ld_c0 = ld_k0 - ld_tap * p.Cin;
    if (tmask != 0x1FFu && tmask != 0u) {
      ld_tap = __builtin_ctz(tmask);
      ld_c0 = 0;
      ld_k0 = ld_tap * p.Cin;
    }
    ld_dy = ld_tap / 3;
    ld_dx = ld_tap - ld_dy * 3;
    ld_tapoff = (ld_dy * p.W + ld_dx) * p.Cin;
  }

  // SPEC == 2: the loader waves stage through REGISTERS (global_load_dwordx4 -> ds_write_b128) instead of LDS-DMA: the
  // L2 -> LDS-DMA path tops out near 30 B/clk/CU, plain vector loads from L2 reach about twice that
  constexpr int NX = AR + BR;
  f16x8 rtmp[SPEC == 2 ? NX : 1];
  char* rdst[SPEC == 2 ? NX : 1];
  int rn = 0;
  auto xfer = [&](const f16* src, char* lds_piece) {
    if (SPEC == 2) {
      rtmp[rn] = *(const f16x8*)src;
      rdst[rn] = lds_piece + lane * 16;
      ++rn;
    } else {
      glds16(src, lds_piece);
    }
  };
  auto stage = [&](int buf) {
    rn = 0;
    char* abuf = smem + buf * Cf::STAGE_BYTES + piece_off;
    char* bbuf = abuf + Cf::A_BYTES;
    if (UNI) {
      const bool cvalid = (KS == 3) || (ld_c0 + lc * 8 < p.Cin);
      const int koff = ld_tapoff + ld_c0;  // scalar: (dy*W + dx)*Cin + c0
#pragma unroll
      for (int rd = 0; rd < AR; ++rd) {
        const bool ok = cvalid && ((a_vmask[rd] >> ld_tap) & 1u);
        const f16* src;
        if (KS == 3 && p.tconv) {
          const int u = (a_hi0[rd] + ld_dy) >> 1, v = (a_wi0[rd] + ld_dx) >> 1;
          src = ok ? p.x + (((a_b[rd] * p.Hs + u) * p.Ws + v) * p.Cin + lc * 8 + ld_c0) : p.zero;
        } else {
          src = ok ? p.x + (a_base[rd] + koff) : p.zero;
        }
        xfer(src, abuf + rd * RPR * ROWB);
      }
    } else {
      const int k = ld_k0 + lc * 8;
      const int tap = k / p.Cin;
      const int dy = tap / 3, dx = tap - dy * 3;
      const int cin = k - tap * p.Cin;
      const bool kvalid = k < p.Ktot;
      const int koff = (dy * p.W + dx) * p.Cin + cin - lc * 8;
#pragma unroll
      for (int rd = 0; rd < AR; ++rd) {
        const int hi = a_hi0[rd] + dy, wi = a_wi0[rd] + dx;
        const bool ok = kvalid && (unsigned)hi < (unsigned)p.H && (unsigned)wi < (unsigned)p.W;
        const f16* src = ok ? p.x + (a_base[rd] + koff) : p.zero;
        xfer(src, abuf + rd * RPR * ROWB);
      }
    }
#pragma unroll
    for (int rd = 0; rd < BR; ++rd) xfer(wrow + (long long)rd * RPR * p.Kstride + ld_k0, bbuf + rd * RPR * ROWB);
    if (SPEC == 2) {
#pragma unroll
      for (int i = 0; i < NX; ++i) *(f16x8*)rdst[i] = rtmp[i];
    }
    // advance to the next step
    ld_k0 += BK;
    if (UNI) {
      ld_c0 += BK;
      if (KS == 3 && ld_c0 >= p.Cin) {
        ld_c0 = 0;
        ++ld_tap;
        if (++ld_dx == 3) {
          ld_dx = 0;
          ++ld_dy;
          ld_tapoff += (p.W - 2) * p.Cin;
        } else {
          ld_tapoff += p.Cin;
        }
        while (ld_tap < 9 && !((tmask >> ld_tap) & 1u)) {  // taps that are zero for the whole tile (transposed mode)
          ++ld_tap;
          ld_k0 += p.Cin;
          if (++ld_dx == 3) {
            ld_dx = 0;
            ++ld_dy;
          }
        }
      }
    }
  };

  // ---- main loop: STAGES-deep LDS ring, counted vmcnt, one raw barrier per K step ------------------------------
  const int wm = wave / WN, wn = wave - wm * WN;
  f32x4 acc[MT][NTL];
#pragma unroll
  for (int i = 0; i < MT; ++i)
#pragma unroll
    for (int j = 0; j < NTL; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  if (is_loader) {
#pragma unroll
    for (int s = 0; s < STAGES - 1; ++s)
      if (s < nk) stage(s);
  }

  const int swz = l15 & 7;
  int buf = 0;
  for (int ks = 0; ks < nk; ++ks) {
    // retire this step's DMA (issued STAGES-1 steps ago); later steps stay in flight.  Consumers have no DMA of their own.
    if (is_loader) {
      if (STAGES > 2 && ks + (STAGES - 2) < nk)
        wait_vmcnt<Cf::LOADS*(STAGES > 2 ? STAGES - 2 : 0)>();
      else
        wait_vmcnt<0>();
    }
    if (SPEC == 2) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();  // every wave's piece of step ks landed; everyone finished reading step ks-1
    {
      const int nxt = ks + STAGES - 1;
      int nb = buf + STAGES - 1;
      if (nb >= STAGES) nb -= STAGES;
      if (is_loader && nxt < nk) stage(nb);  // overwrites the buffer read at step ks-1
    }
    const char* abuf = smem + buf * Cf::STAGE_BYTES;
    const char* bbuf = abuf + Cf::A_BYTES;
    __builtin_amdgcn_s_setprio(1);
    if (is_consumer)
#pragma unroll
    for (int kh = 0; kh < BK / 32; ++kh) {
      f16x8 xa[MT], wb[NTL];
      if (BK == 64) {
        const int coff = ((kh * 4 + lq) ^ swz) * 16;
#pragma unroll
        for (int i = 0; i < MT; ++i) xa[i] = *(const f16x8*)(abuf + (wm * WTM + i * 16 + l15) * ROWB + coff);
#pragma unroll
        for (int j = 0; j < NTL; ++j) wb[j] = *(const f16x8*)(bbuf + (wn * WTN + j * 16 + l15) * ROWB + coff);
      } else {
        const int coff = lq * 256 + l15 * 16;
#pragma unroll
        for (int i = 0; i < MT; ++i) xa[i] = *(const f16x8*)(abuf + (wm * WTM + i * 16) * ROWB + coff);
#pragma unroll
        for (int j = 0; j < NTL; ++j) wb[j] = *(const f16x8*)(bbuf + (wn * WTN + j * 16) * ROWB + coff);
      }
#pragma unroll
      for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < NTL; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wb[j], xa[i], acc[i][j], 0, 0, 0);
    }
    __builtin_amdgcn_s_setprio(0);
    if (++buf == STAGES) buf = 0;
  }
  __syncthreads();  // all fragment reads done before the ring is reused as epilogue staging

  conv_epilogue<BN, WM, WN, MT, NTL, Cf::NTHREADS, STATS, EPI>(p, smem, acc, m0, n0, tid_all, is_consumer ? wm : -1, wn, l15, lq);
}

// split-K finish: out = act(scale * sum_s slab[s] + bias) (+ residual); slabs summed in ascending s (deterministic)
__global__ __launch_bounds__(256) void od_conv_finish(ConvKP p) {
  const long long nvec = (long long)p.M * (p.Cout >> 3);
  const int C8 = p.Cout >> 3;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < nvec; i += (long long)gridDim.x * 256) {
    const int m = (int)(i / C8), n = (int)(i - (long long)m * C8) * 8;
    const float* wsp = p.ws + (long long)m * p.Cout + n;
    const long long slab = (long long)p.M * p.Cout;
    float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int sidx = 0; sidx < p.splitk; ++sidx) {
      const f32x4 a0 = *(const f32x4*)(wsp + sidx * slab), a1 = *(const f32x4*)(wsp + sidx * slab + 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        v[e] += a0[e];
        v[4 + e] += a1[e];
      }
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      v[e] = v[e] * p.scale[n + e] + p.bias[n + e];
      if (p.act == OD_ACT_LEAKY) v[e] = od_leaky(v[e], p.alpha);
      else if (p.act == OD_ACT_ELU) v[e] = v[e] > 0.f ? v[e] : p.alpha * od_expm1_fast(v[e]);
    }
    const unsigned b = (unsigned)m / (unsigned)p.HoWo;
    const unsigned pix = (unsigned)m - b * (unsigned)p.HoWo;
    if (p.res_mode != OD_RES_NONE) {
      long long roff;
      if (p.res_mode == OD_RES_SAME) {
        roff = (long long)m * p.Cout + n;
      } else {
        const unsigned ho = pix / (unsigned)p.Wo, wo = pix - ho * (unsigned)p.Wo;
        roff = ((long long)(b * (unsigned)(p.Ho >> 1) + (ho >> 1)) * (p.Wo >> 1) + (wo >> 1)) * p.Cout + n;
      }
      const f16x8 r = *(const f16x8*)(p.res + roff);
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] += (float)r[e];
    }
    const long long ooff = (long long)b * p.obs + (long long)pix * p.ops + n;
    if (p.out_f32) {
      float* o = (float*)p.out + ooff;
      *(f32x4*)o = f32x4{v[0], v[1], v[2], v[3]};
      *(f32x4*)(o + 4) = f32x4{v[4], v[5], v[6], v[7]};
    } else {
      f16x8 h;
#pragma unroll
      for (int e = 0; e < 8; ++e) h[e] = (f16)v[e];
      *(f16x8*)((f16*)p.out + ooff) = h;
    }
  }
}

// One row per table config: the tile and, per kernel variant, the plain kernel and the STATS one (od_conv_desc.bn_partials:
// BatchNorm partial sums written by the epilogue).  Private to this file: the dispatcher asks od_conv_igemm_select.
struct TileCfg {
  int BM, BN, BK, threads;
  size_t lds;
  // k[variant][STATS]; variant 0: KS == 1 (channel tail masked per lane: any Cin % 8 == 0), 1: KS == 3 with Cin % BK == 0,
  // 2: KS == 3 with any Cin % 8 == 0 (per-lane tap decomposition; fn is null where the config does not have it)
  struct { const void* fn; const char* name; } k[3][2];
  // fx[variant 0 / 1][i]: the plain kernel compiled for epilogue policy kFxEpi[i]
  struct { const void* fn; const char* name; } fx[2][4];
};
// the policies of the f16 plans' table-kernel launches: backbone 1x1 / 3x3 (+ residual), neck and prediction module.
// Deliberately f16 only: every policy costs 16 more instantiations (8 configs x 1x1 / 3x3) in this translation unit, and the
// f32-output launches of the mixed plan on the table configs (laterals, stage-5 residual stream) are not on the
// benchmarked plan -- they run the run-time instantiation (tests/test_gpu_conv_epilogue_variants.py pins that).
constexpr int kFxEpi[4] = {OD_EPI_LEAKY_NONE_F16, OD_EPI_LEAKY_SAME_F16, OD_EPI_ELU_NONE_F16, OD_EPI_ELU_UP2_F16};

// an od_conv_igemm instantiation and its name; OD_K: the pair plain / STATS of one variant, OD_NOK: a variant left out
#define OD_K1(BM, BN, BK, ST, WM, WN, KS, MINW, UNI, SPEC, STATS)                                                       \
  {(const void*)&od_conv_igemm<BM, BN, BK, ST, WM, WN, KS, MINW, UNI, SPEC, STATS>,                                     \
   "od_conv_igemm<" #BM ", " #BN ", " #BK ", " #ST ", " #WM ", " #WN ", " #KS ", " #MINW ", " #UNI ", " #SPEC ", " #STATS ", -1>"}
#define OD_KX1(BM, BN, BK, ST, WM, WN, KS, MINW, UNI, SPEC, EPI)                                                         \
  {(const void*)&od_conv_igemm<BM, BN, BK, ST, WM, WN, KS, MINW, UNI, SPEC, false, EPI>,                                \
   "od_conv_igemm<" #BM ", " #BN ", " #BK ", " #ST ", " #WM ", " #WN ", " #KS ", " #MINW ", " #UNI ", " #SPEC ", false, " OD_STR(EPI) ">"}
#define OD_KX(BM, BN, BK, ST, WM, WN, KS, MINW, UNI, SPEC)                                                             \
  {OD_KX1(BM, BN, BK, ST, WM, WN, KS, MINW, UNI, SPEC, OD_EPI_LEAKY_NONE_F16),                                          \
   OD_KX1(BM, BN, BK, ST, WM, WN, KS, MINW, UNI, SPEC, OD_EPI_LEAKY_SAME_F16),                                          \
   OD_KX1(BM, BN, BK, ST, WM, WN, KS, MINW, UNI, SPEC, OD_EPI_ELU_NONE_F16),                                            \
   OD_KX1(BM, BN, BK, ST, WM, WN, KS, MINW, UNI, SPEC, OD_EPI_ELU_UP2_F16)}
#define OD_K(BM, BN, BK, ST, WM, WN, KS, MINW, UNI, SPEC)                                                              \
  {OD_K1(BM, BN, BK, ST, WM, WN, KS, MINW, UNI, SPEC, false), OD_K1(BM, BN, BK, ST, WM, WN, KS, MINW, UNI, SPEC, true)}
#define OD_NOK(BM, BN, BK, ST, WM, WN, KS, MINW, UNI, SPEC) {}
// SPEC = 1: wave-specialised, twice the threads; K3G = OD_K: the config has the generic 3x3 kernel
#define OD_CFG(BM, BN, BK, ST, WM, WN, MINW, SPEC, K3G)                                                                 \
  {BM, BN, BK, WM * WN * 64 * (SPEC + 1), (size_t)ConvCfg<BM, BN, BK, ST, WM, WN, SPEC>::LDS_BYTES,                     \
   {OD_K(BM, BN, BK, ST, WM, WN, 1, MINW, true, SPEC), OD_K(BM, BN, BK, ST, WM, WN, 3, MINW, true, SPEC),               \
    K3G(BM, BN, BK, ST, WM, WN, 3, MINW, false, SPEC)},                                                                 \
   {OD_KX(BM, BN, BK, ST, WM, WN, 1, MINW, true, SPEC), OD_KX(BM, BN, BK, ST, WM, WN, 3, MINW, true, SPEC)}}

//         BM   BN  BK ST WM WN minwaves/SIMD, SPEC
// Only what pick_cfg can select (round 3: the 22 table configs, the LDS-window kernels and the persistent window kernel
// that never won a layer are gone -- profiles/r01/conv_cfg_sweep.txt, profiles/r02/spec64_sweep.txt record what they
// measured).
const TileCfg g_cfgs[] = {
    OD_CFG(128, 128, 64, 2, 2, 2, 2, 0, OD_K),    // 0: generic geometry (any Cin % 8 == 0; 64 KiB, 2 WG/CU)
    OD_CFG(128, 64, 64, 2, 2, 2, 2, 0, OD_K),     // 1
    OD_CFG(64, 128, 64, 2, 2, 2, 2, 0, OD_K),     // 2
    OD_CFG(64, 64, 64, 2, 2, 2, 2, 0, OD_K),      // 3
    OD_CFG(128, 128, 64, 2, 2, 2, 4, 1, OD_NOK),  // 4: 4 MFMA waves + 4 DMA waves, 64 KiB, 2 WG/CU
    OD_CFG(128, 128, 64, 3, 2, 2, 2, 1, OD_NOK),  // 5: same, 3-deep ring (96 KiB, 1 WG/CU): few tiles, long K
    OD_CFG(64, 64, 64, 4, 2, 2, 2, 0, OD_NOK),    // 6: deep ring for the short-K 1x1 layers (cold L2: latency, not bandwidth)
    OD_CFG(64, 128, 64, 3, 2, 2, 4, 1, OD_NOK),   // 7: specialised 64 x 128, 72 KiB: small-M layers
};
constexpr int kNumCfgs = sizeof(g_cfgs) / sizeof(g_cfgs[0]);

}  // namespace

int od_conv_igemm_num_cfgs() { return kNumCfgs; }

bool od_conv_igemm_select(int cfg, int ksize, int Cin, bool want_stats, int epi, ConvKernelInfo* info) {
  if (cfg < 0 || cfg >= kNumCfgs) return false;
  const TileCfg& tc = g_cfgs[cfg];
  // kernel variant: 1x1 / 3x3-uniform-tap / 3x3-generic
  const int var = ksize == 1 ? 0 : ((Cin % tc.BK) == 0 ? 1 : 2);
  const auto& k = tc.k[var][want_stats];
  *info = {k.fn, k.name, tc.BM, tc.BN, tc.BK, tc.threads, tc.lds};
  for (int i = 0; i < 4 && var < 2 && !want_stats; ++i)
    if (kFxEpi[i] == epi) {  // the same tile with the epilogue compiled for this launch's policy
      info->fn = tc.fx[var][i].fn;
      info->name = tc.fx[var][i].name;
    }
  return info->fn != nullptr;
}

int od_conv_finish_prepare(const ConvKP& p, od_launches* L) {
  const long long nvec = (long long)p.M * (p.Cout / 8);
  long long fb = (nvec + 255) / 256;
  if (fb > 2048) fb = 2048;
  return od_add_launch(L, {"od_conv_finish", od_issue_kp, (const void*)&od_conv_finish, dim3((unsigned)fb), dim3(256), 0}, p);
}
