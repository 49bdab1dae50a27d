// Shared by the DIRECT convolution kernels (conv_stem, conv_bneck, conv_rdirect, conv_stream3, conv_tconv): the HBM-bound
// ends of the network, each a persistent or weights-resident kernel that computes 16-pixel MFMA fragments and stores
// straight from the accumulators.  One copy of every device idiom those files share, its invariant stated on it.
// No fp-contract pragma here: conv_bneck / conv_stem are built with contraction on (v * s + b is one v_fma), the other
// three with contraction off (v_mul + v_add), and every helper compiles to whatever its translation unit asks for.
#pragma once
#include "conv_common.h"

// ---- activation ---------------------------------------------------------------------------------------------------------
// Compile-time form (conv_stem, conv_bneck).  As a run-time enum tested per element the compiler kept the dispatch as
// control flow inside the unrolled epilogues: 328 branches and 40 v_exp_f32 in od_bneck<64>, 405 / 48 in od_stem_k, the
// ELU path with its divergent v > 0 test laid out for every element even when the network only asks for LeakyReLU.
template <int ACT>
static __device__ __forceinline__ float od_act(float v, float alpha) {
  if (ACT == OD_ACT_LEAKY) return od_leaky(v, alpha);
  if (ACT == OD_ACT_ELU) return v > 0.f ? v : alpha * od_expm1_fast(v);
  return v;
}
// Run-time form (conv_rdirect, conv_stream3): ONE test per row of 8, not per element.
static __device__ __forceinline__ void od_act_rt(float (&o)[8], int act, float alpha) {
  if (act == OD_ACT_LEAKY) {
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = od_leaky(o[e], alpha);
  } else if (act == OD_ACT_ELU) {
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = o[e] > 0.f ? o[e] : alpha * od_expm1_fast(o[e]);
  }
}

// ---- buffer-addressed LDS-DMA (resource in SGPRs, per-lane byte offset, scalar byte offset; out-of-range lanes, e.g.
//      voff = 0x80000000, load nothing).  These stay plain __device__ functions: the host pass of hipcc (ROCm 7.2)
//      silently drops a kernel TEMPLATE whose body names the buffer builtins.
static __device__ __forceinline__ __amdgpu_buffer_rsrc_t od_buffer_rsrc(const void* base, unsigned bytes) {
  return __builtin_amdgcn_make_buffer_rsrc((void*)base, 0, (int)bytes, 0x00020000);
}
static __device__ __forceinline__ void od_buffer_dma16(__amdgpu_buffer_rsrc_t rs, int voff, int soff, char* lds) {
  __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (__attribute__((address_space(3))) void*)lds, 16, voff, soff, 0, 0);
}

// ---- accumulators -> one row of 8 channels ------------------------------------------------------------------------------
// After od_pair_row8 on the 16-channel fragments frag0 (even) and frag0 + 1, lane (l15, lq) holds the 8 consecutive
// channels OD_LANE_CH8_AT(lq, frag0) .. +7 of pixel l15 (OD_LANE_CH8(lq): frag0 = 0): one 16-byte store per lane, four
// lanes cover a 64-byte line.  Macros, not functions: behind a function, however it is declared, hipcc allocates
// od_tconv_64_32 one VGPR more and orders od_conv_stream3's prologue differently.
#define OD_LANE_CH8(lq) (((lq) & 1) * 16 + ((lq) >> 1) * 8)
#define OD_LANE_CH8_AT(lq, frag0) (((frag0) + ((lq) & 1)) * 16 + ((lq) >> 1) * 8)
// Precondition: od_mfma_results_ready() has run since the last MFMA that wrote `even` / `odd` (od_permlane16_swap).
static __device__ __forceinline__ void od_pair_row8(const f32x4& even, const f32x4& odd, float (&o)[8]) {
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    float a = even[e], b = odd[e];
    od_permlane16_swap(a, b);
    o[e] = a;
    o[4 + e] = b;
  }
}
// The epilogue of every direct kernel is the same steps in the same order, on the 8 values of od_pair_row8:
//   o * scale + bias (od_scale_bias8 where scale / bias sit in memory) -> od_act<ACT> / od_act_rt -> + residual (an f16x8
//   the kernel fetched: registers, the x window in LDS, or global memory) -> ONE rounding to f16 -> ONE 16-byte store.
// The steps are separate helpers and the residual / rounding / store stay spelled out in the kernels on purpose: folded
// into one function (or into any helper that holds both the run-time activation and the residual test) hipcc lays the
// epilogues of conv_rdirect out differently: other register counts, packed instead of scalar multiplies, spills in the
// 3x3 kernel at 248 VGPRs.
// scale / bias of the lane's 8 channels from memory (LDS or global, 16-byte aligned)
static __device__ __forceinline__ void od_scale_bias8(float (&o)[8], const float* sc, const float* bi) {
  const f32x4 s0 = *(const f32x4*)sc, s1 = *(const f32x4*)(sc + 4);
  const f32x4 b0 = *(const f32x4*)bi, b1 = *(const f32x4*)(bi + 4);
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    o[e] = o[e] * s0[e] + b0[e];
    o[4 + e] = o[4 + e] * s1[e] + b1[e];
  }
}

// ---- LDS chunk swizzle ----------------------------------------------------------------------------------------------------
// Every LDS row of these kernels (a pixel's channels, or one weight row of one tap) is a whole number of 16-byte chunks,
// and chunk c of row r is stored at chunk c ^ od_swz_key<K>(r).  The XOR is applied on the DMA SOURCE side (lane i of a
// 1-KiB piece fetches the chunk that belongs at its slot), so the LDS-DMA destination stays linear; every ds_read_b128 /
// ds_write applies the same key.  A key touches the low chunk bits only (3 for 128-B and longer rows, 2 for 64-B rows).
//
//   key            value               rows
//   OD_SWZ_ROW7X2  (r & 7) << 1        256-B rows of the block kernels
//   OD_SWZ_ROW7    r & 7               128-B rows everywhere; 256-B rows of the stream kernels
//   OD_SWZ_PAIR3   (r >> 1) & 3        64-B rows of the stream kernels
//   OD_SWZ_QUAD3   3 * ((r >> 2) & 1)  64-B rows of the block kernels
//
//   kernel                   LDS region          row    key      read as
//   od_bneck<128>            x window, w1        256 B  ROW7X2   16 consecutive rows (window pixels, any start; weight rows), 2 k chunks
//   od_bneck<128>            t window, w3 taps   128 B  ROW7     16 consecutive rows, any start (tap shift)
//   od_bneck<64>             x window, w1        128 B  ROW7     as above
//   od_bneck<64>             t window, w3 taps    64 B  QUAD3    16 consecutive rows, any start (tap shift)
//   od_stem_k                t window, w3 taps    64 B  QUAD3    16 consecutive rows of one de-interleaved column plane, any start
//   od_conv_stream3<64, *>   window, weights     128 B  ROW7     window: rows q0 + l15 * S; weights: 16 rows from a multiple of 16
//   od_conv_stream3<32, *>   window, weights      64 B  PAIR3    as above
//   od_tconv_64_32           dZ tile, weights    128 B  ROW7     tile: 16 consecutive rows, any start; weights from a multiple of 16
//   od_conv_rdirect<KC, *>   weights             2 KC B ROW7 (KC >= 64), PAIR3 (KC = 32): 16 rows from a multiple of 16
//   od_tconv_rdirect<128,64> weights             256 B  ROW7     16 rows from a multiple of 16
//
// Why two keys for 64-byte rows: two such rows share one 128-byte bank line.  PAIR3 gives the two rows of a line the same
// key and walks the four keys over 8 rows, so that the 16 consecutive rows of a fragment read cover all banks; it was
// chosen for the stream kernels' weight and window reads.  QUAD3 (like ROW7X2 for 256-byte rows) was found by brute force
// against the gfx950 lane-group bank model for the block kernels' window reads, whose 16 rows start at ANY row (the tap
// shift moves them one row at a time); a stride-2 walk over interleaved rows is 2-way conflicted under every XOR key of
// this family, which is why od_stem_k stores its window de-interleaved.  The two families were tuned independently:
// neither 64-byte key has been checked on the other family's access pattern, so they are kept apart, not merged.
enum od_swz { OD_SWZ_ROW7X2, OD_SWZ_ROW7, OD_SWZ_PAIR3, OD_SWZ_QUAD3 };
template <od_swz K>
static __device__ __forceinline__ int od_swz_key(int row) {
  return K == OD_SWZ_ROW7X2 ? ((row & 7) << 1) : K == OD_SWZ_ROW7 ? (row & 7) : K == OD_SWZ_PAIR3 ? ((row >> 1) & 3) : 3 * ((row >> 2) & 1);
}
// chunk -> stored chunk (the ROW7 form spells out that only the low three chunk bits move, whatever the row length)
template <od_swz K>
static __device__ __forceinline__ int od_swz_chunk(int chunk, int row) {
  return K == OD_SWZ_ROW7 ? ((chunk & ~7) | ((chunk ^ row) & 7)) : (chunk ^ od_swz_key<K>(row));
}
// the key of a row of CH chunks: block kernels (od_bneck, od_stem_k) and stream kernels (rdirect, stream3, tconv)
constexpr od_swz od_swz_block(int ch) { return ch == 16 ? OD_SWZ_ROW7X2 : ch == 8 ? OD_SWZ_ROW7 : OD_SWZ_QUAD3; }
constexpr od_swz od_swz_stream(int ch) { return ch >= 8 ? OD_SWZ_ROW7 : OD_SWZ_PAIR3; }

// ---- weights -> LDS, all taps resident ------------------------------------------------------------------------------------
// The packed weights [n][tap * KC + c] (row stride Kstride halfs) land as ROWS = taps * NC rows of ROWB = 2 KC bytes, row
// = tap * NC + n, in 1-KiB LDS-DMA pieces of 1024 / ROWB rows; this is piece q, issued by one whole wave.  ROWS need not
// fill the last piece: its surplus lanes re-write the last row with itself.  Which wave issues which piece is the
// caller's loop; nothing may read the rows before that wave's vmcnt has drained and a barrier has passed.
// Row: the type the row index is computed in.  od_tconv_64_32 asks for unsigned (its r / NC is then a shift without the
// sign fix-up; the others would gain the same few instructions, which is a change of their code and not made here).
template <int ROWS, int ROWB, int NC, od_swz K, class Row = int>
static __device__ __forceinline__ void od_weight_piece_to_lds(const f16* w, int Kstride, char* wlds, int q, int lane) {
  constexpr int LPR = ROWB / 16, RPP = 64 / LPR, KC = ROWB / 2;  // lanes per row, rows per piece
  Row r = q * RPP + lane / LPR;
  if (ROWS % RPP != 0 && r >= ROWS) r = ROWS - 1;
  const int tap = r / NC, n = r - tap * NC;
  const int lc = (lane % LPR) ^ od_swz_key<K>(r);
  glds16(w + ((long long)n * Kstride + tap * KC + lc * 8), wlds + q * 1024);
}
template <int ROWS, int ROWB>
constexpr int od_weight_pieces() { return (ROWS + 1024 / ROWB - 1) / (1024 / ROWB); }

// ---- persistent tile walk -------------------------------------------------------------------------------------------------
// Workgroup `first` of `step` takes tiles first, first + step, ...; tiles are numbered image-major, then row-major.
struct od_tile_pos {
  int img, ty, tx;
};
static __device__ __forceinline__ od_tile_pos od_tile_decode(int tile, int tiles_per_img, int tiles_x) {
  const int img = tile / tiles_per_img, t2 = tile - img * tiles_per_img;
  const int ty = t2 / tiles_x;
  return {img, ty, t2 - ty * tiles_x};
}
static __device__ __forceinline__ int od_tiles_of(int first, int step, int ntiles) {
  return first < ntiles ? (ntiles - first + step - 1) / step : 0;
}

// ---- window ring (od_conv_stream3, od_tconv_64_32) --------------------------------------------------------------------------
// NBUF window buffers, AHEAD = NBUF - 1 tiles staged beyond the one being computed: the prologue stages tiles 0 ..
// AHEAD - 1, iteration `it` waits for window `it` (buffer it % NBUF), passes the barrier, stages tile it + AHEAD into the
// buffer tile it - 1 just left, computes, and issues its NS output stores.  Every wave issues exactly ND LDS-DMAs per
// staged tile and exactly NS stores per computed tile -- the counts below rest on that -- and vector memory retires in
// issue order.  Behind the DMAs of window `it` this wave has issued
//   stores(it - AHEAD) .. stores(it - 1)                     AHEAD * NS
//   the DMAs of windows it + 1 .. it + AHEAD - 1, if staged  ND each
// and exactly those may stay in flight.  The first AHEAD iterations drain everything (the weights came first).
template <int NBUF, int NS, int ND>
static __device__ __forceinline__ void od_ring_wait(int it, int nmine) {
  static_assert(NBUF == 2 || NBUF == 3, "one or two windows ahead");
  constexpr int AHEAD = NBUF - 1;
  if (it < AHEAD) {
    wait_vmcnt<0>();
  } else if (AHEAD == 1) {
    wait_vmcnt<NS>();
  } else if (it + 1 < nmine) {
    wait_vmcnt<2 * NS + ND>();
  } else {
    wait_vmcnt<2 * NS>();
  }
}

// ---- host side ------------------------------------------------------------------------------------------------------------
// a table entry of the layer-specialised kernels: the layer it serves and the launchable kernel
struct DirectKernel {
  int kc, nc, stride, ks;
  ConvKernelInfo k;  // (BM / BN / BK unused: these kernels have no GEMM tile)
};
template <int N>
static inline const DirectKernel* od_direct_find(const DirectKernel (&tab)[N], const od_conv_desc* d) {
  for (const DirectKernel& e : tab)
    if (e.kc == d->Cin && e.nc == d->Cout && e.stride == d->stride && e.ks == d->ksize) return &e;
  return nullptr;
}
// persistent grid: per_cu workgroups on every CU, never more workgroups than units of work
static inline int od_persistent_grid(int per_cu, int num_cu, int work) { return per_cu * num_cu < work ? per_cu * num_cu : work; }
// raise the kernel's LDS limit and record its launch: kernel(p), or kernel(p, n) for the tile-walking block kernels
template <class KP>
static inline int od_direct_launch(od_ctx* ctx, od_launches* L, const ConvKernelInfo& k, int grid, const KP& p) {
  if (int rc = od_ensure_lds(ctx, k.fn, k.lds)) return rc;
  return od_add_launch(L, {k.name, od_issue_kp, k.fn, dim3((unsigned)grid), dim3((unsigned)k.threads), k.lds}, p);
}
template <class KP>
static inline int od_direct_launch(od_ctx* ctx, od_launches* L, const ConvKernelInfo& k, int grid, const KP& p, int n) {
  if (int rc = od_ensure_lds(ctx, k.fn, k.lds)) return rc;
  return od_add_launch(L, {k.name, od_issue_kp_int<KP>, k.fn, dim3((unsigned)grid), dim3((unsigned)k.threads), k.lds},
                       od_kp_int<KP>{p, n});
}
