// The one copy of what the exact top-K selection, the sort / gather in front of the NMS and the IoU predicate are made of
// (included from post_common.h).  The three-call path (topk.hip -> nms.hip), od_detect (detect.hip), its streamed form
// (detect_wide.hip) and the TTA merge (tta.hip) promise the same keys, counts and kept indices bit for bit: they get them
// by calling the same code, not copies of it.  A change to the key format, the digit widths or the tie rule is made here.
#pragma once

typedef unsigned long long u64;

// ---- the key: total order (conf desc, flat index asc) = descending u64 -------------------------------------------------
__device__ __forceinline__ u64 od_make_key(unsigned score_bits, unsigned flat) {
  return ((u64)score_bits << 32) | (u64)(0xFFFFFFFFu - flat);
}
__device__ __forceinline__ unsigned od_key_flat(u64 key) { return 0xFFFFFFFFu - (unsigned)key; }
__device__ __forceinline__ unsigned od_key_score_bits(u64 key) { return (unsigned)(key >> 32); }

// What is left of a key below its first radix digit od_digit0(sb, dbase, dshift): the low dshift bits of (sb - dbase), then
// ~flat (<= 51 bits; low_mask = (1 << dshift) - 1).  The three-call path's first digit is score bits [30:19] = dbase 0,
// dshift 19: for positive floats od_digit0(sb, 0, 19) is (sb >> 19) & 4095 and the sub-key's score part is sb & 0x7FFFF.
__device__ __forceinline__ u64 od_refine_subkey(u64 key, unsigned dbase, unsigned low_mask) {
  return ((u64)((od_key_score_bits(key) - dbase) & low_mask) << 32) | (key & 0xFFFFFFFFull);
}

// ---- refine inside the d0 bin ------------------------------------------------------------------------------------------
// One workgroup of 1024 threads radix-selects the krem best of the nc keys whose first digit is d0, on the sub-key's digits
// of 11, 8, 11, 11, 10 bits from the top, and stops as soon as a bin is taken whole.  key_at(i), i < n, is candidate i's key,
// or 0 for "not in the d0 bin"; emit(key) is called once for every winner (any order, any thread).  All threads call it.
template <class KeyAt, class Emit>
__device__ __forceinline__ void od_radix_refine(int n, int nc, int krem, unsigned dbase, int dshift, KeyAt key_at, Emit emit) {
  __shared__ int lh[OD_TOPK_NB];
  __shared__ int sh_digit, sh_above, sh_inbin;
  const int tid = threadIdx.x;
  const unsigned low_mask = (1u << dshift) - 1u;
  u64 prefix = 0, pmask = 0;  // the digits fixed so far, and the sub-key bits they cover
  const int shifts[5] = {40, 32, 21, 10, 0};
  const int widths[5] = {11, 8, 11, 11, 10};
  bool whole = (nc == krem);  // take the whole bin
  for (int ps = 0; ps < 5 && !whole; ++ps) {
    const int sh = shifts[ps], nbins = 1 << widths[ps];
    for (int i = tid; i < OD_TOPK_NB; i += 1024) lh[i] = 0;
    __syncthreads();
    for (int i = tid; i < n; i += 1024) {
      const u64 key = key_at(i);
      if (!key) continue;
      const u64 sub = od_refine_subkey(key, dbase, low_mask);
      if ((sub & pmask) == prefix) atomicAdd(&lh[(int)((sub >> sh) & (u64)(nbins - 1))], 1);
    }
    __syncthreads();
    if (tid < 64) {
      int above, in_bin;
      const int d = od_find_digit(lh, OD_TOPK_NB, krem, &above, &in_bin);  // bins >= nbins are empty
      if (tid == 0) {
        sh_digit = d;
        sh_above = above;
        sh_inbin = in_bin;
      }
    }
    __syncthreads();
    prefix |= (u64)sh_digit << sh;
    pmask |= (u64)(nbins - 1) << sh;
    krem -= sh_above;
    whole = (sh_inbin == krem);
    __syncthreads();
  }
  // winners: sub-key > prefix on the masked bits, or == prefix (then the whole remaining bin is taken)
  for (int i = tid; i < n; i += 1024) {
    const u64 key = key_at(i);
    if (key && (od_refine_subkey(key, dbase, low_mask) & pmask) >= prefix) emit(key);
  }
}

// ---- sort + gather in front of the NMS ---------------------------------------------------------------------------------
// Bitonic sort of s[0..KP) in LDS (KP a power of two <= 1024), descending = (conf desc, flat asc).  1024 threads; the caller
// has published s with a barrier; ends on a barrier.
__device__ __forceinline__ void od_bitonic_sort_desc(u64* s, int KP) {
  const int tid = threadIdx.x;
  for (int k = 2; k <= KP; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      const int ixj = tid ^ j;
      if (tid < KP && ixj > tid) {
        const u64 a = s[tid], c = s[ixj];
        const bool desc = (tid & k) == 0;
        if (desc ? (a < c) : (a > c)) {
          s[tid] = c;
          s[ixj] = a;
        }
      }
      __syncthreads();
    }
  }
}

// Thread tid takes rank tid of image b's sorted s[0..KP): the key goes to skeys, and for the first n ranks the box and the class
// (flat -> (p, c)) to sbox / scls, which is what od_nms_greedy_k reads.  Where the caller asks for them (non-null):
// keys = the API's key set (K slots: sorted, unused slots 0), counts[b] = n, and the image's first-digit histogram is zeroed
// again for the next call; lbox / lcls [n] (LDS) = a copy of the image's sbox / scls for a caller that goes on to the NMS itself.
__device__ __forceinline__ void od_rank_gather(const u64* s, int n, int b, const float* __restrict__ boxes, int P, int NC, int K,
                                               int KP, u64* __restrict__ skeys, f32x4* __restrict__ sbox, int* __restrict__ scls,
                                               u64* __restrict__ keys, int* __restrict__ counts, int* __restrict__ hist,
                                               f32x4* lbox = nullptr, int* lcls = nullptr) {
  const int tid = threadIdx.x;
  if (tid < KP) {
    const u64 key = s[tid];
    skeys[(long long)b * KP + tid] = key;
    if (keys && tid < K) keys[(long long)b * K + tid] = key;
    if (tid < n) {
      const unsigned flat = od_key_flat(key);
      const unsigned p = flat / (unsigned)NC;
      const unsigned c = flat - p * (unsigned)NC;
      const f32x4 box = *(const f32x4*)(boxes + ((long long)b * P + p) * 4);
      sbox[(long long)b * KP + tid] = box;
      scls[(long long)b * KP + tid] = (int)c;
      if (lbox) {
        lbox[tid] = box;
        lcls[tid] = (int)c;
      }
    }
  }
  if (counts && tid == 0) counts[b] = n;
  if (hist) {
    int* gh = hist + (long long)b * OD_TOPK_NB;
    for (int i = tid; i < OD_TOPK_NB; i += 1024) gh[i] = 0;
  }
}

// ---- pass 2 of od_detect (either dispatch): 256 threads, 1024 priors per workgroup ---------------------------------------
constexpr int OD_DT_ROWS = 256;  // priors per workgroup in pass 1 (one thread each)
constexpr int OD_DT2_RPT = 4;    // priors per thread in pass 2

// The workgroup's priors [p_base, p_base + 1024) whose best score (rowmax) reaches the d0 bin -- a few per cent at most -- are
// COMPACTED into hot_list [1024] (LDS) through the LDS counter *n_hot (zeroed and published by the caller) and then taken one
// per thread: walking them where they sit ran every wave through the row code at a few per cent lane occupancy.  Ends on a
// barrier; returns their number.
__device__ __forceinline__ int od_compact_hot_priors(const float* __restrict__ rowmax_b, int P, int p_base, float thr,
                                                     unsigned dbase, int dshift, int d0, int* hot_list, int* n_hot) {
  const int tid = threadIdx.x;
  float mxv[OD_DT2_RPT];
#pragma unroll
  for (int u = 0; u < OD_DT2_RPT; ++u) {
    const int p = p_base + u * OD_DT_ROWS + tid;
    mxv[u] = p < P ? rowmax_b[p] : 0.f;
  }
#pragma unroll
  for (int u = 0; u < OD_DT2_RPT; ++u) {
    const unsigned sb = od_score_bits(mxv[u], thr);
    if (sb && od_digit0(sb, dbase, dshift) >= d0) hot_list[atomicAdd(n_hot, 1)] = p_base + u * OD_DT_ROWS + tid;
  }
  __syncthreads();
  return *n_hot;
}

// The workgroup's n keys in l (LDS; n published by the caller's barrier) go to dst[base..base + n), the range reserved with ONE
// atomic on *total -- a global atomic per element serialises on a few addresses.  Its barrier also publishes whatever else
// thread 0 wrote to LDS just before the call.
__device__ __forceinline__ void od_block_copy_out(const u64* l, int n, int* total, u64* __restrict__ dst, int* sh_base) {
  const int tid = threadIdx.x;
  if (tid == 0) *sh_base = n ? atomicAdd(total, n) : 0;
  __syncthreads();
  u64* o = dst + *sh_base;
  for (int j = tid; j < n; j += 256) o[j] = l[j];
}

// ---- the suppression predicate -----------------------------------------------------------------------------------------
// IoU(a, c) > thr, division-free and in a fixed f32 op order (oracle/nms.py; every TU here is -ffp-contract=off):
// inter > thr * ((area_a + area_c) - inter).  area_a = (a[2] - a[0]) * (a[3] - a[1]), computed once per row by the caller.
__device__ __forceinline__ bool od_iou_exceeds(const f32x4 a, float area_a, const f32x4 c, float thr) {
  const float ix1 = fmaxf(a[0], c[0]), iy1 = fmaxf(a[1], c[1]);
  const float ix2 = fminf(a[2], c[2]), iy2 = fminf(a[3], c[3]);
  const float iw = fmaxf(ix2 - ix1, 0.f), ih = fmaxf(iy2 - iy1, 0.f);
  const float inter = iw * ih;
  const float area_c = (c[2] - c[0]) * (c[3] - c[1]);
  const float uni = (area_a + area_c) - inter;
  return inter > thr * uni;
}

// ---- the greedy suppression of one image ---------------------------------------------------------------------------------
// Row a (class ca) suppresses column c (class cc): same class unless strict, and IoU(a, c) > thr.
__device__ __forceinline__ bool od_suppresses(const f32x4 a, int ca, const f32x4 c, int cc, float thr, int strict) {
  const float area_a = (a[2] - a[0]) * (a[3] - a[1]);
  return (strict || cc == ca) && od_iou_exceeds(a, area_a, c, thr);
}

__device__ __forceinline__ u64 od_readlane64(u64 v, int l) {
  const unsigned lo = __builtin_amdgcn_readlane((unsigned)v, l);
  const unsigned hi = __builtin_amdgcn_readlane((unsigned)(v >> 32), l);
  return ((u64)hi << 32) | lo;
}

// Class-aware greedy NMS of one image's n <= 1024 candidates in rank order by one workgroup of 1024 threads: candidate j is kept
// unless a kept candidate i < j suppresses it; the first max_det kept go to keep_flat (flat index of their key, -1 padded), their
// number to *keep_count.  lb / lc / skeys [n]: the candidates' boxes / classes / keys in LDS, published by the caller's barrier.
// The only IoU tests made are the ones the answer depends on -- kept rows against later columns -- and none once max_det are
// kept.  64 columns (one per lane) at a time:
//   (1) the 16 waves share out the rows kept so far (wave-uniform row: LDS broadcast reads) and OR what they suppress of the
//       block's columns into one 64-bit word;
//   (2) every wave takes four rows of the block itself: __ballot of (row suppresses column, column > row) is that row's word of
//       the 64 x 64 diagonal block;
//   (3) one wave resolves the diagonal block with scalar 64-bit ops on SGPRs (v_readlane; only rows that suppress something take
//       a step), appends the block's kept rows to the list and writes their flat indices.
// Same predicate on the same operands as a full suppression matrix would hold (od_suppresses: oracle/nms.py's op order), so the
// kept indices are oracle/nms.py's bit for bit.
__device__ __forceinline__ void od_nms_greedy(const f32x4* lb, const int* lc, const u64* skeys, int n, float thr, int strict,
                                              int max_det, int* __restrict__ keep_flat, int* __restrict__ keep_count) {
  __shared__ int kept[1024];  // ranks of the kept rows, ascending
  __shared__ u64 dgw[64];     // the diagonal block's row words
  __shared__ u64 remw;        // columns of the block suppressed by rows kept in earlier blocks
  __shared__ int nkept;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  if (tid == 0) {
    remw = 0ull;
    nkept = 0;
  }
  __syncthreads();
  const int W = (n + 63) >> 6;
  int total = 0;  // rows kept so far (workgroup-uniform)
  for (int blk = 0; blk < W && total < max_det; ++blk) {
    const int j = blk * 64 + lane;
    const bool colok = j < n;
    const f32x4 c = colok ? lb[j] : f32x4{0.f, 0.f, 0.f, 0.f};
    const int cc = colok ? lc[j] : -1;
    bool rem = false;
    for (int e = wv; e < total; e += 16) {
      const int r = kept[e];
      rem |= colok && od_suppresses(lb[r], lc[r], c, cc, thr, strict);
    }
    const u64 rw = __ballot(rem);
    if (lane == 0 && rw) atomicOr((u64*)&remw, rw);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int rr = wv * 4 + q, i = blk * 64 + rr;
      const bool hit = i < n && colok && j > i && od_suppresses(lb[i], lc[i], c, cc, thr, strict);
      const u64 wd = __ballot(hit);
      if (lane == 0) dgw[rr] = wd;
    }
    __syncthreads();
    if (wv == 0) {
      const int nv = n - blk * 64;
      const u64 valid = nv >= 64 ? ~0ull : ((1ull << nv) - 1ull);
      u64 alive = ~remw & valid;
      const u64 dg = dgw[lane];
      u64 todo = __ballot(dg != 0ull) & alive;
      while (todo) {
        const int r = __builtin_ctzll(todo);
        todo &= todo - 1ull;
        if ((alive >> r) & 1ull) {
          alive &= ~od_readlane64(dg, r);
          todo &= alive;
        }
      }
      const int pos = total + __popcll(alive & ((1ull << lane) - 1ull));
      if ((alive >> lane) & 1ull) {
        kept[pos] = j;
        if (pos < max_det) keep_flat[pos] = (int)od_key_flat(skeys[j]);
      }
      if (lane == 0) {
        nkept = total + __popcll(alive);
        remw = 0ull;
      }
    }
    __syncthreads();
    total = __builtin_amdgcn_readfirstlane(nkept);
  }
  total = min(total, max_det);
  for (int i = total + tid; i < max_det; i += 1024) keep_flat[i] = -1;
  if (tid == 0) *keep_count = total;
}
