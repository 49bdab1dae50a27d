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
// (flat -> (p, c)) to sbox / scls, which is what od_nms_mask / od_nms_scan read.  Where the caller asks for them (non-null):
// keys = the API's key set (K slots: sorted, unused slots 0), counts[b] = n, and the image's first-digit histogram is zeroed
// again for the next call.
__device__ __forceinline__ void od_rank_gather(const u64* s, int n, int b, const float* __restrict__ boxes, int P, int NC, int K,
                                               int KP, u64* __restrict__ skeys, f32x4* __restrict__ sbox, int* __restrict__ scls,
                                               u64* __restrict__ keys, int* __restrict__ counts, int* __restrict__ hist) {
  const int tid = threadIdx.x;
  if (tid < KP) {
    const u64 key = s[tid];
    skeys[(long long)b * KP + tid] = key;
    if (keys && tid < K) keys[(long long)b * K + tid] = key;
    if (tid < n) {
      const unsigned flat = od_key_flat(key);
      const unsigned p = flat / (unsigned)NC;
      const unsigned c = flat - p * (unsigned)NC;
      sbox[(long long)b * KP + tid] = *(const f32x4*)(boxes + ((long long)b * P + p) * 4);
      scls[(long long)b * KP + tid] = (int)c;
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
