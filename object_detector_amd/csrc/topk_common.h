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

// ---- Soft-NMS (DESIGN.md "Soft-NMS") ---------------------------------------------------------------------------------------
// exp(-x) for x >= 0 in a fixed f32 op order (Cephes' expf reduction and polynomial, every mul and add rounded on its own:
// the TU is -ffp-contract=off), so that tests/soft_nms_ref.py's numpy restatement has the same bits.  expf / __expf do not.
__device__ __forceinline__ float od_exp_neg(float x) {
  if (x > 80.f) return 0.f;
  const float n = rintf(1.44269504f * x);
  const float r = (x - n * 0.693359375f) - n * (-2.12194440e-4f);
  const float y = -r;
  float p = 1.9875691500e-4f;
  p = p * y + 1.3981999507e-3f;
  p = p * y + 8.3334519073e-3f;
  p = p * y + 4.1665795894e-2f;
  p = p * y + 1.6666665459e-1f;
  p = p * y + 5.0000001201e-1f;
  const float e = ((p * (y * y)) + y) + 1.f;
  return e * __uint_as_float((unsigned)(127 - (int)n) << 23);
}

// The score of live column c (class cc) after row a (class ca, area_a) has been emitted; 0 = no longer a candidate (removed,
// or not > min_conf any more).  inter / uni are od_iou_exceeds' (same ops, same order).
__device__ __forceinline__ float od_soft_rescore(const f32x4 a, float area_a, int ca, const f32x4 c, int cc, float s,
                                                 const od_soft_nms_cfg& cfg) {
  if (!(cfg.strict || cc == ca)) return s;
  const float ix1 = fmaxf(a[0], c[0]), iy1 = fmaxf(a[1], c[1]);
  const float ix2 = fminf(a[2], c[2]), iy2 = fminf(a[3], c[3]);
  const float iw = fmaxf(ix2 - ix1, 0.f), ih = fmaxf(iy2 - iy1, 0.f);
  const float inter = iw * ih;
  if (!(inter > 0.f)) return s;
  const float area_c = (c[2] - c[0]) * (c[3] - c[1]);
  const float uni = (area_a + area_c) - inter;
  if (cfg.method == 2) {
    const float iou = inter / uni;
    s = s * od_exp_neg((iou * iou) / cfg.sigma);
  } else if (inter > cfg.iou_threshold * uni) {
    s = cfg.method == 1 ? s * (1.f - inter / uni) : 0.f;
  }
  return s > cfg.min_conf ? s : 0.f;
}

// max of a 64-bit key over the wave, valid in LANE 63: six DPP steps in registers (row_shr 1 / 2 / 4 / 8 inside the rows of 16
// lanes, then row_bcast 15 and 31 across them), no LDS traffic -- the shuffle form (ds_bpermute) measured 1.5x slower per
// round.  A lane the step does not reach keeps its own value (old = v), which max() absorbs.
template <int CTRL>
__device__ __forceinline__ u64 od_dpp_max64(u64 v) {
  const int lo = (int)(unsigned)v, hi = (int)(unsigned)(v >> 32);
  const unsigned olo = (unsigned)__builtin_amdgcn_update_dpp(lo, lo, CTRL, 0xf, 0xf, false);
  const unsigned ohi = (unsigned)__builtin_amdgcn_update_dpp(hi, hi, CTRL, 0xf, 0xf, false);
  const u64 o = ((u64)ohi << 32) | olo;
  return o > v ? o : v;
}
__device__ __forceinline__ u64 od_wave_max64_lane63(u64 v) {
  v = od_dpp_max64<0x111>(v);  // row_shr:1
  v = od_dpp_max64<0x112>(v);  // row_shr:2
  v = od_dpp_max64<0x114>(v);  // row_shr:4
  v = od_dpp_max64<0x118>(v);  // row_shr:8 -> lane 15 of every row holds the row's max
  v = od_dpp_max64<0x142>(v);  // row_bcast:15 -> lanes 31 / 63 hold the max of their half
  v = od_dpp_max64<0x143>(v);  // row_bcast:31 -> lane 63 holds the wave's
  return v;
}

// Soft-NMS of one image's n <= NT * CPL candidates in rank order by one workgroup of NT threads (a power of two >= 64), CPL
// candidates per thread in registers (candidate j = tid + q * NT): box, class and the running score (0 = not live).  A round
// emits the live candidate with the largest (score bits, inverted rank) key -- the wave's max by DPP steps, the workgroup's
// through one LDS slot per wave, double-buffered so that a round costs ONE barrier (none for NT = 64) -- and rescores the
// live candidates against it (od_soft_rescore).  The emitted ranks / scores are collected in LDS and written at the end:
// keep_flat [max_det] (flat index of the key, -1 padded), keep_conf [max_det] (0 padded), *keep_count, and when det is
// non-null the image's record block [1 + 6 * max_det] in od_gather_detections' layout with the rescored confidence.
// lb / lc / skeys [n]: the candidates' boxes / classes / keys in LDS, published by the caller's barrier.  No atomics, no
// dependence on scheduling: every thread computes the same winner from the same 64-bit keys.
template <int NT, int CPL>
__device__ __forceinline__ void od_soft_nms_scan(const f32x4* lb, const int* lc, const u64* skeys, int n,
                                                 const od_soft_nms_cfg cfg, int* __restrict__ keep_flat,
                                                 float* __restrict__ keep_conf, int* __restrict__ keep_count,
                                                 float* __restrict__ det) {
  constexpr int NW = NT / 64;
  __shared__ int e_rank[NT * CPL];    // emitted ranks, in emission order
  __shared__ float e_conf[NT * CPL];  // and their scores at emission
  __shared__ u64 part[2][NW];
  const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63;
  f32x4 box[CPL];
  int cls[CPL];
  float sc[CPL];
#pragma unroll
  for (int q = 0; q < CPL; ++q) {
    const int j = tid + q * NT;
    const bool ok = j < n;
    box[q] = ok ? lb[j] : f32x4{0.f, 0.f, 0.f, 0.f};
    cls[q] = ok ? lc[j] : -1;
    const float s = ok ? __uint_as_float(od_key_score_bits(skeys[j])) : 0.f;
    sc[q] = s > cfg.min_conf ? s : 0.f;
  }
  const int limit = min(cfg.max_det, n);
  int kept = 0;
  while (kept < limit) {
    u64 best = 0ull;
#pragma unroll
    for (int q = 0; q < CPL; ++q) {
      const u64 k = sc[q] > 0.f ? od_make_key(__float_as_uint(sc[q]), (unsigned)(tid + q * NT)) : 0ull;
      best = k > best ? k : best;
    }
    best = od_wave_max64_lane63(best);
    if (NW > 1) {
      u64* pp = part[kept & 1];
      if (lane == 63) pp[wv] = best;
      __syncthreads();
      best = pp[0];
#pragma unroll
      for (int w = 1; w < NW; ++w) {
        const u64 o = pp[w];
        best = o > best ? o : best;
      }
    } else {
      best = od_readlane64(best, 63);
    }
    if (!best) break;  // workgroup-uniform
    const int i = (int)od_key_flat(best);
    const float si = __uint_as_float(od_key_score_bits(best));
    if (tid == 0) {
      e_rank[kept] = i;
      e_conf[kept] = si;
    }
    ++kept;
    const f32x4 a = lb[i];
    const int ca = lc[i];
    const float area_a = (a[2] - a[0]) * (a[3] - a[1]);
#pragma unroll
    for (int q = 0; q < CPL; ++q) {
      if (tid + q * NT == i) sc[q] = 0.f;
      else if (sc[q] > 0.f) sc[q] = od_soft_rescore(a, area_a, ca, box[q], cls[q], sc[q], cfg);
    }
  }
  __syncthreads();  // e_rank / e_conf
  for (int r = tid; r < cfg.max_det; r += NT) {
    const bool ok = r < kept;
    const int i = ok ? e_rank[r] : 0;
    const int flat = ok ? (int)od_key_flat(skeys[i]) : -1;
    const float conf = ok ? e_conf[r] : 0.f;
    keep_flat[r] = flat;
    keep_conf[r] = conf;
    if (det) {
      float* rec = det + 1 + 6 * (size_t)r;
      const f32x4 bx = ok ? lb[i] : f32x4{0.f, 0.f, 0.f, 0.f};
      rec[0] = __int_as_float(flat);
      rec[1] = conf;
      rec[2] = bx[0];
      rec[3] = bx[1];
      rec[4] = bx[2];
      rec[5] = bx[3];
    }
  }
  if (tid == 0) {
    *keep_count = kept;
    if (det) det[0] = __int_as_float(kept);
  }
}
