// Shared by post.hip (K5/K6), topk.hip (K7), nms.hip (K8), soft_nms.hip, detect.hip and detect_wide.hip (the fused product
// path), merge.hip (the merged candidate tables of TTA and sliced inference) and slice.hip:
// the confidence arithmetic and the histogram searches here; the key format, the radix refine, the sort / gather and the IoU
// predicate in topk_common.h (included at the end).  Every TU that includes this is compiled with -ffp-contract=off, so the
// same source is the same f32 op sequence everywhere (and the one of oracle/postprocess.py): confidences are bit-identical
// across kernels.
#pragma once
#include "common.h"

constexpr int OD_TOPK_NB = 4096;  // histogram bins: first radix digit = score bits [30:19]

struct TopkState {  // per image
  int d0;           // first digit of the K-th key; -1 = take every candidate (fewer than K exist)
  int krem;         // how many to take from the d0 bin
  int nout;         // output slots used
  int ncand;        // candidate-list length
};

// conf[c] = sigmoid(l1 - l0) * softmax(classes)[c]  (docs/MODEL.md:54-58), written over out[0..NC); `out` may alias
// row + 2 (in place over the class logits): every logit is read before its slot is written.
__device__ __forceinline__ void od_row_conf(const float* row, int NC, float* out) {
  const float obj = 1.f / (1.f + expf(row[0] - row[1]));
  float mx = row[2];
  for (int c = 1; c < NC; ++c) mx = fmaxf(mx, row[2 + c]);
  float s = 0.f;
  for (int c = 0; c < NC; ++c) {
    const float e = expf(row[2 + c] - mx);
    out[c] = e;
    s += e;
  }
  for (int c = 0; c < NC; ++c) out[c] = obj * (out[c] / s);
}

// ---- class counts beyond a [256][NC+6] LDS row block (NC > 76, up to OD_MAX_NC) ----
// The same confidence as od_row_conf, taken apart into its three sweeps over a row (max; sum of expf in ascending c;
// obj * (e / s)) so that the class columns can be streamed instead of held: every op happens in the same order on the
// same inputs, and expf(l - mx) recomputed in the third sweep is the same instruction on the same operands, so the
// confidences are bit-identical to od_row_conf's (and to oracle/postprocess.confidence).
constexpr int OD_MAX_LDS_NC = 76;  // the largest NC whose [256][NC+6] rows (+ histogram / output) fit the LDS kernels
constexpr int OD_MAX_NC = 1024;
constexpr int OD_MERGE_MAX_K = 1024;  // the longest candidate list: one thread per entry in the one-workgroup-per-image kernels
constexpr int OD_WIDE_CW = 32;              // class columns per LDS chunk
constexpr int OD_WIDE_LD = OD_WIDE_CW + 1;  // tile row pitch: a thread walking its own row hits a different bank per lane

struct OdRowStats {
  float obj, mx, s;  // objectness probability, max class logit, sum of expf(l - mx)
};

__device__ __forceinline__ float od_wide_conf(float l, const OdRowStats& r) { return r.obj * (expf(l - r.mx) / r.s); }

// sweeps 1-2 of one row read straight from memory (the few rows pass 2 / the gather look at again)
__device__ __forceinline__ OdRowStats od_row_stats(const float* row, int NC) {
  OdRowStats r;
  r.obj = 1.f / (1.f + expf(row[0] - row[1]));
  r.mx = row[2];
  for (int c = 1; c < NC; ++c) r.mx = fmaxf(r.mx, row[2 + c]);
  r.s = 0.f;
  for (int c = 0; c < NC; ++c) r.s += expf(row[2 + c] - r.mx);
  return r;
}

// tile[r][0..ncols) = src[r * C + col0 + 0..ncols) for r < nrows; 256 threads, 4-byte loads (for odd NC a row start is only
// 4-byte aligned), 32 consecutive lanes on 32 consecutive floats of one row
__device__ __forceinline__ void od_wide_stage(const float* __restrict__ src, int C, int nrows, int col0, int ncols,
                                              float* tile) {
  for (int i = threadIdx.x; i < nrows * OD_WIDE_CW; i += 256) {
    const int r = i / OD_WIDE_CW, c = i % OD_WIDE_CW;
    if (c < ncols) tile[r * OD_WIDE_LD + c] = src[(long long)r * C + col0 + c];
  }
}

// sweeps 1-2 for the rows [0, nrows) of src (row stride C, <= 256 rows, one thread each), the class columns streamed
// through `tile` [256][OD_WIDE_LD].  Thread tid < nrows gets its row's stats.  All 256 threads call it (barriers); it
// ends on a barrier, so the caller may reuse the tile at once.
__device__ __forceinline__ OdRowStats od_wide_stats(const float* __restrict__ src, int C, int NC, int nrows, float* tile) {
  const int tid = threadIdx.x;
  OdRowStats r = {0.f, 0.f, 0.f};
  const float* row = src + (long long)tid * C;
  if (tid < nrows) r.obj = 1.f / (1.f + expf(row[0] - row[1]));
  for (int sweep = 0; sweep < 2; ++sweep) {
    for (int c0 = 0; c0 < NC; c0 += OD_WIDE_CW) {
      const int w = min(OD_WIDE_CW, NC - c0);
      od_wide_stage(src, C, nrows, 2 + c0, w, tile);
      __syncthreads();
      if (tid < nrows) {
        const float* t = tile + tid * OD_WIDE_LD;
        if (sweep == 0) {
          for (int c = 0; c < w; ++c) r.mx = (c0 + c == 0) ? t[c] : fmaxf(r.mx, t[c]);
        } else {
          for (int c = 0; c < w; ++c) r.s += expf(t[c] - r.mx);
        }
      }
      __syncthreads();
    }
  }
  return r;
}

__device__ __forceinline__ unsigned od_score_bits(float v, float thr) {
  return v > thr ? __float_as_uint(v) : 0u;  // positive floats: bit pattern is monotone in value
}

// boxes = prior + (loc * loc_scale) * [pw, ph, pw, ph], optional clip to [0,1]   (od.pb.decode_locs,
// reference check_assign.py:27: zero offsets decode to the prior itself)
__device__ __forceinline__ f32x4 od_decode_one(f32x4 loc, f32x4 pr, float loc_scale, int clip) {
  const float pw = pr[2] - pr[0], ph = pr[3] - pr[1];
  f32x4 o;
  o[0] = pr[0] + (loc[0] * loc_scale) * pw;
  o[1] = pr[1] + (loc[1] * loc_scale) * ph;
  o[2] = pr[2] + (loc[2] * loc_scale) * pw;
  o[3] = pr[3] + (loc[3] * loc_scale) * ph;
  if (clip) {
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = fminf(fmaxf(o[e], 0.f), 1.f);
  }
  return o;
}

// First radix digit.  Confidences are products of two probabilities, so a candidate's bit pattern lies in (bits(thr),
// bits(1.0)]: the 4096 bins are spread over THAT range (dbase = bits(thr), dshift = the smallest shift that fits it) instead of
// over all exponents -- at thr = 0.01 a bin is 2^14 ulps (0.2 % of the value) wide instead of 2^19 (4.4 %): the threshold bin
// holds 22x fewer scores, and far fewer priors have to be looked at again in pass 2.
__device__ __forceinline__ int od_digit0(unsigned sb, unsigned dbase, int dshift) { return (int)((sb - dbase) >> dshift); }

// Block-wide (256 threads) search of a 4096-bin GLOBAL histogram for the bin where the count of elements in higher bins first
// reaches >= krem: every thread owns 16 consecutive bins in registers (one round of loads), a suffix scan over the 256
// partial sums (wave shuffles + four partials through LDS) finds the owner, the owner walks its 16 bins.
__device__ __forceinline__ void od_find_digit_256(const int* __restrict__ gh, int krem, int* sh /* [8] LDS */, int* d_out,
                                                  int* above_out) {
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  int v[16];
  int tot = 0;
  const int4* g4 = (const int4*)(gh + tid * 16);
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int4 t = g4[q];
    v[4 * q] = t.x, v[4 * q + 1] = t.y, v[4 * q + 2] = t.z, v[4 * q + 3] = t.w;
    tot += t.x + t.y + t.z + t.w;
  }
  int suf = tot;  // inclusive suffix sum over the lanes of this wave
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int o = __shfl_down(suf, off);
    if (lane + off < 64) suf += o;
  }
  if (lane == 0) sh[wv] = suf;  // the wave's total
  if (tid == 0) {
    sh[4] = -1;
    sh[5] = 0;
  }
  __syncthreads();
  int higher_waves = 0;
  for (int w = wv + 1; w < 4; ++w) higher_waves += sh[w];
  const int incl = suf + higher_waves, higher = incl - tot;  // elements in the bins of this thread and above / strictly above
  if (higher < krem && incl >= krem) {  // exactly one thread
    int run = higher;
#pragma unroll
    for (int q = 15; q >= 0; --q) {
      if (run + v[q] >= krem) {
        sh[4] = tid * 16 + q;
        sh[5] = run;
        break;
      }
      run += v[q];
    }
  }
  __syncthreads();
  *d_out = sh[4];
  *above_out = sh[5];
}

// Wave-level search of an nbins-bin histogram (in LDS or global) for the bin where the count of elements in HIGHER
// bins first reaches >= krem.  Returns digit (uniform) and *above = #elements in bins above it.  One wave.
__device__ __forceinline__ int od_find_digit(const int* hist, int nbins, int krem, int* above, int* in_bin) {
  const int lane = threadIdx.x & 63;
  const int per = nbins / 64;  // bins per lane; lane l owns bins [l*per, (l+1)*per)
  int s = 0;
  for (int i = 0; i < per; ++i) s += hist[lane * per + i];
  // inclusive suffix sum over lanes: suf = sum over lanes >= lane
  int suf = s;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int o = __shfl_down(suf, off);
    if (lane + off < 64) suf += o;
  }
  const int higher = suf - s;  // elements in lanes above this one
  const bool mine = higher < krem && suf >= krem;
  const unsigned long long bal = __ballot(mine);
  int digit = -1, ab = 0, ib = 0;
  if (bal) {
    const int owner = __ffsll((long long)bal) - 1;
    if (lane == owner) {
      int run = higher;
      for (int i = per - 1; i >= 0; --i) {
        const int c = hist[lane * per + i];
        if (run + c >= krem) {
          digit = lane * per + i;
          ab = run;
          ib = c;
          break;
        }
        run += c;
      }
    }
    digit = __shfl(digit, owner);
    ab = __shfl(ab, owner);
    ib = __shfl(ib, owner);
  }
  *above = ab;
  *in_bin = ib;
  return digit;
}

#include "topk_common.h"

// a prior that may hold a d0-bin candidate, as pass 2 of the NC > 76 pipeline records it (detect_wide.hip)
struct HotRow {
  int p;
  OdRowStats r;
};
// detect_wide.hip: od_detect's pass 1 / pass 2 / refine launches for NC > 76 (the caller launches the NMS)
int od_detect_wide_launch(const float* pred, const float* priors, int B, int P, int NC, float loc_scale, int clip, float thr,
                          unsigned dbase, int dshift, int K, int KP, float* boxes, float* conf, unsigned long long* keys,
                          int* counts, int* hist, TopkState* st, float* rowmax, int* nhot, HotRow* hot,
                          unsigned long long* skeys, f32x4* sbox, int* scls, hipStream_t s);
// detect_wide.hip: od_gather_detections_pred's launch for NC > 76
int od_gather_det_pred_wide_launch(const float* pred, const float* boxes, const int32_t* keep_flat, const int32_t* keep_count,
                                   int B, int P, int NC, int max_det, float* out, hipStream_t s);
// nms.hip: the greedy-suppression launch of od_nms on already sorted / gathered candidates
int od_nms_greedy_launch(void* nms_workspace, const int32_t* counts, int B, int K, float iou_threshold, int strict, int max_det,
                         int32_t* keep_flat, int32_t* keep_count, hipStream_t stream);
// nms.hip: where od_nms keeps the sorted keys / gathered boxes / classes inside its workspace (KP = next power of two >= K)
void od_nms_sorted_buffers(void* nms_workspace, int B, int K, unsigned long long** skeys, f32x4** sbox, int** scls, int* KP);
// nms.hip: od_nms's sort launch (keys -> the rank-ordered keys / boxes / classes of the workspace)
int od_nms_sort_launch(void* nms_workspace, const float* boxes, const unsigned long long* keys, const int32_t* counts, int B, int P,
                       int NC, int K, hipStream_t s);
// nms.hip: the part of the NMS workspace behind the rank-ordered buffers, >= B * KP * 8 bytes that no scan reads or writes:
// where the soft merges (merge.hip) keep the kept rows' rescored confidences between the scan and the vote-and-gather kernel
float* od_nms_scratch(void* nms_workspace, int B, int K);
// soft_nms.hip: the argument checks every soft entry shares (OD_OK or OD_ERR_*, error text set), and the soft scan's launch on
// the rank-ordered buffers of the NMS workspace (det may be null)
int od_soft_cfg_check(const char* who, const od_soft_nms_cfg* cfg, int K);
int od_soft_scan_launch(void* nms_workspace, const int32_t* counts, int B, int K, const od_soft_nms_cfg& cfg, int32_t* keep_flat,
                        float* keep_conf, int32_t* keep_count, float* det, hipStream_t s);
