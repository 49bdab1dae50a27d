// K9: prior-box assignment + target encoding = `od.pb.encode_truth` (reference check_assign.py:21,25-27).
// Per image: GT boxes x priors IoU, argmax both ways, dense target rows y[P, 2+NC+4]:
//   y[p,0]=1 background | y[p,1]=1 assigned (check_assign.py:25) | y[p,2:2+NC] one-hot class (:26) |
//   y[p,-4:] corner-form regression target, the inverse of decode_locs (:27)
// [BUILD-DEFINED] rule (the reference does not pin it; mirrored op-for-op by oracle/assign.py):
//   1. prior p takes GT g* = argmax_g IoU(g,p) (ties: lowest g) if IoU >= pos_thr; if neg_thr <= IoU < pos_thr the
//      row is "ignore" (all zeros: no objectness loss); otherwise background
//   2. every GT g (ascending g, later wins) force-takes p* = argmax_p IoU(g,p) (ties: lowest p) when that IoU > 0
// Ignore regions (od_assign_anchors_ign, gt_flags bit 0; [BUILD-DEFINED] like the rule above, mirrored by
// tests/assign_ign_ref.py): a flagged GT (COCO iscrowd, VOC difficult, a mosaic sliver) never owns a prior -- it is left out
// of steps 1 and 2 and of npos -- and
//   3. a prior that came out of 1 + 2 as BACKGROUND becomes "ignore" (all-zero row, assigned_gt -3) when
//      inter(prior, r) / area(prior) >= ign_thr for any flagged box r.  Positives stay positive; -2 rows stay -2.
// HBM-bound elementwise work; IoU uses IEEE f32 division; compiled with -ffp-contract=off => bit-exact vs numpy.
#include "assign_common.h"

namespace {

// the per-prior loop of pass 1 over the boxes in LDS; SKIP: a flagged box (bit g of smask) owns no prior
template <bool SKIP>
__device__ __forceinline__ void match_boxes(const f32x4* sg, u64* sbest, const u64* smask, int G, const f32x4 pr, int p,
                                            int& bg, float& bi) {
  for (int g = 0; g < G; ++g) {
    if (SKIP && ((smask[g >> 6] >> (g & 63)) & 1ull)) continue;
    const float v = iou_f32(sg[g], pr);
    if (v > bi) {
      bi = v;
      bg = g;
    }
    if (v > 0.f) atomicMax(&sbest[g], ((u64)__float_as_uint(v) << 32) | (u64)(0xFFFFFFFFu - (unsigned)p));
  }
}

// pass 1: per prior best GT; per GT best prior (u64 atomicMax on (iou_bits << 32 | ~p))
template <bool IGN>
__global__ __launch_bounds__(256) void od_assign_match(const float* __restrict__ priors, const float* __restrict__ gt_boxes,
                                                       const int* __restrict__ gt_counts,
                                                       const int* __restrict__ gt_flags, int P, int Gmax,
                                                       int* __restrict__ best_g, float* __restrict__ best_iou,
                                                       u64* __restrict__ gt_best) {
  __shared__ f32x4 sg[GMAX];
  __shared__ u64 sbest[GMAX];
  __shared__ u64 smask[GMAX / 64];
  const int b = blockIdx.y, tid = threadIdx.x;
  const int G = min(gt_counts[b], Gmax);
  for (int g = tid; g < G; g += 256) {
    sg[g] = *(const f32x4*)(gt_boxes + ((long long)b * Gmax + g) * 4);
    sbest[g] = 0ull;
  }
  if (IGN) stage_flags(gt_flags + (long long)b * Gmax, G, tid, smask);
  __syncthreads();
  const int p = blockIdx.x * 256 + tid;
  if (p < P) {
    const f32x4 pr = *(const f32x4*)(priors + (long long)p * 4);
    int bg = -1;
    float bi = 0.f;
    // an image without regions (the usual case) runs the loop of od_assign_anchors; with regions, flagged boxes are skipped
    if (!IGN || !(smask[0] | smask[1]))
      match_boxes<false>(sg, sbest, smask, G, pr, p, bg, bi);
    else
      match_boxes<true>(sg, sbest, smask, G, pr, p, bg, bi);
    best_g[(long long)b * P + p] = bg;
    best_iou[(long long)b * P + p] = bi;
  }
  __syncthreads();
  for (int g = tid; g < G; g += 256)
    if (sbest[g]) atomicMax(&gt_best[(long long)b * Gmax + g], sbest[g]);
}

// pass 2: resolve + encode dense rows; counts positives per image
template <bool IGN>
__global__ __launch_bounds__(256) void od_assign_encode(const float* __restrict__ priors, const float* __restrict__ gt_boxes,
                                                        const int* __restrict__ gt_classes,
                                                        const int* __restrict__ gt_counts,
                                                        const int* __restrict__ gt_flags, int P, int Gmax, int NC,
                                                        float pos_thr, float neg_thr, float ign_thr, float loc_scale,
                                                        const int* __restrict__ best_g, const float* __restrict__ best_iou,
                                                        const u64* __restrict__ gt_best, float* __restrict__ y,
                                                        int* __restrict__ assigned_gt, int* __restrict__ npos) {
  __shared__ unsigned sforce[GMAX];
  __shared__ int scount;
  __shared__ u64 smask[GMAX / 64];
  const int b = blockIdx.y, tid = threadIdx.x;
  const int G = min(gt_counts[b], Gmax);
  for (int g = tid; g < G; g += 256) {
    const u64 k = gt_best[(long long)b * Gmax + g];  // 0 for a flagged box: the match pass never offered it a prior
    sforce[g] = k ? 0xFFFFFFFFu - (unsigned)(k & 0xFFFFFFFFull) : 0xFFFFFFFFu;
  }
  if (IGN) stage_flags(gt_flags + (long long)b * Gmax, G, tid, smask);
  if (tid == 0) scount = 0;
  __syncthreads();
  const int p = blockIdx.x * 256 + tid;
  if (p < P) {
    const int C = NC + 6;
    int g = -1;        // assigned GT
    bool ignore = false;
    const int bg = best_g[(long long)b * P + p];
    const float bi = best_iou[(long long)b * P + p];
    if (bg >= 0 && bi >= pos_thr) g = bg;
    else if (bg >= 0 && bi >= neg_thr) ignore = true;
    for (int q = 0; q < G; ++q)
      if (sforce[q] == (unsigned)p) g = q;  // later GT wins
    bool region = false;
    if (IGN && g < 0 && !ignore && (smask[0] | smask[1])) {  // background prior of an image that has regions
      const f32x4 pr = *(const f32x4*)(priors + (long long)p * 4);
      region = region_covers(gt_boxes + (long long)b * Gmax * 4, smask, pr, ign_thr);
    }
    float* row = y + ((long long)b * P + p) * C;
    for (int c = 0; c < C; ++c) row[c] = 0.f;
    if (g >= 0) {
      const f32x4 pr = *(const f32x4*)(priors + (long long)p * 4);
      const f32x4 gb = *(const f32x4*)(gt_boxes + ((long long)b * Gmax + g) * 4);
      write_owned_row(row, NC, pr, gb, gt_classes[(long long)b * Gmax + g], loc_scale);
      atomicAdd(&scount, 1);
    } else if (!ignore && !region) {
      row[0] = 1.f;
    }
    if (assigned_gt) assigned_gt[(long long)b * P + p] = g >= 0 ? g : (ignore ? -2 : (region ? -3 : -1));
  }
  __syncthreads();
  if (tid == 0 && scount) atomicAdd(&npos[b], scount);
}

struct AssignLayout {
  size_t best_g, best_iou, gt_best, total;
};
AssignLayout assign_layout(int B, int P, int Gmax) {
  AssignLayout l;
  size_t o = 0;
  l.gt_best = o;
  o += ((size_t)B * Gmax * 8 + 255) & ~(size_t)255;
  l.best_g = o;
  o += (size_t)B * P * 4;
  l.best_iou = o;
  o += (size_t)B * P * 4;
  l.total = o;
  return l;
}

}  // namespace

extern "C" size_t od_assign_workspace_bytes(int B, int P, int Gmax) {
  if (B <= 0 || P <= 0 || Gmax <= 0) return 0;
  return assign_layout(B, P, Gmax).total;
}

namespace {
template <bool IGN>
int assign_launch(const char* who, od_ctx* ctx, const float* priors, const float* gt_boxes, const int32_t* gt_classes,
                  const int32_t* gt_counts, const int32_t* gt_flags, int B, int P, int Gmax, int NC, float pos_thr,
                  float neg_thr, float ign_thr, float loc_scale, float* y, int32_t* assigned_gt, int32_t* npos,
                  void* workspace, size_t workspace_bytes, void* stream) {
  OD_REQUIRE(ctx && priors && gt_boxes && gt_classes && gt_counts && y && npos && workspace && (!IGN || gt_flags),
             "%s: null argument", who);
  OD_REQUIRE(B > 0 && B <= 65535 && P > 0 && NC > 0 && Gmax > 0 && Gmax <= GMAX, "%s: bad dims (Gmax <= %d)", who, GMAX);
  OD_REQUIRE(loc_scale > 0.f && pos_thr >= neg_thr && (!IGN || ign_thr > 0.f), "%s: bad thresholds", who);
  const AssignLayout l = assign_layout(B, P, Gmax);
  if (workspace_bytes < l.total) {
    od_set_error("%s: workspace %zu < %zu bytes", who, workspace_bytes, l.total);
    return OD_ERR_WORKSPACE;
  }
  char* ws = (char*)workspace;
  hipStream_t s = (hipStream_t)stream;
  OD_CHECK_HIP(hipMemsetAsync(ws + l.gt_best, 0, (size_t)B * Gmax * 8, s));
  OD_CHECK_HIP(hipMemsetAsync(npos, 0, (size_t)B * 4, s));
  dim3 grid(od_ceil_div(P, 256), B);
  hipLaunchKernelGGL(od_assign_match<IGN>, grid, dim3(256), 0, s, priors, gt_boxes, gt_counts, gt_flags, P, Gmax,
                     (int*)(ws + l.best_g), (float*)(ws + l.best_iou), (u64*)(ws + l.gt_best));
  OD_CHECK_LAUNCH();
  hipLaunchKernelGGL(od_assign_encode<IGN>, grid, dim3(256), 0, s, priors, gt_boxes, gt_classes, gt_counts, gt_flags, P,
                     Gmax, NC, pos_thr, neg_thr, ign_thr, loc_scale, (const int*)(ws + l.best_g),
                     (const float*)(ws + l.best_iou), (const u64*)(ws + l.gt_best), y, assigned_gt, npos);
  OD_CHECK_LAUNCH();
  return OD_OK;
}
}  // namespace

extern "C" int od_assign_anchors(od_ctx* ctx, const float* priors, const float* gt_boxes, const int32_t* gt_classes,
                                 const int32_t* gt_counts, int B, int P, int Gmax, int NC, float pos_thr, float neg_thr,
                                 float loc_scale, float* y, int32_t* assigned_gt, int32_t* npos, void* workspace,
                                 size_t workspace_bytes, void* stream) {
  return assign_launch<false>("od_assign_anchors", ctx, priors, gt_boxes, gt_classes, gt_counts, nullptr, B, P, Gmax, NC,
                              pos_thr, neg_thr, 0.f, loc_scale, y, assigned_gt, npos, workspace, workspace_bytes, stream);
}

// the same two passes with ignore regions (rule 3 of the header comment); workspace: od_assign_workspace_bytes
extern "C" int od_assign_anchors_ign(od_ctx* ctx, const float* priors, const float* gt_boxes, const int32_t* gt_classes,
                                     const int32_t* gt_counts, const int32_t* gt_flags, float ign_thr, int B, int P,
                                     int Gmax, int NC, float pos_thr, float neg_thr, float loc_scale, float* y,
                                     int32_t* assigned_gt, int32_t* npos, void* workspace, size_t workspace_bytes,
                                     void* stream) {
  return assign_launch<true>("od_assign_anchors_ign", ctx, priors, gt_boxes, gt_classes, gt_counts, gt_flags, B, P, Gmax,
                             NC, pos_thr, neg_thr, ign_thr, loc_scale, y, assigned_gt, npos, workspace, workspace_bytes,
                             stream);
}
