// K8: class-aware greedy NMS on the K best candidates of every image (docs/MODEL.md:78-82: among the confident
// predictions, same-class overlaps keep only the most confident).  Integer / bit work, latency-bound; two launches:
//   sort : one workgroup per image, bitonic sort of the K 64-bit keys in LDS (descending = (conf desc, flat asc)),
//          gather of the candidates' boxes / classes into rank order (od_bitonic_sort_desc / od_rank_gather of
//          topk_common.h: the sort and gather at the end of od_detect's refine kernels are the same functions)
//   greedy : one workgroup per image (od_nms_greedy of topk_common.h, which od_detect's tail kernel runs on the candidates it has
//          just sorted): 64 columns at a time, the rows kept so far against the block's columns, the block's own 64 x 64 words by
//          __ballot, one wave resolving them with scalar 64-bit ops -- only the IoU tests the answer depends on, none once
//          max_det rows are kept, no suppression matrix in memory
// The IoU predicate (od_iou_exceeds, topk_common.h) is division-free f32 arithmetic in a fixed order; this TU is compiled with
// -ffp-contract=off so it is bit-identical to numpy's (oracle/nms.py), which is what makes the kept-index output bit-exact.
#include "post_common.h"

namespace {

__global__ __launch_bounds__(1024) void od_nms_sort(const float* __restrict__ boxes, const u64* __restrict__ keys,
                                                    const int* __restrict__ counts, int P, int NC, int K, int KP,
                                                    u64* __restrict__ skeys, f32x4* __restrict__ sbox,
                                                    int* __restrict__ scls) {
  __shared__ u64 s[1024];
  const int b = blockIdx.x, tid = threadIdx.x;
  if (tid < KP) s[tid] = tid < K ? keys[(long long)b * K + tid] : 0ull;
  __syncthreads();
  od_bitonic_sort_desc(s, KP);
  od_rank_gather(s, counts[b], b, boxes, P, NC, K, KP, skeys, sbox, scls, nullptr, nullptr, nullptr);
}

// One workgroup per image: the candidates' keys / boxes / classes from the workspace into LDS, then od_nms_greedy.
// Dynamic LDS: keys [KP] | boxes [KP] | classes [KP].
__global__ __launch_bounds__(1024) void od_nms_greedy_k(const u64* __restrict__ skeys, const f32x4* __restrict__ sbox,
                                                       const int* __restrict__ scls, const int* __restrict__ counts, int KP,
                                                       float thr, int strict, int max_det, int* __restrict__ keep_flat,
                                                       int* __restrict__ keep_count) {
  extern __shared__ __attribute__((aligned(16))) char sm[];
  f32x4* lb = (f32x4*)sm;        // [KP]
  u64* lk = (u64*)(lb + KP);     // [KP]
  int* lc = (int*)(lk + KP);     // [KP]
  const int b = blockIdx.x, tid = threadIdx.x;
  const int n = min(counts[b], KP);
  if (tid < n) {
    lb[tid] = sbox[(long long)b * KP + tid];
    lk[tid] = skeys[(long long)b * KP + tid];
    lc[tid] = scls[(long long)b * KP + tid];
  }
  __syncthreads();
  od_nms_greedy(lb, lc, lk, n, thr, strict, max_det, keep_flat + (long long)b * max_det, keep_count + b);
}

int next_pow2(int v) {
  int p = 64;
  while (p < v) p <<= 1;
  return p;
}

struct NmsLayout {
  size_t skeys, sbox, scls, mask, total;
};
NmsLayout nms_layout(int B, int KP) {
  NmsLayout l;
  size_t o = 0;
  l.skeys = o;
  o += (size_t)B * KP * 8;
  l.sbox = o;
  o += (size_t)B * KP * 16;
  l.scls = o;
  o += (size_t)B * KP * 4;
  l.mask = o;
  o += (size_t)B * KP * (KP / 64) * 8;
  l.total = o;
  return l;
}

}  // namespace

void od_nms_sorted_buffers(void* nms_workspace, int B, int K, unsigned long long** skeys, f32x4** sbox, int** scls, int* KP) {
  const int kp = next_pow2(K);
  const NmsLayout l = nms_layout(B, kp);
  char* ws = (char*)nms_workspace;
  *skeys = (unsigned long long*)(ws + l.skeys);
  *sbox = (f32x4*)(ws + l.sbox);
  *scls = (int*)(ws + l.scls);
  *KP = kp;
}

float* od_nms_scratch(void* nms_workspace, int B, int K) {
  return (float*)((char*)nms_workspace + nms_layout(B, next_pow2(K)).mask);
}

int od_nms_sort_launch(void* nms_workspace, const float* boxes, const unsigned long long* keys, const int32_t* counts, int B, int P,
                       int NC, int K, hipStream_t s) {
  const int KP = next_pow2(K);
  const NmsLayout l = nms_layout(B, KP);
  char* ws = (char*)nms_workspace;
  hipLaunchKernelGGL(od_nms_sort, dim3(B), dim3(1024), 0, s, boxes, (const u64*)keys, counts, P, NC, K, KP, (u64*)(ws + l.skeys),
                     (f32x4*)(ws + l.sbox), (int*)(ws + l.scls));
  OD_CHECK_LAUNCH();
  return OD_OK;
}

int od_nms_greedy_launch(void* nms_workspace, const int32_t* counts, int B, int K, float iou_threshold, int strict, int max_det,
                         int32_t* keep_flat, int32_t* keep_count, hipStream_t s) {
  const int KP = next_pow2(K);
  const NmsLayout l = nms_layout(B, KP);
  char* ws = (char*)nms_workspace;
  hipLaunchKernelGGL(od_nms_greedy_k, dim3(B), dim3(1024), (size_t)KP * 28, s, (const u64*)(ws + l.skeys),
                     (const f32x4*)(ws + l.sbox), (const int*)(ws + l.scls), counts, KP, iou_threshold, strict, max_det, keep_flat,
                     keep_count);
  OD_CHECK_LAUNCH();
  return OD_OK;
}

extern "C" size_t od_nms_workspace_bytes(int B, int K) {
  if (B <= 0 || K <= 0 || K > 1024) return 0;
  return nms_layout(B, next_pow2(K)).total;
}

extern "C" int od_nms(od_ctx* ctx, const float* boxes, const uint64_t* keys, const int32_t* counts, int B, int P, int NC,
                      int K, float iou_threshold, int strict, int max_det, int32_t* keep_flat, int32_t* keep_count,
                      void* workspace, size_t workspace_bytes, void* stream) {
  OD_REQUIRE(ctx && boxes && keys && counts && keep_flat && keep_count && workspace, "od_nms: null argument");
  OD_REQUIRE(B > 0 && B <= 65535 && P > 0 && NC > 0 && K > 0 && K <= 1024 && max_det > 0,
             "od_nms: bad dims (K <= 1024)");
  const int KP = next_pow2(K);
  const NmsLayout l = nms_layout(B, KP);
  if (workspace_bytes < l.total) {
    od_set_error("od_nms: workspace %zu < %zu bytes", workspace_bytes, l.total);
    return OD_ERR_WORKSPACE;
  }
  hipStream_t s = (hipStream_t)stream;
  if (int rc = od_nms_sort_launch(workspace, boxes, (const unsigned long long*)keys, counts, B, P, NC, K, s)) return rc;
  return od_nms_greedy_launch(workspace, counts, B, K, iou_threshold, strict, max_det, keep_flat, keep_count, s);
}
