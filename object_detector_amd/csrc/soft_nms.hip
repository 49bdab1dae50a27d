// Soft-NMS (Bodla et al. 2017): the suppression stage with linear / Gaussian score decay instead of deletion.  DESIGN.md
// "Soft-NMS" freezes the semantics; tests/soft_nms_ref.py is their numpy restatement and tests/test_gpu_soft_nms.py
// compares the two bit for bit.
//
// od_soft_scan_k: one workgroup per image on the rank-ordered keys / boxes / classes a sort (od_nms_sort), refine
// (od_detect_refine_sort and its streamed form) or merge-rank kernel (od_merge_rank, merge.hip) left in the NMS
// workspace: the candidates go to LDS, then od_soft_nms_scan (topk_common.h) -- every thread keeps its candidate's box, class
// and running score in registers; a round is one 64-bit argmax (DPP steps in the wave + one LDS slot per wave, one barrier) and
// one rescoring pass against the winner.  Latency-bound: up to max_det rounds, each a few hundred cycles.
//   od_soft_nms      = od_nms's sort launch + the scan
//   od_detect_soft   = od_detect_candidates' launches + the scan
//   od_tta_merge_soft / od_slice_merge_soft (merge.hip) = the rank kernel + the scan + the vote-and-gather kernel
// Compiled with -ffp-contract=off: the IoU terms, the decay and od_exp_neg are one rounding per op, as numpy's.
#include "post_common.h"

namespace {

// threads of the scan x candidates per thread: 512 x 2 measured fastest of 1024 x 1, 512 x 2, 256 x 4 and 64 x 16 (one wave, no
// barrier) on the worst-case list (DESIGN.md "Soft-NMS")
constexpr int SOFT_NT = 512, SOFT_CPL = 2;

// Dynamic LDS: boxes [KP] | keys [KP] | classes [KP].
__global__ __launch_bounds__(SOFT_NT) void od_soft_scan_k(const u64* __restrict__ skeys, const f32x4* __restrict__ sbox,
                                                          const int* __restrict__ scls, const int* __restrict__ counts, int KP,
                                                          const od_soft_nms_cfg cfg, int* __restrict__ keep_flat,
                                                          float* __restrict__ keep_conf, int* __restrict__ keep_count,
                                                          float* __restrict__ det) {
  extern __shared__ __attribute__((aligned(16))) char sm[];
  f32x4* lb = (f32x4*)sm;     // [KP]
  u64* lk = (u64*)(lb + KP);  // [KP]
  int* lc = (int*)(lk + KP);  // [KP]
  const int b = blockIdx.x, tid = threadIdx.x;
  const int n = min(max(counts[b], 0), KP);
  for (int i = tid; i < n; i += SOFT_NT) {
    lb[i] = sbox[(long long)b * KP + i];
    lk[i] = skeys[(long long)b * KP + i];
    lc[i] = scls[(long long)b * KP + i];
  }
  __syncthreads();
  od_soft_nms_scan<SOFT_NT, SOFT_CPL>(lb, lc, lk, n, cfg, keep_flat + (long long)b * cfg.max_det, keep_conf + (long long)b * cfg.max_det,
                               keep_count + b, det ? det + (size_t)b * (1 + 6 * (size_t)cfg.max_det) : nullptr);
}

}  // namespace

int od_soft_cfg_check(const char* who, const od_soft_nms_cfg* cfg, int K) {
  OD_REQUIRE(cfg, "%s: null cfg", who);
  OD_REQUIRE(cfg->method >= 0 && cfg->method <= 2, "%s: method = %d outside 0 (hard), 1 (linear), 2 (gaussian)", who, cfg->method);
  OD_REQUIRE(cfg->method != 2 || cfg->sigma > 0.f, "%s: the gaussian method needs sigma > 0", who);
  OD_REQUIRE(cfg->min_conf >= 1e-6f, "%s: min_conf must be >= 1e-6", who);
  OD_REQUIRE(K > 0 && K <= OD_MERGE_MAX_K, "%s: bad dims (K <= %d)", who, OD_MERGE_MAX_K);
  OD_REQUIRE(cfg->max_det > 0, "%s: max_det must be > 0", who);
  return OD_OK;
}

int od_soft_scan_launch(void* nms_workspace, const int32_t* counts, int B, int K, const od_soft_nms_cfg& cfg, int32_t* keep_flat,
                        float* keep_conf, int32_t* keep_count, float* det, hipStream_t s) {
  u64* skeys;
  f32x4* sbox;
  int* scls;
  int KP;
  od_nms_sorted_buffers(nms_workspace, B, K, &skeys, &sbox, &scls, &KP);
  hipLaunchKernelGGL(od_soft_scan_k, dim3(B), dim3(SOFT_NT), (size_t)KP * 28, s, (const u64*)skeys, (const f32x4*)sbox,
                     (const int*)scls, counts, KP, cfg, keep_flat, keep_conf, keep_count, det);
  OD_CHECK_LAUNCH();
  return OD_OK;
}

extern "C" int od_soft_nms(od_ctx* ctx, const float* boxes, const uint64_t* keys, const int32_t* counts, int B, int P, int NC,
                           int K, const od_soft_nms_cfg* cfg, int32_t* keep_flat, float* keep_conf, int32_t* keep_count,
                           float* det, void* workspace, size_t workspace_bytes, void* stream) {
  OD_REQUIRE(ctx && boxes && keys && counts && keep_flat && keep_conf && keep_count && workspace, "od_soft_nms: null argument");
  if (int rc = od_soft_cfg_check("od_soft_nms", cfg, K)) return rc;
  OD_REQUIRE(B > 0 && B <= 65535 && P > 0 && NC > 0, "od_soft_nms: bad dims (K <= 1024)");
  const size_t need = od_nms_workspace_bytes(B, K);
  if (workspace_bytes < need) {
    od_set_error("od_soft_nms: workspace %zu < %zu bytes", workspace_bytes, need);
    return OD_ERR_WORKSPACE;
  }
  hipStream_t s = (hipStream_t)stream;
  if (int rc = od_nms_sort_launch(workspace, boxes, (const unsigned long long*)keys, counts, B, P, NC, K, s)) return rc;
  return od_soft_scan_launch(workspace, counts, B, K, *cfg, keep_flat, keep_conf, keep_count, det, s);
}

extern "C" int od_detect_soft(od_ctx* ctx, const float* pred, const float* priors, int B, int P, int NC, float loc_scale, int clip,
                              float conf_threshold, int K, const od_soft_nms_cfg* cfg, float* boxes, float* conf, uint64_t* keys,
                              int32_t* counts, int32_t* keep_flat, float* keep_conf, int32_t* keep_count, float* det,
                              void* workspace, size_t workspace_bytes, void* nms_workspace, size_t nms_workspace_bytes,
                              void* stream) {
  OD_REQUIRE(keep_flat && keep_conf && keep_count, "od_detect_soft: null argument");
  if (int rc = od_soft_cfg_check("od_detect_soft", cfg, K)) return rc;
  if (int rc = od_detect_candidates(ctx, pred, priors, B, P, NC, loc_scale, clip, conf_threshold, K, boxes, conf, keys, counts,
                                    workspace, workspace_bytes, nms_workspace, nms_workspace_bytes, stream))
    return rc;
  return od_soft_scan_launch(nms_workspace, counts, B, K, *cfg, keep_flat, keep_conf, keep_count, det, (hipStream_t)stream);
}
