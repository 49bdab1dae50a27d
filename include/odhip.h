/*
 * odhip.h — C ABI of libodhip.so, the MI355X (gfx950) drop-in for the hot path of
 * ak110/object_detector (Darknet53 backbone + multi-scale prior-box head -> decode -> per-class NMS,
 * plus prior-box assignment / loss for training).
 *
 * The reference has NO FFI for this path: everything below `ObjectDetector.predict`
 * (reference voc_validate.py:27, voc_evaluate.py:27) and `od.pb.encode_truth / decode_locs`
 * (reference check_assign.py:21,27) lives in the un-vendored `pytoolkit` submodule.
 * The entry points here are therefore BUILD-DEFINED; each one names the reference call site whose
 * device work it replaces.  INTEGRATION.md shows the ctypes binding a pytoolkit maintainer would add.
 *
 * Conventions
 *   - every function returns 0 on success, a negative OD_ERR_* otherwise; od_last_error() gives text
 *   - all tensor arguments are raw DEVICE pointers + explicit dims; `stream` is a hipStream_t passed as void*
 *   - no hidden allocation in any per-step call: the caller owns every buffer, including workspaces whose
 *     size is returned by the matching *_workspace_bytes() query.  od_ctx owns only an 8 KiB zero page and an 8 KiB
 *     vector of ones (allocated once in od_ctx_create).
 *   - kernels are asynchronous on `stream`; launch errors are mapped to return codes right after launch
 *   - activations are NHWC; f16 storage, f32 accumulation (MFMA v_mfma_f32_16x16x32_f16)
 */
#ifndef ODHIP_H
#define ODHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OD_OK 0
#define OD_ERR_INVALID (-1)   /* bad argument / unsupported shape */
#define OD_ERR_HIP (-2)       /* HIP runtime error (text in od_last_error) */
#define OD_ERR_WORKSPACE (-3) /* workspace too small */
#define OD_ERR_COMM (-4)      /* RCCL error */

/* activation enum of the fused conv epilogue (backbone leaky(0.1), neck/head ELU) */
#define OD_ACT_LINEAR 0
#define OD_ACT_LEAKY 1
#define OD_ACT_ELU 2

#define OD_RES_NONE 0
#define OD_RES_SAME 1 /* residual tensor has the output's shape: Darknet53 shortcut */
#define OD_RES_UP2 2  /* residual tensor is [B,Ho/2,Wo/2,Cout], nearest-upsampled 2x: FPN top-down add */

#define OD_DT_F16 0
#define OD_DT_F32 1
#define OD_DT_BF16 2 /* od_allreduce payload only */

typedef struct od_ctx od_ctx;

const char* od_last_error(void);
int od_version(void);

int od_ctx_create(int device, od_ctx** out);
int od_ctx_destroy(od_ctx* ctx);

/* ABI self-description, so that a foreign-language binding (ctypes, cgo, JNI ...) can verify its mirror of the structs
 * below against THIS build of the library instead of against a copy of the header: size in bytes of a struct of this
 * header by name ("od_conv_desc", ...), and the byte offset of one of its fields ("od_conv_desc", "tile_cfg").
 * -1 = unknown struct / field.  od_struct_fields writes the comma-separated field names of a struct, in declaration
 * order, into buf (returns the number of fields, -1 unknown struct or buffer too small). */
long od_sizeof(const char* struct_name);
long od_offsetof(const char* struct_name, const char* field_name);
int od_struct_fields(const char* struct_name, char* buf, int buf_bytes);

/* ------------------------------------------------------------------------------------------------
 * K1/K2: fused conv2d forward.  Replaces the Keras Conv2D+BatchNormalization+activation(+Add) layers
 * that `ObjectDetector.predict` executes (reference voc_validate.py:27; network per docs/MODEL.md:5-21).
 * out = act(scale[c] * conv(x, w)[c] + bias[c]) (+ residual), 'same' padding (ksize/2).
 *   x      f16 [B,H,W,Cin] NHWC, Cin % 8 == 0
 *   w      f16 packed [Cout_pad][Kpad], k = (dy*ksize+dx)*Cin + cin, zero padded
 *          (dims from od_conv_weight_dims; rows beyond Cout and k beyond ksize*ksize*Cin are zero)
 *   scale, bias  f32 [Cout_pad]  (inference: BatchNorm folded; training fwd: identity/conv bias)
 *   res    f16 residual or NULL (res_mode)
 *   out    f16 or f32; element (b, ho, wo, c) is written at
 *          out[b*out_batch_stride + (ho*Wo+wo)*out_pix_stride + c]  (0 strides = dense NHWC)
 * ---------------------------------------------------------------------------------------------- */
typedef struct od_conv_desc {
  const void* x;
  const void* w;
  const float* scale;
  const float* bias;
  const void* res;
  void* out;
  int32_t B, H, W, Cin, Cout;
  int32_t ksize;  /* 1 or 3 */
  int32_t stride; /* 1 or 2 */
  int32_t act;    /* OD_ACT_* */
  float alpha;    /* leaky slope / ELU alpha */
  int32_t res_mode;
  int32_t out_dtype; /* OD_DT_* */
  int64_t out_batch_stride;
  int64_t out_pix_stride;
  int32_t tile_cfg; /* -1 = auto (fastest launch on an idle chip); -2 = auto for launches that overlap other work (batches
                       in flight): least CU x time; otherwise index into the tile-config table (od_conv_num_tile_cfgs) */
  int32_t transposed; /* != 0: backward-data of a 3x3 stride-2 conv: x is [B,H,W,Cin] = dZ, out is [B,2H,2W,Cout];
                         w must be the flipped / channel-swapped pack written by od_pack_weights */
  int32_t splitk;     /* split-K factor for small-M layers: 0 = library decides, 1 = off; needs splitk_workspace */
  void* splitk_workspace; /* f32 scratch for the partial slabs [splitk][B*Ho*Wo*Cout] (NULL = never split) */
  int64_t splitk_workspace_bytes; /* its size; the factor is clamped so that the slabs fit */
  float* bn_partials; /* training forward (NULL otherwise): the epilogue also writes per-channel partial sums of the f16
                         values it stores, one row per m-tile: f32 [rows][2][Cout] = (sum z, sum z^2), rows =
                         od_conv2d_fwd_bn_rows(); od_bn_stats_from_partials turns them into the batch statistics, so the
                         separate pass of od_bn_stats over z is not needed.  Needs out_dtype f16; disables split-K */
  int64_t bn_partials_bytes;
  /* optional (w2 == NULL: none): the pointwise (1x1, stride 1) layer that consumes this launch's output, e.g. the first
   * conv of the next residual block:   out2 = act2(scale2 * conv1x1(out, w2) + bias2),  f16 dense [B,Ho,Wo,Cout2].
   * `out` is written as usual (f16, dense, no transposed / bn_partials).  When the selected kernel holds all channels of
   * a pixel in one workgroup (8-wave kernel, Cout == 256, Cout2 == 128) the second layer runs in its epilogue on the
   * rounded f16 rows -- one launch, `out` is not read back; otherwise the library issues the 1x1 as a second launch on
   * the same stream.  Same rounding points either way.  w2 is packed like w (od_conv_weight_dims(Cout2, Cout, 1)). */
  const void* w2;
  const float* scale2;
  const float* bias2;
  void* out2;
  int32_t Cout2;
  int32_t act2;
  float alpha2;
  int32_t pad2_;
  /* optional (nseg <= 1: none): GROUPED launch -- the same layer (w, scale, bias, activation, B, Cin, Cout, 3x3, stride 1,
   * out_dtype / out_batch_stride / out_pix_stride) applied to nseg <= 3 input maps of different sizes, the prediction
   * module whose weights the pyramid levels share (reference docs/MODEL.md:8): segment i reads seg_x[i] f16
   * [B, seg_H[i], seg_W[i], Cin] and writes seg_out[i]; x / out / H / W are ignored.  No residual, w2, bn_partials or
   * transposed mode.  One launch when the 8-wave kernel takes the layer (every m-tile lies inside one segment), otherwise
   * the library issues the nseg launches itself -- identical results either way. */
  int32_t nseg;
  int32_t pad3_;
  const void* seg_x[3];
  void* seg_out[3];
  int32_t seg_H[3];
  int32_t seg_W[3];
} od_conv_desc;

int od_conv_weight_dims(int cout, int cin, int ksize, int* cout_pad, int* kpad);
int od_conv_num_tile_cfgs(void);
int od_conv2d_fwd(od_ctx* ctx, const od_conv_desc* d, void* stream);
/* number of partial rows a launch of this descriptor writes into bn_partials (depends on the tile the library picks);
 * <= 0 on error */
int od_conv2d_fwd_bn_rows(od_ctx* ctx, const od_conv_desc* d);

/* K1+K2 fused residual block of the early Darknet53 stages (one launch instead of two layers + add):
 *   out = x + act(scale3 * conv3x3(act(scale1 * conv1x1(x) + bias1)) + bias3)
 * x, out f16 [B,H,W,C]; the middle tensor has C/2 channels and never leaves the CU.  w1 / w3 are the packed weights
 * of the 1x1 (C -> C/2) and 3x3 (C/2 -> C) convolutions exactly as od_conv2d_fwd takes them.  Supported: C in {64, 128},
 * H and W multiples of 16 (od_bottleneck_supported); everything else runs as two od_conv2d_fwd calls.
 * Replaces the same Keras layers as od_conv2d_fwd (reference voc_validate.py:27; docs/MODEL.md:15-17). */
typedef struct od_bneck_desc {
  const void* x;
  const void* w1;
  const float* scale1;
  const float* bias1;
  const void* w3;
  const float* scale3;
  const float* bias3;
  void* out;
  int32_t B, H, W, C;
  int32_t act; /* OD_ACT_*, both convolutions */
  float alpha;
} od_bneck_desc;
int od_bottleneck_supported(int H, int W, int C);
int od_bottleneck_fwd(od_ctx* ctx, const od_bneck_desc* d, void* stream);

/* K3+K1 fused stem: the first two Darknet53 layers (uint8 image -> 3x3 conv 3->32 -> 3x3 stride-2 conv 32->64, each with
 * folded BatchNorm + activation) in one launch; the 32-channel full-resolution tensor stays on chip.
 *   x u8 [B,H,W,3]; w0 f16 [32][32] as od_conv_first_fwd takes it; w3 = packed weights of the stride-2 conv as
 *   od_conv2d_fwd takes them; out f16 [B,H/2,W/2,64].  H and W multiples of 32 (od_stem_supported).
 * Replaces the preprocess + first two Conv2D layers of predict (reference voc_validate.py:27; docs/MODEL.md:15-17). */
typedef struct od_stem_desc {
  const uint8_t* x;
  const void* w0;
  const float* scale0;
  const float* bias0;
  const void* w3;
  const float* scale3;
  const float* bias3;
  void* out;
  int32_t B, H, W;
  int32_t act; /* OD_ACT_*, both convolutions */
  float alpha;
} od_stem_desc;
int od_stem_supported(int H, int W);
int od_stem_fwd(od_ctx* ctx, const od_stem_desc* d, void* stream);

/* K3: first layer, uint8 RGB image in, 3x3 stride-1 conv 3->Cout (Cout = 32), input normalisation folded
 * into scale.  x u8 [B,H,W,3]; w f16 packed [Cout][32] (k = (dy*3+dx)*3 + c, k >= 27 zero);
 * out f16 [B,H,W,Cout].  Replaces the image preprocess + first Conv2D of predict (voc_validate.py:27). */
int od_conv_first_fwd(od_ctx* ctx, const uint8_t* x, const void* w, const float* scale, const float* bias,
                      void* out, int B, int H, int W, int Cout, int act, float alpha, void* stream);

/* K4 (standalone form; the planner fuses it into the lateral conv via OD_RES_UP2):
 * out[b,y,x,c] = a[b,y,x,c] + up[b,y/2,x/2,c], all f16 NHWC.  docs/MODEL.md:7 "FPN-like" top-down path. */
int od_upsample2x_add(od_ctx* ctx, const void* a, const void* up, void* out, int B, int H, int W, int C,
                      void* stream);

/* ------------------------------------------------------------------------------------------------
 * K5+K6: head post-process.  pred f32 [B,P,2+NC+4] (col 0/1 = not-object/object logits, 2..2+NC class logits,
 * last 4 = corner-form box offsets: reference check_assign.py:25-27 layout).
 *   conf[b,p,c]  = softmax2(pred[b,p,0:2])[1] * softmax(pred[b,p,2:2+NC])[c]      (docs/MODEL.md:54-58)
 *   boxes[b,p,:] = clip01(priors[p] + loc * loc_scale * [pw,ph,pw,ph])              (od.pb.decode_locs)
 * priors f32 [P,4] corner form, normalised image coordinates.  1 <= NC <= 1024.
 * ---------------------------------------------------------------------------------------------- */
int od_head_postprocess(od_ctx* ctx, const float* pred, const float* priors, float* conf, float* boxes,
                        int B, int P, int NC, float loc_scale, int clip, void* stream);

/* K6 alone: od.pb.decode_locs(locs) (reference check_assign.py:27): zero offsets decode to the priors. */
int od_decode_locs(od_ctx* ctx, const float* locs, const float* priors, float* boxes, int N, int P,
                   float loc_scale, int clip, void* stream);

/* K7: per image, the K candidates with the largest (conf desc, flat index asc) among conf > conf_threshold,
 * flat index = p*NC + c.  keys u64 [B,K] = (float_bits(conf) << 32) | (0xFFFFFFFF - flat), unsorted,
 * unused slots 0; counts i32 [B].  Exact radix select: no ties, no approximation. */
size_t od_topk_workspace_bytes(int B, int N, int K);
int od_topk_scores(od_ctx* ctx, const float* conf, int B, int N, int K, float conf_threshold,
                   uint64_t* keys, int32_t* counts, void* workspace, size_t workspace_bytes, void* stream);

/* K8: sort the K keys (bitonic), class-aware greedy NMS with a 64-bit wavefront suppression bitmask
 * (docs/MODEL.md:78-82).  A candidate is suppressed by a kept higher-ranked candidate of the SAME class when
 * inter > iou_threshold * (area_a + area_b - inter), all f32, no FMA contraction.
 *   boxes f32 [B,P,4]; keys u64 [B,K]; counts i32 [B]
 *   keep_flat i32 [B,max_det] (flat index p*NC+c in rank order, -1 padded); keep_count i32 [B]
 *   strict != 0: suppression ignores the class (strict_nms kwarg, voc_validate.py:26; BUILD-DEFINED). K <= 1024. */
size_t od_nms_workspace_bytes(int B, int K);
int od_nms(od_ctx* ctx, const float* boxes, const uint64_t* keys, const int32_t* counts, int B, int P, int NC,
           int K, float iou_threshold, int strict, int max_det, int32_t* keep_flat, int32_t* keep_count,
           void* workspace, size_t workspace_bytes, void* stream);

/* The kept detections of a batch as ONE dense record block, so that `predict` copies a single buffer back per batch
 * (reference voc_validate.py:27 returns per-image classes / confs / bboxes):
 *   out f32 [B][1 + 6*max_det]: out[b][0] = keep_count[b] (int bits); row r = out[b][1 + 6r ...] =
 *   {flat index p*NC+c (int bits; -1 beyond the count), conf[b][flat], boxes[b][p][0..3]} in rank order. */
int od_gather_detections(od_ctx* ctx, const float* conf, const float* boxes, const int32_t* keep_flat,
                         const int32_t* keep_count, int B, int P, int NC, int max_det, float* out, void* stream);

/* K5-K8 as ONE call, the path `predict` runs (reference voc_validate.py:27; docs/MODEL.md:54-58,78-82): pred -> decoded boxes,
 * the exact top-K key set, class-aware NMS kept indices -- three launches (four for NC > 76), the confidence tensor is never materialised
 * (one pass over pred computes the confidences on chip, their first-digit histogram and one max per prior; the second pass
 * recomputes only the priors that can hold a top-K candidate).  Results are bit-identical to od_head_postprocess ->
 * od_topk_scores -> od_nms on the same pred (keys come back SORTED descending here, unused slots 0).
 *   conf: optional dense f32 [B,P,NC] output (NULL in the product path);  workspace: od_detect_workspace_bytes, zeroed once
 *   with od_detect_workspace_init (every call leaves it ready for the next);  nms_workspace: od_nms_workspace_bytes(B, K).
 *   P even, 1 <= NC <= 1024, K <= 1024.  NC <= 76 holds 256 whole rows in LDS; larger class counts stream the class columns
 *   (same results) and use a workspace of O(B*P) bytes instead of O(B*P*NC). */
size_t od_detect_workspace_bytes(int B, int P, int NC, int K);
int od_detect_workspace_init(od_ctx* ctx, void* workspace, size_t workspace_bytes, int B, int P, int NC, void* stream);
int od_detect(od_ctx* ctx, const float* pred, const float* priors, int B, int P, int NC, float loc_scale, int clip,
              float conf_threshold, int K, float iou_threshold, int strict, int max_det, float* boxes, float* conf,
              uint64_t* keys, int32_t* counts, int32_t* keep_flat, int32_t* keep_count, void* workspace,
              size_t workspace_bytes, void* nms_workspace, size_t nms_workspace_bytes, void* stream);
/* od_gather_detections without a confidence tensor: the kept detections' confidences are recomputed from pred (same code,
 * same bits). */
int od_gather_detections_pred(od_ctx* ctx, const float* pred, const float* boxes, const int32_t* keep_flat,
                              const int32_t* keep_count, int B, int P, int NC, int max_det, float* out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Test-time augmentation (BUILD-DEFINED; DESIGN.md "Flip test-time augmentation"): several views of a batch are run
 * through the network, each view's top-K candidates are taken with od_detect_candidates, and od_tta_merge merges the
 * lists, runs ONE NMS over the merged list and refines the kept boxes by confidence-weighted box voting.
 * ---------------------------------------------------------------------------------------------- */

/* dst[b,y,x,:] = src[b,y,W-1-x,:] for uint8 NHWC [B,H,W,3].  src and dst must not overlap. */
int od_hflip_u8(od_ctx* ctx, const uint8_t* src, uint8_t* dst, int B, int H, int W, void* stream);

/* od_detect without the NMS: pred -> boxes [B,P,4], SORTED keys [B,K] (unused slots 0) and counts [B], bit-identical
 * to what od_detect returns for the same pred, by the same kernels (both dispatches: NC <= 76 and the streamed ones above).
 * Same workspace as od_detect (left ready for the next call of either).  nms_workspace (od_nms_workspace_bytes(B, K)) receives
 * the rank-ordered keys / boxes / classes the sort kernel gathers, as in od_detect; nothing else in it is touched. */
int od_detect_candidates(od_ctx* ctx, const float* pred, const float* priors, int B, int P, int NC, float loc_scale, int clip,
                         float conf_threshold, int K, float* boxes, float* conf, uint64_t* keys, int32_t* counts,
                         void* workspace, size_t workspace_bytes, void* nms_workspace, size_t nms_workspace_bytes,
                         void* stream);

/* One view of od_tta_merge: the keys / counts / boxes od_detect_candidates (or od_detect) produced for it with the same NC and
 * K, its prior count, and whether its input was mirrored left-to-right. */
typedef struct od_tta_view {
  const uint64_t* keys;  /* u64 [B,K], sorted descending */
  const int32_t* counts; /* i32 [B] */
  const float* boxes;    /* f32 [B,P,4] */
  int32_t P;
  int32_t flip;
} od_tta_view;

/* Merge V views (1 <= V <= 8, host array `views`; the views may differ in P), all f32, one rounding per op, no contraction:
 *   candidate (v, r), r < counts_v[b]: conf = float(key >> 32), flat = 0xFFFFFFFF - low word, p = flat / NC, c = flat % NC,
 *       box = boxes_v[b][p], mirrored to (1 - x2, y1, 1 - x1, y2) when flip_v
 *   merged order: conf bits desc, view asc, flat asc; the first Km = min(K, sum_v counts_v[b]) are kept
 *   greedy NMS over the merged list by od_nms's rule (same class unless strict, at most max_det kept, rank order)
 *   vote_iou > 0: every kept candidate i takes the box  sum_j conf_j * box_j / sum_j conf_j  over j = i and every merged
 *       candidate j (kept or not) of i's class with inter(i,j) > vote_iou * union(i,j), accumulated in ascending rank j
 *       (multiply and add rounded separately); confidence and rank stay.  vote_iou <= 0: the box stays.
 *   out f32 [B][1 + 6*max_det] in od_gather_detections' layout, word 0 of a row = the CLASS (int bits; -1 beyond the count)
 *   src i32 [B,max_det,2] (may be NULL): (view, flat index in that view) of each kept detection, -1 beyond the count
 *   keep_count i32 [B].  K <= 1024.  workspace: od_tta_merge_workspace_bytes(B, V, K), needs no initialisation. */
size_t od_tta_merge_workspace_bytes(int B, int V, int K);
int od_tta_merge(od_ctx* ctx, const od_tta_view* views, int V, int B, int NC, int K, float iou_threshold, int strict,
                 int max_det, float vote_iou, float* out, int32_t* src, int32_t* keep_count, void* workspace,
                 size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Soft-NMS (Bodla et al. 2017; BUILD-DEFINED, DESIGN.md "Soft-NMS" freezes the semantics): the suppression stage decays the
 * scores of a kept box's neighbours instead of deleting them.  One image's n <= K <= 1024 candidates in rank order (box_j,
 * cls_j, s_j = the f32 in the key's high word), all f32, one rounding per op, no contraction:
 *   while kept < max_det:  i = the live j with the largest s_j (ties: the smaller rank); stop unless s_i > min_conf;
 *     emit i with score s_i and remove it; for every live j with (strict or cls_j == cls_i) and inter(i,j) > 0, inter / uni
 *     as od_nms computes them:   hard:     inter > thr * uni: remove j
 *                                linear:   inter > thr * uni: s_j = s_j * (1 - inter / uni)
 *                                gaussian: iou = inter / uni; s_j = s_j * od_exp_neg((iou * iou) / sigma)
 *   (od_exp_neg: a fixed-order f32 exp(-x)).  Detections come out in SCORE order with the rescored confidence;
 *   method = hard keeps exactly od_nms's indices.
 * ---------------------------------------------------------------------------------------------- */
typedef struct od_soft_nms_cfg {
  int32_t method;      /* 0 hard, 1 linear, 2 gaussian */
  int32_t strict;
  int32_t max_det;
  float iou_threshold;
  float sigma;         /* > 0, gaussian */
  float min_conf;      /* >= 1e-6 */
} od_soft_nms_cfg;

/* The counterpart of od_nms (same boxes / keys / counts, workspace = od_nms_workspace_bytes(B, K)): its sort launch, then
 * the soft scan, one workgroup per image.
 *   keep_flat i32 [B,max_det] in emission order, -1 padded;  keep_conf f32 [B,max_det], 0 padded;  keep_count i32 [B]
 *   det (may be NULL) f32 [B][1 + 6*max_det] in od_gather_detections' layout, conf = the rescored one. */
int od_soft_nms(od_ctx* ctx, const float* boxes, const uint64_t* keys, const int32_t* counts, int B, int P, int NC, int K,
                const od_soft_nms_cfg* cfg, int32_t* keep_flat, float* keep_conf, int32_t* keep_count, float* det,
                void* workspace, size_t workspace_bytes, void* stream);
/* The counterpart of od_detect: od_detect_candidates' launches (either dispatch), then the soft scan on the rank-ordered
 * candidates they leave in the NMS workspace.  Same workspaces as od_detect, left ready for the next call of either. */
int od_detect_soft(od_ctx* ctx, const float* pred, const float* priors, int B, int P, int NC, float loc_scale, int clip,
                   float conf_threshold, int K, const od_soft_nms_cfg* cfg, float* boxes, float* conf, uint64_t* keys,
                   int32_t* counts, int32_t* keep_flat, float* keep_conf, int32_t* keep_count, float* det, void* workspace,
                   size_t workspace_bytes, void* nms_workspace, size_t nms_workspace_bytes, void* stream);
/* od_tta_merge with the soft scan in place of the greedy one: same merged order, same box voting (members weighted by their
 * ORIGINAL confidences); the kept list, its order and the reported confidence are the soft scan's.  Same workspace. */
int od_tta_merge_soft(od_ctx* ctx, const od_tta_view* views, int V, int B, int NC, int K, const od_soft_nms_cfg* cfg,
                      float vote_iou, float* out, int32_t* src, int32_t* keep_count, void* workspace,
                      size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * K9: prior-box assignment + target encoding = od.pb.encode_truth (reference check_assign.py:21,25-27).
 *   priors f32 [P,4]; gt_boxes f32 [B,Gmax,4] corner form, normalised; gt_classes i32 [B,Gmax]; gt_counts i32 [B]
 *   y f32 [B,P,2+NC+4]: col 0 = background, col 1 = assigned ("y[:,1]==1", :25), cols 2..2+NC one-hot class (:26),
 *   last 4 = regression target = inverse of od_decode_locs (:27).  An all-zero row = ignored prior.
 *   assigned_gt i32 [B,P] (may be NULL): GT index, -1 background, -2 ignore;  npos i32 [B] assigned priors per image.
 * od_assign_anchors_ign: the same with ignore regions.  gt_flags i32 [B,Gmax], bit 0 = ignore region (COCO iscrowd, VOC
 *   difficult, a mosaic sliver): such a box owns no prior and is not counted in npos; a prior that would be background
 *   becomes an all-zero "ignore" row (assigned_gt -3) when inter(prior, region) / area(prior) >= ign_thr for any region.
 *   With no flag set the result equals od_assign_anchors bit for bit.  Same workspace.
 * Rule [BUILD-DEFINED]: best GT per prior with IoU >= pos_thr; neg_thr <= IoU < pos_thr ignored; every GT force-takes
 * its best prior (ascending GT index, later wins).  Gmax <= 128.
 * ---------------------------------------------------------------------------------------------- */
size_t od_assign_workspace_bytes(int B, int P, int Gmax);
int od_assign_anchors(od_ctx* ctx, const float* priors, const float* gt_boxes, const int32_t* gt_classes,
                      const int32_t* gt_counts, int B, int P, int Gmax, int NC, float pos_thr, float neg_thr,
                      float loc_scale, float* y, int32_t* assigned_gt, int32_t* npos, void* workspace,
                      size_t workspace_bytes, void* stream);
int od_assign_anchors_ign(od_ctx* ctx, const float* priors, const float* gt_boxes, const int32_t* gt_classes,
                          const int32_t* gt_counts, const int32_t* gt_flags, float ign_thr, int B, int P, int Gmax,
                          int NC, float pos_thr, float neg_thr, float loc_scale, float* y, int32_t* assigned_gt,
                          int32_t* npos, void* workspace, size_t workspace_bytes, void* stream);

/* K9b: the same target rows under the ATSS rule (Zhang et al., CVPR 2020), the opt-in assigner [BUILD-DEFINED; the frozen
 * rule is the header comment of csrc/assign_atss.hip, restated by tests/atss_ref.py].  Per box the candidates are all
 * priors_per_cell priors of the min(topk, gh*gw) cells nearest to the box centre on each of the n_levels pyramid levels; a
 * candidate is positive when its IoU (on a 2^-20 lattice) reaches mean + population std of the candidates' IoUs and its cell
 * centre lies strictly inside the box; a box with no positive force-takes its best candidate; a prior claimed twice goes to
 * a forced claim, then to the larger IoU, then to the lower box index.  No IoU ignore band: assigned_gt is never -2.
 *   priors f32 [P,4] in row order (level, y, x, prior); grid_hw i32 [n_levels,2] = (gh, gw) per level, HOST memory, read
 *   before the call returns; sum gh*gw*priors_per_cell == P; 1 <= n_levels <= 4; 1 <= priors_per_cell <= 8; 1 <= topk <= 32.
 *   gt_flags may be NULL (no ignore regions); otherwise as in od_assign_anchors_ign, with ign_thr > 0.  Gmax <= 128.
 *   workspace: od_assign_atss_workspace_bytes.  Other arguments and outputs as od_assign_anchors. */
size_t od_assign_atss_workspace_bytes(int B, int P, int Gmax);
int od_assign_atss(od_ctx* ctx, const float* priors, const int32_t* grid_hw, int n_levels, int priors_per_cell,
                   const float* gt_boxes, const int32_t* gt_classes, const int32_t* gt_counts, const int32_t* gt_flags,
                   float ign_thr, int topk, int B, int P, int Gmax, int NC, float loc_scale, float* y, int32_t* assigned_gt,
                   int32_t* npos, void* workspace, size_t workspace_bytes, void* stream);

/* K9c: the same target rows under the task-aligned rule (TOOD, Feng et al., ICCV 2021), the prediction-aware opt-in assigner
 * [BUILD-DEFINED; the frozen rule is the header comment of csrc/assign_tal.hip, restated by tests/tal_ref.py].  pred f32
 * [B,P,2+NC+4] are the network's raw outputs of THIS step (16-byte aligned).  Per prior: la = log P(object) from the two
 * objectness logits, lse = log-sum-exp of the class logits, pbox = od_decode_locs of its offsets (no clip, corners sorted).
 * Per unflagged box the candidates are the priors whose cell centre lies strictly inside the box and whose
 * u = IoU(box, pbox) > 0; the box claims the min(topk, #candidates) of the largest
 * l = alpha * (la + z_class - lse) + beta * log u (ties: lower prior index; a class outside 0..NC-1 drops the class term).
 * A box without a candidate force-takes the prior of its largest static IoU > 0.  A prior claimed twice goes to a forced
 * claim, then to the larger IoU (u, or the static one of a forced claim), then to the lower box index.  Targets are hard
 * (objectness 1, one-hot class), rows / ignore regions / assigned_gt / npos exactly as od_assign_atss.
 *   alpha, beta finite and > 0 (TOOD: 1, 6); 1 <= topk <= 32 (TOOD: 13); 1 <= NC <= 1024; grid_hw, n_levels,
 *   priors_per_cell, gt_flags, ign_thr, Gmax as od_assign_atss.
 *   metric f32 [B,P] (may be NULL): l of the winning normal claim; 0 for background, ignored and forced rows.
 *   workspace: od_assign_tal_workspace_bytes = 32 bytes per prior of the batch (16-byte aligned); it does not grow with Gmax. */
size_t od_assign_tal_workspace_bytes(int B, int P, int Gmax);
int od_assign_tal(od_ctx* ctx, const float* priors, const int32_t* grid_hw, int n_levels, int priors_per_cell,
                  const float* pred, const float* gt_boxes, const int32_t* gt_classes, const int32_t* gt_counts,
                  const int32_t* gt_flags, float ign_thr, float alpha, float beta, int topk, int B, int P, int Gmax, int NC,
                  float loc_scale, float* y, int32_t* assigned_gt, int32_t* npos, float* metric, void* workspace,
                  size_t workspace_bytes, void* stream);

/* K10: loss forward + gradient (reference docs/MODEL.md:33-52): focal(objectness, 2-class softmax) +
 * softmax-CE(classes, assigned priors) + box loss (box_mode 0 smooth-L1 / 1 MSE, assigned priors), each weighted and
 * divided by max(1, #assigned).  pred, y, grad f32 [B,P,2+NC+4]; losses f32 [4] = obj, cls, box, total.  1 <= NC <= 1024. */
size_t od_loss_workspace_bytes(int B, int P);
int od_loss_fwd_bwd(od_ctx* ctx, const float* pred, const float* y, float* grad, float* losses, int B, int P, int NC,
                    float focal_alpha, float focal_gamma, int box_mode, float w_obj, float w_cls, float w_box,
                    void* workspace, size_t workspace_bytes, void* stream);
/* The same with an IoU-family box loss: box_mode 2 = giou, 3 = diou, 4 = ciou is 1 - GIoU / DIoU / CIoU between the DECODED
 * predicted and target boxes of every assigned prior (decode = od_decode_locs without clip, prior of row r = priors[r % P],
 * priors f32 [P,4], 16-byte aligned), in the same single pass over pred / y.  A predicted box with crossed corners is sorted
 * first (GIoU paper, Algorithm 2); eps = 1e-9 keeps every denominator positive for a zero-size predicted box; CIoU's alpha
 * is a constant in the gradient.  box_mode 0 / 1: priors may be NULL, loc_scale is not read, and the result is
 * od_loss_fwd_bwd's bit for bit.  Same workspace (od_loss_workspace_bytes). */
int od_loss_fwd_bwd_iou(od_ctx* ctx, const float* pred, const float* y, const float* priors, float* grad, float* losses,
                        int B, int P, int NC, float focal_alpha, float focal_gamma, int box_mode, float loc_scale,
                        float w_obj, float w_cls, float w_box, void* workspace, size_t workspace_bytes, void* stream);
/* The same with a quality-aware objectness term [BUILD-DEFINED, opt-in]: quality f32 [B,P] holds q in [0,1] per prior (clamped
 * on read, NaN = 0; read on assigned rows only; a constant in the gradient).  z = l1 - l0, p = sigmoid(z),
 * CE = q * log(1 + e^-z) + (1 - q) * log(1 + e^z), a = focal_alpha on assigned rows:
 *   obj_mode 0 (focal): quality is not read (may be NULL); the result is od_loss_fwd_bwd_iou's bit for bit.
 *   obj_mode 1 (quality focal loss, Li et al. 2020; TOOD's classification loss): L = a * |q - p|^gamma * CE, focal_gamma >= 1.
 *   obj_mode 2 (varifocal loss, Zhang et al. 2021): assigned rows with q > 0 take L = q * CE; assigned rows with q == 0 take
 *     focal's background term, (1 - focal_alpha) included.
 * Background rows take focal's background term in every mode, bit for bit; ignore rows add nothing; class and box terms, the
 * normaliser max(1, #assigned), the workspace and the non-finite rule (a NaN / Inf objectness logit of a non-ignored row makes
 * its gradient and losses[3] non-finite) are od_loss_fwd_bwd_iou's. */
int od_loss_fwd_bwd_quality(od_ctx* ctx, const float* pred, const float* y, const float* priors, float* grad, float* losses,
                            int B, int P, int NC, float focal_alpha, float focal_gamma, int box_mode, float loc_scale,
                            float w_obj, float w_cls, float w_box, const float* quality, int obj_mode, void* workspace,
                            size_t workspace_bytes, void* stream);

/* K10b: quality targets for od_loss_fwd_bwd_quality (csrc/quality.hip; the frozen rules are its header comment, restated by
 * tests/quality_ref.py).  q f32 [B,P]: one number in [0,1] per assigned prior (y[..., 1] > 0.5), 0 on every other row.
 * pbox = od_decode_locs of the row's predicted offsets (no clip, corners sorted; a non-finite coordinate gives IoU 0).
 * pred, priors 16-byte aligned; 1 <= NC <= 1024.
 *   od_quality_iou: q = IoU(decoded target box of the row, pbox).  Works behind any assigner and on a ready-made target.
 *   od_quality_tal: TOOD's normalised alignment metric, behind od_assign_tal (its gt_boxes [B,Gmax,4], assigned_gt [B,P] and
 *     metric [B,P]).  u = IoU(gt box of the row's object, pbox).  A row is aligned iff metric < 0; per object lmax / umax are
 *     the maxima of metric / u over its aligned rows; aligned rows get q = exp(metric - lmax) * umax, forced rows (metric = 0)
 *     q = max(u, IoU(gt box, prior)).  An assigned row whose assigned_gt lies outside 0..Gmax-1 reads no box and gets q = 0;
 *     od_assign_tal never writes one (its owners are box indices below min(gt_counts, Gmax)), so this only guards buffers
 *     from elsewhere.  Order-independent: two calls give the same bytes.  The workspace
 *     (od_quality_tal_workspace_bytes = 8 bytes per (image, box slot), 4-byte aligned) may arrive dirty. */
int od_quality_iou(od_ctx* ctx, const float* pred, const float* y, const float* priors, float loc_scale, int B, int P, int NC,
                   float* q, void* stream);
size_t od_quality_tal_workspace_bytes(int B, int Gmax);
int od_quality_tal(od_ctx* ctx, const float* pred, const float* y, const float* priors, float loc_scale, const float* gt_boxes,
                   const int32_t* assigned_gt, const float* metric, int B, int P, int Gmax, int NC, float* q, void* workspace,
                   size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * K11/K12: training-side kernels (the Keras fit() machinery behind tk.dl.od.ObjectDetector: Conv2D backward,
 * BatchNormalization in training mode, activation backward, SGD with per-layer LR multipliers -- docs/MODEL.md:19-21,
 * 84-90).  Activations / gradients f16 NHWC (gradients loss-scaled), statistics and parameters f32.
 *   backward-data  = od_conv2d_fwd on dZ with the w_bwd pack of od_pack_weights (stride 1), or with
 *                    od_conv_desc.transposed = 1 (stride 2); the epilogue's residual input accumulates gradients
 *   backward-weight= od_conv2d_bwd_weight: dw f32 [Cout][k*k*Cin] (dense, the layout of the f32 master weights)
 *                    += dZ^T . shifted(X)   (atomic f32 adds; zero it first)
 * ---------------------------------------------------------------------------------------------- */
/* backward-data as ONE call (SURVEY.md §8b names it as an export): dx[B, Ho*stride, Wo*stride, Cin] f16
 * (= dx_accumulate + ..., when dx_accumulate != NULL; it may alias dx) from dz [B,Ho,Wo,Cout] f16 and the w_bwd pack of
 * od_pack_weights.  A thin wrapper: it fills an od_conv_desc (x = dz, w = w_bwd, identity scale / zero bias owned by the
 * context, transposed = stride == 2) and runs the SAME implicit-GEMM kernels as od_conv2d_fwd -- there is no separate
 * backward-data kernel, which is why the trainer calls od_conv2d_fwd directly. */
int od_conv2d_bwd_data(od_ctx* ctx, const void* dz, const void* w_bwd, const void* dx_accumulate, void* dx, int B, int Ho,
                       int Wo, int Cin, int Cout, int ksize, int stride, void* stream);
/* inference-time BatchNorm folding on the device: scale = gamma / sqrt(var + eps), bias = beta - mean*scale,
 * f32 [C], bit-identical to the numpy f32 expression the loader (object_detector_amd/weights.py fold_bn) evaluates on the
 * host -- the loader folds once on the host at load time, this export is for callers that keep the statistics on the
 * device (e.g. evaluating during training).  The training-mode forward/backward of BatchNorm are od_bn_stats +
 * od_scale_act and od_bn_bwd below (§8b's od_bn_train_fwd / od_bn_train_bwd). */
int od_bn_fold(od_ctx* ctx, const float* gamma, const float* beta, const float* mean, const float* var, float eps,
               float* scale, float* bias, int C, void* stream);
size_t od_bn_workspace_bytes(long long M, int C);
/* batch statistics of z [M,C] -> mean, rstd, and the fused (scale, shift) = (gamma*rstd, beta - mean*scale);
 * run_mean/run_var (may be NULL) updated with `momentum` */
int od_bn_stats(od_ctx* ctx, const void* z, long long M, int C, const float* gamma, const float* beta, float eps,
                float* mean, float* rstd, float* scale, float* shift, float* run_mean, float* run_var, float momentum,
                void* workspace, size_t workspace_bytes, void* stream);
/* the same statistics from the partial rows a conv epilogue wrote (od_conv_desc.bn_partials): fixed-order sum over the
 * rows, then mean / rstd / scale / shift / running statistics exactly as od_bn_stats computes them */
int od_bn_stats_from_partials(od_ctx* ctx, const float* partials, int rows, long long M, int C, const float* gamma,
                              const float* beta, float eps, float* mean, float* rstd, float* scale, float* shift,
                              float* run_mean, float* run_var, float momentum, void* stream);
/* y = act(scale*z + shift) (+ res / up2(res)), f16 */
int od_scale_act(od_ctx* ctx, const void* z, const float* scale, const float* shift, const void* res, int res_mode,
                 void* y, int B, int H, int W, int C, int act, float alpha, void* stream);
/* dz from dy through activation and (bn != 0) BatchNorm; dgamma/dbeta f32 [C] are ACCUMULATED (shared layers);
 * workspace >= od_bn_workspace_bytes(M,C) + 2*C*4 */
int od_bn_bwd(od_ctx* ctx, const void* z, const void* dy, const float* scale, const float* shift, const float* mean,
              const float* rstd, long long M, int C, int act, float alpha, int bn, float* dgamma, float* dbeta,
              void* dz, void* workspace, size_t workspace_bytes, void* stream);
int od_conv2d_bwd_weight(od_ctx* ctx, const void* x, const void* dz, float* dw, int B, int H, int W, int Cin, int Cout,
                         int ksize, int stride, void* stream);
/* gradient of the nearest-2x upsample add: dup[b,y,x,c] (+)= sum of the 2x2 block of d */
int od_down2_sum_add(od_ctx* ctx, const void* d, void* dup, int B, int Hh, int Wh, int C, int accumulate, void* stream);
int od_add_f16(od_ctx* ctx, void* a, const void* b, long long n, void* stream);
/* loss gradient rows of one pyramid level (f32 [B,P,C]) -> loss-scaled f16 gradient of that level's prediction conv */
int od_pred_grad_to_level(od_ctx* ctx, const float* grad_pred, void* dz, int B, int P, int C, int row_off, int rows,
                          float loss_scale, void* stream);
/* w -= lr*(m = momentum*m + g*inv_loss_scale + weight_decay*w) on a flat f32 segment */
int od_sgd_step(od_ctx* ctx, float* w, float* m, const float* g, long long n, float lr, float momentum,
                float weight_decay, float inv_loss_scale, void* stream);
/* master f32 [Cout][k*k*Cin] -> f16 forward pack [Cout_pad][Kpad] and (w_bwd != NULL) backward-data pack
 * [Cin_pad][Kpad_t] (taps flipped, channels swapped); both destinations must be pre-zeroed once (padding).  The
 * backward-data pack is stored in groups of 8 output channels: w_bwd != NULL needs Cout % 8 == 0 (od_conv2d_fwd, its
 * consumer, needs that of both channel counts anyway), and w_fwd / w_bwd must be 16-byte aligned (vector stores);
 * otherwise OD_ERR_INVALID. */
int od_pack_weights(od_ctx* ctx, const float* w, void* w_fwd, void* w_bwd, int Cout, int Cin, int ksize, void* stream);

/* Deterministic weight gradients: od_conv2d_bwd_weight_slabs writes the per-split partial sums as
 * od_conv2d_bwd_weight_splits(...) dense f32 slabs [split][Cout][k*k*Cin] (plain stores, no atomics); one
 * od_wgrad_reduce_multi launch per step then sums every layer's slabs in ascending order into the flat gradient buffer
 * (`table` = DEVICE array; a layer shared by several pyramid levels lists all of their slabs). */
typedef struct od_wgrad_red {
  int64_t dw_offset; /* into the flat gradient buffer */
  int64_t count;     /* Cout * k*k*Cin */
  const float* slabs;
  int32_t nslabs;
  int32_t pad_;
} od_wgrad_red;
int od_conv2d_bwd_weight_splits(od_ctx* ctx, int B, int H, int W, int Cin, int Cout, int ksize, int stride);
/* The kernel a layer's weight gradient runs on, decided by the same plan that the launch and the split count come from:
 * "od_conv_wgrad" (128 x 128 tile), "od_conv_wgrad_w8" (256 x 256), "od_conv_wgrad_thin<1>" / "od_conv_wgrad_thin<2>"
 * (32 -> 64 channels, 3x3, stride 1 / 2; slab form only).  slabs != 0: od_conv2d_bwd_weight_slabs, 0: the atomic-add
 * od_conv2d_bwd_weight.  NULL for arguments the launch would reject.  The training-side counterpart of
 * od_plan_op_kernel_name; the string is static. */
const char* od_conv2d_bwd_weight_kernel_name(od_ctx* ctx, int B, int H, int W, int Cin, int Cout, int ksize, int stride,
                                             int slabs);
int od_conv2d_bwd_weight_slabs(od_ctx* ctx, const void* x, const void* dz, float* slabs, int B, int H, int W, int Cin,
                               int Cout, int ksize, int stride, void* stream);
int od_wgrad_reduce_multi(od_ctx* ctx, const od_wgrad_red* table, int nlayers, float* grads, void* stream);

/* Multi-tensor forms (one launch for the whole parameter set instead of one per tensor -- ~240 launches per step):
 *   od_sgd_step_multi: `segs` is a DEVICE array of od_sgd_seg over one flat f32 parameter / momentum / gradient buffer;
 *   od_pack_weights_multi: `layers` is a DEVICE array of od_pack_layer (w_offset into the same flat buffer). */
typedef struct od_sgd_seg {
  int64_t offset; /* first element of the segment in the flat buffers */
  int64_t count;
  float lr;
  float weight_decay;
} od_sgd_seg;
typedef struct od_pack_layer {
  int64_t w_offset; /* master weights f32 [Cout][k*k*Cin] inside the flat parameter buffer */
  void* w_fwd;      /* f16 [Cout_pad][Kpad] */
  void* w_bwd;      /* f16 [Cin_pad][Kpad_t] or NULL */
  int32_t Cout, Cin, ksize, pad_;
} od_pack_layer;
/* skip_if_nonzero (DEVICE int32, may be NULL): when *skip_if_nonzero != 0 the launch leaves w and m untouched -- the flag
 * od_grad_nonfinite writes, so that one f16 overflow in the loss-scaled backward pass cannot poison the master weights */
int od_sgd_step_multi(od_ctx* ctx, float* w, float* m, const float* g, const od_sgd_seg* segs, int nseg, float momentum,
                      float inv_loss_scale, const int32_t* skip_if_nonzero, void* stream);
/* od_sgd_step_multi, and in the same pass over each segment an exponential moving average of the new weights:
 *   d = w_new - ema; p = ema_one_minus_decay * d; ema = ema + p      (three separately rounded f32 operations)
 * `ema` is a fourth flat buffer with the layout of w; it must not be w, m or g.  This form, not decay*ema + omd*w, is the
 * contract: it leaves ema bitwise unchanged where w_new == ema.  ema_one_minus_decay must lie in [0, 1].  A set
 * skip_if_nonzero leaves w, m and ema untouched; elements that belong to no segment are never written.  Any offset and any
 * 4-byte-aligned base pointers are accepted; a segment that starts at the same distance from a 16-byte boundary in all
 * four buffers moves as 16-byte accesses, with the same bits. */
int od_sgd_step_multi_ema(od_ctx* ctx, float* w, float* m, const float* g, float* ema, const od_sgd_seg* segs, int nseg,
                          float momentum, float inv_loss_scale, float ema_one_minus_decay,
                          const int32_t* skip_if_nonzero, void* stream);
/* ema[i] = ema[i] + one_minus_decay * (x[i] - ema[i]) over a flat buffer (the same three operations; the trainer's
 * average of the BatchNorm running statistics).  skip_if_nonzero (DEVICE int32, may be NULL) as above; ema != x. */
int od_ema_update(od_ctx* ctx, float* ema, const float* x, long long n, float one_minus_decay,
                  const int32_t* skip_if_nonzero, void* stream);
/* flag[0] (DEVICE int32) = 1 when any of g[0..n) is Inf / NaN, else 0.  Run it on the flat gradient buffer AFTER the
 * all-reduce: a non-finite value on one rank reaches every rank through the sum, so all ranks skip the same step. */
int od_grad_nonfinite(od_ctx* ctx, const float* g, long long n, int32_t* flag, void* stream);

/* ---- Optimizers beyond plain momentum SGD, and gradient clipping by global norm.  Three launches per step, no host
 * synchronisation: od_grad_stats -> od_optim_prepare -> od_optim_step_multi.  All f32 arithmetic below is a sequence of
 * single, separately rounded operations in the order written (the sum of squares alone is f64), so a numpy restatement
 * reproduces every result bit for bit, and every rank of a data-parallel run computes the same bits from the same
 * all-reduced gradient buffer. */
#define OD_OPT_SGD 0      /* w -= lr*(m = momentum*m + g*inv + wd*w): od_sgd_step_multi's rule */
#define OD_OPT_NESTEROV 1 /* grad = g*inv + wd*w; m = momentum*m + grad; w -= lr*(grad + momentum*m) */
#define OD_OPT_ADAMW 2    /* decoupled weight decay; bias correction from od_optim_state */
/* DEVICE-resident state of the optimizer, 32 bytes; the host initialises it to step = 0, b1pow = b2pow = 1 (the other
 * fields are written by od_optim_prepare before anything reads them). */
typedef struct od_optim_state {
  int32_t step;        /* updates applied so far (skipped steps do not count) */
  float b1pow;         /* beta1 ** step as a running product of f32 multiplications */
  float b2pow;         /* beta2 ** step likewise */
  float grad_norm;     /* the step's true gradient norm: unscaled, before clipping; Inf / NaN on a flagged step */
  float clip_coef;     /* min(1, max_grad_norm / (grad_norm + 1e-6)), 1 without clipping; may be NaN on a flagged step */
  float inv_scale_eff; /* inv_loss_scale * clip_coef: what every update rule multiplies g by */
  float bc1;           /* 1 - b1pow */
  float bc2;           /* 1 - b2pow */
} od_optim_state;
/* HOST struct of the hyper-parameters the three launches share */
typedef struct od_optim_cfg {
  int32_t kind;              /* OD_OPT_* */
  float momentum;            /* SGD kinds: momentum; AdamW: beta1.  In [0, 1) */
  float beta2;               /* AdamW, in [0, 1) */
  float eps;                 /* AdamW, > 0 */
  float inv_loss_scale;      /* as od_sgd_step_multi's */
  float max_grad_norm;       /* <= 0: no clipping */
  float ema_one_minus_decay; /* read when od_optim_step_multi is given `ema`; in [0, 1] */
  int32_t pad_;
} od_optim_cfg;
/* od_grad_stats: od_grad_nonfinite (same `flag` contract: cleared, then set to 1 when any of g[0..n) is Inf / NaN) and, in
 * the same pass, the sum of squares of g: `workspace` (DEVICE, 8-byte aligned, od_grad_stats_workspace_bytes(n) bytes)
 * receives one f64 partial per workgroup.  Every element is widened to f64, squared (exact) and added in f64; which
 * elements a lane adds in which order, the in-workgroup reduction and the number of partials are fixed functions of n
 * alone, and no float atomic is used: the same bits on every run and every rank.  g must be 16-byte aligned. */
size_t od_grad_stats_workspace_bytes(long long n);
int od_grad_stats(od_ctx* ctx, const float* g, long long n, int32_t* flag, void* workspace, void* stream);
/* od_optim_prepare: one small launch behind od_grad_stats(g, n, flag, workspace) that turns the partials into the step's
 * scalars in *state (DEVICE):
 *   s = sum of the partials in ascending index order (f64);  norm_raw = sqrtf((float)s)
 *   grad_norm = norm_raw * inv_loss_scale
 *   clip_coef = max_grad_norm > 0 ? fminf(1.0f, max_grad_norm / (grad_norm + 1e-6f)) : 1.0f   (clip_grad_norm_'s formula)
 *   inv_scale_eff = inv_loss_scale * clip_coef
 *   if (*flag == 0) { step += 1; b1pow = b1pow * momentum; b2pow = b2pow * beta2; bc1 = 1.0f - b1pow; bc2 = 1.0f - b2pow; }
 * A flagged step leaves step, b1pow, b2pow, bc1 and bc2 untouched; its grad_norm, clip_coef and inv_scale_eff may be
 * Inf / NaN (od_optim_step_multi skips that step, so nothing consumes them).  The bias correction is a running product,
 * not powf: numpy reproduces it, and the device -- not the host -- knows which steps were skipped. */
int od_optim_prepare(od_ctx* ctx, const od_optim_cfg* cfg, const void* workspace, long long n, const int32_t* flag,
                     od_optim_state* state, void* stream);
/* od_optim_step_multi: one launch over the segment table of od_sgd_step_multi (per-segment lr and weight_decay as there).
 * Every kind multiplies g by state->inv_scale_eff.  Per element:
 *   OD_OPT_SGD       sgd_update: with clip_coef == 1 the bits of od_sgd_step_multi
 *   OD_OPT_NESTEROV  grad = g*inv + wd*w; mv = momentum*m + grad; m = mv; u = grad + momentum*mv; w = w - lr*u
 *   OD_OPT_ADAMW     gh = g*inv; m = beta1*m + (1.0f-beta1)*gh; v = beta2*v + (1.0f-beta2)*(gh*gh);
 *                    mh = m/bc1; vh = v/bc2; den = sqrtf(vh) + eps; u = mh/den; w = w - lr*(u + wd*w)
 * v: the second-moment buffer, required for OD_OPT_ADAMW, NULL otherwise.  ema: NULL, or the averaged model, updated
 * behind the weight update per element exactly as od_sgd_step_multi_ema does (cfg->ema_one_minus_decay); it must not be
 * w, m, v or g.  *skip_if_nonzero != 0 (DEVICE, may be NULL) leaves w, m, v and ema untouched; elements of no segment are
 * never written.  Any offset is accepted: a segment whose buffers share the 16-byte phase moves as 16-byte accesses,
 * any other one element by element, with the same bits.  OD_ERR_INVALID, and nothing written, for an unknown kind, nseg
 * outside 1..65535, v against the kind, an aliasing ema, ema_one_minus_decay outside [0, 1], momentum / beta2 outside
 * [0, 1) or eps <= 0 (AdamW). */
int od_optim_step_multi(od_ctx* ctx, const od_optim_cfg* cfg, float* w, float* m, float* v, const float* g, float* ema,
                        const od_sgd_seg* segs, int nseg, const od_optim_state* state, const int32_t* skip_if_nonzero,
                        void* stream);

/* dst[0..n) = src[0..n) when *flag (DEVICE int32) != 0, untouched otherwise.  The trainer keeps a copy of the BatchNorm
 * running statistics taken before forward and restores it with this call when od_grad_nonfinite flagged the step: the
 * skipped step's forward has already folded its (possibly overflowed) batch statistics into them. */
int od_copy_if_nonzero(od_ctx* ctx, float* dst, const float* src, long long n, const int32_t* flag, void* stream);
/* f32 <-> bf16 (round to nearest even) for the bf16 gradient payload of od_allreduce(OD_DT_BF16) */
int od_cast_f32_bf16(od_ctx* ctx, const float* src, void* dst, long long n, void* stream);
int od_cast_bf16_f32(od_ctx* ctx, const void* src, float* dst, long long n, void* stream);
int od_pack_weights_multi(od_ctx* ctx, const float* w, const od_pack_layer* layers, int nlayers, void* stream);

/* ---- Trainer -> detector weight refresh: one launch rewrites the inference tensors of a live network (f16 pack, folded
 * f32 scale and bias per layer) from the trainer's flat f32 buffers.  `layers` is a DEVICE array, one entry per pack. */
typedef struct od_refresh_layer {
  int64_t w_offset;     /* master weights f32 [Cout][k*k*Cin] in params_flat */
  int64_t gamma_offset; /* has_bn: gamma[Cout] in params_flat */
  int64_t beta_offset;  /* has_bn: beta[Cout] in params_flat; otherwise the layer's bias[Cout] */
  int64_t mean_offset;  /* has_bn: running mean[Cout] in run_stats_flat */
  int64_t var_offset;   /* has_bn: running variance[Cout] in run_stats_flat */
  void* w_dst;          /* f16 [Cout_pad][Kpad], written whole */
  void* scale_dst;      /* f32 [Cout_pad], written whole; NULL (with bias_dst) = this entry writes the pack alone */
  void* bias_dst;       /* f32 [Cout_pad] */
  int32_t Cout, Cin, ksize;
  int32_t Cout_pad, Kpad; /* od_conv_weight_dims(Cout, cin_repeat * Cin, ksize); the image layer: Cout, 32 */
  int32_t cin_repeat;     /* 1, or 2: the pack of the weights repeated along the input channels ([w | w], the operand of
                           * a layer that reads an f16 (hi, lo) pair) */
  int32_t first;          /* the image layer: scale is additionally divided by 255.0f */
  int32_t has_bn;
} od_refresh_layer;
/* Per entry, for EVERY element of the three destination tensors (padding is written as zero, never assumed):
 *   w_dst[co][tap*cin_repeat*Cin + r*Cin + ci] = (f16)w[co][tap*Cin + ci]     (round to nearest even, overflow to Inf,
 *                                                                             f16 subnormals kept)
 *   has_bn:  scale = gamma / sqrtf(var + eps);  bias = beta - mean * scale    (od_bn_fold's expression: one correctly
 *            first: scale = scale / 255.0f                                     rounded f32 operation each, no contraction)
 *   else:    scale = 1;  bias = bias
 * Offsets are in elements and may have any 4-byte alignment (rows that are 16-byte aligned move as 16-byte loads); the
 * destination pointers must be 16-byte aligned (the launch cannot see them: the table is on the device).  Returns
 * OD_ERR_INVALID for a null ctx / params_flat / run_stats_flat / layers or nlayers outside 1..65535. */
int od_net_refresh(od_ctx* ctx, const float* params_flat, const float* run_stats_flat, const od_refresh_layer* layers,
                   int nlayers, float eps, void* stream);

/* first layer's weight gradient: dw f32 [32][27] += dz^T . shifted(x_u8) * in_scale (no dX: the input is the image).
 * Streaming kernel (W a multiple of 32: the uint8 window is read in place, one 32 x 32 f32 partial slab per workgroup);
 * other widths run the MFMA weight-gradient kernel over an f16 x 8-channel copy of the image kept in `workspace`.  Either way
 * a fixed-order slab sum, no atomics: bit-reproducible.  workspace: 16-byte aligned, caller-owned, sized by
 * od_conv_first_bwd_weight_workspace_bytes (which knows which of the two forms a shape takes). */
size_t od_conv_first_bwd_weight_workspace_bytes(od_ctx* ctx, int B, int H, int W);
int od_conv_first_bwd_weight(od_ctx* ctx, const uint8_t* x, const void* dz, float* dw, int B, int H, int W, int Cout,
                             float in_scale, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * K13: data-parallel gradient exchange over RCCL / xGMI (reference knob use_multi_gpu=True, check_assign.py:19).
 * One process per GPU; the launcher (Python) creates the unique id on rank 0 (od_comm_get_unique_id) and ships it to
 * the other ranks itself.  od_allreduce: in-place sum over ranks, asynchronous on `stream`.
 * ---------------------------------------------------------------------------------------------- */
typedef struct od_comm od_comm;
int od_comm_unique_id_bytes(void);
int od_comm_get_unique_id(void* out, int bytes);
int od_comm_init(od_ctx* ctx, int rank, int nranks, const void* unique_id, od_comm** out);
int od_allreduce(od_comm* comm, void* buf, long long count, int dtype, void* stream); /* dtype: OD_DT_F32 / F16 / BF16 */
int od_comm_count(od_comm* comm, int* rank, int* nranks); /* as RCCL reports them (ncclCommUserRank / ncclCommCount) */
int od_comm_destroy(od_comm* comm);

/* ------------------------------------------------------------------------------------------------
 * K14: device-side pixel work of the training generator (reference check_generator.py:17-18; docs/MODEL.md:60-64).
 * Parameters are sampled on the host; one od_aug_params per output image (device array).  src = packed uint8 RGB source
 * images (any sizes, located by src_offset/src_h/src_w); out uint8 [B,H,W,3].
 * crop -> bilinear resize -> flip -> saturation/contrast/brightness -> up to 3 Random-Erasing rectangles.
 * ---------------------------------------------------------------------------------------------- */
typedef struct od_aug_params {
  int64_t src_offset;
  int32_t src_h, src_w;
  float crop_x1, crop_y1, crop_x2, crop_y2;
  int32_t flip;
  float brightness, contrast, saturation;
  int32_t n_erase;
  float erase[3][4];
  uint8_t erase_rgb[3][4];
} od_aug_params;
int od_aug_params_bytes(void);
int od_augment_batch(od_ctx* ctx, const uint8_t* src, const void* params, uint8_t* out, int B, int H, int W,
                     void* stream);
/* Mosaic: four sources composed into one output image.  The frame is cut at (split_x, split_y), 1 <= split_x <= W and
 * 1 <= split_y <= H in output pixels; tile[0..3] = TL, TR, BL, BR.  A pixel of a tile with origin (X0, Y0) and extent
 * Wt x Ht samples its source at u = ((x - X0) + 0.5) / Wt, v = ((y - Y0) + 0.5) / Ht with od_augment_batch's arithmetic and
 * that tile's parameters (a tile's n_erase must be 0); an empty tile (split_x == W, split_y == H) is never sampled.  The
 * erase list acts on the whole frame, in normalised output coordinates.  split = (W, H): the output is od_augment_batch's
 * for tile[0] (+ the erase list), byte for byte.  src / src_offset as in od_augment_batch. */
typedef struct od_mosaic_params {
  int32_t split_x, split_y;
  od_aug_params tile[4];
  int32_t n_erase;
  int32_t pad_;
  float erase[3][4];
  uint8_t erase_rgb[3][4];
} od_mosaic_params;
int od_mosaic_params_bytes(void);
int od_augment_mosaic(od_ctx* ctx, const uint8_t* src, const void* params, uint8_t* out, int B, int H, int W,
                      void* stream);
/* K14b: affine warp + colour matrix + MixUp.  One od_warp_params per output image: n_frames (1 or 2) mosaic frames
 * (frame[f]: tiles and split as in od_augment_mosaic, its own n_erase must be 0; a single image is the degenerate mosaic),
 * each seen through the INVERSE affine matrix a[f] and the colour matrix k[f]; fill_rgb where a frame does not reach; the
 * MixUp weights; one erase list for the final image.  Per output pixel (x, y), all f32 without contraction, in this order:
 *  1. px = (float)x + 0.5f, py = (float)y + 0.5f
 *  2. frame f: fx = (a0*px + a1*py) + a2, fy = (a3*px + a4*py) + a5 -- frame coordinates in OUTPUT-PIXEL units (not
 *     normalised), so the identity matrix {1,0,0, 0,1,0} is exact
 *  3. fx < 0 || fx >= W || fy < 0 || fy >= H: the frame's colour is fill_rgb; no colour matrix is applied to it
 *  4. else right = fx >= split_x, low = fy >= split_y choose the tile (X0, Y0, Wt, Ht) as od_augment_mosaic does;
 *     u = (fx - X0) / Wt, v = (fy - Y0) / Ht; c = the tile's od_augment_batch colour at (u, v), already rounded and clamped;
 *     t[ch] = ((k[ch][0]*c0 + k[ch][1]*c1) + k[ch][2]*c2) + k[ch][3], rounded half up, clamped to [0, 255]
 *  5. n_frames == 2: t = A*mix_a + B*mix_b of the two frames' finished colours, rounded half up, clamped
 *  6. the erase list on normalised output coordinates, then the 3-byte store, as in od_augment_mosaic.
 * With one frame, a = identity and k = identity (offset column 0) the output is od_augment_mosaic's for frame[0] and the
 * erase list, byte for byte.  src / src_offset as in od_augment_batch.  Split range, n_frames and the tiles' n_erase are
 * the caller's to keep valid. */
typedef struct od_warp_params {
  int32_t n_frames;
  float mix_a, mix_b;
  uint8_t fill_rgb[4];
  float a[2][6];
  float k[2][3][4];
  od_mosaic_params frame[2];
  int32_t n_erase;
  int32_t pad_;
  float erase[3][4];
  uint8_t erase_rgb[3][4];
} od_warp_params;
int od_warp_params_bytes(void);
int od_augment_warp(od_ctx* ctx, const uint8_t* src, const void* params, uint8_t* out, int B, int H, int W,
                    void* stream);

/* ------------------------------------------------------------------------------------------------
 * K15: image decode + resize into the network input for ObjectDetector(image_decode="device") (reference
 * voc_validate.py:27: predict() on image files).  The output equals the host path (PIL decode + BILINEAR resize) byte
 * for byte.  One od_img_desc per image; the host packs every image's data into one `blob` (device copy) at the *_off
 * byte offsets (16-byte aligned); od_img_workspace_plan lays the per-image workspace out (the *_ws offsets) and returns
 * its size.  out = uint8 [B,H,W,3]: image b's resized out_w x out_h rectangle at the top-left, zeros elsewhere.
 *   OD_IMG_JPEG  baseline Huffman JPEG: stream = unstuffed entropy-coded bytes; sub = OD_JPEG_SUB_INTS int32 per
 *                subsequence of the parallel Huffman decode (start bit, end bit, restart-interval end bit, interval's
 *                first block, end block, first-of-interval flag, 0, 0); huff = 6 decode tables of OD_JPEG_HUFF_INTS
 *                int32 (DC, AC of components 0..2; layout in object_detector_amd/jpeg.py); quant = 3 x 64 int32,
 *                natural order.  ncomp 1 (grey) or 3 (YCbCr, luma sampling samp_h x samp_v, chroma 1x1).
 *   OD_IMG_RGB   packed uint8 [height,width,3] at src_off.
 * hcoef / vcoef: int32 [out_w][2 + hk] / [out_h][2 + vk] rows of (first source index, taps, weights << 22), Pillow's
 * BILINEAR tables (object_detector_amd/resample.py); a pass whose size does not change is skipped.  The horizontal pass
 * runs first, except for an image more than 100 times as tall as wide that shrinks vertically (Image.resize's order).
 * od_jpeg_decode_resize handles the OD_IMG_JPEG entries of the batch, od_rgb_resize the OD_IMG_RGB ones: both may run
 * on the same batch and output.  descs_host is the host copy of descs (validated against blob_bytes / ws_bytes).
 * ---------------------------------------------------------------------------------------------- */
#define OD_IMG_JPEG 1
#define OD_IMG_RGB 2
#define OD_JPEG_HUFF_INTS 804
#define OD_JPEG_SUB_INTS 8
typedef struct od_img_desc {
  int32_t kind;
  int32_t width, height;
  int32_t out_w, out_h;
  int32_t ncomp, samp_h, samp_v;
  int32_t mcux, mcuy, n_sub;
  int32_t hk, vk;
  int32_t pad_;
  int64_t stream_off, stream_bytes;
  int64_t sub_off, huff_off, quant_off, src_off, hcoef_off, vcoef_off;
  int64_t coef_ws, plane_ws, rgb_ws, tmp_ws, state_ws;
} od_img_desc;
int od_img_workspace_plan(od_img_desc* descs_host, int B, long long* workspace_bytes);
int od_jpeg_decode_resize(od_ctx* ctx, const od_img_desc* descs_host, const od_img_desc* descs, int B,
                          const uint8_t* blob, long long blob_bytes, void* workspace, long long ws_bytes, uint8_t* out,
                          int H, int W, void* stream);
int od_rgb_resize(od_ctx* ctx, const od_img_desc* descs_host, const od_img_desc* descs, int B, const uint8_t* blob,
                  long long blob_bytes, void* workspace, long long ws_bytes, uint8_t* out, int H, int W, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Sliced inference (BUILD-DEFINED; DESIGN.md "Sliced inference"): ObjectDetector(slices=(ny, nx)) cuts every image into
 * T overlapping tiles (+ the whole image as the last tile), runs them as T rows of the network batch and merges the T
 * candidate lists of an image in ONE NMS + box voting.  object_detector_amd/slicing.py defines the rectangles.
 *
 * od_tiles_resize: row n of out uint8 [N,H,W,3] = the rectangle (x0, y0, x1, y1) of tile n's source image resized to W x H
 * = PIL crop((x0, y0, x1, y1)).resize((W, H), BILINEAR), byte for byte (resize of the crop, not resize(box=)).  The source
 * sits once in `blob` at full resolution: packed uint8 rows of src_w pixels, `pitch` bytes apart (any pitch >= 3 * src_w),
 * pixel (0, 0) at src_off (no alignment needed).  hcoef / vcoef: the tables of od_img_desc for (x1 - x0 -> W) and
 * (y1 - y0 -> H), 4-byte aligned.  Passes, their order (vertical first for a tile more than 100 times as tall as wide that
 * shrinks vertically) and the skipping of a pass whose length does not change are Image.resize's.  No source byte outside
 * the rectangle is read.  od_tiles_workspace_plan lays the intermediate images out (tmp_ws) and returns the workspace
 * size (it may be 0; pass a valid pointer all the same).  Rows of out from N on are not touched.
 * ---------------------------------------------------------------------------------------------- */
typedef struct od_tile_desc {
  int64_t src_off; /* byte offset of the source image in blob */
  int64_t pitch;   /* source row pitch in bytes */
  int32_t src_w, src_h;
  int32_t x0, y0, x1, y1; /* 0 <= x0 < x1 <= src_w, 0 <= y0 < y1 <= src_h */
  int32_t hk, vk;         /* taps per row of the two tables */
  int64_t hcoef_off, vcoef_off;
  int64_t tmp_ws;
} od_tile_desc;
int od_tiles_workspace_plan(od_tile_desc* descs_host, int N, int H, int W, long long* workspace_bytes);
int od_tiles_resize(od_ctx* ctx, const od_tile_desc* descs_host, const od_tile_desc* descs, int N, const uint8_t* blob,
                    long long blob_bytes, void* workspace, long long ws_bytes, uint8_t* out, int H, int W, void* stream);

/* od_slice_merge: image g of G owns the batch rows g*T .. g*T + T - 1 (1 <= T <= 16) of what od_detect_candidates (clip = 1)
 * produced for the whole batch: keys u64 [.,K] sorted descending, counts i32 [.], boxes f32 [.,P,4] in tile coordinates.
 * tiles f32 [G*T,4] = (ox, oy, sx, sy), the tile's origin and size as fractions of its image; edges i32 [G*T]: bit 0 / 1 /
 * 2 / 3 = the tile's left / top / right / bottom side is interior (not on the image border).  All f32, one rounding per op:
 *   candidate (t, r), r < counts[g*T + t], box (x1, y1, x2, y2): dropped when cut at a seam, i.e. when edge_lo >= 0 and
 *       (left interior and x1 <= edge_lo) or (top interior and y1 <= edge_lo) or (right interior and x2 >= edge_hi) or
 *       (bottom interior and y2 >= edge_hi);  edge_lo < 0 disables the rule
 *   a survivor's box in image coordinates: X = min(max(ox + sx * x, 0), 1), Y = min(max(oy + sy * y, 0), 1)
 *   merged order: conf bits desc, tile asc, flat asc; the first Km = min(K, survivors) are kept
 *   then exactly od_tta_merge: greedy NMS, box voting (vote_iou), the record block `out` f32 [G][1 + 6*max_det] with the
 *       class in word 0 of a row, src i32 [G,max_det,2] (may be NULL) = (tile, flat index in that row), keep_count i32 [G].
 * K <= 1024.  workspace: od_slice_merge_workspace_bytes(G, T, K), needs no initialisation. */
size_t od_slice_merge_workspace_bytes(int G, int T, int K);
int od_slice_merge(od_ctx* ctx, const uint64_t* keys, const int32_t* counts, const float* boxes, const float* tiles,
                   const int32_t* edges, int G, int T, int P, int NC, int K, float edge_lo, float edge_hi,
                   float iou_threshold, int strict, int max_det, float vote_iou, float* out, int32_t* src,
                   int32_t* keep_count, void* workspace, size_t workspace_bytes, void* stream);
/* od_slice_merge with the soft scan (od_soft_nms_cfg above) in place of the greedy one, as od_tta_merge_soft. */
int od_slice_merge_soft(od_ctx* ctx, const uint64_t* keys, const int32_t* counts, const float* boxes, const float* tiles,
                        const int32_t* edges, int G, int T, int P, int NC, int K, float edge_lo, float edge_hi,
                        const od_soft_nms_cfg* cfg, float vote_iou, float* out, int32_t* src, int32_t* keep_count,
                        void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * K16: COCO bbox evaluation (tk.data.coco.evaluate; object_detector_amd/cocoeval.py states the protocol and packs the
 * inputs).  pycocotools COCOeval parameters, fixed: T IoU thresholds, A area ranges, R recall thresholds, M maxDets.
 * All f64 arithmetic is the exact op sequence of the protocol (no contraction), so results are bit-identical to numpy.
 *
 * od_coco_match: one wave per group g (an (image, category) pair).  GTs of g are gt[gt_off[g] .. gt_off[g+1]) in file
 * order, detections det[det_off[g] .. det_off[g+1]) in rank order (descending score, at most 100).
 *   gt_box f64 [n_gt][4] pixel xywh, gt_area f64 [n_gt] (the annotation's area), gt_crowd i32 [n_gt]
 *   det_box f64 [.][4] pixel xywh; det_out i32 [.]: the slot of the detection in matched / ignored
 *   iou_thrs f64 [T], area_rng f64 [A][2] (inclusive)
 *   matched / ignored u64 [.]: bit t*A + a = the detection is matched / ignored under (iou_thrs[t], area_rng[a])
 *   workspace: od_coco_match_workspace_bytes(n_gt) bytes (match state of groups too large for LDS)
 * od_coco_accumulate: one wave per (t, k, a, m).  Category k's detections are slots cat_off[k] .. cat_off[k+1) of
 * rank / score / matched / ignored, in accumulation order (descending score, then image, then rank).
 *   npig i32 [K][A] (GTs not ignored), rec_thrs f64 [R], max_dets i32 [M]
 *   precision f64 [T][R][K][A][M], recall f64 [T][K][A][M], scores f64 [T][R][K][A][M]; -1 where npig == 0
 * ---------------------------------------------------------------------------------------------- */
#define OD_COCO_T 10
#define OD_COCO_A 4
#define OD_COCO_R 101
#define OD_COCO_M 3
size_t od_coco_match_workspace_bytes(long long n_gt);
int od_coco_match(od_ctx* ctx, const int32_t* gt_off, const int32_t* det_off, int n_groups, const double* gt_box,
                  const double* gt_area, const int32_t* gt_crowd, long long n_gt, const double* det_box,
                  const int32_t* det_out, const double* iou_thrs, const double* area_rng, uint64_t* matched,
                  uint64_t* ignored, void* workspace, size_t workspace_bytes, void* stream);
int od_coco_accumulate(od_ctx* ctx, const int32_t* cat_off, int K, const int32_t* rank, const double* score,
                       const uint64_t* matched, const uint64_t* ignored, const int32_t* npig, const double* rec_thrs,
                       const int32_t* max_dets, double* precision, double* recall, double* scores, void* stream);

/* Wide (f32) add paths of the mixed-precision inference plan (ObjectDetector(precision="mixed"); replaces the Keras `Add`
 * layers of the residual blocks, reference docs/MODEL.md:15-17, where the reference's fp32 path keeps the sum in fp32):
 *   v = y (+ res);  out32 = v;  out16 = f16(v);  out_hilo[r] = [f16(v) | f16(v - f16(v))]  (row of 2*C halves)
 * y f32 [M,C] is the producing conv's f32 output; res is the f32 (res_f32 != 0) or f16 tensor it is added to -- the residual
 * stream, or with res_up2 the half-size map of the FPN sum (docs/MODEL.md:5-8) -- or NULL;
 * any of the three outputs may be NULL.  A conv over the [hi | lo] tensor with its weights repeated along Cin sees ~22
 * significant bits of v on f16 MFMA operands. */
typedef struct od_wide_desc {
  const float* y;
  const void* res;
  float* out32;
  void* out16;
  void* out_hilo;
  int64_t M;
  int32_t C;
  int32_t res_f32;
  int32_t res_up2; /* != 0: res is [B, H/2, W/2, C] and every element adds its nearest-neighbour parent (the FPN sums) */
  int32_t H, W;    /* the OUTPUT map (res_up2 only; M = B * H * W) */
  int32_t pad_;
} od_wide_desc;
int od_wide_add(od_ctx* ctx, const od_wide_desc* d, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Native forward plan: the whole layer list of one network executed from C++ (one call per batch, optional
 * hipGraph replay) so Python is not in the per-layer loop.  ops is an array of od_plan_op.
 * ---------------------------------------------------------------------------------------------- */
#define OD_OP_CONV 1
#define OD_OP_CONV_FIRST 2
#define OD_OP_BNECK 3
#define OD_OP_STEM 4
#define OD_OP_WIDE 5

typedef struct od_plan_op {
  int32_t kind; /* OD_OP_* */
  int32_t pad_;
  od_conv_desc conv; /* OD_OP_CONV; OD_OP_CONV_FIRST uses x(u8), w, scale, bias, out, B,H,W,Cout,act,alpha */
  od_bneck_desc bneck; /* OD_OP_BNECK */
  od_stem_desc stem;   /* OD_OP_STEM */
  od_wide_desc wide;   /* OD_OP_WIDE */
} od_plan_op;

typedef struct od_plan od_plan;
/* resolves every op once, here: validation and kernel selection (what od_conv2d_fwd & co. do on each call) happen at
 * creation, and the plan keeps the ready-to-issue launches of each op; an op that is invalid fails the creation */
int od_plan_create(od_ctx* ctx, const od_plan_op* ops, int n_ops, od_plan** out);
int od_plan_run(od_plan* plan, void* stream);   /* eager launches: issues the launches resolved at creation */
int od_plan_capture(od_plan* plan, void* stream); /* capture into a hipGraph (stream must be capturable) */
int od_plan_replay(od_plan* plan, void* stream);
int od_plan_destroy(od_plan* plan);
/* per-op timing for bench.py: runs the plan once with hipEvents around every op; ms[n_ops] */
int od_plan_time_ops(od_plan* plan, void* stream, float* ms, int n_ops);
/* name of the device kernel an op launches (its first launch, as resolved at creation; for matching rocprofv3 rows) */
const char* od_plan_op_kernel_name(od_plan* plan, int op_index);

#ifdef __cplusplus
}
#endif
#endif /* ODHIP_H */
