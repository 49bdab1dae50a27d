// od_conv2d_fwd: which kernel runs a convolution, with what grid, LDS size and parameters.  No kernels here: every family
// keeps its kernels and their table in its own file and exports *_supported / *_prepare or *_select (conv_common.h).
#include <string.h>

#include "conv_common.h"

namespace {

// Tile choice from the measured table (profiles/r01/conv_cfg_sweep.txt; MI355X, batch-32 Darknet53 shapes).
int pick_cfg(const od_ctx* ctx, int M, int Cin, int Cout, int ksize, bool e8_ok, bool throughput) {
  const int cus = ctx->num_cu;
  const int cfg_e8 = od_conv_igemm_num_cfgs();
  const bool spec_ok = (Cin % 64) == 0;  // wave-specialised kernels are tap-uniform only
  if (Cout <= 64) return (ksize == 3 && od_ceil_div(M, 128) >= 8 * cus) ? 1 : 3;
  const long t128 = (long)od_ceil_div(M, 128) * od_ceil_div(Cout, 128);
  if (ksize == 1) {
    if (!spec_ok) return 3;
    // small-M layers, measured IN the network (scripts/sweep_net_cfg.py, profiles/r01/conv_innet_sweep.txt): their input
    // was just written by the previous kernel, every first touch misses L2, so ring depth matters more than in a
    // back-to-back microbenchmark -- 3-deep specialised 64x128 (7) for M <= 16 k, 4-deep 64x64 (6) for long-K 1x1 at M <= 4 k.
    // (Round 2 tried a SPECIALISED 64 x 64 tile -- 4 MFMA + 4 DMA waves -- for these short-K layers: slower than the plain
    // one on every 1x1 shape, 15.9 vs 13.0 us on s3.a; profiles/r02/spec64_sweep.txt.)
    if (M <= 4096) return (M >= 2048 && Cin >= 512) ? 6 : 3;
    if (M <= 16384) return 7;
    if (Cout < 256) return 3;
    // wide 1x1 (neck laterals): fall through to the 128x128 / 8-wave comparison below
    if (t128 < cus) return 4;
  }
  if (!spec_ok) return t128 >= 2L * cus ? 0 : 2;
  const int nk = od_ceil_div(ksize * ksize * Cin, 64);
  if (throughput && e8_ok && ksize == 3 && Cout >= 192 && M >= 2048) {
    // tile_cfg = -2: other launches overlap this one (batches in flight on several streams), so an under-filled grid is
    // not wasted and the figure of merit is CU x time, not time: the 8-wave kernel (one workgroup per CU, half the
    // L2->LDS bytes per flop) then also takes the stage-4 / stage-5 layers (profiles/r01/inflight_sweep.txt: +4.5 % img/s)
    double best = t128 >= cus ? t128 * (7.5 + 1.07 * nk) * 0.5 : t128 * (10.0 + 0.55 * nk);
    int pick = t128 >= cus ? 4 : (Cout <= 256 ? 7 : 5);
    for (int i = 0; i < od_conv_8ph_num_cfgs(); ++i) {
      const long tiles = od_conv_8ph_tiles(i, M, Cout);
      if (tiles * 3 < cus) continue;  // a grid below a third of the chip gained nothing (stage 5, coarse head levels)
      const double c = (double)tiles * od_conv_8ph_tile_cost(i, nk);
      if (c < 0.95 * best) {
        best = c / 0.95;
        pick = cfg_e8 + i;
      }
    }
    return pick;
  }
  if (t128 >= cus) {
    if (Cout == 128) return 2;
    // 128x128 specialised kernel (2 workgroups per CU) vs the 8-wave BM x 256 kernel (1 per CU): whole rounds x
    // (fixed cost + K tiles x cost per tile), constants in us from profiles/r01/conv_8ph_sweep_{320,640}.txt
    const double c13 = (double)od_ceil_div((int)t128, 2 * cus) * (7.5 + 1.07 * nk);
    double best = 0.93 * c13;
    int pick = 4;
    for (int i = 0; e8_ok && i < od_conv_8ph_num_cfgs(); ++i) {
      const double c = (double)((od_conv_8ph_tiles(i, M, Cout) + cus - 1) / cus) * od_conv_8ph_tile_cost(i, nk);
      if (c < best) {
        best = c;
        pick = cfg_e8 + i;
      }
    }
    return pick;
  }
  if (Cout <= 256) return M < 2048 ? 3 : 7;       // few, narrow tiles (neck / prediction module on the coarse levels)
  // few tiles, long K.  Up to half a round of 128 x 128 tiles (backward-data of stage 5: M = 3200, Cout = 512, K = 9216) the
  // 64-row specialised tile doubles the workgroups: 55.6 vs 78.8 us (profiles/r02/dgrad_cfg_sweep.txt); above that one
  // deep-ring workgroup per CU
  return (M >= 2048 && 2 * t128 <= cus) ? 7 : 5;  // (batch-1 maps keep their split-K plan on 5)
}

// Step 1: validate d and describe the convolution.  *v receives the descriptor the later steps read (grouped: the first
// segment stands in for x / out / H / W), *kp the geometry and every other ConvKP field that does not depend on the tile.
int conv_describe(const od_ctx* ctx, const od_conv_desc* d, bool want_stats, od_conv_desc* v, ConvKP* kp) {
  if (d && d->nseg > 1) {
    OD_REQUIRE(d->nseg <= 3, "od_conv2d_fwd: nseg %d > 3", d->nseg);
    OD_REQUIRE(d->ksize == 3 && d->stride == 1 && d->res_mode == OD_RES_NONE && !d->w2 && !want_stats && !d->transposed,
               "od_conv2d_fwd: a grouped launch (nseg > 1) is a 3x3 stride-1 layer without residual / w2 / bn_partials / "
               "transposed mode");
    for (int i = 0; i < d->nseg; ++i)
      OD_REQUIRE(d->seg_x[i] && d->seg_out[i] && d->seg_H[i] > 0 && d->seg_W[i] > 0, "od_conv2d_fwd: segment %d is incomplete", i);
  }
  OD_REQUIRE(ctx && d, "od_conv2d_fwd: null ctx/desc");
  *v = *d;
  const bool grouped = d->nseg > 1;  // (validated above: 3x3, stride 1, plain epilogue)
  if (grouped) {
    v->x = d->seg_x[0];
    v->out = d->seg_out[0];
    v->H = d->seg_H[0];
    v->W = d->seg_W[0];
  }
  d = v;
  OD_REQUIRE(d->x && d->w && d->scale && d->bias && d->out, "od_conv2d_fwd: null tensor");
  OD_REQUIRE(d->ksize == 1 || d->ksize == 3, "od_conv2d_fwd: ksize %d unsupported", d->ksize);
  OD_REQUIRE(d->stride == 1 || d->stride == 2, "od_conv2d_fwd: stride %d unsupported", d->stride);
  OD_REQUIRE(d->B > 0 && d->H > 0 && d->W > 0 && d->Cin > 0 && d->Cout > 0, "od_conv2d_fwd: bad dims");
  OD_REQUIRE(d->Cin % 8 == 0 && d->Cout % 8 == 0, "od_conv2d_fwd: Cin/Cout must be multiples of 8 (got %d/%d)",
             d->Cin, d->Cout);
  OD_REQUIRE(d->res_mode == OD_RES_NONE || d->res, "od_conv2d_fwd: res_mode set but res is null");
  OD_REQUIRE(d->act >= OD_ACT_LINEAR && d->act <= OD_ACT_ELU, "od_conv2d_fwd: bad act");
  OD_REQUIRE(d->act != OD_ACT_LEAKY || (d->alpha >= 0.f && d->alpha <= 1.f), "od_conv2d_fwd: leaky slope must be in [0, 1]");
  ConvKP& p = *kp;
  p.pad = d->ksize / 2;
  p.tconv = d->transposed != 0;
  if (p.tconv)
    OD_REQUIRE(d->ksize == 3 && d->stride == 2 && d->Cin % 64 == 0,
               "od_conv2d_fwd: transposed mode is the backward-data of a 3x3 stride-2 conv (Cin %% 64 == 0)");
  // transposed: a stride-1 conv over the 2x zero-upsampled [B, 2H, 2W, Cin] view of x
  p.H = p.tconv ? 2 * d->H : d->H;
  p.W = p.tconv ? 2 * d->W : d->W;
  p.stride = p.tconv ? 1 : d->stride;
  p.Hs = d->H;
  p.Ws = d->W;
  p.Ho = (p.H + 2 * p.pad - d->ksize) / p.stride + 1;
  p.Wo = (p.W + 2 * p.pad - d->ksize) / p.stride + 1;
  if (d->res_mode == OD_RES_UP2)
    OD_REQUIRE(p.Ho % 2 == 0 && p.Wo % 2 == 0, "od_conv2d_fwd: OD_RES_UP2 needs even output size");
  const long long M64 = (long long)d->B * p.Ho * p.Wo;
  OD_REQUIRE(M64 * d->Cout < (1LL << 31) && (long long)d->B * d->H * d->W * d->Cin < (1LL << 31),
             "od_conv2d_fwd: tensor too large for 32-bit element offsets");
  p.HoWo = p.Ho * p.Wo;
  long long Mg = 0;
  long long seg_x_max = 0;  // elements of the largest input map of a grouped launch (d->H / d->W are the first segment's only)
  for (int i = 0; grouped && i < d->nseg; ++i) {
    const long long Mi = (long long)d->B * d->seg_H[i] * d->seg_W[i];
    Mg += Mi;
    seg_x_max = seg_x_max > Mi * d->Cin ? seg_x_max : Mi * d->Cin;
  }
  OD_REQUIRE(!grouped || (Mg * d->Cout < (1LL << 31) && seg_x_max < (1LL << 31)),
             "od_conv2d_fwd: grouped launch too large for 32-bit element offsets");
  p.M = grouped ? (int)Mg : (int)M64;
  p.nseg = grouped ? d->nseg : 0;

  if (want_stats)
    OD_REQUIRE(!p.tconv && d->out_dtype == OD_DT_F16 && d->act == OD_ACT_LINEAR && d->res_mode == OD_RES_NONE,
               "od_conv2d_fwd: bn_partials needs the raw convolution (f16 output, no activation, no residual, no transposed "
               "gather; scale / bias are NOT applied)");
  if (d->w2) {
    OD_REQUIRE(d->scale2 && d->bias2 && d->out2 && d->Cout2 > 0 && d->Cout2 % 8 == 0,
               "od_conv2d_fwd: w2 needs scale2, bias2, out2 and Cout2 (a multiple of 8)");
    OD_REQUIRE(d->act2 >= OD_ACT_LINEAR && d->act2 <= OD_ACT_ELU, "od_conv2d_fwd: bad act2");
    OD_REQUIRE(d->act2 != OD_ACT_LEAKY || (d->alpha2 >= 0.f && d->alpha2 <= 1.f), "od_conv2d_fwd: leaky slope (alpha2) must be in [0, 1]");
    OD_REQUIRE(d->out_dtype == OD_DT_F16 && !p.tconv && !want_stats && d->Cout % 8 == 0 &&
                   (d->out_batch_stride == 0 || d->out_batch_stride == (long long)p.HoWo * d->Cout) &&
                   (d->out_pix_stride == 0 || d->out_pix_stride == d->Cout),
               "od_conv2d_fwd: w2 (the consuming pointwise layer) needs a dense f16 output of the first layer");
  }
  p.x = (const f16*)d->x;
  p.w = (const f16*)d->w;
  p.scale = d->scale;
  p.bias = d->bias;
  p.res = (const f16*)d->res;
  p.out = d->out;
  p.zero = (const f16*)ctx->zero_page;
  p.Cin = d->Cin;
  p.Cout = d->Cout;
  p.Ktot = d->ksize * d->ksize * d->Cin;
  p.Kstride = od_round_up(p.Ktot, 64);
  p.act = d->act;
  p.alpha = d->alpha;
  p.res_mode = d->res_mode;
  p.out_f32 = d->out_dtype == OD_DT_F32;
  p.stats = d->bn_partials;
  p.w2 = nullptr;  // set by conv_prepare when the selected kernel runs the consuming pointwise layer in its epilogue
  p.scale2 = d->scale2;
  p.bias2 = d->bias2;
  p.out2 = (f16*)d->out2;
  p.Cout2 = d->Cout2;
  p.act2 = d->act2;
  p.alpha2 = d->alpha2;
  p.K2stride = od_round_up(d->Cout, 64);
  p.w2_bytes = (unsigned)((long long)od_round_up(d->Cout2 > 0 ? d->Cout2 : 1, 256) * p.K2stride * 2);
  // grouped: the extent of the LARGEST segment, so that what is decided on x_bytes (conv_choose_cfg, od_conv_8ph_select:
  // 31-bit byte offsets) holds for every segment; the kernel takes each segment's own extent from the segment table
  p.x_bytes = (unsigned)((grouped ? seg_x_max : (long long)d->B * d->H * d->W * d->Cin) * 2);
  p.w_bytes = (unsigned)((long long)od_round_up(d->Cout, 256) * p.Kstride * 2);
  p.obs = d->out_batch_stride ? d->out_batch_stride : (long long)p.HoWo * d->Cout;
  p.ops = d->out_pix_stride ? d->out_pix_stride : d->Cout;
  // 32-bit output offsets (the epilogues compiled for one activation / residual / output type form them that way): the
  // last element an image's rows can reach through the strides, on the largest map of a grouped launch
  long long hw_max = p.HoWo;
  for (int i = 0; grouped && i < d->nseg; ++i) hw_max = hw_max > (long long)d->seg_H[i] * d->seg_W[i] ? hw_max : (long long)d->seg_H[i] * d->seg_W[i];
  p.off32 = p.obs >= 0 && p.ops >= 0 && (long long)d->B * p.obs < (1LL << 31) &&
            (long long)(d->B - 1) * p.obs + (hw_max - 1) * p.ops + d->Cout < (1LL << 31);
  p.splitk = 1;
  p.steps_per_split = 0;
  p.ws = (float*)d->splitk_workspace;
  return OD_OK;
}

// Step 3: the config index, d->tile_cfg or pick_cfg's choice (-2: for batches in flight), checked against what the
// 8-wave configs (the indices behind the table's) can do.
int conv_choose_cfg(const od_ctx* ctx, const od_conv_desc* d, const ConvKP& p, bool want_stats, int* cfg_out) {
  int cfg = d->tile_cfg;
  if (cfg < 0)  // (the 8-wave kernel has its own epilogue without the statistics path: not offered when they are asked for)
    cfg = pick_cfg(ctx, p.M, d->Cin, d->Cout, d->ksize, !want_stats && !p.tconv && (long long)p.x_bytes < 0x7F000000LL, cfg == -2);
  const int cfg_e8 = od_conv_igemm_num_cfgs();
  OD_REQUIRE(cfg < cfg_e8 + od_conv_8ph_num_cfgs(), "od_conv2d_fwd: tile_cfg %d out of range", cfg);
  OD_REQUIRE(!(want_stats && cfg >= cfg_e8), "od_conv2d_fwd: bn_partials is supported by the table kernels only (tile_cfg %d)", cfg);
  OD_REQUIRE(!p.tconv || cfg < cfg_e8, "od_conv2d_fwd: transposed mode runs on the table kernels only (tile_cfg %d)", cfg);
  *cfg_out = cfg;
  return OD_OK;
}

// Step 4: the kernel of config cfg for this layer (with p.w2 set: the one that runs the consuming pointwise layer).
int conv_select(int cfg, const od_conv_desc* d, const ConvKP& p, bool want_stats, ConvKernelInfo* k) {
  const int cfg_e8 = od_conv_igemm_num_cfgs();
  if (cfg >= cfg_e8) {
    // 8-wave / 256-wide schedule (conv_8ph.hip): same launch path (split-K slabs, finish kernel) as the table kernels
    if (od_conv_8ph_select(cfg - cfg_e8, p, d->ksize, k)) return OD_OK;
    od_set_error("od_conv2d_fwd: tile_cfg %d (8-phase kernel) needs Cin %% 64 == 0 and no transposed gather", cfg);
    return OD_ERR_INVALID;
  }
  if (od_conv_igemm_select(cfg, d->ksize, d->Cin, want_stats, od_epi_of(p), k)) return OD_OK;
  od_set_error("od_conv2d_fwd: tile_cfg %d needs Cin %% %d == 0 for 3x3 (Cin = %d); use cfg 0-3", cfg, k->BK, d->Cin);
  return OD_ERR_INVALID;
}

// Step 5: the tile grid of kernel k: m-tiles (segment table, transposed row padding) and n-tiles.
void conv_tile_kp(const od_conv_desc* d, const ConvKernelInfo& k, ConvKP* kp) {
  ConvKP& p = *kp;
  p.mtiles = od_ceil_div(p.M, k.BM);
  if (p.nseg > 1) {  // every segment's rows padded to whole m-tiles
    int t0 = 0;
    for (int i = 0; i < 3; ++i) {
      const bool used = i < d->nseg;
      p.seg_tile0[i] = t0;
      p.seg_x[i] = used ? (const f16*)d->seg_x[i] : nullptr;
      p.seg_out[i] = used ? d->seg_out[i] : nullptr;
      p.seg_H[i] = used ? d->seg_H[i] : 0;
      p.seg_W[i] = used ? d->seg_W[i] : 0;
      p.seg_M[i] = d->B * p.seg_H[i] * p.seg_W[i];
      t0 += od_ceil_div(p.seg_M[i], k.BM);
    }
    p.seg_tile0[3] = t0;
    p.mtiles = t0;
    if (!d->out_batch_stride) p.obs = 0;  // dense outputs: the kernel takes every segment's own H * W * Cout
  }
  p.Mq = 0;
  if (p.tconv) {  // rows per parity class padded to whole tiles, classes interleaved tile by tile (od_tconv_pixel)
    p.Mq = p.M / 4;
    p.mtiles = 4 * od_ceil_div(p.Mq, k.BM);
    p.M = p.mtiles * k.BM;
  }
  // weights/scale/bias are padded to a multiple of 256 output channels, so any BN <= 256 tile stays in bounds.
  p.ntiles = od_ceil_div(d->Cout, k.BN);
}

// Validates d, selects its kernel and appends the launches: the kernel (+ split-K finish); one launch per segment when the
// 8-wave kernel does not take a grouped layer; w2 as a second launch when the selected kernel cannot run it in its epilogue.
// want_stats selects the BatchNorm-statistics kernels (d->bn_partials).
int conv_prepare(od_ctx* ctx, const od_conv_desc* desc, bool want_stats, od_launches* L) {
  od_conv_desc v;
  ConvKP p;
  if (int rc = conv_describe(ctx, desc, want_stats, &v, &p)) return rc;
  const od_conv_desc* d = &v;
  const bool grouped = p.nseg > 1;
  // Step 2: the specialised families
  if (d->tile_cfg < 0 && !want_stats && !grouped) {  // (these kernels have neither the statistics epilogue nor a segment table)
    if (p.tconv && od_tconv_small_supported(d)) return od_tconv_small_prepare(ctx, d, L);
    if (od_conv_rdirect_supported(d)) return od_conv_rdirect_prepare(ctx, d, L);  // (also the transposed form of b.down2's backward-data)
    if (!p.tconv && od_conv_stream3_supported(d)) return od_conv_stream3_prepare(ctx, d, L);
  }
  int cfg;
  if (int rc = conv_choose_cfg(ctx, d, p, want_stats, &cfg)) return rc;
  const bool use_e8 = cfg >= od_conv_igemm_num_cfgs();
  if (grouped && !(use_e8 && d->Cin % 64 == 0)) {  // the table kernels have no segment table: one launch per segment
    od_conv_desc q = *d;
    q.nseg = 0;
    for (int i = 0; i < d->nseg; ++i) {
      q.x = d->seg_x[i];
      q.out = d->seg_out[i];
      q.H = d->seg_H[i];
      q.W = d->seg_W[i];
      if (int rc = conv_prepare(ctx, &q, false, L)) return rc;
    }
    return OD_OK;
  }
  ConvKernelInfo k;
  if (int rc = conv_select(cfg, d, p, want_stats, &k)) return rc;
  conv_tile_kp(d, k, &p);
  if (d->bn_partials) {
    const long long need = (long long)p.mtiles * 2 * d->Cout * 4;
    if (d->bn_partials_bytes < need) {
      od_set_error("od_conv2d_fwd: bn_partials holds %lld bytes, %d rows x 2 x %d channels need %lld", (long long)d->bn_partials_bytes,
                   p.mtiles, d->Cout, need);
      return OD_ERR_WORKSPACE;
    }
  }
  // Step 6: split-K for layers that cannot fill the chip with output tiles (batch-1 inference): every K-range workgroup writes
  // its partial tile to its own slab of the caller's f32 workspace; d->splitk == 0 lets the library choose
  if (d->splitk_workspace && d->splitk != 1 && !p.tconv && !want_stats && !grouped) {  // transposed mode orders its rows by parity class: no slabs
    const int cus = ctx->num_cu;
    const int tiles = p.mtiles * p.ntiles;
    const int nk = od_ceil_div(p.Ktot, k.BK);
    constexpr int thr_mul = 8;  // measured on MI355X (profiles/r01/splitk_sweep.txt): split only when <= CUs/8 tiles,
    constexpr int tgt_mul = 1;  // aiming at ~CUs/2 workgroups
    int sk = d->splitk > 1 ? d->splitk : ((tiles * thr_mul <= cus && nk >= 8) ? od_ceil_div(tgt_mul * cus / 2, tiles) : 1);
    if (sk > nk / 4) sk = nk / 4;  // >= 4 K steps per workgroup
    const long long slab_bytes = (long long)p.M * d->Cout * 4;
    if ((long long)sk * slab_bytes > (long long)d->splitk_workspace_bytes) sk = (int)(d->splitk_workspace_bytes / slab_bytes);
    if (sk > 1) {
      p.steps_per_split = od_ceil_div(nk, sk);
      p.splitk = od_ceil_div(nk, p.steps_per_split);
    }
  }
  if (d->w2 && use_e8 && od_conv_8ph_can_fuse_pointwise(p)) p.w2 = (const f16*)d->w2;
  // split-K and the fused layer are settled: the instantiation for this launch's epilogue (same tile as above; split-K
  // slabs take the run-time one)
  if (int rc = conv_select(cfg, d, p, want_stats, &k)) return rc;
  // Step 7: the launch records
  if (int rc = od_ensure_lds(ctx, k.fn, k.lds)) return rc;
  // the 8-wave kernel's epilogue needs no LDS unless it writes split-K slabs: ask only for the two K-tile buffers then
  // (128 KiB), which leaves room on the CU for a small workgroup of another stream
  const size_t launch_lds = (use_e8 && p.splitk <= 1 && k.lds > (size_t)128 * 1024) ? (size_t)128 * 1024 : k.lds;
  if (int rc = od_add_launch(L, {k.name, od_issue_kp, k.fn, dim3(p.mtiles * p.ntiles * p.splitk), dim3(k.threads), launch_lds}, p))
    return rc;
  if (p.splitk > 1)
    if (int rc = od_conv_finish_prepare(p, L)) return rc;
  if (!d->w2 || p.w2) return OD_OK;
  // the consuming pointwise layer as a second launch right behind the first
  od_conv_desc q;
  memset(&q, 0, sizeof(q));
  q.x = d->out;
  q.w = d->w2;
  q.scale = d->scale2;
  q.bias = d->bias2;
  q.out = d->out2;
  q.B = d->B;
  q.H = p.Ho;
  q.W = p.Wo;
  q.Cin = d->Cout;
  q.Cout = d->Cout2;
  q.ksize = 1;
  q.stride = 1;
  q.act = d->act2;
  q.alpha = d->alpha2;
  q.res_mode = OD_RES_NONE;
  q.out_dtype = OD_DT_F16;
  q.tile_cfg = d->tile_cfg < 0 ? d->tile_cfg : -1;
  q.splitk = d->splitk;
  q.splitk_workspace = d->splitk_workspace;  // same stream: the first launch's finish kernel is done with it
  q.splitk_workspace_bytes = d->splitk_workspace_bytes;
  return conv_prepare(ctx, &q, false, L);
}

}  // namespace

extern "C" int od_conv_num_tile_cfgs(void) { return od_conv_igemm_num_cfgs() + od_conv_8ph_num_cfgs(); }

extern "C" int od_conv_weight_dims(int cout, int cin, int ksize, int* cout_pad, int* kpad) {
  OD_REQUIRE(cout > 0 && cin > 0 && (ksize == 1 || ksize == 3), "od_conv_weight_dims: bad dims");
  if (cout_pad) *cout_pad = od_round_up(cout, 256);
  if (kpad) *kpad = od_round_up(ksize * ksize * cin, 64);
  return OD_OK;
}

int od_conv_prepare(od_ctx* ctx, const od_conv_desc* d, od_launches* L) {
  return conv_prepare(ctx, d, d && d->bn_partials, L);
}

extern "C" int od_conv2d_fwd(od_ctx* ctx, const od_conv_desc* d, void* stream) {
  return od_prepare_issue(stream, od_conv_prepare, ctx, d);
}

// The row count of bn_partials = the statistics kernel's m-tile count, whatever buffer is (or is not) given.
extern "C" int od_conv2d_fwd_bn_rows(od_ctx* ctx, const od_conv_desc* d) {
  od_conv_desc v;
  ConvKP p;
  ConvKernelInfo k;
  int cfg;
  if (conv_describe(ctx, d, true, &v, &p) || conv_choose_cfg(ctx, &v, p, true, &cfg) || conv_select(cfg, &v, p, true, &k)) return -1;
  conv_tile_kp(&v, k, &p);
  return p.mtiles;
}

extern "C" int od_conv2d_bwd_data(od_ctx* ctx, const void* dz, const void* w_bwd, const void* dx_accumulate, void* dx, int B,
                                  int Ho, int Wo, int Cin, int Cout, int ksize, int stride, void* stream) {
  OD_REQUIRE(ctx && dz && w_bwd && dx, "od_conv2d_bwd_data: null argument");
  OD_REQUIRE(Cin > 0 && Cin <= 2048, "od_conv2d_bwd_data: Cin out of range (1..2048)");
  od_conv_desc d;
  memset(&d, 0, sizeof(d));
  d.x = dz;
  d.w = w_bwd;
  d.scale = ctx->ones;
  d.bias = (const float*)ctx->zero_page;
  d.res = dx_accumulate;
  d.res_mode = dx_accumulate ? OD_RES_SAME : OD_RES_NONE;
  d.out = dx;
  d.B = B;
  d.H = Ho;
  d.W = Wo;
  d.Cin = Cout;  // the backward-data conv contracts over the forward conv's output channels
  d.Cout = Cin;
  d.ksize = ksize;
  d.stride = stride;
  d.act = OD_ACT_LINEAR;
  d.out_dtype = OD_DT_F16;
  d.tile_cfg = -1;
  d.transposed = stride == 2;
  d.splitk = 1;
  return od_conv2d_fwd(ctx, &d, stream);
}
