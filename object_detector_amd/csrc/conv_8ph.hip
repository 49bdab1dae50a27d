// The 8-wave convolution kernel (conv_8ph_kernel.h): its tile heights, cost model and the choice of an instantiation.
// The instantiations themselves are in conv_8ph_inst.hip, one object per tile height.
#include "conv_8ph_tile.h"
#include "conv_common.h"

namespace {

// idx -> tile height and the instantiations of that height (conv_8ph_inst.hip)
struct E8Entry {
  int BM;
  bool (*variant)(int ksize, bool pw, int epi, int epi2, const void** fn, const char** name);
};
const E8Entry g_e8[] = {{256, od_conv_8ph_variant_mf4}, {224, od_conv_8ph_variant_mf3}, {192, od_conv_8ph_variant_mf2},
                        {160, od_conv_8ph_variant_mf1}};
constexpr int kNumE8 = sizeof(g_e8) / sizeof(g_e8[0]);

}  // namespace

int od_conv_8ph_num_cfgs() { return kNumE8; }

long od_conv_8ph_tiles(int idx, int M, int Cout) { return (long)od_ceil_div(M, g_e8[idx].BM) * od_ceil_div(Cout, E_BN); }
// us per BM x 256 tile: fixed cost + K tiles x cost per K tile (profiles/r01/conv_8ph_sweep_{320,640}.txt)
double od_conv_8ph_tile_cost(int idx, int nk) { return 13.0 + 1.78 * nk * (0.5 + 0.0625 * (g_e8[idx].BM / 32)); }

// one n tile holding all 256 channels of a pixel, 128 output channels (W2 = 64 KiB of LDS), no split-K slabs
bool od_conv_8ph_can_fuse_pointwise(const ConvKP& p) { return p.splitk == 1 && p.Cout == E_BN && p.Cout2 == 128; }

bool od_conv_8ph_select(int idx, const ConvKP& p, int ksize, ConvKernelInfo* info) {
  if (idx < 0 || idx >= kNumE8) return false;
  if ((p.Cin & 63) != 0 || p.tconv) return false;
  if (p.x_bytes >= 0x7F000000u || p.w_bytes >= 0x7F000000u || p.x_bytes == 0) return false;  // E_OOB must stay out of range
  const E8Entry& e = g_e8[idx];
  const bool pw = p.w2 != nullptr;  // the caller (od_conv2d_fwd) has checked od_conv_8ph_can_fuse_pointwise
  if (p.nseg > 1 && (ksize != 3 || pw || p.stride != 1 || p.res_mode != OD_RES_NONE)) return false;
  const size_t epi = (size_t)(e.BM / 2) * (E_BN + 4) * 4;
  // the instantiation whose epilogue is compiled for this launch's activation / residual / output type (and the fused
  // layer's), else the one that reads them at run time.  Ordinary 3x3 launches run the segment-capable instantiation
  // too (its segment table is empty: nseg <= 1), so that the kernel is ONE symbol whether or not a layer is grouped
  const int epi1 = od_epi_of(p);
  // the fused pointwise layer as the kernel sets it up: act2, no residual, dense f16 (fewer elements than the first layer's)
  const int epi2 = (pw && epi1 != OD_EPI_RT) ? od_epi(p.act2, OD_RES_NONE, false) : OD_EPI_RT;
  const void* fn;
  const char* name;
  if (!e.variant(ksize, pw, epi1, epi2, &fn, &name) &&
      !e.variant(ksize, pw, OD_EPI_RT, OD_EPI_RT, &fn, &name))
    return false;
  *info = {fn, name, e.BM, E_BN, E_BK, 512, epi > (size_t)2 * E_BUF ? epi : (size_t)2 * E_BUF};
  return true;
}
