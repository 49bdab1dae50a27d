// Instantiations of the 8-wave convolution kernel (conv_8ph_kernel.h) for ONE tile height: the Makefile compiles this file
// four times, -DOD_E8_MF1=4..1 (BM = 256..160), so that the objects build side by side.  Per kernel shape (1x1, 3x3 with
// segment table, either with the fused pointwise layer) there is the run-time epilogue (OD_EPI_RT) and one instantiation
// per epilogue policy the forward plans use; od_conv_8ph_select (conv_8ph.hip) asks for one through od_conv_8ph_variant_mf<N>.
#include "conv_8ph_kernel.h"

#ifndef OD_E8_MF1
#error "compile with -DOD_E8_MF1=1..4"
#endif

namespace {

struct E8Variant {
  int ksize;
  bool pw;
  int epi, epi2;
  const void* fn;
  const char* name;
};
// (the leading template arguments are what bench.py's roofline reads from the name: ksize, MF1)
#define OD_E8V(KS, PW, SEG, EPI, EPI2)                                                                                  \
  {KS, PW, EPI, EPI2, (const void*)&od_conv_8ph<KS, OD_E8_MF1, EPI, EPI2, PW, SEG>,                                     \
   "od_conv_8ph<" #KS ", " OD_STR(OD_E8_MF1) ", " OD_STR(EPI) ", " OD_STR(EPI2) ", " #PW ", " #SEG ">"}
// Every tile height gets the whole list (the four objects build side by side, so the clean build takes as long as before), although pick_cfg uses few of
// the pairs at the benchmark sizes (kernel traces, profiles/epilogue/): at 32x320^2 with three batches in flight the 3x3
// launches run MF1 = 4 with LEAKY_SAME, LEAKY_NONE, ELU_NONE, LINEAR_NONE_F32 and both fused pairs, and the one 1x1
// launch (n.lat3) MF1 = 3 with ELU_UP2; with one batch in flight all of these run MF1 = 3.  16x640^2 picks the same
// heights.  MF1 = 2 and 1 serve smaller batches and maps.
const E8Variant g_variants[] = {
    // 1x1: the FPN laterals (ELU, with and without the up-sampled sum; f32 in the mixed plan) and the wide block 1x1s
    OD_E8V(1, false, false, OD_EPI_RT, OD_EPI_RT),
    OD_E8V(1, false, false, OD_EPI_LEAKY_NONE_F16, OD_EPI_RT),
    OD_E8V(1, false, false, OD_EPI_ELU_NONE_F16, OD_EPI_RT),
    OD_E8V(1, false, false, OD_EPI_ELU_UP2_F16, OD_EPI_RT),
    OD_E8V(1, false, false, OD_EPI_ELU_NONE_F32, OD_EPI_RT),
    // 3x3: backbone blocks and stride-2 layers, neck / prediction module (grouped or not), the f32 logits and the f32
    // outputs of the mixed plan
    OD_E8V(3, false, true, OD_EPI_RT, OD_EPI_RT),
    OD_E8V(3, false, true, OD_EPI_LEAKY_NONE_F16, OD_EPI_RT),
    OD_E8V(3, false, true, OD_EPI_LEAKY_SAME_F16, OD_EPI_RT),
    OD_E8V(3, false, true, OD_EPI_ELU_NONE_F16, OD_EPI_RT),
    OD_E8V(3, false, true, OD_EPI_ELU_UP2_F16, OD_EPI_RT),
    OD_E8V(3, false, true, OD_EPI_LINEAR_NONE_F32, OD_EPI_RT),
    OD_E8V(3, false, true, OD_EPI_LEAKY_NONE_F32, OD_EPI_RT),
    OD_E8V(3, false, true, OD_EPI_ELU_NONE_F32, OD_EPI_RT),
    // + the consuming pointwise layer (256 -> 128, leaky) of the next residual block
    OD_E8V(1, true, false, OD_EPI_RT, OD_EPI_RT),
    OD_E8V(3, true, false, OD_EPI_RT, OD_EPI_RT),
    OD_E8V(3, true, false, OD_EPI_LEAKY_NONE_F16, OD_EPI_LEAKY_NONE_F16),
    OD_E8V(3, true, false, OD_EPI_LEAKY_SAME_F16, OD_EPI_LEAKY_NONE_F16),
};

}  // namespace

#define OD_CAT_(a, b) a##b
#define OD_CAT(a, b) OD_CAT_(a, b)
bool OD_CAT(od_conv_8ph_variant_mf, OD_E8_MF1)(int ksize, bool pw, int epi, int epi2, const void** fn, const char** name) {
  for (const E8Variant& v : g_variants)
    if (v.ksize == ksize && v.pw == pw && v.epi == epi && v.epi2 == epi2) {
      *fn = v.fn;
      *name = v.name;
      return true;
    }
  return false;
}
