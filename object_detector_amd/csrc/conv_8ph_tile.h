// Tile constants of the 8-wave convolution kernel, shared by the kernel (conv_8ph_kernel.h) and by its table and selection
// (conv_8ph.hip), which does not need the kernel itself.
#pragma once

namespace {

constexpr int E_BN = 256, E_BK = 64;
constexpr int E_REGION = 128 * 128;  // one staged region: 128 rows x 64 f16
constexpr int E_BUF = 4 * E_REGION;  // A-lo, A-hi, B-lo, B-hi

}  // namespace
