// g1mul.hpp -- a table of G1 points times a column of scalars, point by point (g1mul.hip): out[i] = [scalars[i]] points[i].
// The work of an SRS update (Params.update): g[i] -> [tau^i] g[i].
#pragma once
#include "common.hpp"

namespace h2 {
// the digit schedule of k_g1_mul_each, for the tools that count what it issues: signed digits of G1MUL_WINDOW bits, MSB first
constexpr uint32_t G1MUL_BLOCK = 256;
constexpr uint32_t G1MUL_WINDOW = 3;
constexpr uint32_t G1MUL_DIGITS = 85;  // 3 x 85 = 255 bits; bit 255 is a digit of its own (0 for every scalar below r)
// argument checks of the entry point, host-only (the C ABI runs them before it touches a device); H2_OK or H2_ERR_INVALID
int g1_mul_each_args(const void* d_points, const void* d_scalars, size_t n, const void* d_out);
int g1_mul_each_launch(const uint64_t* d_points, const Fr* d_scalars, size_t n, uint64_t* d_out, hipStream_t stream);
}  // namespace h2
