// g1ntt.hpp -- the number-theoretic transform over G1 (g1ntt.hip): the Lagrange basis of an SRS from its powers,
// g_lagrange[i] = n^-1 sum_j w^(-ij) g[j], and the forward direction out[i] = sum_j w^(ij) in[j].
//
// Iterative radix-2 decimation in time: the input is bit-reversed into a scratch of XYZZ points (128 B each) -- the inverse
// also multiplies every point by n^-1 there -- then one launch per stage runs n / 2 butterflies (A, B) -> (A + wB, A - wB),
// and a last launch normalises to affine (one inversion per point).  w is the root of unity of EvaluationDomain::new for
// 2^log_n points; its powers come from the two-level tables of the field NTT's plan for w (or w^-1).
#pragma once
#include "common.hpp"

namespace h2 {
size_t g1_ntt_scratch_bytes(uint32_t log_n);
// argument checks of the entry point, host-only (the C ABI runs them before it touches a device); H2_OK or H2_ERR_INVALID
int g1_ntt_args(const void* d_in, const void* d_out, uint32_t log_n, int inverse, const void* d_scratch, size_t scratch_bytes);
int g1_ntt_launch(DeviceCtx* ctx, const uint64_t* d_in, uint64_t* d_out, uint32_t log_n, bool inverse, void* d_scratch,
                  hipStream_t stream);
}  // namespace h2
