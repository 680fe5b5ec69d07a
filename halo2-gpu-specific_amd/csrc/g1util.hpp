// g1util.hpp -- G1 work beside the MSM (g1util.hip)
#pragma once
#include "common.hpp"
#include "ec.hpp"

namespace h2 {
int random_points_launch(uint64_t seed, size_t n, uint64_t* d_out, hipStream_t stream);
int points_decompress_launch(const void* d_bytes, size_t n, uint64_t* d_out, uint32_t* d_bad, hipStream_t stream);
int points_compress_launch(const uint64_t* d_points, size_t n, void* d_bytes, hipStream_t stream);
int fixed_base_mul_launch(const Fr* d_scalars, const uint64_t* d_table, size_t n, uint64_t* d_out, hipStream_t stream);
int g1_fold_launch(const uint64_t* d_points, uint32_t world, uint32_t count, uint64_t* d_out, hipStream_t stream);
void g1_sum_host(const uint64_t* points, size_t count, uint64_t out_xyz[12]);
}  // namespace h2
