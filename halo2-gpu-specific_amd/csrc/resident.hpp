// resident.hpp -- registered host ranges and the host-buffer MSM drivers (resident.hip)
#pragma once
#include "common.hpp"

namespace h2 {
int bases_register(const uint64_t* bases, size_t n);
int bases_unregister(const uint64_t* bases);
int poly_register(const uint64_t* values, size_t n);
const Fr* poly_resident(DeviceCtx* ctx, const uint64_t* values, size_t n);
int msm_host(DeviceCtx* ctx, const uint64_t* scalars, const uint64_t* bases, size_t n, uint32_t max_bits,
             uint64_t out_xyz[12]);
int msm_host_resident_scalars(DeviceCtx* ctx, const Fr* d_scalars, const uint64_t* bases, size_t n,
                              uint32_t max_bits, uint64_t out_xyz[12]);
int msm_host_multi(const uint64_t* scalars, const uint64_t* bases, size_t n, uint32_t max_bits, uint64_t out_xyz[12]);
}  // namespace h2
