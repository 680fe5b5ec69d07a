// msm.hpp -- the MSM as the rest of the library calls it: the drivers (msm.hip), the launch list (msm_kernels.hip) and the
// shifted-base tables (msm_table.hip)
#pragma once
#include "common.hpp"

namespace h2 {
size_t msm_scratch_bytes(size_t n, uint32_t max_bits);
void msm_shape_query(size_t n, uint32_t max_bits, uint32_t* c, uint32_t* windows, uint32_t* buckets_per_window);
void msm_identity(uint64_t out_xyz[12]);
// the launches of the calling thread's most recent msm_device* call (h2_msm_last_launches): returns their count
size_t msm_last_launches(h2_msm_launch_info* out, size_t cap);
// device-resident scalars + bases; result to host memory (synchronises `stream` for the final
// W*G-point read-back and the host-side window combine)
int msm_device(DeviceCtx* ctx, const Fr* d_scalars, const uint64_t* d_bases, size_t n, uint32_t max_bits,
               void* d_scratch, size_t scratch_bytes, uint64_t* out_xyz, hipStream_t stream);
int msm_device_batch(DeviceCtx* ctx, const Fr* const* d_scalars, size_t count, const uint64_t* d_bases, size_t n,
                     uint32_t max_bits, void* d_scratch, size_t scratch_bytes, uint64_t* out_xyz, hipStream_t stream);
int msm_device_batch_ex(DeviceCtx* ctx, const Fr* const* d_scalars, const uint64_t* const* bases_each,
                        const uint32_t* bits_each, size_t count, const uint64_t* d_bases, size_t n, uint32_t max_bits,
                        void* d_scratch, size_t scratch_bytes, uint64_t* out_xyz, hipStream_t stream);
size_t msm_batch_scratch_bytes(size_t n, uint32_t max_bits, size_t count);
// shifted-base table of a device-resident base set (msm_table.hip): built once, used by every
// msm_device* call whose bases lie inside [d_bases, d_bases + n)
int bases_precompute(const uint64_t* d_bases, size_t n, uint32_t digits, hipStream_t stream);
int bases_forget(const uint64_t* d_bases);
size_t bases_precompute_bytes(size_t n, uint32_t digits);
size_t msm_library_bytes(DeviceCtx* ctx);

}  // namespace h2
