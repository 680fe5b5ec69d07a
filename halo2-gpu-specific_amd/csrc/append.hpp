// append.hpp -- the record append of the device-side checks (check.hip: a witness, srscheck.hip: an SRS), device only.
// A caller-owned buffer of `cap` h2_check_records with a caller-zeroed 64-bit count (check.hpp: the append scheme).
#pragma once
#include "common.hpp"

namespace h2 {

// The slot of this lane among the lanes of its wave that `take`, in a buffer whose fill count is *counter: one agent-scope
// atomic per wave.  Called by every lane of the wave (wave-uniform control flow); the lanes that do not take get garbage.
__device__ __forceinline__ unsigned long long wave_slot(bool take, unsigned long long* counter) {
    const unsigned long long mask = __ballot(take);
    if (mask == 0) return 0;
    const uint32_t lane = threadIdx.x & 63;
    const int leader = __ffsll(mask) - 1;
    unsigned long long base = 0;
    if ((int)lane == leader)
        base = __hip_atomic_fetch_add(counter, (unsigned long long)__popcll(mask), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    base = __shfl(base, leader, 64);
    return base + (unsigned long long)__popcll(mask & ((1ull << lane) - 1));
}

__device__ __forceinline__ void check_append(bool fail, uint32_t kind, uint32_t index, uint32_t sub, uint32_t row,
                                             unsigned long long* count, h2_check_record* out, unsigned long long cap) {
    const unsigned long long slot = wave_slot(fail, count);
    if (fail && slot < cap) *reinterpret_cast<uint4*>(out + slot) = make_uint4(kind, index, sub, row);
}

}  // namespace h2
