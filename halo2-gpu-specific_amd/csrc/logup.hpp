// logup.hpp -- multiplicity column of a logup lookup (logup.hip)
#pragma once
#include "common.hpp"

namespace h2 {
// The slot table of a compressed lookup table (shared with check.hip): open addressing over `cap` (a power of two) u32 slots,
// each SLOT_EMPTY or the lowest row of the table that holds a value; probed linearly from key_hash(value) & (cap - 1).
static constexpr uint32_t SLOT_EMPTY = 0xffffffffu;

__device__ __forceinline__ uint32_t key_hash(const Fr& k) {
    uint32_t h = 0x9e3779b9u;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        h ^= k.l[i];
        h *= 0x85ebca6bu;
        h ^= h >> 13;
    }
    h *= 0xc2b2ae35u;
    return h ^ (h >> 16);
}

// slots for `usable` table rows (at most half of them used)
uint32_t logup_table_capacity(size_t usable);
// fill d_slots (cap u32, cap = logup_table_capacity(usable) or larger) from the first `usable` rows of d_table; asynchronous
void logup_build_launch(const Fr* d_table, size_t usable, uint32_t* d_slots, uint32_t cap, hipStream_t stream);
size_t logup_scratch_bytes(size_t n);
int logup_multiplicity_launch(const Fr* d_table, const Fr* const* d_inputs, size_t n_inputs, size_t usable, size_t n,
                              Fr* d_m, void* d_scratch, size_t scratch_bytes, hipStream_t stream, uint32_t* max_count_out = nullptr);
int logup_counts_launch(const Fr* d_table, const Fr* const* d_inputs, size_t n_inputs, size_t usable, size_t n, size_t row_begin,
                        size_t row_end, uint32_t* d_counts, void* d_scratch, size_t scratch_bytes, hipStream_t stream);
int logup_emit_launch(const uint32_t* d_counts, size_t usable, size_t n, Fr* d_m, hipStream_t stream);
}  // namespace h2
