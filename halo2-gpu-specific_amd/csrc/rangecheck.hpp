// rangecheck.hpp -- completion of the witness of `advice_column_range` columns on the device (rangecheck.hip)
#pragma once
#include "common.hpp"

namespace h2 {
// counting-sort cap: vmax - vmin below this (the host code's own cap, prover.complete_range_check_witness)
static constexpr uint64_t RC_MAX_WIDTH = 1ull << 24;

// u32 counters of one pair: its bins and the end sentinel, rounded up to whole scan tiles (0 for an unsupported width)
size_t range_check_pair_words(uint64_t vmin, uint64_t vmax);
size_t range_check_scratch_bytes(const uint64_t* vmin, const uint64_t* vmax, size_t pairs);
// the argument checks of h2_dev_range_check_complete: nullptr when the arguments are usable, else what is wrong with them.
// Host only -- nothing here touches a device.
const char* range_check_validate(void* const* d_origins, void* const* d_companions, const uint32_t* origin_forms,
                                 const uint32_t* companion_forms, const uint64_t* vmin, const uint64_t* vmax, const uint64_t* step,
                                 size_t pairs, size_t usable, size_t n, const void* d_status, const void* d_scratch,
                                 size_t scratch_bytes);
// validated arguments only; asynchronous on `stream`
int range_check_complete_launch(void* const* d_origins, void* const* d_companions, const uint32_t* origin_forms,
                                const uint32_t* companion_forms, const uint64_t* vmin, const uint64_t* vmax, const uint64_t* step,
                                const uint64_t* first_unassigned, size_t pairs, size_t usable, size_t n, uint32_t* d_status,
                                void* d_scratch, hipStream_t stream);
}  // namespace h2
