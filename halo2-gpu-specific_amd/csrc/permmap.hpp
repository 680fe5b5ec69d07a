// permmap.hpp -- the copy constraints' cycle mapping built on the device (permmap.hip)
#pragma once
#include "common.hpp"

namespace h2 {
// entries a workgroup of the radix sort ranks (k_pm_hist / k_pm_scatter)
static constexpr uint32_t PM_SORT_TILE = H2_PERM_MAPPING_SORT_TILE;

size_t permutation_mapping_scratch_bytes(size_t n_columns, size_t n, size_t copies);
// the argument checks of h2_dev_permutation_mapping: nullptr when the arguments are usable, else what is wrong with them.
// Host only -- nothing here touches a device.
const char* permutation_mapping_validate(const uint32_t* d_copies, size_t copies, size_t n_columns, size_t n,
                                         const uint32_t* d_map_col, const uint32_t* d_map_row, const uint32_t* d_status,
                                         const void* d_scratch, size_t scratch_bytes);
// validated arguments only; asynchronous on `stream` unless `phase_ms` (3 floats: components, compaction + sort, successors)
// is given: then the phases are timed by events and the call returns when the stream has drained
int permutation_mapping_launch(const uint32_t* d_copies, size_t copies, size_t n_columns, size_t n, uint32_t* d_map_col,
                               uint32_t* d_map_row, uint32_t* d_status, void* d_scratch, float* phase_ms, hipStream_t stream);
}  // namespace h2
