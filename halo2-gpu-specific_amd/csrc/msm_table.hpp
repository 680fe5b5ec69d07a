// msm_table.hpp -- the registry of shifted-base tables as the MSM drivers use it (msm_table.hip); the public side
// (bases_precompute, bases_forget, bases_precompute_bytes) is declared in msm.hpp
#pragma once
#include <vector>

#include "common.hpp"
#include "ec.hpp"
#include "msm_plan.hpp"

namespace h2 {

struct ShiftTable {
    const Affine* table;  // level 0 = a copy of the bases
    TableDesc desc;       // points per level, digits and their balanced cut of 255 bits
    const Affine* blocks; // sums of BLOCK_ROWS consecutive bases (see "dominant value over whole blocks"); null in a view
                          // that does not start on a block boundary
};

// table whose bases contain [d_bases, d_bases + n): a view that starts at d_bases's row
bool table_find(const uint64_t* d_bases, size_t n, const MsmKnobs& k, ShiftTable* out);
// drops the table whose bases contain d_bases (its bases no longer hold the points it was built from)
void table_drop_containing(const uint64_t* d_bases);
// the tables of at least n points: every table a call of n rows could be served by
std::vector<TableDesc> tables_covering(size_t n);
// device memory of all tables (they are keyed by device address)
size_t table_library_bytes();
// 64 sampled base rows against level 0 of their table: *stale = 1 when they differ (see k_table_check)
void table_check_launch(const Affine* bases, const Affine* level0, size_t n, uint32_t* stale, hipStream_t stream);

}  // namespace h2
