// coverage.hpp -- which cells each region of an assignment pass assigned, as bits, and the test of every cell an enabled gate
// reads against them: MockProver's CellNotAssigned (synthesis.py: DeviceCoverage; DESIGN.md 3b, "Checking assignments").
// The definitions, the argument checks and the host twins (coverage_host.cpp) include no HIP header; the kernels and their
// launches (coverage.hip) see the same inline functions as __host__ __device__.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "../../include/halo2_hip.h"

#ifdef __HIPCC__
#define H2_COV_FN __host__ __device__ __forceinline__
#else
#define H2_COV_FN inline
#endif

namespace h2 {
// units one workgroup takes -- words of stride-1 segments, cells of strided ones, enabled rows of uses: 256 lanes x 4, the
// prefix sums they can fall under staged in LDS (8 KiB), as k_selectors_mark
static constexpr uint32_t COV_THREADS = 256;
static constexpr uint32_t COV_CHUNK = 1024;
static constexpr size_t COV_MAX_WORDS = (size_t)1 << 30;  // 4 GiB of bits

// a segment as the mark kernel takes it: its first bit in the whole array; `count` cells `stride` bits apart
struct alignas(16) CovSeg {
    uint64_t first_bit;
    uint32_t count;
    uint32_t stride;
};

// the mark launch's tables: the stride-1 and the one-cell segments first (split by the WORDS they touch, word_prefix),
// then the rest (split by CELLS, cell_prefix); a prefix has one entry more than its segments, or none
struct CovMarkPlan {
    std::vector<CovSeg> segs;
    std::vector<uint64_t> word_prefix, cell_prefix;
    size_t by_word() const { return word_prefix.empty() ? 0 : word_prefix.size() - 1; }
    size_t by_cell() const { return cell_prefix.empty() ? 0 : cell_prefix.size() - 1; }
};

// the bits of word `w` that a stride-1 run of `count` cells from `first_bit` on sets (w is one of the words it touches)
H2_COV_FN uint32_t coverage_word_mask(uint64_t first_bit, uint32_t count, uint64_t w) {
    const uint64_t lo = first_bit > (w << 5) ? first_bit : (w << 5);
    const uint64_t end = first_bit + count < ((w + 1) << 5) ? first_bit + count : ((w + 1) << 5);
    const uint32_t len = (uint32_t)(end - lo);
    return (len == 32 ? 0xffffffffu : (1u << len) - 1) << (lo & 31);
}

// is `row` one of the rows of `u`?
H2_COV_FN bool coverage_use_holds(const h2_coverage_use& u, uint64_t row) {
    if (row < u.first_row) return false;
    const uint64_t d = row - u.first_row;
    return d % u.stride == 0 && d / u.stride < u.count;
}

// does an earlier use of the same region and gate hold `row` already?
H2_COV_FN bool coverage_row_repeated(const h2_coverage_use* uses, const uint32_t* earlier, const h2_coverage_use& u, uint64_t row) {
    for (uint32_t e = 0; e < u.num_earlier; e++)
        if (coverage_use_holds(uses[earlier[u.first_earlier + e]], row)) return true;
    return false;
}

// the row of the cell `q` reads from `row`, and whether the region assigned it
H2_COV_FN bool coverage_assigned(const h2_coverage_plane* planes, const uint32_t* bits, const h2_coverage_query& q, uint64_t row,
                                 uint64_t n, uint32_t& cell_row) {
    cell_row = (uint32_t)((row + n + (uint64_t)(int64_t)q.rotation) % n);  // |rotation| < n: validated on the host
    if (q.plane == H2_COVERAGE_NO_PLANE) return false;
    const h2_coverage_plane p = planes[q.plane];
    if (cell_row < p.row_lo || cell_row - p.row_lo >= p.rows) return false;
    const uint32_t off = cell_row - p.row_lo;
    return (bits[p.first_word + (off >> 5)] >> (off & 31)) & 1;
}

size_t coverage_scratch_bytes(size_t segments, size_t planes, size_t queries, size_t uses, size_t earlier);
// the argument checks: nullptr when the arguments are usable, else what is wrong.  `device`: the scratch is looked at too.
const char* coverage_mark_validate(const h2_coverage_plane* planes, size_t num_planes, const h2_coverage_segment* segs, size_t count,
                                   const void* bits, size_t words, bool device, const void* d_scratch, size_t scratch_bytes);
const char* coverage_check_validate(const h2_coverage_plane* planes, size_t num_planes, const h2_coverage_query* queries,
                                    size_t num_queries, const h2_coverage_use* uses, size_t num_uses, const uint32_t* earlier,
                                    size_t num_earlier, size_t n, const void* bits, size_t words, bool device, const void* d_scratch,
                                    size_t scratch_bytes, const uint64_t* count, const h2_check_record* records, size_t cap);
// validated arguments only
CovMarkPlan coverage_mark_plan(const h2_coverage_plane* planes, const h2_coverage_segment* segs, size_t count);
void coverage_mark_host(const h2_coverage_plane* planes, const h2_coverage_segment* segs, size_t count, uint32_t* bits);
void coverage_check_host(const h2_coverage_plane* planes, const h2_coverage_query* queries, const h2_coverage_use* uses,
                         size_t num_uses, const uint32_t* earlier, size_t n, const uint32_t* bits, uint64_t* count,
                         h2_check_record* records, size_t cap);

#ifdef __HIPCC__
// validated arguments only; asynchronous on `stream` (the host tables are read before these return)
int coverage_mark_launch(const h2_coverage_plane* planes, const h2_coverage_segment* segs, size_t count, uint32_t* d_bits,
                         void* d_scratch, hipStream_t stream);
int coverage_check_launch(const h2_coverage_plane* planes, size_t num_planes, const h2_coverage_query* queries, size_t num_queries,
                          const h2_coverage_use* uses, size_t num_uses, const uint32_t* earlier, size_t num_earlier, size_t n,
                          const uint32_t* d_bits, void* d_scratch, uint64_t* d_count, h2_check_record* d_records, size_t cap,
                          hipStream_t stream);
#endif
}  // namespace h2
