// selectors.hpp -- selector activations as device bitmaps and the combination columns made of them (selectors.hip): the device
// side of the front end's selectors (synthesis.py: DeviceSelectors; DESIGN.md 3b, "Selectors")
#pragma once
#include "common.hpp"

namespace h2 {
// cells one workgroup marks: 256 lanes x 4 cells, the prefix sums of their segments staged in LDS (8 KiB), as k_cells_place
static constexpr uint32_t SEL_THREADS = 256;
static constexpr uint32_t SEL_CHUNK = 1024;
// members one k_selectors_combine launch takes as kernel arguments (a longer combination: further launches over the column)
static constexpr uint32_t SEL_MEMBERS = 16;

// the words of one selector's bitmap: bit r % 32 of word r / 32 is row r
static inline size_t selectors_words(size_t n) { return (n + 31) / 32; }

// what a segment looks like on the device: 16 bytes
struct alignas(16) MarkSeg {
    uint32_t selector;
    uint32_t first;
    uint32_t stride;
    uint32_t pad;
};

// the members of (a slice of) one combination, passed by value: the plan is copied when the launch is queued
struct CombineArgs {
    Fr value[SEL_MEMBERS];
    uint32_t selector[SEL_MEMBERS];
    uint32_t count;
};

// the value of `row` in a combination column: that of the (one) member whose bit is set; `hit` says whether one was
__host__ __device__ __forceinline__ Fr selectors_row_value(const CombineArgs& a, const uint32_t* bitmaps, size_t words,
                                                             uint32_t row, bool& hit) {
    Fr v = fp_zero<FrParams>();
    hit = false;
    for (uint32_t m = 0; m < a.count; m++) {
        const uint32_t w = bitmaps[(size_t)a.selector[m] * words + (row >> 5)];
        if ((w >> (row & 31)) & 1) {
            v = a.value[m];
            hit = true;
        }
    }
    return v;
}

size_t selectors_mark_scratch_bytes(size_t count);
// the argument checks of the three entry points: nullptr when the arguments are usable, else what is wrong.  Host only.
const char* selectors_mark_validate(const h2_selector_segment* segs, size_t count, size_t n, size_t num_selectors,
                                    const void* d_bitmaps, const void* d_scratch, size_t scratch_bytes);
const char* selectors_conflicts_validate(const void* d_bitmaps, size_t num_selectors, size_t n, const void* d_matrix);
const char* selectors_combine_validate(const h2_selector_column* plan, size_t columns, const h2_selector_member* members,
                                       size_t num_members, size_t n, size_t num_selectors, const void* bitmaps, uint32_t out_form);
// validated arguments only; asynchronous on `stream` (the host tables are read before these return)
int selectors_mark_launch(const h2_selector_segment* segs, size_t count, size_t n, uint32_t* d_bitmaps, void* d_scratch,
                          hipStream_t stream);
int selectors_conflicts_launch(const uint32_t* d_bitmaps, size_t num_selectors, size_t n, uint8_t* d_matrix, hipStream_t stream);
int selectors_combine_launch(const h2_selector_column* plan, size_t columns, const h2_selector_member* members, size_t n,
                             const uint32_t* d_bitmaps, hipStream_t stream);
// the host twin of selectors_combine_launch: bitmaps and columns in host memory
void selectors_combine_host(const h2_selector_column* plan, size_t columns, const h2_selector_member* members, size_t n,
                            const uint32_t* bitmaps);
}  // namespace h2
