// place.hpp -- bulk placement of assigned cells into resident columns (place.hip): the device side of the circuit front end
#pragma once
#include "common.hpp"

namespace h2 {
// cells one workgroup places: 256 lanes x 4 cells.  The workgroup stages the prefix sums of the segments its cells can belong
// to in LDS -- PLACE_CHUNK + 1 u64 = 8 KiB, so that the LDS never limits residency (160 KiB per CU).
static constexpr uint32_t PLACE_THREADS = 256;
static constexpr uint32_t PLACE_CHUNK = 1024;

// what a segment looks like on the device: 32 bytes, read as two 16-byte loads
struct alignas(16) PlaceSeg {
    uint64_t dst;     // column base (n x 4 u64)
    uint64_t src;     // first source cell
    uint32_t first;   // first destination row
    uint32_t stride;  // destination row stride
    uint32_t form;    // H2_PLACE_FORM_*
    uint32_t pad;
};

size_t cells_place_scratch_bytes(size_t count);
// the argument checks of h2_dev_cells_place: nullptr when the arguments are usable, else what is wrong with them.  Host only.
const char* cells_place_validate(const h2_place_segment* segs, size_t count, size_t n, uint32_t out_form, const void* d_scratch,
                                 size_t scratch_bytes);
// validated arguments only; asynchronous on `stream` (the segment table is read before this returns)
int cells_place_launch(const h2_place_segment* segs, size_t count, size_t n, uint32_t out_form, void* d_scratch,
                       hipStream_t stream);
}  // namespace h2
