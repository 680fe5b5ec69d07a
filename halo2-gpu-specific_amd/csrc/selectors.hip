// selectors.hip -- selector activations kept on the device as bitmaps, and the fixed columns compress_selectors makes of them.
//
// A selector is one bit per row.  The front end queues (selector, first_row, stride, count) segments as the regions enable
// them and flushes the queue here; the 32-byte fixed columns the prover reads are written on the device from the bits, so
// that with resident keygen neither the bits nor the columns cross PCIe ("Selectors").
//
//   k_selectors_mark       sets the bit of every enabled row.  The work is split by CELLS, as k_cells_place splits it: cell c
//                          of the batch belongs to the segment s with prefix[s] <= c < prefix[s + 1]; a workgroup takes
//                          SEL_CHUNK consecutive cells and stages the prefix sums they can fall under in LDS.  The bit is
//                          set by atomicOr on the word, so two segments -- or two lanes -- that enable one row agree.
//   k_selectors_conflicts  one lane per bitmap WORD (32 rows).  It walks the selectors' words of its rows once, keeping
//                          `seen` (the rows some selector so far enables) and `twice` (the rows two of them do).  Only a
//                          lane with twice != 0 goes on to name the pairs: for every selector i with a row in `twice`, every
//                          j > i that shares one of those rows gets matrix[i][j] = matrix[j][i] = 1 -- a byte store of the
//                          constant 1, checked first so that the same pair found in many words is written once or a few
//                          times.  A circuit whose selectors are disjoint costs ONE pass over the bitmaps; a word where t
//                          selectors overlap costs t further passes over that word's column of the bitmaps.
//   k_selectors_combine    one lane per row of one output column: the value of the member whose bit is set, else zero, as two
//                          16-byte stores; consecutive lanes write consecutive cells.  The members (selector index and
//                          32-byte value, in the column's form already) are kernel arguments, so the plan is copied when the
//                          launch is queued.  32 bytes written per row against 4 bytes read per member and 32 rows.
#include "selectors.hpp"

#include <string>
#include <vector>

namespace h2 {

namespace {

__global__ void __launch_bounds__(SEL_THREADS) k_selectors_mark(const MarkSeg* __restrict__ segs,
                                                                const uint64_t* __restrict__ prefix, uint32_t nseg,
                                                                uint64_t total, uint32_t* __restrict__ bitmaps, uint32_t words) {
    __shared__ uint64_t sh_prefix[SEL_CHUNK + 1];
    const uint64_t begin = (uint64_t)blockIdx.x * SEL_CHUNK;
    uint32_t lo = 0, hi = nseg;  // prefix[lo] <= begin < prefix[hi]
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (prefix[mid] <= begin)
            lo = mid;
        else
            hi = mid;
    }
    // the segments of this chunk's cells are lo .. lo + SEL_CHUNK - 1 at most (every segment has a cell)
    const uint32_t have = min((uint32_t)SEL_CHUNK + 1, nseg + 1 - lo);
    for (uint32_t i = threadIdx.x; i < have; i += SEL_THREADS) sh_prefix[i] = prefix[lo + i];
    __syncthreads();
#pragma unroll
    for (uint32_t t = 0; t < SEL_CHUNK / SEL_THREADS; t++) {
        const uint64_t c = begin + t * SEL_THREADS + threadIdx.x;
        if (c >= total) break;
        uint32_t a = 0, b = have - 1;  // sh_prefix[a] <= c < sh_prefix[b]
        while (b - a > 1) {
            const uint32_t mid = a + (b - a) / 2;
            if (sh_prefix[mid] <= c)
                a = mid;
            else
                b = mid;
        }
        const MarkSeg sg = segs[lo + a];
        const uint64_t row = (uint64_t)sg.first + (c - sh_prefix[a]) * sg.stride;  // below n <= 2^31: validated on the host
        atomicOr(bitmaps + ((size_t)sg.selector * words + (row >> 5)), 1u << (row & 31));
    }
}

__global__ void __launch_bounds__(SEL_THREADS) k_selectors_conflicts(const uint32_t* __restrict__ bitmaps, uint32_t count,
                                                                     uint32_t words, uint32_t last_mask,
                                                                     uint8_t* __restrict__ matrix) {
    const uint32_t w = blockIdx.x * SEL_THREADS + threadIdx.x;
    if (w >= words) return;
    const uint32_t mask = w == words - 1 ? last_mask : 0xffffffffu;  // rows at and beyond n do not exist
    const uint32_t* column = bitmaps + w;
    uint32_t seen = 0, twice = 0;
    for (uint32_t s = 0; s < count; s++) {
        const uint32_t x = column[(size_t)s * words] & mask;
        twice |= seen & x;
        seen |= x;
    }
    if (!twice) return;
    for (uint32_t i = 0; i + 1 < count; i++) {
        const uint32_t xi = column[(size_t)i * words] & twice;
        if (!xi) continue;
        for (uint32_t j = i + 1; j < count; j++) {
            if (!(column[(size_t)j * words] & xi)) continue;
            uint8_t* up = matrix + ((size_t)i * count + j);
            uint8_t* down = matrix + ((size_t)j * count + i);
            if (!*up) *up = 1;
            if (!*down) *down = 1;
        }
    }
}

template <bool FIRST>
__global__ void __launch_bounds__(SEL_THREADS) k_selectors_combine(const CombineArgs args, const uint32_t* __restrict__ bitmaps,
                                                                   uint32_t words, uint32_t n, Fr* __restrict__ dst) {
    const uint32_t row = blockIdx.x * SEL_THREADS + threadIdx.x;
    if (row >= n) return;
    bool hit;
    const Fr v = selectors_row_value(args, bitmaps, words, row, hit);
    if (FIRST || hit) fp_store(dst + row, v);  // a later slice of a long combination leaves the other rows as they are
}

bool below_modulus(const uint64_t* v) {
    for (int i = 3; i >= 0; i--) {
        const uint64_t m = ((uint64_t)FrParams::MOD[2 * i + 1] << 32) | FrParams::MOD[2 * i];
        if (v[i] != m) return v[i] < m;
    }
    return false;
}

CombineArgs combine_args(const h2_selector_member* members, size_t count) {
    CombineArgs a;
    a.count = (uint32_t)count;
    for (size_t m = 0; m < SEL_MEMBERS; m++) {
        a.selector[m] = m < count ? members[m].selector : 0;
        for (int l = 0; l < 8; l++)
            a.value[m].l[l] = m < count ? (uint32_t)(members[m].value[l / 2] >> (32 * (l & 1))) : 0;
    }
    return a;
}

}  // namespace

size_t selectors_mark_scratch_bytes(size_t count) {
    // the device segment table, then the count + 1 prefix sums; both 16-byte aligned
    return count * sizeof(MarkSeg) + ((count + 1) * sizeof(uint64_t) + 15) / 16 * 16;
}

static const char* selectors_shape(size_t n, size_t num_selectors, const void* bitmaps) {
    if (n == 0 || n > ((size_t)1 << 31)) return "n must be between 1 and 2^31";
    if (num_selectors == 0 || num_selectors >= ((size_t)1 << 16)) return "the number of selectors must be between 1 and 2^16 - 1";
    if (!bitmaps || ((uintptr_t)bitmaps & 3)) return "the bitmaps must be a 4-byte aligned pointer";
    return nullptr;
}

const char* selectors_mark_validate(const h2_selector_segment* segs, size_t count, size_t n, size_t num_selectors,
                                    const void* d_bitmaps, const void* d_scratch, size_t scratch_bytes) {
    if (count == 0) return nullptr;
    if (!segs) return "null segment table";
    if (const char* what = selectors_shape(n, num_selectors, d_bitmaps)) return what;
    if (count >= ((size_t)1 << 31)) return "2^31 segments or more";
    if (!d_scratch || ((uintptr_t)d_scratch & 15)) return "the scratch must be a 16-byte aligned device pointer";
    if (scratch_bytes < selectors_mark_scratch_bytes(count)) return "the scratch is smaller than h2_selectors_mark_scratch_bytes";
    uint64_t total = 0;
    for (size_t s = 0; s < count; s++) {
        const h2_selector_segment& g = segs[s];
        if (g.selector >= num_selectors) return "a segment names a selector that does not exist";
        if (g.count == 0) continue;
        if (g.stride == 0 || g.stride > n) return "a segment's stride must be between 1 and n";
        // the last row marked, first + (count - 1) stride, must be below n (no product here can overflow: all are <= n^2 <= 2^62)
        if (g.first_row >= n || g.count > n || (g.count - 1) * g.stride >= n - g.first_row) return "a segment reaches beyond row n - 1";
        total += g.count;
    }
    if ((total + SEL_CHUNK - 1) / SEL_CHUNK >= ((uint64_t)1 << 31)) return "too many cells for one launch";
    return nullptr;
}

const char* selectors_conflicts_validate(const void* d_bitmaps, size_t num_selectors, size_t n, const void* d_matrix) {
    if (const char* what = selectors_shape(n, num_selectors, d_bitmaps)) return what;
    if (!d_matrix) return "null conflict matrix";
    return nullptr;
}

const char* selectors_combine_validate(const h2_selector_column* plan, size_t columns, const h2_selector_member* members,
                                       size_t num_members, size_t n, size_t num_selectors, const void* bitmaps, uint32_t out_form) {
    if (columns == 0) return nullptr;
    if (!plan) return "null plan";
    if (const char* what = selectors_shape(n, num_selectors, bitmaps)) return what;
    if (out_form != H2_PLACE_OUT_CANONICAL && out_form != H2_PLACE_OUT_MONTGOMERY) return "unknown output form";
    if (num_members && !members) return "null member table";
    for (size_t c = 0; c < columns; c++) {
        const h2_selector_column& col = plan[c];
        if (!col.dst || ((uintptr_t)col.dst & 15)) return "an output column must be a 16-byte aligned pointer";
        if (col.first_member > num_members || col.num_members > num_members - col.first_member)
            return "a column's members lie outside the member table";
        for (size_t m = 0; m < col.num_members; m++) {
            const h2_selector_member& mem = members[col.first_member + m];
            if (mem.selector >= num_selectors) return "a member names a selector that does not exist";
            if (!below_modulus(mem.value)) return "a member's value is not below the modulus";
        }
    }
    return nullptr;
}

int selectors_mark_launch(const h2_selector_segment* segs, size_t count, size_t n, uint32_t* d_bitmaps, void* d_scratch,
                          hipStream_t stream) {
    std::vector<MarkSeg> table;
    std::vector<uint64_t> prefix;
    table.reserve(count);
    prefix.reserve(count + 1);
    uint64_t total = 0;
    for (size_t s = 0; s < count; s++) {
        const h2_selector_segment& g = segs[s];
        if (g.count == 0) continue;  // the kernel relies on it: every segment of its table has a cell
        table.push_back(MarkSeg{g.selector, (uint32_t)g.first_row, (uint32_t)g.stride, 0});
        prefix.push_back(total);
        total += g.count;
    }
    if (total == 0) return H2_OK;
    prefix.push_back(total);
    const size_t nseg = table.size();
    MarkSeg* d_table = (MarkSeg*)d_scratch;
    uint64_t* d_prefix = (uint64_t*)((char*)d_scratch + nseg * sizeof(MarkSeg));
    H2_HIP(hipMemcpyAsync(d_table, table.data(), nseg * sizeof(MarkSeg), hipMemcpyHostToDevice, stream));
    H2_HIP(hipMemcpyAsync(d_prefix, prefix.data(), (nseg + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, stream));
    H2_HIP(hipStreamSynchronize(stream));  // the staging vectors die with this frame
    const unsigned blocks = (unsigned)((total + SEL_CHUNK - 1) / SEL_CHUNK);
    hipLaunchKernelGGL(k_selectors_mark, dim3(blocks), dim3(SEL_THREADS), 0, stream, d_table, d_prefix, (uint32_t)nseg, total,
                       d_bitmaps, (uint32_t)selectors_words(n));
    H2_HIP(hipGetLastError());
    return H2_OK;
}

int selectors_conflicts_launch(const uint32_t* d_bitmaps, size_t num_selectors, size_t n, uint8_t* d_matrix, hipStream_t stream) {
    const uint32_t words = (uint32_t)selectors_words(n);
    const uint32_t last_mask = (n & 31) ? (1u << (n & 31)) - 1 : 0xffffffffu;
    H2_HIP(hipMemsetAsync(d_matrix, 0, num_selectors * num_selectors, stream));
    if (num_selectors < 2) return H2_OK;
    hipLaunchKernelGGL(k_selectors_conflicts, dim3((words + SEL_THREADS - 1) / SEL_THREADS), dim3(SEL_THREADS), 0, stream,
                       d_bitmaps, (uint32_t)num_selectors, words, last_mask, d_matrix);
    H2_HIP(hipGetLastError());
    return H2_OK;
}

int selectors_combine_launch(const h2_selector_column* plan, size_t columns, const h2_selector_member* members, size_t n,
                             const uint32_t* d_bitmaps, hipStream_t stream) {
    const uint32_t words = (uint32_t)selectors_words(n);
    const dim3 grid((unsigned)((n + SEL_THREADS - 1) / SEL_THREADS));
    for (size_t c = 0; c < columns; c++) {
        const h2_selector_column& col = plan[c];
        size_t done = 0;
        do {  // a column without members is a column of zeros
            const size_t take = col.num_members - done < SEL_MEMBERS ? col.num_members - done : SEL_MEMBERS;
            const CombineArgs args = combine_args(members + col.first_member + done, take);
            if (done == 0)
                hipLaunchKernelGGL(k_selectors_combine<true>, grid, dim3(SEL_THREADS), 0, stream, args, d_bitmaps, words,
                                   (uint32_t)n, (Fr*)col.dst);
            else
                hipLaunchKernelGGL(k_selectors_combine<false>, grid, dim3(SEL_THREADS), 0, stream, args, d_bitmaps, words,
                                   (uint32_t)n, (Fr*)col.dst);
            H2_HIP(hipGetLastError());
            done += take;
        } while (done < col.num_members);
    }
    return H2_OK;
}

void selectors_combine_host(const h2_selector_column* plan, size_t columns, const h2_selector_member* members, size_t n,
                            const uint32_t* bitmaps) {
    const size_t words = selectors_words(n);
    for (size_t c = 0; c < columns; c++) {
        const h2_selector_column& col = plan[c];
        size_t done = 0;
        do {
            const size_t take = col.num_members - done < SEL_MEMBERS ? col.num_members - done : SEL_MEMBERS;
            const CombineArgs args = combine_args(members + col.first_member + done, take);
            for (size_t row = 0; row < n; row++) {
                bool hit;
                const Fr v = selectors_row_value(args, bitmaps, words, (uint32_t)row, hit);
                if (done == 0 || hit) ((Fr*)col.dst)[row] = v;
            }
            done += take;
        } while (done < col.num_members);
    }
}

}  // namespace h2
