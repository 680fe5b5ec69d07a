// place.hip -- the circuit front end's device assembly: one launch places a whole batch of assigned cell ranges ("segments")
// into resident columns.
//
// A region of a circuit assigns RANGES of cells (synthesis.py: Region.assign_advice / assign_fixed); the ranges of many regions
// are gathered into one segment table and placed here, so that neither the number of regions nor their sizes decide how the
// machine is filled: the work is split by CELLS.  Cell c of the batch (0 <= c < total, the segments laid end to end) belongs
// to the segment s with prefix[s] <= c < prefix[s + 1], prefix being the running sums of the counts.  A workgroup takes
// PLACE_CHUNK consecutive cells; empty segments are dropped on the host, so those cells belong to at most PLACE_CHUNK
// consecutive segments, whose prefix sums the workgroup stages in LDS (8 KiB) after ONE binary search of the whole table;
// every lane then finds its segment in LDS.  Consecutive lanes take consecutive cells, hence consecutive source cells and --
// inside a stride-1 segment -- consecutive 32-byte destination cells: a wave's two 16-byte stores cover 2 KiB contiguously.
// A source cell is 32 bytes (canonical), 8 bytes (compact: the value, below 2^64) or one 32-byte cell for the whole segment
// (broadcast).  The batch is written canonical, or as Montgomery residues (fp_to_mont: keygen's fixed columns).
//
// Two segments of one call must not write the same cell: which of them wins is not defined.  The front end flushes its
// queue before it queues a segment that overlaps a queued one ("Synthesising a circuit").
#include "place.hpp"

#include <string>
#include <vector>

namespace h2 {

namespace {

__device__ __forceinline__ Fr place_source(const PlaceSeg& sg, uint64_t i) {
    if (sg.form == H2_PLACE_FORM_COMPACT) {
        const uint64_t x = ((const uint64_t*)sg.src)[i];
        Fr v = fp_zero<FrParams>();
        v.l[0] = (uint32_t)x;
        v.l[1] = (uint32_t)(x >> 32);
        return v;
    }
    return fp_load((const Fr*)sg.src + (sg.form == H2_PLACE_FORM_BROADCAST ? 0 : i));
}

template <bool MONT>
__global__ void __launch_bounds__(PLACE_THREADS) k_cells_place(const PlaceSeg* __restrict__ segs,
                                                               const uint64_t* __restrict__ prefix, uint32_t nseg,
                                                               uint64_t total) {
    __shared__ uint64_t sh_prefix[PLACE_CHUNK + 1];
    const uint64_t begin = (uint64_t)blockIdx.x * PLACE_CHUNK;
    // lo = the segment of cell `begin`: the largest s with prefix[s] <= begin (uniform over the workgroup)
    uint32_t lo = 0, hi = nseg;  // prefix[lo] <= begin < prefix[hi]
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (prefix[mid] <= begin)
            lo = mid;
        else
            hi = mid;
    }
    // the segments of this chunk's cells are lo .. lo + PLACE_CHUNK - 1 at most (every segment has a cell)
    const uint32_t have = min((uint32_t)PLACE_CHUNK + 1, nseg + 1 - lo);
    for (uint32_t i = threadIdx.x; i < have; i += PLACE_THREADS) sh_prefix[i] = prefix[lo + i];
    __syncthreads();
#pragma unroll
    for (uint32_t t = 0; t < PLACE_CHUNK / PLACE_THREADS; t++) {
        const uint64_t c = begin + t * PLACE_THREADS + threadIdx.x;
        if (c >= total) break;
        uint32_t a = 0, b = have - 1;  // sh_prefix[a] <= c < sh_prefix[b]
        while (b - a > 1) {
            const uint32_t mid = a + (b - a) / 2;
            if (sh_prefix[mid] <= c)
                a = mid;
            else
                b = mid;
        }
        const PlaceSeg sg = segs[lo + a];
        const uint64_t i = c - sh_prefix[a];
        Fr v = place_source(sg, i);
        if (MONT) v = fp_to_mont(v);
        fp_store((Fr*)sg.dst + ((uint64_t)sg.first + i * sg.stride), v);
    }
}

}  // namespace

size_t cells_place_scratch_bytes(size_t count) {
    // the device segment table, then the count + 1 prefix sums; both 16-byte aligned
    return count * sizeof(PlaceSeg) + ((count + 1) * sizeof(uint64_t) + 15) / 16 * 16;
}

const char* cells_place_validate(const h2_place_segment* segs, size_t count, size_t n, uint32_t out_form, const void* d_scratch,
                                 size_t scratch_bytes) {
    if (count == 0) return nullptr;
    if (!segs) return "null segment table";
    if (n == 0 || n > ((size_t)1 << 31)) return "n must be between 1 and 2^31";
    if (count >= ((size_t)1 << 31)) return "2^31 segments or more";
    if (out_form != H2_PLACE_OUT_CANONICAL && out_form != H2_PLACE_OUT_MONTGOMERY) return "unknown output form";
    if (!d_scratch || ((uintptr_t)d_scratch & 15)) return "the scratch must be a 16-byte aligned device pointer";
    if (scratch_bytes < cells_place_scratch_bytes(count)) return "the scratch is smaller than h2_cells_place_scratch_bytes";
    uint64_t total = 0;
    for (size_t s = 0; s < count; s++) {
        const h2_place_segment& g = segs[s];
        if (g.form > H2_PLACE_FORM_BROADCAST) return "unknown segment form";
        if (g.count == 0) continue;
        if (!g.dst || ((uintptr_t)g.dst & 15)) return "a destination column must be a 16-byte aligned device pointer";
        if (!g.src || ((uintptr_t)g.src & (g.form == H2_PLACE_FORM_COMPACT ? 7 : 15))) return "a misaligned or null source";
        if (g.stride == 0 || g.stride > n) return "a segment's stride must be between 1 and n";
        // the last row written, first + (count - 1) stride, must be below n (no product here can overflow: all are <= n^2 <= 2^62)
        if (g.first_row >= n || g.count > n || (g.count - 1) * g.stride >= n - g.first_row) return "a segment reaches beyond row n - 1";
        total += g.count;
    }
    if ((total + PLACE_CHUNK - 1) / PLACE_CHUNK >= ((uint64_t)1 << 31)) return "too many cells for one launch";
    return nullptr;
}

int cells_place_launch(const h2_place_segment* segs, size_t count, size_t n, uint32_t out_form, void* d_scratch,
                       hipStream_t stream) {
    (void)n;
    std::vector<PlaceSeg> table;
    std::vector<uint64_t> prefix;
    table.reserve(count);
    prefix.reserve(count + 1);
    uint64_t total = 0;
    for (size_t s = 0; s < count; s++) {
        const h2_place_segment& g = segs[s];
        if (g.count == 0) continue;  // the kernel relies on it: every segment of its table has a cell
        table.push_back(PlaceSeg{(uint64_t)(uintptr_t)g.dst, (uint64_t)(uintptr_t)g.src, (uint32_t)g.first_row, (uint32_t)g.stride,
                                 g.form, 0});
        prefix.push_back(total);
        total += g.count;
    }
    if (total == 0) return H2_OK;
    prefix.push_back(total);
    const size_t nseg = table.size();
    PlaceSeg* d_table = (PlaceSeg*)d_scratch;
    uint64_t* d_prefix = (uint64_t*)((char*)d_scratch + nseg * sizeof(PlaceSeg));
    H2_HIP(hipMemcpyAsync(d_table, table.data(), nseg * sizeof(PlaceSeg), hipMemcpyHostToDevice, stream));
    H2_HIP(hipMemcpyAsync(d_prefix, prefix.data(), (nseg + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, stream));
    H2_HIP(hipStreamSynchronize(stream));  // the staging vectors die with this frame
    const unsigned blocks = (unsigned)((total + PLACE_CHUNK - 1) / PLACE_CHUNK);
    if (out_form == H2_PLACE_OUT_MONTGOMERY)
        hipLaunchKernelGGL(k_cells_place<true>, dim3(blocks), dim3(PLACE_THREADS), 0, stream, d_table, d_prefix, (uint32_t)nseg,
                           total);
    else
        hipLaunchKernelGGL(k_cells_place<false>, dim3(blocks), dim3(PLACE_THREADS), 0, stream, d_table, d_prefix, (uint32_t)nseg,
                           total);
    H2_HIP(hipGetLastError());
    return H2_OK;
}

}  // namespace h2
