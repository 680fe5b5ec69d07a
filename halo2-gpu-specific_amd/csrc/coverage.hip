// coverage.hip -- the cells each region assigned, kept on the device as bits, and MockProver's CellNotAssigned read off them.
//
// A plane is one (region, column) pair over the rows the region spans in that column; all planes lie end to end in one u32
// array (coverage.hpp; DESIGN.md 3b, "Checking assignments").  The front end queues every assignment and every
// enable_selector of a synthesis and flushes them here in two launches:
//
//   k_coverage_mark   sets the bit of every assigned cell.  The grid has two parts that share the code of the prefix search
//                     (as k_selectors_mark: a workgroup takes COV_CHUNK consecutive units and stages the prefix sums they
//                     can fall under in LDS).  The first part splits the stride-1 segments by WORDS: a lane builds the mask
//                     of one word of its segment and issues one atomicOr for up to 32 cells; consecutive lanes take
//                     consecutive words, so a wave's atomics cover 256 contiguous bytes.  The second part splits the strided
//                     segments by CELLS, one atomicOr each.  Every bit is set by atomicOr, so two segments that share a word
//                     -- the ends of two runs, a strided segment over a run -- agree.
//   k_coverage_check  splits the uses by enabled ROWS with the same search.  A lane takes one row of one use, skips it when
//                     an earlier use of the same region and gate holds the row already, and walks the gate's queries:
//                     cell_row = (row + n + rotation) mod n, the plane's range, the bit.  The loop runs while ANY lane of the
//                     wave has a query left, so that every lane reaches check_append in every round (append.hpp: one
//                     agent-scope atomic per wave and round that has a failure).
#include "common.hpp"

#include "append.hpp"
#include "coverage.hpp"

namespace h2 {

namespace {

// The segment of unit `begin + ...`: stages prefix[lo .. lo + have) in LDS, where prefix[lo] <= begin, and returns lo.
__device__ __forceinline__ uint32_t stage_prefix(const uint64_t* __restrict__ prefix, uint32_t nseg, uint64_t begin,
                                                 uint64_t* sh_prefix, uint32_t& have) {
    uint32_t lo = 0, hi = nseg;  // prefix[lo] <= begin < prefix[hi]
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (prefix[mid] <= begin)
            lo = mid;
        else
            hi = mid;
    }
    // the segments of this chunk's units are lo .. lo + COV_CHUNK - 1 at most (every segment has a unit)
    have = min((uint32_t)COV_CHUNK + 1, nseg + 1 - lo);
    for (uint32_t i = threadIdx.x; i < have; i += COV_THREADS) sh_prefix[i] = prefix[lo + i];
    __syncthreads();
    return lo;
}

// the a with sh_prefix[a] <= u < sh_prefix[a + 1]
__device__ __forceinline__ uint32_t find_segment(const uint64_t* sh_prefix, uint32_t have, uint64_t u) {
    uint32_t a = 0, b = have - 1;
    while (b - a > 1) {
        const uint32_t mid = a + (b - a) / 2;
        if (sh_prefix[mid] <= u)
            a = mid;
        else
            b = mid;
    }
    return a;
}

__global__ void __launch_bounds__(COV_THREADS) k_coverage_mark(const CovSeg* __restrict__ segs,
                                                               const uint64_t* __restrict__ word_prefix, uint32_t by_word,
                                                               uint64_t words, uint32_t word_blocks,
                                                               const uint64_t* __restrict__ cell_prefix, uint32_t by_cell,
                                                               uint64_t cells, uint32_t* __restrict__ bits) {
    __shared__ uint64_t sh_prefix[COV_CHUNK + 1];
    const bool wordwise = blockIdx.x < word_blocks;  // uniform over the workgroup
    const uint64_t begin = (uint64_t)(wordwise ? blockIdx.x : blockIdx.x - word_blocks) * COV_CHUNK;
    const uint64_t total = wordwise ? words : cells;
    if (!wordwise) segs += by_word;
    uint32_t have;
    const uint32_t lo = stage_prefix(wordwise ? word_prefix : cell_prefix, wordwise ? by_word : by_cell, begin, sh_prefix, have);
#pragma unroll
    for (uint32_t t = 0; t < COV_CHUNK / COV_THREADS; t++) {
        const uint64_t u = begin + t * COV_THREADS + threadIdx.x;
        if (u >= total) break;
        const uint32_t a = find_segment(sh_prefix, have, u);
        const CovSeg sg = segs[lo + a];
        const uint64_t off = u - sh_prefix[a];
        if (wordwise) {
            const uint64_t w = (sg.first_bit >> 5) + off;  // inside the segment's plane: validated on the host
            atomicOr(bits + w, coverage_word_mask(sg.first_bit, sg.count, w));
        } else {
            const uint64_t bit = sg.first_bit + off * sg.stride;
            atomicOr(bits + (bit >> 5), 1u << (bit & 31));
        }
    }
}

__global__ void __launch_bounds__(COV_THREADS) k_coverage_check(const h2_coverage_plane* __restrict__ planes,
                                                                const h2_coverage_query* __restrict__ queries,
                                                                const h2_coverage_use* __restrict__ uses,
                                                                const uint32_t* __restrict__ earlier,
                                                                const uint64_t* __restrict__ prefix, uint32_t nuse, uint64_t total,
                                                                uint64_t n, const uint32_t* __restrict__ bits,
                                                                unsigned long long* count, h2_check_record* out,
                                                                unsigned long long cap) {
    __shared__ uint64_t sh_prefix[COV_CHUNK + 1];
    const uint64_t begin = (uint64_t)blockIdx.x * COV_CHUNK;
    uint32_t have;
    const uint32_t lo = stage_prefix(prefix, nuse, begin, sh_prefix, have);
    for (uint32_t t = 0; t < COV_CHUNK / COV_THREADS; t++) {  // no lane leaves before its wave's last append
        const uint64_t u = begin + t * COV_THREADS + threadIdx.x;
        h2_coverage_use use = {};
        uint64_t row = 0;
        uint32_t nq = 0;
        if (u < total) {
            const uint32_t a = find_segment(sh_prefix, have, u);
            use = uses[lo + a];
            row = use.first_row + (u - sh_prefix[a]) * use.stride;  // below n: validated on the host
            if (!coverage_row_repeated(uses, earlier, use, row)) nq = use.num_queries;
        }
        for (uint32_t q = 0; __any(q < nq); q++) {
            bool fail = false;
            uint32_t cell_row = 0;
            if (q < nq) fail = !coverage_assigned(planes, bits, queries[use.first_query + q], row, n, cell_row);
            check_append(fail, H2_CHECK_CELL, use.gate << 16 | q, use.region, cell_row, count, out, cap);
        }
    }
}

// the device address of `bytes` copied to the scratch at `at`, which advances by them rounded up to 16
template <class T>
const T* stage_table(const T* host, size_t count, char*& at, hipStream_t stream) {
    const T* d = (const T*)at;
    if (count) H2_HIP(hipMemcpyAsync(at, host, count * sizeof(T), hipMemcpyHostToDevice, stream));
    at += (count * sizeof(T) + 15) / 16 * 16;
    return d;
}

}  // namespace

int coverage_mark_launch(const h2_coverage_plane* planes, const h2_coverage_segment* segs, size_t count, uint32_t* d_bits,
                         void* d_scratch, hipStream_t stream) {
    const CovMarkPlan plan = coverage_mark_plan(planes, segs, count);
    if (plan.segs.empty()) return H2_OK;
    const uint64_t words = plan.by_word() ? plan.word_prefix.back() : 0, cells = plan.by_cell() ? plan.cell_prefix.back() : 0;
    char* at = (char*)d_scratch;
    const CovSeg* d_segs = stage_table(plan.segs.data(), plan.segs.size(), at, stream);
    const uint64_t* d_word_prefix = stage_table(plan.word_prefix.data(), plan.word_prefix.size(), at, stream);
    const uint64_t* d_cell_prefix = stage_table(plan.cell_prefix.data(), plan.cell_prefix.size(), at, stream);
    H2_HIP(hipStreamSynchronize(stream));  // the staging vectors die with this frame
    const unsigned word_blocks = (unsigned)((words + COV_CHUNK - 1) / COV_CHUNK);
    const unsigned cell_blocks = (unsigned)((cells + COV_CHUNK - 1) / COV_CHUNK);
    hipLaunchKernelGGL(k_coverage_mark, dim3(word_blocks + cell_blocks), dim3(COV_THREADS), 0, stream, d_segs, d_word_prefix,
                       (uint32_t)plan.by_word(), words, word_blocks, d_cell_prefix, (uint32_t)plan.by_cell(), cells, d_bits);
    H2_HIP(hipGetLastError());
    return H2_OK;
}

int coverage_check_launch(const h2_coverage_plane* planes, size_t num_planes, const h2_coverage_query* queries, size_t num_queries,
                          const h2_coverage_use* uses, size_t num_uses, const uint32_t* earlier, size_t num_earlier, size_t n,
                          const uint32_t* d_bits, void* d_scratch, uint64_t* d_count, h2_check_record* d_records, size_t cap,
                          hipStream_t stream) {
    // the uses that have a row, their `earlier` entries renumbered to match (an earlier use without rows holds none)
    std::vector<h2_coverage_use> table;
    std::vector<uint64_t> prefix;
    std::vector<uint32_t> slot(num_uses, H2_COVERAGE_NO_PLANE), kept;
    uint64_t total = 0;
    for (size_t i = 0; i < num_uses; i++) {
        if (uses[i].count == 0) continue;
        h2_coverage_use u = uses[i];
        u.first_earlier = (uint32_t)kept.size();
        for (uint32_t e = 0; e < uses[i].num_earlier; e++) {
            const uint32_t to = slot[earlier[uses[i].first_earlier + e]];
            if (to != H2_COVERAGE_NO_PLANE) kept.push_back(to);
        }
        u.num_earlier = (uint32_t)kept.size() - u.first_earlier;
        slot[i] = (uint32_t)table.size();
        table.push_back(u);
        prefix.push_back(total);
        total += u.count;
    }
    if (total == 0) return H2_OK;
    prefix.push_back(total);
    char* at = (char*)d_scratch;
    const h2_coverage_plane* d_planes = stage_table(planes, num_planes, at, stream);
    const h2_coverage_query* d_queries = stage_table(queries, num_queries, at, stream);
    const h2_coverage_use* d_uses = stage_table(table.data(), table.size(), at, stream);
    const uint32_t* d_earlier = stage_table(kept.data(), kept.size(), at, stream);
    const uint64_t* d_prefix = stage_table(prefix.data(), prefix.size(), at, stream);
    H2_HIP(hipStreamSynchronize(stream));  // the staging vectors die with this frame
    const unsigned blocks = (unsigned)((total + COV_CHUNK - 1) / COV_CHUNK);
    hipLaunchKernelGGL(k_coverage_check, dim3(blocks), dim3(COV_THREADS), 0, stream, d_planes, d_queries, d_uses, d_earlier,
                       d_prefix, (uint32_t)table.size(), total, (uint64_t)n, d_bits, (unsigned long long*)d_count, d_records,
                       (unsigned long long)cap);
    H2_HIP(hipGetLastError());
    return H2_OK;
}

}  // namespace h2
