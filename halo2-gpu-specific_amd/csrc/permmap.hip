// permmap.hip -- the permutation argument's cycle mapping, built from the copy constraints on the device.
// The reference keeps the cycles as it is handed the copies one by one (plonk/permutation/keygen.rs:49-110) and then sorts
// every cycle by (column, row) and points each cell at its successor, the last at the first (:113-145).  That result is a
// function of the PARTITION the copies induce, so it is built here in data-parallel phases, with cells numbered
// id = column position * n + row (ascending id = ascending (column, row)):
//   k_pm_union    per copy, in a scattered order: bounds check (the lowest bad copy index by atomicMin), both cells flagged in
//                 a bitmap, and a lock-free union: find both roots with path halving, hook the LARGER root under the SMALLER by
//                 compare-and-swap.  parent[x] <= x always, so every tree's root is its smallest cell whoever won which race.
//   k_pm_count / pm_scan / k_pm_emit     the flagged cells, compacted in ascending id order (M <= 2 x copies)
//   k_pm_labels   label = root of each compacted cell (the flatten, over the M cells that can have a parent at all)
//   k_pm_hist / pm_scan / k_pm_scatter   stable LSD radix sort of the (label, id) pairs by label, 8 bits a pass: every cycle
//                 becomes a contiguous run that starts with its label and ascends in id
//   k_pm_identity, k_pm_succ   every cell maps to itself; entry i of a run maps to entry i + 1, the last one to the label
// Every phase that orders anything is a scan or a stable rank: no atomic's arrival order reaches the output.
//
// The eight XCDs of the chip have private L2s and a plain load may return, for a whole launch, a word another workgroup has
// since replaced.  While parent[] is being changed it is therefore read with agent-scope atomic loads and written with
// agent-scope atomics only, and a failed compare-and-swap continues from the value IT returned.  No workgroup waits for
// another; launch boundaries order the phases.  Every loop over parent[] is bounded by `cells` steps: an overrun (which the
// invariant parent[x] <= x excludes) ends the walk and makes the status H2_PERM_MAPPING_INTERNAL.
#include "permmap.hpp"

namespace h2 {

namespace {

using u32 = uint32_t;
constexpr u32 PM_NONE = 0xffffffffu;
constexpr u32 PM_SCAN_TILE = 256 * 16;        // pm_scan: 16 words a lane
constexpr u32 PM_WORDS_PER_BLOCK = 256;       // bitmap words (32 cells each) a workgroup of the compaction takes
constexpr u32 PM_ROUNDS = PM_SORT_TILE / 256;
constexpr int MISC_M = 0, MISC_OVERRUN = 1;   // words of the misc block: the number of flagged cells, the overrun flag
static_assert(PM_SORT_TILE % 256 == 0, "a sort tile is whole rounds of 256 entries");

size_t round64(size_t words) { return (words + 63) & ~(size_t)63; }
size_t ceil_div(size_t a, size_t b) { return (a + b - 1) / b; }

// u32 words of the partial sums of every level of pm_scan over n words
size_t scan_tmp_words(size_t n) {
    size_t total = 0;
    for (;;) {
        const size_t tiles = n ? ceil_div(n, PM_SCAN_TILE) : 1;
        total += round64(tiles);
        if (tiles == 1) return total;
        n = tiles;
    }
}

struct PmLayout {
    size_t cells, words, count_blocks, mmax, sort_blocks, hist_words;
    size_t parent, bits, tot, keys[2], vals[2], hist, scan, misc, total;   // offsets in u32 words
    u32 passes;
};

PmLayout pm_layout(size_t n_columns, size_t n, size_t copies) {
    PmLayout l;
    l.cells = n_columns * n;
    l.words = ceil_div(l.cells, 32);
    l.count_blocks = ceil_div(l.words, PM_WORDS_PER_BLOCK);
    l.mmax = copies > l.cells / 2 ? l.cells : 2 * copies;
    l.sort_blocks = ceil_div(l.mmax, PM_SORT_TILE);
    l.hist_words = 256 * l.sort_blocks;
    u32 bits = 0;
    while (bits < 32 && ((l.cells - 1) >> bits)) bits++;
    l.passes = (bits + 7) / 8;
    size_t at = 0;
    auto take = [&](size_t words) {
        const size_t here = at;
        at += round64(words);
        return here;
    };
    l.misc = take(64);
    l.parent = take(l.cells);
    l.bits = take(l.words);
    l.tot = take(l.count_blocks);
    for (int i = 0; i < 2; i++) l.keys[i] = take(l.mmax), l.vals[i] = take(l.mmax);
    l.hist = take(l.hist_words);
    l.scan = take(scan_tmp_words(l.hist_words > l.count_blocks ? l.hist_words : l.count_blocks));
    l.total = at;
    return l;
}

__device__ __forceinline__ u32 pm_ald(const u32* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The root of x's tree, with path halving: every visited cell is pointed at its grandparent.  The new parent is an
// ancestor and smaller, so atomicMin keeps parent[] falling whatever else is written to the word meanwhile.  x strictly
// falls from step to step; `limit` steps is the bound a broken invariant would hit.
__device__ __forceinline__ u32 pm_find(u32* parent, u32 x, u32 limit, u32* overrun) {
    for (u32 step = 0; step <= limit; step++) {
        const u32 p = pm_ald(&parent[x]);
        if (p == x) return x;
        const u32 gp = pm_ald(&parent[p]);
        if (gp == p) return p;
        __hip_atomic_fetch_min(&parent[x], gp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        x = gp;
    }
    __hip_atomic_store(overrun, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return x;
}

__global__ void __launch_bounds__(256) k_pm_iota(u32* parent, u32 cells) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < cells; i += (size_t)gridDim.x * 256) parent[i] = (u32)i;
}

// flags cell id.  The bit is looked at first: a star sends every copy's left cell to ONE word, and atomics on one address run
// one after the other (2^21 of them: 24 ms); once the bit is seen set nothing is sent.  Bits are only ever set, so the look
// can only err towards one atomic more.
__device__ __forceinline__ void pm_flag(u32* bits, u32 id) {
    u32* word = &bits[id >> 5];
    const u32 bit = 1u << (id & 31);
    if (!(pm_ald(word) & bit)) atomicOr(word, bit);
}

// Thread t takes the copies in the order of a Weyl sequence: groups of four copies (one 64-byte line), group (t / 4) * mult
// mod 2^bits with mult / 2^bits ~ the golden ratio, so the groups in flight at any moment lie evenly over the whole list.
// Copies that arrive SORTED along a chain (cell i copied to cell i + 1, in order) would otherwise be hooked all at once into a
// path as long as the threads in flight, and every later find would walk it (measured at k = 20: 22 - 186 ms against 0.3 ms
// for random copies); spread out, neighbouring pieces of a chain meet as trees of similar size and the paths stay short.
__global__ void __launch_bounds__(256) k_pm_union(const uint4* copies, size_t count, size_t slots, uint64_t mult, uint64_t mask,
                                                  u32 n_columns, u32 n, u32* parent, u32* bits, u32* status, u32* misc,
                                                  u32 limit) {
    u32* overrun = misc + MISC_OVERRUN;
    for (size_t t = (size_t)blockIdx.x * 256 + threadIdx.x; t < slots; t += (size_t)gridDim.x * 256) {
        const size_t i = ((((uint64_t)(t >> 2) * mult) & mask) << 2) | (t & 3);
        if (i >= count) continue;
        const uint4 c = copies[i];
        if (c.x >= n_columns || c.z >= n_columns || c.y >= n || c.w >= n) {
            atomicMin(&status[1], i < PM_NONE - 1 ? (u32)i : PM_NONE - 1);
            continue;
        }
        const u32 a = c.x * n + c.y, b = c.z * n + c.w;
        pm_flag(bits, a);
        if (a == b) continue;
        pm_flag(bits, b);
        u32 u = pm_find(parent, a, limit, overrun), v = pm_find(parent, b, limit, overrun);
        for (u32 tries = 0; u != v; tries++) {
            if (tries >= limit) {
                __hip_atomic_store(overrun, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                break;
            }
            const u32 hi = u > v ? u : v, lo = u > v ? v : u;
            u32 seen = hi;
            if (__hip_atomic_compare_exchange_strong(&parent[hi], &seen, lo, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                     __HIP_MEMORY_SCOPE_AGENT))
                break;
            // hi had been hooked already: `seen` is the parent it was given (below hi).  Go on from there.
            u = pm_find(parent, seen, limit, overrun);
            v = pm_find(parent, lo, limit, overrun);
        }
    }
}

// exclusive prefix of v over the 256 lanes of a workgroup and the workgroup's total; s_wave: 4 words of LDS, free again
// after the next __syncthreads()
__device__ __forceinline__ u32 pm_block_excl(u32 v, u32* s_wave, u32& total) {
    const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    u32 incl = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const u32 o = (u32)__shfl_up((int)incl, off, 64);
        if ((int)lane >= off) incl += o;
    }
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    u32 before = 0;
    total = 0;
#pragma unroll
    for (int w = 0; w < 4; w++) {
        if (w < (int)wave) before += s_wave[w];
        total += s_wave[w];
    }
    return before + incl - v;
}

// data[0, n) -> its exclusive prefix sums tile by tile, in place; sums[tile] = the tile's total
__global__ void __launch_bounds__(256) k_pm_scan_tile(u32* data, size_t n, u32* sums, u32* total_out) {
    __shared__ u32 s_wave[4];
    const size_t base = (size_t)blockIdx.x * PM_SCAN_TILE + (size_t)threadIdx.x * 16;
    u32 q[16], sum = 0;
#pragma unroll
    for (int i = 0; i < 16; i++) {
        q[i] = base + i < n ? data[base + i] : 0;
        sum += q[i];
    }
    u32 total;
    u32 run = pm_block_excl(sum, s_wave, total);
#pragma unroll
    for (int i = 0; i < 16; i++) {
        if (base + i < n) data[base + i] = run;
        run += q[i];
    }
    if (threadIdx.x == 0) {
        sums[blockIdx.x] = total;
        if (total_out && gridDim.x == 1) *total_out = total;
    }
}

__global__ void __launch_bounds__(256) k_pm_scan_add(u32* data, size_t n, const u32* sums) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) data[i] += sums[i / PM_SCAN_TILE];
}

u32 grid_for(size_t items, size_t per_block, size_t cap = (size_t)1 << 24) {
    const size_t blocks = ceil_div(items, per_block);
    return (u32)(blocks < 1 ? 1 : blocks > cap ? cap : blocks);
}

// exclusive prefix sums of data[0, n) in place (u32, wrapping); *total_out = the sum of all of them
void pm_scan(u32* data, size_t n, u32* tmp, u32* total_out, hipStream_t stream) {
    const size_t tiles = n ? ceil_div(n, PM_SCAN_TILE) : 1;
    hipLaunchKernelGGL(k_pm_scan_tile, dim3((u32)tiles), dim3(256), 0, stream, data, n, tmp, total_out);
    if (tiles == 1) return;
    pm_scan(tmp, tiles, tmp + round64(tiles), total_out, stream);
    hipLaunchKernelGGL(k_pm_scan_add, dim3(grid_for(n, 256)), dim3(256), 0, stream, data, n, (const u32*)tmp);
}

__global__ void __launch_bounds__(256) k_pm_count(const u32* bits, size_t words, u32* tot) {
    __shared__ u32 s_wave[4];
    const size_t w = (size_t)blockIdx.x * PM_WORDS_PER_BLOCK + threadIdx.x;
    u32 total;
    pm_block_excl(w < words ? (u32)__popc(bits[w]) : 0, s_wave, total);
    if (threadIdx.x == 0) tot[blockIdx.x] = total;
}

// tot: the exclusive prefix of k_pm_count's totals.  ids[0, M) = the flagged cells in ascending order.
__global__ void __launch_bounds__(256) k_pm_emit(const u32* bits, size_t words, const u32* tot, u32* ids, size_t mmax) {
    __shared__ u32 s_wave[4];
    const size_t w = (size_t)blockIdx.x * PM_WORDS_PER_BLOCK + threadIdx.x;
    u32 word = w < words ? bits[w] : 0, total;
    size_t pos = (size_t)tot[blockIdx.x] + pm_block_excl((u32)__popc(word), s_wave, total);
    while (word) {
        const u32 bit = (u32)__ffs((int)word) - 1;
        if (pos < mmax) ids[pos] = (u32)(w * 32 + bit);
        pos++;
        word &= word - 1;
    }
}

__global__ void __launch_bounds__(256) k_pm_labels(const u32* ids, u32* labels, u32* parent, u32* misc, u32 limit) {
    const u32 M = misc[MISC_M];
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < M) labels[i] = pm_find(parent, ids[i], limit, misc + MISC_OVERRUN);
}

// hist[digit * blocks + block] = entries of the block's tile with that digit (zeros for a tile past M)
__global__ void __launch_bounds__(256) k_pm_hist(const u32* keys, u32* hist, const u32* misc, u32 shift, u32 blocks) {
    __shared__ u32 s_h[256];
    const u32 M = misc[MISC_M];
    const size_t start = (size_t)blockIdx.x * PM_SORT_TILE;
    s_h[threadIdx.x] = 0;
    __syncthreads();
    for (u32 r = 0; r < PM_ROUNDS; r++) {
        const size_t i = start + r * 256 + threadIdx.x;
        if (i < M) atomicAdd(&s_h[(keys[i] >> shift) & 255], 1u);
    }
    __syncthreads();
    hist[(size_t)threadIdx.x * blocks + blockIdx.x] = s_h[threadIdx.x];
}

// offs: the exclusive prefix of hist.  Entry i of the tile goes behind every entry of a lower digit, every entry of its digit
// in an earlier tile and every entry of its digit earlier in this tile: the tile is ranked 256 entries a round, a wave's
// lanes of one digit found by eight ballots and ranked by lane, the waves by their order, the rounds by a running count.
__global__ void __launch_bounds__(256) k_pm_scatter(const u32* keys_in, const u32* vals_in, u32* keys_out, u32* vals_out,
                                                    const u32* offs, const u32* misc, u32 shift, u32 blocks) {
    __shared__ u32 s_run[256];
    __shared__ u32 s_w[4][256];
    const u32 M = misc[MISC_M];
    const size_t start = (size_t)blockIdx.x * PM_SORT_TILE;
    if (start >= M) return;
    const u32 t = threadIdx.x, lane = t & 63, wave = t >> 6;
    s_run[t] = offs[(size_t)t * blocks + blockIdx.x];
    for (u32 r = 0; r < PM_ROUNDS; r++) {
        const size_t i = start + r * 256 + t;
        const bool valid = i < M;
        const u32 key = valid ? keys_in[i] : 0, val = valid ? vals_in[i] : 0;
        const u32 d = (key >> shift) & 255;
#pragma unroll
        for (int w = 0; w < 4; w++) s_w[w][t] = 0;
        __syncthreads();
        uint64_t same = __ballot(valid);
#pragma unroll
        for (int bit = 0; bit < 8; bit++) {
            const bool set = (d >> bit) & 1;
            const uint64_t b = __ballot(set);
            same &= set ? b : ~b;
        }
        const u32 rank = (u32)__popcll(same & (((uint64_t)1 << lane) - 1));
        if (valid && rank == 0) s_w[wave][d] = (u32)__popcll(same);
        __syncthreads();
        if (valid) {
            u32 pos = s_run[d] + rank;
            for (u32 w = 0; w < wave; w++) pos += s_w[w][d];
            if (pos < M) keys_out[pos] = key, vals_out[pos] = val;
        }
        __syncthreads();
        s_run[t] += s_w[0][t] + s_w[1][t] + s_w[2][t] + s_w[3][t];
    }
}

__global__ void __launch_bounds__(256) k_pm_identity(u32* map_col, u32* map_row, u32 cells, u32 n) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < cells; i += (size_t)gridDim.x * 256) {
        const u32 col = (u32)i / n;
        map_col[i] = col;
        map_row[i] = (u32)i - col * n;
    }
}

__global__ void __launch_bounds__(256) k_pm_succ(const u32* labels, const u32* ids, const u32* misc, u32 cells, u32 n,
                                                 u32* map_col, u32* map_row) {
    const u32 M = misc[MISC_M];
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= M) return;
    const u32 id = ids[i], label = labels[i];
    const u32 succ = i + 1 < M && labels[i + 1] == label ? ids[i + 1] : label;
    if (id >= cells) return;
    const u32 col = succ / n;
    map_col[id] = col;
    map_row[id] = succ - col * n;
}

__global__ void k_pm_finish(u32* status, const u32* misc) {
    status[0] = misc[MISC_OVERRUN] ? H2_PERM_MAPPING_INTERNAL
                : status[1] != PM_NONE ? H2_PERM_MAPPING_OUT_OF_BOUNDS : H2_PERM_MAPPING_OK;
}

}  // namespace

size_t permutation_mapping_scratch_bytes(size_t n_columns, size_t n, size_t copies) {
    if (n_columns == 0 || n == 0 || n > 0xffffffffull / n_columns) return 0;
    return pm_layout(n_columns, n, copies).total * sizeof(u32);
}

const char* permutation_mapping_validate(const uint32_t* d_copies, size_t copies, size_t n_columns, size_t n,
                                         const uint32_t* d_map_col, const uint32_t* d_map_row, const uint32_t* d_status,
                                         const void* d_scratch, size_t scratch_bytes) {
    if (!d_map_col) return "d_map_col is null";
    if (!d_map_row) return "d_map_row is null";
    if (!d_status) return "d_status is null";
    if (!d_scratch) return "d_scratch is null";
    if (copies && !d_copies) return "d_copies is null";
    if (n_columns == 0) return "n_columns is zero";
    if (n == 0) return "n is zero";
    if (n > 0xffffffffull / n_columns) return "n_columns * n is 2^32 or more";
    if ((uintptr_t)d_copies % 16 || (uintptr_t)d_scratch % 16 || (uintptr_t)d_map_col % 4 || (uintptr_t)d_map_row % 4 ||
        (uintptr_t)d_status % 4)
        return "d_copies / d_map_col / d_map_row / d_status / d_scratch is misaligned";
    if (scratch_bytes < permutation_mapping_scratch_bytes(n_columns, n, copies))
        return "scratch too small (h2_permutation_mapping_scratch_bytes)";
    return nullptr;
}

int permutation_mapping_launch(const uint32_t* d_copies, size_t copies, size_t n_columns, size_t n, uint32_t* d_map_col,
                               uint32_t* d_map_row, uint32_t* d_status, void* d_scratch, float* phase_ms, hipStream_t stream) {
    const PmLayout l = pm_layout(n_columns, n, copies);
    u32* const base = (u32*)d_scratch;
    u32 *misc = base + l.misc, *parent = base + l.parent, *bits = base + l.bits, *tot = base + l.tot, *hist = base + l.hist,
        *scan = base + l.scan;
    u32 *keys[2] = {base + l.keys[0], base + l.keys[1]}, *vals[2] = {base + l.vals[0], base + l.vals[1]};
    const u32 cells = (u32)l.cells, n32 = (u32)n;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    struct Events {
        hipEvent_t* e;
        ~Events() {
            for (int i = 0; i < 4; i++)
                if (e[i]) (void)hipEventDestroy(e[i]);
        }
    } events{ev};
    auto mark = [&](int i) {
        if (!phase_ms) return;
        H2_HIP(hipEventCreate(&ev[i]));
        H2_HIP(hipEventRecord(ev[i], stream));
    };
    mark(0);
    H2_HIP(hipMemsetAsync(d_status, 0xff, H2_PERM_MAPPING_STATUS_WORDS * sizeof(u32), stream));
    H2_HIP(hipMemsetAsync(misc, 0, 64 * sizeof(u32), stream));
    int cur = 0;
    if (copies) {
        // components
        H2_HIP(hipMemsetAsync(bits, 0, l.words * sizeof(u32), stream));
        hipLaunchKernelGGL(k_pm_iota, dim3(grid_for(l.cells, 256, 1 << 16)), dim3(256), 0, stream, parent, cells);
        u32 group_bits = 0;
        while (((size_t)1 << group_bits) < ceil_div(copies, 4)) group_bits++;
        const uint64_t mask = ((uint64_t)1 << group_bits) - 1;
        const uint64_t mult = group_bits ? (0x9E3779B97F4A7C15ull >> (64 - group_bits)) | 1 : 1;   // odd: a bijection mod 2^bits
        const size_t slots = (size_t)4 << group_bits;
        hipLaunchKernelGGL(k_pm_union, dim3(grid_for(slots, 256, 1 << 20)), dim3(256), 0, stream, (const uint4*)d_copies, copies,
                           slots, mult, mask, (u32)n_columns, n32, parent, bits, d_status, misc, cells);
        mark(1);
        // compaction, labels, sort
        hipLaunchKernelGGL(k_pm_count, dim3((u32)l.count_blocks), dim3(256), 0, stream, (const u32*)bits, l.words, tot);
        pm_scan(tot, l.count_blocks, scan, misc + MISC_M, stream);
        hipLaunchKernelGGL(k_pm_emit, dim3((u32)l.count_blocks), dim3(256), 0, stream, (const u32*)bits, l.words,
                           (const u32*)tot, vals[0], l.mmax);
        hipLaunchKernelGGL(k_pm_labels, dim3(grid_for(l.mmax, 256)), dim3(256), 0, stream, (const u32*)vals[0], keys[0], parent,
                           misc, cells);
        const u32 blocks = (u32)l.sort_blocks;
        for (u32 pass = 0; pass < l.passes && blocks; pass++, cur ^= 1) {
            hipLaunchKernelGGL(k_pm_hist, dim3(blocks), dim3(256), 0, stream, (const u32*)keys[cur], hist, (const u32*)misc,
                               8 * pass, blocks);
            pm_scan(hist, l.hist_words, scan, nullptr, stream);
            hipLaunchKernelGGL(k_pm_scatter, dim3(blocks), dim3(256), 0, stream, (const u32*)keys[cur], (const u32*)vals[cur],
                               keys[cur ^ 1], vals[cur ^ 1], (const u32*)hist, (const u32*)misc, 8 * pass, blocks);
        }
    } else {
        mark(1);
    }
    mark(2);
    // successors
    hipLaunchKernelGGL(k_pm_identity, dim3(grid_for(l.cells, 256, 1 << 16)), dim3(256), 0, stream, d_map_col, d_map_row, cells, n32);
    if (copies)
        hipLaunchKernelGGL(k_pm_succ, dim3(grid_for(l.mmax, 256)), dim3(256), 0, stream, (const u32*)keys[cur],
                           (const u32*)vals[cur], (const u32*)misc, cells, n32, d_map_col, d_map_row);
    hipLaunchKernelGGL(k_pm_finish, dim3(1), dim3(1), 0, stream, d_status, (const u32*)misc);
    mark(3);
    H2_HIP(hipGetLastError());
    if (phase_ms) {
        H2_HIP(hipEventSynchronize(ev[3]));
        for (int i = 0; i < 3; i++) H2_HIP(hipEventElapsedTime(&phase_ms[i], ev[i], ev[i + 1]));
    }
    return H2_OK;
}

}  // namespace h2
