// msm_kernels.hip -- Pippenger multi-scalar multiplication over BN254 G1 for gfx950: the pipeline.
//
// Replaces ec-gpu-gen's `SingleMultiexpKernel::multiexp_bound` (called from
// halo2_proofs/src/arithmetic.rs:334-367) ; the CPU twin that fixes the
// semantics is `multiexp_serial` (arithmetic.rs:20-108): result = sum_i scalar_i * base_i.
// The output is a group element, so window size, digit form and summation order are free
// (results are compared after affine normalisation, like the reference's own `==`).
//
// Pipeline (one stream, no host round trip until the final 1-2 KB read-back):
//   k_sample      64 scalars -> host: does one value dominate the column? (it then gets its own window, see k_digits)
//   k_digits      scalar -> canonical (one Montgomery mul), signed digits of BALANCED width (c or c - 1 bits), keys, and
//                 the histogram of (window, bucket >> lo_bits) partitions; narrow columns: rows cut into ranges = windows
//   k_scan_parts / k_partition / k_bucket_sort   two-level counting sort of (point index, sign) by (window, bucket); over a
//                 shifted-base table k_partition is k_part_a + k_part_b: two passes that reorder their tile in LDS first
//   k_acc_slice   one thread per fixed-size SLICE of the sorted list: exactly S mixed XYZZ
//                 additions per lane whatever the bucket sizes are; a partial sum is emitted at
//                 every bucket boundary inside the slice                              [hot loop]
//   k_finish      a QUAD per bucket folds its slice partials (<= 32), heavier buckets are queued
//   k_finish_mid  queued buckets with <= 512 partials: one wave each (strided fold + shuffle tree)
//   k_finish_heavy / _heavy2   the rest: ceil(P / 256) workgroups per bucket (strided fold + quad tree), then their fold
//   k_reduce      per window: sum_b (b+1) * B_b by chunked running sums on quads + small scalar mul + quad tree; the last
//                 workgroup of a window folds its groups
//   host          W window sums -> Horner (W additions, max_bits + 1 doublings); the dominant scalar's multiplication
// Everything after k_acc_slice runs on quads (ec_quad.hpp): four lanes per chain of dependent additions.
// Slicing the *sorted list* evenly (instead of giving each bucket to a thread) keeps every lane of
// the hot loop busy for any digit distribution: Poisson-sized buckets of a uniform MSM as well as
// the skewed columns real witnesses have (boolean / small-valued columns put most points into a
// handful of buckets -- SURVEY.md section 7 "hard parts (ii)").  The partial of (bucket b, slice s)
// lives in slot b + s: along the sorted list either b or s grows at every emission, so slots are
// unique, a bucket's partials are contiguous, and no second prefix sum is needed.
//
// This file: the pipeline's kernels and msm_enqueue, which starts one planned launch.  What is decided -- the shape, the
// partition, the finish and reduce forms, every grid -- is decided in msm_plan.cpp; the drivers are in msm.hip.
#include <initializer_list>
#include <type_traits>
#include <vector>

#include "ec_quad.hpp"
#include "msm.hpp"
#include "msm_kernels.hpp"

namespace h2 {

static_assert(sizeof(Fr) == FR_BYTES && sizeof(Affine) == AFFINE_BYTES && sizeof(XYZZ) == XYZZ_BYTES,
              "msm_plan.hpp lays the scratch out for these sizes");

// ---------------------------------------------------------------- k_digits
// One thread per scalar (grid-stride): Montgomery -> canonical, signed c-bit digits, keys[w][i] =
// bucket | sign (KEY_INVALID for a zero digit), and the histogram of (window, bucket >> lo_bits)
// partitions, privatised in LDS and flushed once per workgroup.
//
// Dominant scalar.  Committed columns are often constant over most rows -- a grand-product / grand-sum column over
// the padding rows of a circuit, a default value -- and Pippenger would pay W additions for each of those rows.  When
// sampling finds a value v on >= 1/4 of the rows (`hot_on`), the rows holding v contribute no digits at all; instead
// they enter bucket 0 of one extra window (index W), whose sum E = sum of their points is multiplied by v once on the
// host: sum_i s_i P_i = sum_{s_i != v} s_i P_i + v * E.  One addition per such row instead of W.
extern __shared__ __attribute__((aligned(16))) uint32_t h2_msm_smem[];

// Fused multi-column form (col_scalars != nullptr): blockIdx.y is the column; its scalars, its dominant value and its
// flag come from the tables, its W + 1 windows start at window blockIdx.y * (W + 1), and `np` counts the partitions of
// ONE column -- the rest of the pipeline just sees more windows over the same bases.
__global__ void __launch_bounds__(256) k_digits(const Fr* scalars, size_t n, uint32_t c, uint32_t W, uint32_t nb,
                                                uint32_t max_bits, uint32_t lo_bits, uint32_t hi_bits, uint32_t np,
                                                uint32_t* keys, uint32_t* pcount, int hot_on, Fr hot,
                                                const Fr* const* col_scalars, const Fr* col_hot, uint64_t col_hot_mask,
                                                uint32_t range_shift, uint32_t R, uint32_t wfull, uint32_t tabmode,
                                                size_t block_rows_end, uint8_t* block_flags) {
    // tabmode (shifted-base table): every digit's bucket belongs to window 0, the dominant-scalar window is window 1
    // block_rows_end (dominant value over whole blocks): rows below it lie in complete blocks of BLOCK_ROWS bases whose
    // SUMS are tabulated next to the bases -- the padding rows of a circuit make a grand-product column one value over
    // millions of consecutive rows: a block of 256 rows all holding the dominant value enters its bucket as ONE point
    // (row 0 of the block carries BLOCK_KEY, the other 255 nothing) instead of 256.
    bool hot_slot = hot_on != 0;  // does key array W exist?
    if (col_scalars != nullptr) {
        const uint32_t col = blockIdx.y, Wc = np >> hi_bits;  // windows (= key arrays) per column: W or W + 1
        scalars = col_scalars[col];
        hot_on = (int)((col_hot_mask >> col) & 1);
        if (hot_on) hot = fp_load(col_hot + col);
        hot_slot = Wc > W;
        keys += (size_t)col * Wc * n;
        pcount += (size_t)col * np;
    }
    uint32_t* hist = h2_msm_smem;
    for (uint32_t k = threadIdx.x; k < np; k += blockDim.x) hist[k] = 0;
    __syncthreads();
    for (size_t base = (size_t)blockIdx.x * blockDim.x; base < n; base += (size_t)gridDim.x * blockDim.x) {
        const size_t i = base + threadIdx.x;
        const bool valid = i < n;
        const Fr raw = valid ? fp_load(scalars + i) : fp_zero<FrParams>();
        if (hot_slot) {  // uniform branch; a fused column of more than two windows always owns the extra window
            const bool is_hot = valid && hot_on && fp_eq(raw, hot);
            bool whole_block = false;
            if (block_rows_end) whole_block = __syncthreads_and(is_hot ? 1 : 0) != 0 && base + BLOCK_ROWS <= block_rows_end;
            if (whole_block) {
                // the W digit keys of these rows are neither written nor read: k_partition skips flagged blocks
                if (threadIdx.x == 0) {
                    atomicAdd(&hist[(tabmode ? 1u : R * W) << hi_bits], 1u);
                    block_flags[base / BLOCK_ROWS] = 1;
                }
                keys[(size_t)W * n + i] = threadIdx.x == 0 ? BLOCK_KEY : KEY_INVALID;
                continue;
            } else {
                const uint64_t m = __ballot(is_hot);
                if (m && (int)(threadIdx.x & 63) == __ffsll((unsigned long long)m) - 1)
                    atomicAdd(&hist[(tabmode ? 1u : R * W) << hi_bits], (uint32_t)__popcll(m));  // partition 0 of the extra window
                if (valid) keys[(size_t)W * n + i] = is_hot ? 0u : KEY_INVALID;
            }
            if (is_hot) {
                for (uint32_t w = 0; w < W; w++) keys[(size_t)w * n + i] = KEY_INVALID;
                continue;
            }
        }
        if (!valid) continue;
        Fr s = fp_from_mont(raw);  // canonical little-endian integer (to_repr, arithmetic.rs:21)
        // keep only the low max_bits bits (multiexp_bound contract)
#pragma unroll
        for (int k = 0; k < 8; k++) {
            int lo_bit = 32 * k;
            if ((int)max_bits <= lo_bit)
                s.l[k] = 0;
            else if ((int)max_bits < lo_bit + 32)
                s.l[k] &= (1u << (max_bits - lo_bit)) - 1;
        }
        uint64_t buf = 0;
        int nbits = 0;
        uint32_t w = 0, carry = 0;
        const uint32_t vw0 = (uint32_t)(i >> range_shift) * W;  // first window of this row's range
        const uint32_t wstep = tabmode ? 0u : 1u;
        auto emit = [&](uint32_t raw, uint32_t cw) {  // cw: width of window w
            raw += carry;
            uint32_t neg = 0, mag = raw;
            if (raw > (1u << (cw - 1))) {  // digit = raw - 2^cw  (negative)
                mag = (1u << cw) - raw;
                neg = SIGN_BIT;
                carry = 1;
            } else {
                carry = 0;
            }
            uint32_t out = KEY_INVALID;
            if (mag != 0) {
                uint32_t bucket = mag - 1;
                out = bucket | neg;
                atomicAdd(&hist[((vw0 + w * wstep) << hi_bits) + (bucket >> lo_bits)], 1u);
            }
            keys[(size_t)w * n + i] = out;
            w++;
        };
#pragma unroll
        for (int k = 0; k < 8; k++) {
            buf |= (uint64_t)s.l[k] << nbits;
            nbits += 32;
            for (;;) {
                const uint32_t cw = c - (w >= wfull ? 1u : 0u);
                if (nbits < (int)cw || w >= W) break;
                emit((uint32_t)buf & ((1u << cw) - 1), cw);
                buf >>= cw;
                nbits -= cw;
            }
        }
        while (w < W) {
            const uint32_t cw = c - (w >= wfull ? 1u : 0u);
            emit((uint32_t)buf & ((1u << cw) - 1), cw);
            buf >>= cw;
        }
    }
    __syncthreads();
    for (uint32_t k = threadIdx.x; k < np; k += blockDim.x) {
        uint32_t v = hist[k];
        if (v) atomicAdd(&pcount[k], v);
    }
}

// ---------------------------------------------------------------- k_scan_parts (single workgroup)
__device__ __forceinline__ uint32_t block_exclusive_scan_256(uint32_t v, uint32_t* sh, uint32_t* total) {
    // inclusive scan inside each wave64 with shuffles, then across the 4 waves through LDS
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t x = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        uint32_t y = __shfl_up(x, off, 64);
        if (lane >= (uint32_t)off) x += y;
    }
    if (lane == 63) sh[wave] = x;
    __syncthreads();
    uint32_t base = 0;
    for (uint32_t w = 0; w < wave; w++) base += sh[w];
    *total = sh[0] + sh[1] + sh[2] + sh[3];
    __syncthreads();
    return base + x - v;
}

// the same over the SORT_T = 1024 threads (16 waves) of k_bucket_sort
__device__ __forceinline__ uint32_t block_exclusive_scan_1024(uint32_t v, uint32_t* sh, uint32_t* total) {
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t x = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        uint32_t y = __shfl_up(x, off, 64);
        if (lane >= (uint32_t)off) x += y;
    }
    if (lane == 63) sh[wave] = x;
    __syncthreads();
    uint32_t base = 0, all = 0;
#pragma unroll
    for (uint32_t w = 0; w < 16; w++) {
        const uint32_t t = sh[w];
        if (w < wave) base += t;
        all += t;
    }
    *total = all;
    __syncthreads();
    return base + x - v;
}

// pbase[p] = sum_{p' < p} pcount[p'] (p <= np), pcursor = pbase, starts[nbt] = total entries
__global__ void __launch_bounds__(256) k_scan_parts(const uint32_t* pcount, uint32_t np, uint32_t* pbase,
                                                    uint32_t* pcursor, uint32_t* starts, uint32_t nbt) {
    __shared__ uint32_t sh[4];
    __shared__ uint32_t carry;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (uint32_t c0 = 0; c0 < np + 1; c0 += 256) {
        uint32_t idx = c0 + threadIdx.x;
        uint32_t v = idx < np ? pcount[idx] : 0;
        uint32_t total;
        uint32_t ex = block_exclusive_scan_256(v, sh, &total);
        if (idx <= np) {
            pbase[idx] = carry + ex;
            pcursor[idx] = carry + ex;
        }
        __syncthreads();
        if (threadIdx.x == 0) carry += total;
        __syncthreads();
    }
    if (threadIdx.x == 0) starts[nbt] = carry;
}

// ---------------------------------------------------------------- k_partition (sort pass A)
// Workgroup = PART_T consecutive keys of one window.  Local ranks come from LDS atomics; each
// non-empty partition costs ONE global atomic per workgroup (space reservation), and the entries of a
// partition land in a contiguous run, so the 8-byte stores of a workgroup merge into full lines.
// TILE = entries per workgroup (256 threads x TILE / 256): 2048 for the windowed shape (256 partitions per window: runs of
// 8); 16384 over a table, whose 2^13 partitions would otherwise cost a global atomic for nearly every entry
template <uint32_t TILE>
__global__ void __launch_bounds__(256) k_partition(const uint32_t* keys, size_t n, uint32_t lo_bits, uint32_t hi_bits,
                                                   uint32_t* pcursor, uint2* tmp, uint32_t range_shift, uint32_t W,
                                                   uint32_t R, uint32_t tab_stride, const uint8_t* block_flags, uint32_t w_first) {
    uint32_t* cnt = h2_msm_smem;               // 2^hi_bits local counters, then the reserved bases
    const uint32_t nparts = 1u << hi_bits, w = blockIdx.y + w_first;
    // window of these PART_T rows: ranges are multiples of PART_T rows; key array W (if present) is the dominant-scalar
    // window, which is not cut into ranges.  Shifted-base table (tab_stride != 0): digit array w feeds window 0 with the
    // points of table level w; the dominant-scalar array feeds window 1 with the bases themselves (level 0)
    uint32_t vw = (R > 1) ? (w == W ? R * W : (uint32_t)(((size_t)blockIdx.x * TILE) >> range_shift) * W + w) : w;
    uint32_t level_base = 0;
    if (tab_stride) {
        vw = (w == W) ? 1u : 0u;
        level_base = (w == W) ? 0u : w * tab_stride;
    }
    for (uint32_t k = threadIdx.x; k < nparts; k += blockDim.x) cnt[k] = 0;
    const uint32_t ITEMS = TILE / 256;
    uint32_t key[TILE / 256], rank[TILE / 256];
    const size_t i0 = (size_t)blockIdx.x * TILE;
    // All of a lane's keys are requested before the first one is used (the loop used to wait for each key, and for the
    // block flag in front of it, in turn: 2 x ITEMS memory latencies per tile).  Rows beyond n read the last row and are
    // discarded; the flags of the tile's blocks (one per 256 rows, the same for every lane) go through LDS.
    uint32_t* sflag = cnt + nparts;   // ITEMS words: block k of the tile is flagged
    if (threadIdx.x < ITEMS) {
        const size_t row0 = i0 + (size_t)threadIdx.x * 256;   // BLOCK_ROWS == 256 == the stride of k
        sflag[threadIdx.x] = (block_flags != nullptr && w != W && row0 < n) ? block_flags[row0 / BLOCK_ROWS] : 0u;
    }
#pragma unroll
    for (uint32_t k = 0; k < ITEMS; k++) {
        const size_t i = i0 + k * 256 + threadIdx.x;
        key[k] = keys[(size_t)w * n + (i < n ? i : n - 1)];
    }
    __syncthreads();
#pragma unroll
    for (uint32_t k = 0; k < ITEMS; k++) {
        const size_t i = i0 + k * 256 + threadIdx.x;
        // rows of a block that entered the dominant-value bucket as one point have no digit keys (k_digits)
        if (i >= n || sflag[k] != 0) key[k] = KEY_INVALID;
        rank[k] = 0;
        if (key[k] != KEY_INVALID) rank[k] = atomicAdd(&cnt[(key[k] & ~(SIGN_BIT | BLOCK_KEY)) >> lo_bits], 1u);
    }
    __syncthreads();
    // reserve the tile's run in every partition; a lane owns nparts / 256 of them and its reservations go out eight at a
    // time (one returning atomic at a time was up to 32 round trips to memory per tile)
    for (uint32_t k0 = threadIdx.x; k0 < nparts; k0 += 8 * blockDim.x) {
        uint32_t v[8], b[8];
#pragma unroll
        for (uint32_t j = 0; j < 8; j++) v[j] = (k0 + j * blockDim.x < nparts) ? cnt[k0 + j * blockDim.x] : 0u;
#pragma unroll
        for (uint32_t j = 0; j < 8; j++) {
            const uint32_t k = k0 + j * blockDim.x;
            b[j] = 0;
            if (TILE >= 16384) {   // nearly every partition receives entries from a tile this large: no branch, no wait
                if (k < nparts) b[j] = atomicAdd(&pcursor[(vw << hi_bits) + k], v[j]);
            } else if (v[j]) {
                b[j] = atomicAdd(&pcursor[(vw << hi_bits) + k], v[j]);
            }
        }
#pragma unroll
        for (uint32_t j = 0; j < 8; j++)
            if (k0 + j * blockDim.x < nparts) cnt[k0 + j * blockDim.x] = b[j];
    }
    __syncthreads();
#pragma unroll
    for (uint32_t k = 0; k < ITEMS; k++) {
        if (key[k] == KEY_INVALID) continue;
        uint32_t bucket = key[k] & ~(SIGN_BIT | BLOCK_KEY);
        const uint32_t row = (uint32_t)(i0 + k * 256 + threadIdx.x);
        // a row that stands for its whole block of BLOCK_ROWS bases (k_digits) refers to the block's tabulated sum
        const uint32_t i = (key[k] & BLOCK_KEY) ? BLOCK_INDEX0 + row / BLOCK_ROWS : level_base + row;
        tmp[cnt[bucket >> lo_bits] + rank[k]] = make_uint2(i | (key[k] & SIGN_BIT), bucket & ((1u << lo_bits) - 1));
    }
}

// ---------------------------------------------------------------- two-level partition over a table
// k_partition leaves 2 x 10^8 separate 8-byte stores at 2^24 (a tile of 16384 keys has two entries per partition, written
// by different lanes at different times).  Here the 2^hi_bits partitions are reached in two passes of 2^a_bits groups and
// 2^b_bits partitions per group; each pass reorders its tile in LDS first, so a lane's neighbours write neighbouring
// entries and a run leaves the CU as whole cache lines.  Entries between the passes: (reference | sign, bucket).
// aux (after the entries of tmpa): cursor_a[G], tile_start[G + 1] (tiles of pass B per group, prefix sums).
__global__ void __launch_bounds__(PARTA_GROUPS_MAX) k_part_init(const uint32_t* pbase, uint32_t a_bits, uint32_t b_bits,
                                                                uint32_t* cursor_a, uint32_t* tile_start) {
    __shared__ uint32_t tiles[PARTA_GROUPS_MAX];
    const uint32_t G = 1u << a_bits, a = threadIdx.x;
    if (a < G) {
        const uint32_t gs = pbase[a << b_bits], ge = pbase[(a + 1) << b_bits];
        cursor_a[a] = gs;
        tiles[a] = (ge - gs + PART_AB_T - 1) / PART_AB_T;
    }
    __syncthreads();
    if (a == 0) {
        uint32_t run = 0;
        for (uint32_t k = 0; k < G; k++) {
            tile_start[k] = run;
            run += tiles[k];
        }
        tile_start[G] = run;
    }
}

// reorder the tile's `total` staged entries group by group and write them out: consecutive staged entries of one group go
// to consecutive addresses
__device__ __forceinline__ void part_ab_flush(const uint2* stage, uint32_t total, const uint32_t* loff, const uint32_t* gbase,
                                              uint32_t shift, uint32_t mask, bool strip, uint32_t lo_mask, uint2* out) {
    for (uint32_t idx = threadIdx.x; idx < total; idx += 256) {
        uint2 e = stage[idx];
        const uint32_t g = (e.y >> shift) & mask;
        const uint32_t dst = gbase[g] + (idx - loff[g]);
        if (strip) e.y &= lo_mask;
        out[dst] = e;
    }
}

// exclusive scan of hist[0..bins) (bins <= 128, two waves) -> loff, total; reserves the tile's run in every group (every
// lane of the workgroup calls this: it contains a barrier)
__device__ __forceinline__ void part_ab_reserve(const uint32_t* hist, uint32_t* loff, uint32_t* gbase, uint32_t bins,
                                                uint32_t* cursors, uint32_t* total_out, uint32_t* wsum) {
    const uint32_t t = threadIdx.x, lane = t & 63, wave = t >> 6;
    uint32_t v = 0, x = 0;
    if (t < 128) {
        v = t < bins ? hist[t] : 0u;
        x = v;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const uint32_t y = __shfl_up(x, off, 64);
            if (lane >= (uint32_t)off) x += y;
        }
        if (lane == 63) wsum[wave] = x;
    }
    __syncthreads();
    if (t < 128) {
        const uint32_t base = wave ? wsum[0] : 0u;
        if (t < bins) {
            loff[t] = base + x - v;
            gbase[t] = v ? atomicAdd(&cursors[t], v) : 0u;
        }
        if (t == 127) *total_out = base + x;
    }
}

__global__ void __launch_bounds__(256) k_part_a(const uint32_t* keys, size_t n, uint32_t lo_bits, uint32_t b_bits,
                                                uint32_t a_bits, uint32_t* cursor_a, uint2* tmpa, uint32_t tab_stride,
                                                const uint8_t* block_flags) {
    constexpr uint32_t ITEMS = PART_AB_T / 256;
    __shared__ uint32_t hist[PARTA_GROUPS_MAX], loff[PARTA_GROUPS_MAX], gbase[PARTA_GROUPS_MAX], sflag[ITEMS], total_sh, wsum[2];
    uint2* stage = (uint2*)h2_msm_smem;  // PART_AB_T entries
    const uint32_t w = blockIdx.y, G = 1u << a_bits;
    const size_t i0 = (size_t)blockIdx.x * PART_AB_T;
    const uint32_t level_base = w * tab_stride;
    if (threadIdx.x < G) hist[threadIdx.x] = 0;
    if (threadIdx.x < ITEMS) {
        const size_t row0 = i0 + (size_t)threadIdx.x * 256;
        sflag[threadIdx.x] = (block_flags != nullptr && row0 < n) ? block_flags[row0 / BLOCK_ROWS] : 0u;
    }
    uint32_t key[ITEMS], rank[ITEMS];
#pragma unroll
    for (uint32_t k = 0; k < ITEMS; k++) {
        const size_t i = i0 + k * 256 + threadIdx.x;
        key[k] = keys[(size_t)w * n + (i < n ? i : n - 1)];
    }
    __syncthreads();
#pragma unroll
    for (uint32_t k = 0; k < ITEMS; k++) {
        const size_t i = i0 + k * 256 + threadIdx.x;
        if (i >= n || sflag[k] != 0) key[k] = KEY_INVALID;
        rank[k] = 0;
        if (key[k] != KEY_INVALID) rank[k] = atomicAdd(&hist[((key[k] & ~(SIGN_BIT | BLOCK_KEY)) >> lo_bits) >> b_bits], 1u);
    }
    __syncthreads();
    part_ab_reserve(hist, loff, gbase, G, cursor_a, &total_sh, wsum);
    __syncthreads();
#pragma unroll
    for (uint32_t k = 0; k < ITEMS; k++) {
        if (key[k] == KEY_INVALID) continue;
        const uint32_t bucket = key[k] & ~(SIGN_BIT | BLOCK_KEY);
        const uint32_t row = (uint32_t)(i0 + k * 256 + threadIdx.x);
        const uint32_t ref = (key[k] & BLOCK_KEY) ? BLOCK_INDEX0 + row / BLOCK_ROWS : level_base + row;
        stage[loff[(bucket >> lo_bits) >> b_bits] + rank[k]] = make_uint2(ref | (key[k] & SIGN_BIT), bucket);
    }
    __syncthreads();
    part_ab_flush(stage, total_sh, loff, gbase, lo_bits + b_bits, G - 1, false, 0, tmpa);
}

__global__ void __launch_bounds__(256) k_part_b(const uint2* tmpa, const uint32_t* pbase, uint32_t lo_bits, uint32_t b_bits,
                                                uint32_t a_bits, const uint32_t* tile_start, uint32_t* pcursor, uint2* tmp) {
    constexpr uint32_t ITEMS = PART_AB_T / 256;
    __shared__ uint32_t hist[PARTA_GROUPS_MAX], loff[PARTA_GROUPS_MAX], gbase[PARTA_GROUPS_MAX], total_sh, group_sh, wsum[2];
    uint2* stage = (uint2*)h2_msm_smem;
    const uint32_t G = 1u << a_bits, P = 1u << b_bits;
    if (blockIdx.x >= tile_start[G]) return;
    if (threadIdx.x < G && tile_start[threadIdx.x] <= blockIdx.x && blockIdx.x < tile_start[threadIdx.x + 1]) group_sh = threadIdx.x;
    if (threadIdx.x < P) hist[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t a = group_sh;
    const uint32_t gs = pbase[a << b_bits], ge = pbase[(a + 1) << b_bits];
    const uint32_t e0 = gs + (blockIdx.x - tile_start[a]) * PART_AB_T;
    uint2 ent[ITEMS];
    uint32_t rank[ITEMS];
#pragma unroll
    for (uint32_t k = 0; k < ITEMS; k++) {
        const uint32_t e = e0 + k * 256 + threadIdx.x;
        ent[k] = tmpa[e < ge ? e : ge - 1];
    }
#pragma unroll
    for (uint32_t k = 0; k < ITEMS; k++) {
        const uint32_t e = e0 + k * 256 + threadIdx.x;
        rank[k] = e < ge ? atomicAdd(&hist[(ent[k].y >> lo_bits) & (P - 1)], 1u) : 0xffffffffu;
    }
    __syncthreads();
    part_ab_reserve(hist, loff, gbase, P, pcursor + (a << b_bits), &total_sh, wsum);
    __syncthreads();
#pragma unroll
    for (uint32_t k = 0; k < ITEMS; k++)
        if (rank[k] != 0xffffffffu) stage[loff[(ent[k].y >> lo_bits) & (P - 1)] + rank[k]] = ent[k];
    __syncthreads();
    part_ab_flush(stage, total_sh, loff, gbase, lo_bits, P - 1, true, (1u << lo_bits) - 1, tmp);
}

// ---------------------------------------------------------------- k_bucket_sort (sort pass B)
// One workgroup per partition: histogram of the low bucket bits in LDS, exclusive scan -> the start
// offset of every bucket of the partition (written to `starts`), then the entries are placed.
// A partition far above the average size means a skewed column (a witness column that is mostly one value:
// every such scalar lands in one bucket): its entries would serialise on one LDS counter, so the counter updates
// are aggregated per wave -- lanes holding the key of the first active lane are served by one atomic, four times over
// (a witness column of three or four distinct values is then served completely), and only what is left falls back to
// per-lane atomics.
static constexpr int SKEW_ROUNDS = 4;  // distinct keys of a wave served by one atomic each (a column of 3-4 values: all of them)
__device__ __forceinline__ uint32_t lds_count_aggregated(uint32_t* bins, uint32_t key, bool valid) {
    const uint32_t lane = threadIdx.x & 63;
    uint64_t active = __ballot(valid);
    uint32_t result = 0;
#pragma unroll
    for (int round = 0; round < SKEW_ROUNDS; round++) {
        if (active == 0) break;
        const int leader = __ffsll((unsigned long long)active) - 1;
        const uint32_t k = __shfl(key, leader, 64);
        const uint64_t same = __ballot(valid && key == k) & active;
        uint32_t base = 0;
        if ((int)lane == leader) base = atomicAdd(&bins[k], (uint32_t)__popcll(same));
        base = __shfl(base, leader, 64);
        if ((same >> lane) & 1) result = base + (uint32_t)__popcll(same & ((1ull << lane) - 1));
        active &= ~same;
    }
    if ((active >> lane) & 1) result = atomicAdd(&bins[key], 1u);
    return result;
}

__global__ void __launch_bounds__(SORT_T) k_bucket_sort(const uint2* tmp, const uint32_t* pbase, uint32_t lo_bits,
                                                        uint32_t hi_bits, uint32_t nb, uint32_t skew_threshold,
                                                        uint32_t hot_partition, uint32_t hot_wc, uint64_t hot_mask,
                                                        uint32_t* starts, uint32_t* sorted, uint32_t stage_cap) {
    uint32_t* bins = h2_msm_smem;  // 2^lo_bits counters, reused as cursors
    __shared__ uint32_t sh[16];
    const uint32_t nbins = 1u << lo_bits, p = blockIdx.x;
    const uint32_t e0 = pbase[p], e1 = pbase[p + 1];
    bool is_hot_partition = p == hot_partition;
    if (hot_wc) {  // fused shape: the dominant-scalar window of column j is window j * hot_wc + hot_wc - 1
        const uint32_t w = p >> hi_bits;
        is_hot_partition = (p & ((1u << hi_bits) - 1)) == 0 && (w % hot_wc) == hot_wc - 1 && ((hot_mask >> (w / hot_wc)) & 1);
    }
    if (is_hot_partition) {
        // the dominant scalar's window: every entry sits in bin 0, so there is nothing to sort -- k_copy_hot moves the
        // references with the whole chip instead of this one workgroup; only the bucket starts are written here
        const uint32_t w = p >> hi_bits, hi = p & ((1u << hi_bits) - 1);
        for (uint32_t b = threadIdx.x; b < nbins; b += SORT_T) starts[(size_t)w * nb + ((hi << lo_bits) | b)] = b ? e1 : e0;
        return;
    }
    const bool skewed = (e1 - e0) > skew_threshold;  // uniform over the workgroup
    for (uint32_t k = threadIdx.x; k < nbins; k += SORT_T) bins[k] = 0;
    __syncthreads();
    if (!skewed) {
        // (eight loads in flight per lane: one at a time, a partition of 24 000 entries was 24 memory latencies per pass)
        for (uint32_t e = e0 + threadIdx.x; e < e1; e += 8 * SORT_T) {
            uint32_t key[8];
#pragma unroll
            for (uint32_t j = 0; j < 8; j++) key[j] = tmp[min(e + j * SORT_T, e1 - 1)].y;
#pragma unroll
            for (uint32_t j = 0; j < 8; j++)
                if (e + j * SORT_T < e1) atomicAdd(&bins[key[j]], 1u);
        }
    } else {
        for (uint32_t e = e0 + threadIdx.x; e < e1 + (SORT_T - 1); e += 4 * SORT_T) {  // whole waves stay in the loop
            uint32_t key[4];
#pragma unroll
            for (int j = 0; j < 4; j++) key[j] = (e + j * SORT_T < e1) ? tmp[e + j * SORT_T].y : 0;
#pragma unroll
            for (int j = 0; j < 4; j++) lds_count_aggregated(bins, key[j], e + j * SORT_T < e1);
        }
    }
    __syncthreads();
    // exclusive scan of the nbins (<= 4096) counters: (nbins / SORT_T) consecutive bins per thread
    const uint32_t per = (nbins + SORT_T - 1) / SORT_T;
    uint32_t local[4] = {0, 0, 0, 0}, sum = 0;
#pragma unroll
    for (uint32_t k = 0; k < 4; k++) {
        if (k < per) {
            uint32_t b = threadIdx.x * per + k;
            uint32_t v = b < nbins ? bins[b] : 0;
            local[k] = sum;
            sum += v;
        }
    }
    __syncthreads();
    // bucket index of bin b of partition p: window w = p >> hi_bits, bucket = ((p & (2^hi_bits - 1)) << lo_bits) | b
    const uint32_t w = p >> hi_bits, hi = p & ((1u << hi_bits) - 1);
    {
        uint32_t total;
        uint32_t ex = block_exclusive_scan_1024(sum, sh, &total);
#pragma unroll
        for (uint32_t k = 0; k < 4; k++) {
            if (k < per) {
                uint32_t b = threadIdx.x * per + k;
                if (b < nbins) {
                    uint32_t st = e0 + ex + local[k];
                    bins[b] = st;
                    starts[(size_t)w * nb + ((hi << lo_bits) | b)] = st;
                }
            }
        }
    }
    __syncthreads();
    if (!skewed) {
        // a partition that fits the staging area is put in order in LDS and leaves as whole lines: placed directly, its
        // entries are 4-byte stores at 2^lo_bits different frontiers (64 transactions per wave and store)
        uint32_t* stage = bins + nbins;
        const bool staged = (e1 - e0) <= stage_cap;   // uniform over the workgroup
        for (uint32_t e = e0 + threadIdx.x; e < e1; e += 8 * SORT_T) {
            uint2 v[8];
#pragma unroll
            for (uint32_t j = 0; j < 8; j++) v[j] = tmp[min(e + j * SORT_T, e1 - 1)];
#pragma unroll
            for (uint32_t j = 0; j < 8; j++) {
                if (e + j * SORT_T >= e1) continue;
                const uint32_t pos = atomicAdd(&bins[v[j].y], 1u);
                if (staged)
                    stage[pos - e0] = v[j].x;
                else
                    sorted[pos] = v[j].x;
            }
        }
        if (staged) {
            __syncthreads();
            for (uint32_t i = threadIdx.x; i < e1 - e0; i += SORT_T) sorted[e0 + i] = stage[i];
        }
    } else {
        for (uint32_t e = e0 + threadIdx.x; e < e1 + (SORT_T - 1); e += 4 * SORT_T) {
            uint2 v[4];
#pragma unroll
            for (int j = 0; j < 4; j++) v[j] = (e + j * SORT_T < e1) ? tmp[e + j * SORT_T] : make_uint2(0, 0);
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const bool valid = e + j * SORT_T < e1;
                uint32_t slot = lds_count_aggregated(bins, v[j].y, valid);
                if (valid) sorted[slot] = v[j].x;
            }
        }
    }
}

__global__ void __launch_bounds__(256) k_copy_hot(const uint2* tmp, const uint32_t* pbase, uint32_t hot_partition,
                                                  uint32_t* sorted) {
    const uint32_t e0 = pbase[hot_partition], e1 = pbase[hot_partition + 1];
    for (uint32_t e = e0 + blockIdx.x * blockDim.x + threadIdx.x; e < e1; e += gridDim.x * blockDim.x) sorted[e] = tmp[e].x;
}

// ---------------------------------------------------------------- k_acc_slice (hot loop)
template <int WAVES>
__global__ void __launch_bounds__(256, WAVES) k_acc_slice(const Affine* bases, const Affine* block_sums, const uint32_t* sorted,
                                                   const uint32_t* starts, uint32_t nbt, uint32_t log_s, XYZZ* partials) {
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;  // slice index
    const uint32_t total = starts[nbt];                        // number of (non-zero digit) entries
    uint32_t e = s << log_s;
    if (e >= total) return;
    uint32_t end = e + (1u << log_s);
    if (end > total) end = total;
    // bucket of the first entry: largest b with starts[b] <= e (ties -> the last one, which is non-empty)
    uint32_t lo = 0, hi = nbt;  // invariant: starts[lo] <= e < starts[hi]
    while (hi - lo > 1) {
        uint32_t mid = (lo + hi) >> 1;
        if (starts[mid] <= e)
            lo = mid;
        else
            hi = mid;
    }
    uint32_t b = lo;
    uint32_t bnext = starts[b + 1];  // first entry of the next non-empty bucket
    XYZZ acc = xyzz_identity();
    for (; e < end; e++) {
        if (e == bnext) {  // bucket boundary inside the slice (rare: once per ~n/2^(c-1) entries)
            xyzz_store(partials + (b + s), acc);
            acc = xyzz_identity();
            b++;
            bnext = starts[b + 1];
            if (bnext == e) {
                // a run of empty buckets (sparse columns: a few distinct values spread over 2^(c-1) buckets): locate the
                // bucket that owns entry e by bisection instead of walking the run one dependent load at a time
                uint32_t l2 = b, h2 = nbt;  // starts[l2] <= e < starts[h2]
                while (h2 - l2 > 1) {
                    uint32_t mid = (l2 + h2) >> 1;
                    if (starts[mid] <= e)
                        l2 = mid;
                    else
                        h2 = mid;
                }
                b = l2;
                bnext = starts[b + 1];
            }
        }
        uint32_t ref = sorted[e];
        const uint32_t idx = ref & ~SIGN_BIT;
        Affine p = affine_load(idx >= BLOCK_INDEX0 ? block_sums + (idx - BLOCK_INDEX0) : bases + idx);
        acc = xyzz_madd(acc, p, (ref & SIGN_BIT) != 0);
    }
    xyzz_store(partials + (b + s), acc);
}

// (A kernel of the shifted-base tables that stays in this file: xyzz_madd is inlined here and into k_acc_slice, and the
// compiler propagates constant arguments between functions BEFORE it inlines.  In a unit where this is xyzz_madd's only
// caller, `negate` = false is folded into it first and the kernel comes out three scalar instructions different.)
// sums of BLOCK_ROWS consecutive bases (blocks of a registered base set; see k_digits "dominant value over whole blocks")
__global__ void __launch_bounds__(64) k_block_sums(const Affine* bases, size_t nblocks, Affine* out) {
    const size_t b = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= nblocks) return;
    XYZZ acc = xyzz_identity();
#pragma unroll 1
    for (uint32_t k = 0; k < BLOCK_ROWS; k++) acc = xyzz_madd(acc, affine_load(bases + b * BLOCK_ROWS + k), false);
    const Fq zero = fp_zero<FqParams>();
    if (fp_is_zero(acc.zz)) {  // the identity (the bases of a block cancel): (0, 0)
        fp_store(&out[b].x, zero);
        fp_store(&out[b].y, zero);
        return;
    }
    const Fq t = fq_inv_device(acc.zzz);
    const Fq u = fp_mul(acc.zz, t);
    fp_store(&out[b].x, fp_mul(acc.x, fp_sqr(u)));
    fp_store(&out[b].y, fp_mul(acc.y, t));
}

void block_sums_launch(const Affine* bases, size_t nblocks, Affine* out, hipStream_t stream) {
    hipLaunchKernelGGL(k_block_sums, dim3((unsigned)((nblocks + 63) / 64)), dim3(64), 0, stream, bases, nblocks, out);
}

// ---------------------------------------------------------------- k_finish / k_finish_heavy
// These kernels and k_reduce are chains and trees of dependent point additions with few of them in flight: they run on
// QUADS (ec_quad.hpp) -- four lanes share one chain and each addition costs 4 dependent field products instead of 14.
// `q` = lane inside the quad, `qd` = quad inside the workgroup; loads are replicated over the quad, lane k stores
// coordinate k.
__device__ __forceinline__ void xyzz_store_q(XYZZ* p, const XYZZ& v, uint32_t q) {
    fp_store(&p->x + q, quad_pick(q, v.x, v.y, v.zz, v.zzz));
}

// sum over the QUADS quads of a workgroup, result in quad 0 (sh: one XYZZ per quad)
template <uint32_t QUADS>
__device__ __forceinline__ XYZZ quad_tree_sum(XYZZ acc, XYZZ* sh, uint32_t qd, uint32_t q) {
    for (uint32_t off = QUADS / 2; off >= 1; off >>= 1) {
        if (qd >= off && qd < 2 * off) xyzz_store_q(sh + qd, acc, q);
        __syncthreads();
        if (qd < off) acc = xyzz_add_q(acc, xyzz_load(sh + qd + off), q);
        __syncthreads();
    }
    return acc;
}

// bucket b's partials are slots b + first .. b + last, first/last = slices of its first/last entry
__global__ void __launch_bounds__(256) k_finish(const XYZZ* partials, const uint32_t* starts, uint32_t nbt,
                                                uint32_t log_s, XYZZ* buckets, uint32_t* heavy_list,
                                                uint32_t* heavy_count) {
    const uint32_t q = threadIdx.x & 3;
    uint32_t b = (blockIdx.x * blockDim.x + threadIdx.x) >> 2;
    if (b >= nbt) return;
    uint32_t e0 = starts[b], e1 = starts[b + 1];
    XYZZ acc = xyzz_identity();
    if (e1 > e0) {
        uint32_t first = e0 >> log_s, last = (e1 - 1) >> log_s;
        if (last - first + 1 > FINISH_SERIAL) {
            if (q == 0) heavy_list[atomicAdd(heavy_count, 1u)] = b;
            return;
        }
        acc = xyzz_load(partials + (b + first));
        XYZZ nxt = first < last ? xyzz_load(partials + (b + first + 1)) : xyzz_identity();
        for (uint32_t sl = first + 1; sl <= last; sl++) {
            const XYZZ cur = nxt;
            if (sl < last) nxt = xyzz_load(partials + (b + sl + 1));  // in flight during the addition below
            acc = xyzz_add_q(acc, cur, q);
        }
    }
    xyzz_store_q(buckets + b, acc, q);
}

// The same fold with ONE LANE per bucket, for bucket counts that fill the chip many times over (2^21 buckets of a
// shifted-base table at 2^24): there the fold is bound by throughput, and a quad spends four lanes on the latency of
// one chain (2^24 over a table, batch of 8: 21.3 -> 20.9 ms per MSM; from 2^19 buckets the lanes win by 1-2 %, at 2^17 the two forms tie,
// below the quads win).
__global__ void __launch_bounds__(256) k_finish_lane(const XYZZ* partials, const uint32_t* starts, uint32_t nbt,
                                                     uint32_t log_s, XYZZ* buckets, uint32_t* heavy_list,
                                                     uint32_t* heavy_count) {
    const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= nbt) return;
    const uint32_t e0 = starts[b], e1 = starts[b + 1];
    XYZZ acc = xyzz_identity();
    if (e1 > e0) {
        const uint32_t first = e0 >> log_s, last = (e1 - 1) >> log_s;
        if (last - first + 1 > FINISH_SERIAL) {
            heavy_list[atomicAdd(heavy_count, 1u)] = b;
            return;
        }
        acc = xyzz_load(partials + (b + first));
        for (uint32_t sl = first + 1; sl <= last; sl++) acc = xyzz_add(acc, xyzz_load(partials + (b + sl)));
    }
    xyzz_store(buckets + b, acc);
}

// Buckets on the heavy list with <= MID_MAX partials (a narrow column: thousands of buckets with a few hundred entries
// each) take ONE WAVE each: its 16 quads fold the partials strided by 16, then a 4-level tree over the wave by lane
// shuffles; a workgroup per such bucket (k_finish_heavy) would spend a 6-level tree on one partial per quad and walk the
// list 64 buckets at a time (2^20 4-bit values: 2048 such buckets, 1.1 ms -> 0.05 ms).
__device__ __forceinline__ XYZZ xyzz_shfl_down(const XYZZ& v, uint32_t delta) {
    XYZZ r;
    const uint32_t* src = (const uint32_t*)&v;
    uint32_t* dst = (uint32_t*)&r;
#pragma unroll
    for (int i = 0; i < 32; i++) dst[i] = (uint32_t)__shfl_down((int)src[i], delta, 64);
    return r;
}

__global__ void __launch_bounds__(256) k_finish_mid(const XYZZ* partials, const uint32_t* starts, uint32_t log_s,
                                                    const uint32_t* heavy_list, const uint32_t* heavy_count,
                                                    XYZZ* buckets) {
    const uint32_t lane = threadIdx.x & 63, q = lane & 3, qd = lane >> 2;  // 16 quads per wave
    const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, nwaves = (gridDim.x * blockDim.x) >> 6;
    const uint32_t nheavy = *heavy_count;
    for (uint32_t h = wave; h < nheavy; h += nwaves) {
        const uint32_t b = heavy_list[h];
        const uint32_t first = starts[b] >> log_s, last = (starts[b + 1] - 1) >> log_s;
        if (last - first + 1 > MID_MAX) continue;  // uniform over the wave: k_finish_heavy's
        XYZZ acc = xyzz_identity();
        for (uint32_t sl = first + qd; sl <= last; sl += 16) acc = xyzz_add_q(acc, xyzz_load(partials + (b + sl)), q);
        for (uint32_t off = 8; off >= 1; off >>= 1) {
            const XYZZ other = xyzz_shfl_down(acc, 4 * off);  // every lane takes part in the exchange
            if (qd < off) acc = xyzz_add_q(acc, other, q);
        }
        if (qd == 0) xyzz_store_q(buckets + b, acc, q);
    }
}

// Heavy bucket h with P > MID_MAX partials is shared by NP = ceil(P / 256) (at most HEAVY_SPLIT) workgroups: part y folds the
// slots first + y, first + y + NP, ... and leaves the result in slot first + y -- a slot of its own set, written after
// its last read, so the parts of one bucket never race.  k_finish_heavy2 then folds the NP leading slots.
__device__ __forceinline__ uint32_t heavy_parts(uint32_t first, uint32_t last) {
    const uint32_t np = (last - first + 256) / 256;  // ceil((last - first + 1) / 256)
    return np < HEAVY_SPLIT ? np : HEAVY_SPLIT;
}
__global__ void __launch_bounds__(256) k_finish_heavy(XYZZ* partials, const uint32_t* starts, uint32_t log_s,
                                                      const uint32_t* heavy_list, const uint32_t* heavy_count) {
    __shared__ XYZZ sh[64];
    const uint32_t q = threadIdx.x & 3, qd = threadIdx.x >> 2, part = blockIdx.y;
    uint32_t nheavy = *heavy_count;
    for (uint32_t h = blockIdx.x; h < nheavy; h += gridDim.x) {
        uint32_t b = heavy_list[h];
        uint32_t first = starts[b] >> log_s, last = (starts[b + 1] - 1) >> log_s;
        if (last - first + 1 <= MID_MAX) continue;  // k_finish_mid's
        const uint32_t np = heavy_parts(first, last);
        if (part >= np) continue;  // uniform over the workgroup
        XYZZ acc = xyzz_identity();
        for (uint32_t sl = first + part + qd * np; sl <= last; sl += 64 * np)
            acc = xyzz_add_q(acc, xyzz_load(partials + (b + sl)), q);
        acc = quad_tree_sum<64>(acc, sh, qd, q);
        if (qd == 0) xyzz_store_q(partials + (b + first + part), acc, q);
    }
}

__global__ void __launch_bounds__(4 * HEAVY_SPLIT) k_finish_heavy2(const XYZZ* partials, const uint32_t* starts,
                                                                    uint32_t log_s, const uint32_t* heavy_list,
                                                                    const uint32_t* heavy_count, XYZZ* buckets) {
    __shared__ XYZZ sh[HEAVY_SPLIT];
    const uint32_t q = threadIdx.x & 3, qd = threadIdx.x >> 2;
    uint32_t nheavy = *heavy_count;
    for (uint32_t h = blockIdx.x; h < nheavy; h += gridDim.x) {
        uint32_t b = heavy_list[h];
        uint32_t first = starts[b] >> log_s, last = (starts[b + 1] - 1) >> log_s;
        if (last - first + 1 <= MID_MAX) continue;  // k_finish_mid's
        XYZZ acc = qd < heavy_parts(first, last) ? xyzz_load(partials + (b + first + qd)) : xyzz_identity();
        acc = quad_tree_sum<HEAVY_SPLIT>(acc, sh, qd, q);
        if (qd == 0) xyzz_store_q(buckets + b, acc, q);
    }
}

// ---------------------------------------------------------------- k_reduce
// window w, group g: sum over this group's buckets of (b + 1) * B_b   (b = index inside the window).  A quad walks
// REDUCE_QM consecutive buckets by summation by parts (arithmetic.rs:98-106), lifts its sum by the offset of its first
// bucket, and the quads of the workgroup are folded by a tree.  The last workgroup of a window to finish (a counter per
// window) folds the RG group results, so the host reads one point per window.
__device__ __forceinline__ XYZZ xyzz_load_coherent(const XYZZ* p) {  // written by other workgroups of this launch
    XYZZ r;
    const volatile uint4* src = (const volatile uint4*)p;
    uint4* dst = (uint4*)&r;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        dst[i].x = src[i].x;
        dst[i].y = src[i].y;
        dst[i].z = src[i].z;
        dst[i].w = src[i].w;
    }
    return r;
}

__global__ void __launch_bounds__(REDUCE_T) k_reduce(const XYZZ* buckets, uint32_t nb, uint32_t RG, uint32_t qm,
                                                     XYZZ* groups, XYZZ* winsum, uint32_t* rcount) {
    __shared__ XYZZ sh[REDUCE_T / 4];
    __shared__ uint32_t last_flag;
    const uint32_t q = threadIdx.x & 3, qd = threadIdx.x >> 2, g = blockIdx.x, w = blockIdx.y;
    const XYZZ* B = buckets + (size_t)w * nb;
    uint32_t k0 = (g * (REDUCE_T / 4) + qd) * qm;
    XYZZ res = xyzz_identity();
    if (k0 < nb) {
        uint32_t k1 = k0 + qm;
        if (k1 > nb) k1 = nb;
        XYZZ running = xyzz_identity(), acc = xyzz_identity();
        XYZZ nxt = xyzz_load(B + (k1 - 1));
        for (uint32_t b = k1; b-- > k0;) {
            const XYZZ cur = nxt;
            if (b > k0) nxt = xyzz_load(B + (b - 1));  // in flight during the two additions below
            running = xyzz_add_q(running, cur, q);
            acc = xyzz_add_q(acc, running, q);
        }
        // acc = sum (b - k0 + 1) * B_b ;  running = sum B_b
        res = acc;
        if (k0 != 0 && !xyzz_is_identity(running)) res = xyzz_add_q(res, xyzz_mul_u32_q(running, k0, q), q);
    }
    res = quad_tree_sum<REDUCE_T / 4>(res, sh, qd, q);
    if (RG == 1) {
        if (qd == 0) xyzz_store_q(winsum + w, res, q);
        return;
    }
    if (qd == 0) xyzz_store_q(groups + (size_t)w * RG + g, res, q);
    __threadfence();
    __syncthreads();
    if (threadIdx.x == 0) last_flag = atomicAdd(rcount + w, 1u) == RG - 1 ? 1u : 0u;
    __syncthreads();
    if (!last_flag) return;
    __threadfence();
    res = xyzz_identity();
    for (uint32_t g2 = qd; g2 < RG; g2 += REDUCE_T / 4) res = xyzz_add_q(res, xyzz_load_coherent(groups + (size_t)w * RG + g2), q);
    res = quad_tree_sum<REDUCE_T / 4>(res, sh, qd, q);
    if (qd == 0) xyzz_store_q(winsum + w, res, q);
}

// ---------------------------------------------------------------- reduce by bit planes (shifted-base tables)
// k_reduce's quads each lift their chunk by the index of its first bucket -- a double-and-add over up to 16-21 bits, ~80
// dependent product levels, the longest part of a chain that is latency and nothing else (273 us for the 2^16 buckets of a
// 2^20 MSM however few points they hold).  The weights factor instead:
//     sum_b (b + 1) B_b  =  sum_c acc_c  +  qm * sum_c c * R_c          (chunk c = buckets c qm .. c qm + qm - 1,
//                                                                         acc_c = sum (b - c qm + 1) B_b,  R_c = sum B_b)
//     sum_c c * R_c      =  sum_p 2^p P_p,   P_p = sum of the R_c whose index has bit p set
// k_reduce_chunks computes acc_c / R_c by summation by parts (2 qm additions per quad) and tree-sums the acc_c of a
// workgroup; k_reduce_planes forms the P_p -- UNWEIGHTED sums, a few elements per quad and two trees deep -- and the sum
// of the workgroups' acc sums; the host adds the planes up by Horner (log2(chunks) doublings and additions on one core,
// ~20 us, next to the window Horner it already does).  Same group element, a different (equally valid) Jacobian
// representative of it; ~4 extra additions per chunk of work, a third of the dependent depth.
__global__ void __launch_bounds__(REDUCE_T) k_reduce_chunks(const XYZZ* buckets, uint32_t nb, uint32_t qm, uint32_t chunks,
                                                            XYZZ* R, XYZZ* group_acc) {
    __shared__ XYZZ sh[REDUCE_T / 4];
    const uint32_t q = threadIdx.x & 3, qd = threadIdx.x >> 2;
    const uint32_t c = blockIdx.x * (REDUCE_T / 4) + qd;
    XYZZ acc = xyzz_identity();
    if (c < chunks) {
        const uint32_t k0 = c * qm;
        uint32_t k1 = k0 + qm;
        if (k1 > nb) k1 = nb;
        XYZZ running = xyzz_identity();
        XYZZ nxt = xyzz_load(buckets + (k1 - 1));
        for (uint32_t b = k1; b-- > k0;) {
            const XYZZ cur = nxt;
            if (b > k0) nxt = xyzz_load(buckets + (b - 1));  // in flight during the two additions below
            running = xyzz_add_q(running, cur, q);
            acc = xyzz_add_q(acc, running, q);
        }
        xyzz_store_q(R + c, running, q);
    }
    acc = quad_tree_sum<REDUCE_T / 4>(acc, sh, qd, q);
    if (qd == 0) xyzz_store_q(group_acc + blockIdx.x, acc, q);
}

// grid (plane_seg, planes): plane p < nbits sums the chunk sums R[c] with bit p of c set -- quad t of the plane takes the
// L consecutive members t L .. t L + L - 1 of that half of the index space; the last plane sums the group_acc of
// k_reduce_chunks' workgroups (segment 0 alone).  Each workgroup's tree result goes to part[p][segment]; the last
// workgroup of a plane to finish (a counter per plane) folds the segments and writes out[p].
__global__ void __launch_bounds__(REDUCE_T) k_reduce_planes(const XYZZ* R, uint32_t chunks, uint32_t nbits, const XYZZ* group_acc,
                                                            uint32_t groups, uint32_t L, XYZZ* part, uint32_t* counters, XYZZ* out) {
    __shared__ XYZZ sh[REDUCE_T / 4];
    __shared__ uint32_t last_flag;
    const uint32_t q = threadIdx.x & 3, qd = threadIdx.x >> 2, seg = blockIdx.x, p = blockIdx.y, nseg = gridDim.x;
    XYZZ acc = xyzz_identity();
    uint32_t expected = nseg;
    if (p == nbits) {
        expected = 1;
        if (seg != 0) return;
        for (uint32_t g = qd; g < groups; g += REDUCE_T / 4) acc = xyzz_add_q(acc, xyzz_load(group_acc + g), q);
    } else {
        const uint32_t half = 1u << (nbits - 1), low_mask = (1u << p) - 1;
        const uint32_t t = seg * (REDUCE_T / 4) + qd;
        uint32_t j = t * L;
        const uint32_t j1 = j + L < half ? j + L : half;
        for (; j < j1; j++) {
            const uint32_t c = ((j >> p) << (p + 1)) | (1u << p) | (j & low_mask);
            if (c < chunks) acc = xyzz_add_q(acc, xyzz_load(R + c), q);
        }
    }
    acc = quad_tree_sum<REDUCE_T / 4>(acc, sh, qd, q);
    if (expected == 1) {
        if (qd == 0) xyzz_store_q(out + p, acc, q);
        return;
    }
    if (qd == 0) xyzz_store_q(part + (size_t)p * nseg + seg, acc, q);
    __threadfence();
    __syncthreads();
    if (threadIdx.x == 0) last_flag = atomicAdd(counters + p, 1u) == expected - 1 ? 1u : 0u;
    __syncthreads();
    if (!last_flag) return;
    __threadfence();
    acc = xyzz_identity();
    for (uint32_t s2 = qd; s2 < nseg; s2 += REDUCE_T / 4) acc = xyzz_add_q(acc, xyzz_load_coherent(part + (size_t)p * nseg + s2), q);
    acc = quad_tree_sum<REDUCE_T / 4>(acc, sh, qd, q);
    if (qd == 0) xyzz_store_q(out + p, acc, q);
}

// The window sums (one point per window, a few KB) go back to the host through a store kernel into mapped pinned
// memory rather than hipMemcpyAsync: a DMA-engine copy queues behind whatever bulk transfer is in flight (the prover
// uploads the next witness column while it commits the current one) and would stall the MSM for the whole transfer.
__global__ void __launch_bounds__(256) k_export(const uint4* src, uint4* dst, size_t count16) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < count16) dst[i] = src[i];
}

void copy16_launch(const void* src, void* dst, size_t count16, hipStream_t stream) {
    hipLaunchKernelGGL(k_export, dim3((unsigned)((count16 + 255) / 256)), dim3(256), 0, stream, (const uint4*)src, (uint4*)dst,
                       count16);
}

void export_to_host(const XYZZ* d_src, XYZZ* h_dst, size_t count, hipStream_t stream) {
    copy16_launch(d_src, h_dst, count * sizeof(XYZZ) / 16, stream);
    H2_HIP(hipGetLastError());
}

// ---------------------------------------------------------------- dominant-scalar detection
__global__ void __launch_bounds__(HOT_SAMPLES) k_sample(const Fr* scalars, size_t n, Fr* out) {
    size_t idx = ((size_t)threadIdx.x * 0x9E3779B1ull + 0x7F4A7C15ull) % n;
    fp_store(out + threadIdx.x, fp_load(scalars + idx));
}

void sample_launch(const Fr* scalars, size_t n, Fr* out, hipStream_t stream) {
    hipLaunchKernelGGL(k_sample, dim3(1), dim3(HOT_SAMPLES), 0, stream, scalars, n, out);
}

// ---------------------------------------------------------------- the enqueue of one planned launch
// raises the dynamic LDS limit of some kernels, once per device (one object per call site)
struct LdsLimit {
    bool raised[64] = {};
    void raise(std::initializer_list<const void*> kernels, int bytes) {
        int dev = 0;
        H2_HIP(hipGetDevice(&dev));
        if (dev >= 0 && dev < 64 && raised[dev]) return;
        for (const void* k : kernels) H2_HIP(hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
        if (dev >= 0 && dev < 64) raised[dev] = true;
    }
};
// The launch record (h2_msm_last_launches): msm_enqueue appends its plan's record to a list of the calling thread;
// the outermost driver on the thread empties the list when it is entered.  Host only; the vector keeps its capacity.
namespace {
thread_local std::vector<h2_msm_launch_info> t_launches;
thread_local int t_launch_depth = 0;
}  // namespace
LaunchScope::LaunchScope() {
    if (t_launch_depth++ == 0) t_launches.clear();
}
LaunchScope::~LaunchScope() { t_launch_depth--; }
size_t msm_last_launches(h2_msm_launch_info* out, size_t cap) {
    const size_t count = t_launches.size();
    if (out)
        for (size_t i = 0; i < count && i < cap; i++) out[i] = t_launches[i];
    return count;
}

// name the k_partition<TILE> / k_acc_slice<WAVES> that msm_enqueue starts
template <uint32_t TILE>
using tile = std::integral_constant<uint32_t, TILE>;
template <int WAVES>
using waves = std::integral_constant<int, WAVES>;

void msm_enqueue(const MsmShape& s, const MsmLaunchPlan& p, const Fr* d_scalars, const Fr& hot_value, const Affine* d_bases,
                 const Affine* block_sums, char* scratch, hipStream_t stream, const FusedCols* fused) {
    uint32_t* keys = (uint32_t*)(scratch + s.off_keys);
    uint32_t* sorted = (uint32_t*)(scratch + s.off_sorted);
    uint2* tmp = (uint2*)(scratch + s.off_tmp);
    uint32_t* pcount = (uint32_t*)(scratch + s.off_pcount);
    uint32_t* pbase = (uint32_t*)(scratch + s.off_pbase);
    uint32_t* pcursor = (uint32_t*)(scratch + s.off_pcursor);
    uint32_t* starts = (uint32_t*)(scratch + s.off_starts);
    uint32_t* heavy = (uint32_t*)(scratch + s.off_heavy);  // [0] = count, [1..] = list
    XYZZ* partials = (XYZZ*)(scratch + s.off_partials);
    XYZZ* buckets = (XYZZ*)(scratch + s.off_buckets);
    XYZZ* winpart = (XYZZ*)(scratch + s.off_winpart);
    const h2_msm_launch_info& rec = p.rec;

    H2_HIP(hipMemsetAsync(pcount, 0, ((size_t)s.np + 2) * 4, stream));
    H2_HIP(hipMemsetAsync(heavy, 0, 4, stream));
    uint8_t* bflags = nullptr;  // per 256-row block: entered the dominant-value bucket as one point (block sums tabulated)
    if (p.bflags) {
        bflags = (uint8_t*)(scratch + s.off_bflags);
        H2_HIP(hipMemsetAsync(bflags, 0, s.n / 256 + 4, stream));
    }
    const FusedCols cols = fused ? *fused : FusedCols{};
    hipLaunchKernelGGL(k_digits, dim3(p.digits_grid_x, p.digits_grid_y), dim3(256), p.digits_lds, stream, d_scalars, s.n, s.c,
                       s.W, s.nb, rec.max_bits, s.lo_bits, s.hi_bits, p.np_col, keys, pcount, (int)(rec.hot_on && !p.fused),
                       hot_value, cols.scalars, cols.hot_values, cols.hot_mask, s.range_shift, s.R, s.wfull, s.tab,
                       p.block_rows_end, bflags);
    hipLaunchKernelGGL(k_scan_parts, dim3(1), dim3(256), 0, stream, pcount, s.np, pbase, pcursor, starts, s.nbt);
    // k_partition<TILE> over the plan's key arrays
    auto partition = [&](auto tile_tag) {
        constexpr uint32_t TILE = decltype(tile_tag)::value;
        hipLaunchKernelGGL(k_partition<TILE>, dim3(p.part_grid_x, p.part_arrays), dim3(256), p.part_lds, stream, keys, s.n,
                           s.lo_bits, s.hi_bits, pcursor, tmp, s.range_shift, s.W, s.R, (uint32_t)s.tab_stride,
                           (const uint8_t*)bflags, p.part_first);
    };
    const bool two_level = rec.partition == H2_MSM_PART_TWO_LEVEL;
    uint2* tmpa = (uint2*)(scratch + s.off_tmpa);   // (two-level shapes only)
    uint32_t* cursor_a = (uint32_t*)(scratch + s.off_tmpa + s.entries * 8);
    uint32_t* tile_start = cursor_a + PARTA_GROUPS_MAX;
    if (two_level) {
        // 64 KiB of staging + the static tables exceed the default dynamic limit
        static LdsLimit raised;
        raised.raise({(const void*)k_part_a, (const void*)k_part_b}, 80 * 1024);
        hipLaunchKernelGGL(k_part_init, dim3(1), dim3(PARTA_GROUPS_MAX), 0, stream, pbase, s.a_bits, p.b_bits, cursor_a, tile_start);
        hipLaunchKernelGGL(k_part_a, dim3(p.part_a_grid_x, s.W), dim3(256), (size_t)PART_AB_T * 8, stream, keys, s.n, s.lo_bits,
                           p.b_bits, s.a_bits, cursor_a, tmpa, (uint32_t)s.tab_stride, (const uint8_t*)bflags);
    }
    if (p.part_arrays) {
        if (p.part_tile == PART_T_TABLE)
            partition(tile<PART_T_TABLE>());
        else
            partition(tile<PART_T>());
    }
    if (two_level)
        hipLaunchKernelGGL(k_part_b, dim3(p.part_b_grid_x), dim3(256), (size_t)PART_AB_T * 8, stream, (const uint2*)tmpa, pbase,
                           s.lo_bits, p.b_bits, s.a_bits, tile_start, pcursor, tmp);
    if (rec.stage_cap) {
        static LdsLimit raised;
        raised.raise({(const void*)k_bucket_sort}, 160 * 1024 - 256);
    }
    hipLaunchKernelGGL(k_bucket_sort, dim3(s.np), dim3(SORT_T), p.sort_lds, stream, tmp, pbase, s.lo_bits, s.hi_bits, s.nb,
                       rec.skew_threshold, rec.hot_partition, p.hot_wc, cols.hot_mask, starts, sorted, rec.stage_cap);
    if (rec.hot_partition != 0xffffffffu)
        hipLaunchKernelGGL(k_copy_hot, dim3(2048), dim3(256), 0, stream, tmp, pbase, rec.hot_partition, sorted);
    if (fused)
        for (uint32_t col = 0; col < s.cols; col++)
            if ((fused->hot_mask >> col) & 1)
                hipLaunchKernelGGL(k_copy_hot, dim3(1024), dim3(256), 0, stream, tmp, pbase,
                                   (col * s.Wc + s.W) << s.hi_bits, sorted);
    auto accumulate = [&](auto waves_tag) {
        hipLaunchKernelGGL(k_acc_slice<decltype(waves_tag)::value>, dim3(p.acc_grid_x), dim3(256), 0, stream, d_bases,
                           p.bflags ? block_sums : (const Affine*)nullptr, sorted, starts, s.nbt, s.log_s, partials);
    };
    if (rec.acc_waves == 5)
        accumulate(waves<5>());
    else
        accumulate(waves<4>());
    if (rec.finish == H2_MSM_FINISH_LANES)
        hipLaunchKernelGGL(k_finish_lane, dim3(p.finish_grid_x), dim3(256), 0, stream, partials, starts, s.nbt, s.log_s,
                           buckets, heavy + 1, heavy);
    else
        hipLaunchKernelGGL(k_finish, dim3(p.finish_grid_x), dim3(256), 0, stream, partials, starts, s.nbt, s.log_s,
                           buckets, heavy + 1, heavy);
    hipLaunchKernelGGL(k_finish_mid, dim3(512), dim3(256), 0, stream, partials, starts, s.log_s, heavy + 1, heavy, buckets);
    hipLaunchKernelGGL(k_finish_heavy, dim3(64, HEAVY_SPLIT), dim3(256), 0, stream, partials, starts, s.log_s, heavy + 1,
                       heavy);
    hipLaunchKernelGGL(k_finish_heavy2, dim3(256), dim3(4 * HEAVY_SPLIT), 0, stream, partials, starts, s.log_s, heavy + 1,
                       heavy, buckets);
    if (s.RG > 1) H2_HIP(hipMemsetAsync(scratch + s.off_rcount, 0, (size_t)s.Wt * 4, stream));
    if (rec.reduce == H2_MSM_REDUCE_PLANES) {
        XYZZ* R = (XYZZ*)(scratch + s.off_planes);
        XYZZ* part = R + s.chunks;
        uint32_t* counters = (uint32_t*)(part + (size_t)s.planes * s.plane_seg);
        XYZZ* group_acc = winpart + s.Wt + s.planes;
        H2_HIP(hipMemsetAsync(counters, 0, (size_t)s.planes * 4, stream));
        hipLaunchKernelGGL(k_reduce_chunks, dim3(p.reduce_groups), dim3(REDUCE_T), 0, stream, buckets, s.nb, s.qm, s.chunks, R,
                           group_acc);
        hipLaunchKernelGGL(k_reduce_planes, dim3(s.plane_seg, s.planes), dim3(REDUCE_T), 0, stream, (const XYZZ*)R, s.chunks,
                           s.planes - 1, (const XYZZ*)group_acc, p.reduce_groups, s.plane_l, part, counters, winpart + s.Wt);
    } else {
        hipLaunchKernelGGL(k_reduce, dim3(s.RG, p.reduce_grid_y), dim3(REDUCE_T), 0, stream, buckets, s.nb, s.RG, s.qm,
                           winpart + s.Wt, winpart, (uint32_t*)(scratch + s.off_rcount));
    }
    if (s.tab && s.Wt > 1)  // the dominant-scalar window only ever fills its bucket 0
        hipLaunchKernelGGL(k_reduce, dim3(1, 1), dim3(REDUCE_T), 0, stream, buckets + s.nb, 1u, 1u, s.qm, winpart + s.Wt,
                           winpart + 1, (uint32_t*)(scratch + s.off_rcount));
    H2_HIP(hipGetLastError());
    t_launches.push_back(rec);
    t_launches.back().scratch = (uint64_t)(uintptr_t)scratch;
}

}  // namespace h2
