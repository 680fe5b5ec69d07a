// sort.hip -- a stable least-significant-digit radix sort over up to H2_SORT_MAX_KEYS columns of field elements, 8 bits a
// pass, that moves INDICES and gathers the digit through them (sort.hpp; DESIGN.md 3b, "Sorting a witness").
//   k_sort_survey   ONE read of every key column: a Montgomery column is converted to its canonical copy (the only time its
//                   cells are multiplied), every cell is held against its promise (the lowest breaking row << 32 | key by a
//                   64-bit atomicMin), and every candidate byte position gets a 256-bin histogram over all n rows -- counted
//                   in LDS (32 positions x 256 counters: 32 KiB), flushed with one global add per non-empty bin.
//   k_sort_decide   one workgroup: a position with exactly one non-empty bin holds the same byte in every cell and is switched
//                   off; the positions left are given the buffer they read (the identity, then the two index buffers in
//                   turn) and counted into d_status[3].  The host has launched every candidate position without knowing
//                   which ones run: a switched-off position's kernels return at once and move no data.
//   per position    k_sort_hist: perm[i] -> the byte of that row, kept in digits[i] and counted per tile; sort_scan: the
//                   exclusive prefix of the 256 x tiles counters, digit-major; k_sort_scatter: every index goes behind all
//                   of a lower digit, all of its digit in earlier tiles and all of its digit earlier in its tile -- 256
//                   entries a round, a wave's lanes of one digit found by eight ballots and ranked by lane, the waves by
//                   their order, the rounds by a running count (permmap.hip's rank).
//   k_sort_emit     the buffer the last position wrote (or the identity) -> d_perm at 4 or 8 bytes an index
// What places a row is a prefix sum or a ballot rank; the atomics only count or take a minimum, and both commute: the output
// is a function of the input.  The XCDs' L2s are not coherent with one another, so nothing is handed from workgroup to
// workgroup inside a launch: launch boundaries order the phases and no workgroup waits for another.
#include "common.hpp"
#include "field.hpp"
#include "sort.hpp"

namespace h2 {

namespace {

using u32 = uint32_t;
constexpr u32 SORT_ROUNDS = SORT_TILE / 256;
static_assert(SORT_TILE % 256 == 0 && SORT_SCAN_TILE == 256 * 16, "tiles are whole rounds of 256 lanes; the scan takes 16 words a lane");

// counts digit d of every `valid` lane of the wave into s_h.  When all of them hold one digit (a byte position of small
// values, the upper bytes of short keys) one lane adds the population instead of 64 lanes queueing on one counter.
__device__ __forceinline__ void sort_count(u32* s_h, u32 d, bool valid) {
    const uint64_t mask = __ballot(valid);
    if (mask == 0) return;
    const u32 leader = (u32)__ffsll((unsigned long long)mask) - 1;
    const u32 first = (u32)__shfl((int)d, (int)leader, 64);
    const uint64_t same = __ballot(valid && d == first);
    if (same == mask) {
        if ((threadIdx.x & 63) == leader) atomicAdd(&s_h[first], (u32)__popcll(mask));
    } else if (valid) {
        atomicAdd(&s_h[d], 1u);
    }
}

template <u32 FORM>
__global__ void __launch_bounds__(256) k_sort_survey(const void* __restrict__ cells, Fr* __restrict__ canon, u32 n, u32 tiles,
                                                     u32 nbytes, u32 bits, u32 key, u32* __restrict__ ghist, u32* misc) {
    __shared__ u32 s_h[32 * 256];
    const u32 t = threadIdx.x;
    for (u32 j = t; j < nbytes * 256; j += 256) s_h[j] = 0;
    __syncthreads();
    for (u32 tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        for (u32 r = 0; r < SORT_ROUNDS; r++) {
            const size_t i = (size_t)tile * SORT_TILE + r * 256 + t;
            const bool valid = i < n;
            Fr v = fp_zero<FrParams>();
            if (valid) {
                if (FORM == H2_ASSIGNED_FORM_COMPACT) {
                    const uint64_t x = ((const uint64_t*)cells)[i];
                    v.l[0] = (u32)x;
                    v.l[1] = (u32)(x >> 32);
                } else {
                    v = fp_load((const Fr*)cells + i);
                    if (FORM == H2_ASSIGNED_FORM_MONTGOMERY) {
                        v = fp_from_mont(v);
                        fp_store(canon + i, v);
                    }
                }
                // the promise: nothing at or above bit `bits` (1 .. 254)
                const u32 word = bits >> 5;
                u32 above = 0;
#pragma unroll
                for (u32 j = 0; j < 8; j++) {
                    if (j == word) above |= v.l[j] >> (bits & 31);
                    if (j > word) above |= v.l[j];
                }
                if (above) atomicMin((unsigned long long*)(misc + SORT_MISC_BAD), (unsigned long long)i << 32 | key);
            }
#pragma unroll
            for (u32 b = 0; b < 32; b++)
                if (b < nbytes) sort_count(s_h + 256 * b, (v.l[b >> 2] >> (8 * (b & 3))) & 255, valid);
        }
    }
    __syncthreads();
    for (u32 j = t; j < nbytes * 256; j += 256)
        if (s_h[j]) atomicAdd(&ghist[j], s_h[j]);
}

__global__ void __launch_bounds__(256) k_sort_decide(const u32* ghist, u32* misc, u32* status, u32 num_pos) {
    __shared__ u32 s_active[SORT_MAX_POS];
    for (u32 p = 0; p < num_pos; p++) {
        const int nonempty = __syncthreads_count(ghist[256 * p + threadIdx.x] != 0);
        if (threadIdx.x == 0) s_active[p] = nonempty > 1;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    u32 cur = SORT_IDENTITY, passes = 0;
    for (u32 p = 0; p < num_pos; p++) {
        misc[SORT_MISC_ACTIVE + p] = s_active[p];
        misc[SORT_MISC_SRC + p] = cur;
        if (s_active[p]) {
            cur = cur == SORT_IDENTITY ? 0 : cur ^ 1;
            passes++;
        }
    }
    misc[SORT_MISC_FINAL] = cur;
    const u32 bad_key = misc[SORT_MISC_BAD], bad_row = misc[SORT_MISC_BAD + 1];
    const bool broken = (bad_key & bad_row) != 0xffffffffu;
    status[0] = broken ? H2_SORT_OUT_OF_RANGE : H2_SORT_OK;
    status[1] = broken ? bad_row : 0xffffffffu;
    status[2] = broken ? bad_key : 0xffffffffu;
    status[3] = passes;
}

// the row entry i of position p's input stands for
__device__ __forceinline__ u32 sort_row(const u32* in, u32 src, size_t i, u32 n) {
    if (src == SORT_IDENTITY) return (u32)i;
    const u32 row = in[i];
    return row < n ? row : n - 1;   // every entry is a row whatever a buffer holds: the gather stays inside the column
}

// hist[digit * tiles + tile] = entries of the tile with that digit; digits[i] = the byte entry i sorts by
__global__ void __launch_bounds__(256) k_sort_hist(const uint8_t* __restrict__ key_bytes, u32 stride, const u32* perm0,
                                                   const u32* perm1, uint8_t* __restrict__ digits, u32* __restrict__ hist,
                                                   const u32* misc, u32 p, u32 n, u32 tiles) {
    __shared__ u32 s_h[256];
    if (!misc[SORT_MISC_ACTIVE + p]) return;
    const u32 src = misc[SORT_MISC_SRC + p];
    const u32* in = src == 0 ? perm0 : perm1;
    const size_t start = (size_t)blockIdx.x * SORT_TILE;
    s_h[threadIdx.x] = 0;
    __syncthreads();
    for (u32 r = 0; r < SORT_ROUNDS; r++) {
        const size_t i = start + r * 256 + threadIdx.x;
        const bool valid = i < n;
        u32 d = 0;
        if (valid) {
            d = key_bytes[(size_t)sort_row(in, src, i, n) * stride];
            digits[i] = (uint8_t)d;
        }
        sort_count(s_h, d, valid);
    }
    __syncthreads();
    hist[(size_t)threadIdx.x * tiles + blockIdx.x] = s_h[threadIdx.x];
}

__global__ void __launch_bounds__(256) k_sort_scatter(const u32* perm0, const u32* perm1, u32* out0, u32* out1,
                                                      const uint8_t* __restrict__ digits, const u32* __restrict__ offs,
                                                      const u32* misc, u32 p, u32 n, u32 tiles) {
    __shared__ u32 s_run[256];
    __shared__ u32 s_w[4][256];
    if (!misc[SORT_MISC_ACTIVE + p]) return;
    const u32 src = misc[SORT_MISC_SRC + p];
    const u32* in = src == 0 ? perm0 : perm1;
    u32* out = src == 0 ? out1 : out0;   // the identity and buffer 1 are followed by buffer 0
    const size_t start = (size_t)blockIdx.x * SORT_TILE;
    const u32 t = threadIdx.x, lane = t & 63, wave = t >> 6;
    s_run[t] = offs[(size_t)t * tiles + blockIdx.x];
    for (u32 r = 0; r < SORT_ROUNDS; r++) {
        const size_t i = start + r * 256 + t;
        const bool valid = i < n;
        const u32 d = valid ? digits[i] : 0, row = valid ? sort_row(in, src, i, n) : 0;
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
            if (pos < n) out[pos] = row;
        }
        __syncthreads();
        s_run[t] += s_w[0][t] + s_w[1][t] + s_w[2][t] + s_w[3][t];
    }
}

// exclusive prefix of v over the 256 lanes of a workgroup and the workgroup's total
__device__ __forceinline__ u32 sort_block_excl(u32 v, u32* s_wave, u32& total) {
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

// data[0, words) -> its exclusive prefix sums tile by tile, in place; sums[tile] = the tile's total
__global__ void __launch_bounds__(256) k_sort_scan_tile(u32* data, size_t words, u32* sums, const u32* misc, u32 p) {
    __shared__ u32 s_wave[4];
    if (!misc[SORT_MISC_ACTIVE + p]) return;
    const size_t base = (size_t)blockIdx.x * SORT_SCAN_TILE + (size_t)threadIdx.x * 16;
    u32 q[16], sum = 0;
#pragma unroll
    for (int i = 0; i < 16; i++) {
        q[i] = base + i < words ? data[base + i] : 0;
        sum += q[i];
    }
    u32 total;
    u32 run = sort_block_excl(sum, s_wave, total);
#pragma unroll
    for (int i = 0; i < 16; i++) {
        if (base + i < words) data[base + i] = run;
        run += q[i];
    }
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

__global__ void __launch_bounds__(256) k_sort_scan_add(u32* data, size_t words, const u32* sums, const u32* misc, u32 p) {
    if (!misc[SORT_MISC_ACTIVE + p]) return;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < words) data[i] += sums[i / SORT_SCAN_TILE];
}

// exclusive prefix sums of data[0, words) in place; tmp: sort_scan_tmp_words(words) words
void sort_scan(u32* data, size_t words, u32* tmp, const u32* misc, u32 p, hipStream_t stream) {
    const size_t tiles = words ? sort_ceil_div(words, SORT_SCAN_TILE) : 1;
    hipLaunchKernelGGL(k_sort_scan_tile, dim3((u32)tiles), dim3(256), 0, stream, data, words, tmp, misc, p);
    if (tiles == 1) return;
    sort_scan(tmp, tiles, tmp + ((tiles + 63) & ~(size_t)63), misc, p, stream);
    hipLaunchKernelGGL(k_sort_scan_add, dim3((u32)sort_ceil_div(words, 256)), dim3(256), 0, stream, data, words,
                       (const u32*)tmp, misc, p);
}

template <class Index>
__global__ void __launch_bounds__(256) k_sort_emit(const u32* perm0, const u32* perm1, const u32* misc, Index* out, u32 n) {
    const u32 src = misc[SORT_MISC_FINAL];
    const u32* in = src == 0 ? perm0 : perm1;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = (Index)sort_row(in, src, i, n);
}

__global__ void __launch_bounds__(256) k_sort_gather(const Fr* __restrict__ in, const u32* __restrict__ perm,
                                                     Fr* __restrict__ out, u32 n) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const u32 row = perm[i];
    fp_store(out + i, fp_load(in + (row < n ? row : n - 1)));
}

}  // namespace

int sort_permutation_launch(const SortPlan& plan, const void* const* d_keys, void* d_perm, uint32_t perm_width,
                            uint32_t* d_status, void* d_scratch, hipStream_t stream) {
    char* const base = (char*)d_scratch;
    u32* const misc = (u32*)(base + plan.off_misc);
    u32* const ghist = (u32*)(base + plan.off_ghist);
    u32* const perm[2] = {(u32*)(base + plan.off_perm[0]), (u32*)(base + plan.off_perm[1])};
    uint8_t* const digits = (uint8_t*)(base + plan.off_digits);
    u32* const hist = (u32*)(base + plan.off_hist);
    u32* const scan = (u32*)(base + plan.off_scan);
    const u32 n = (u32)plan.n, tiles = (u32)plan.tiles;
    H2_HIP(hipMemsetAsync(misc, 0, SORT_MISC_WORDS * sizeof(u32), stream));
    H2_HIP(hipMemsetAsync(misc + SORT_MISC_BAD, 0xff, 8, stream));
    const uint8_t* bytes[SORT_MAX_KEYS] = {};
    u32 stride[SORT_MAX_KEYS] = {};
    if (n) {
        H2_HIP(hipMemsetAsync(ghist, 0, (size_t)plan.num_pos * 256 * sizeof(u32), stream));
        const u32 grid = tiles < SORT_SURVEY_BLOCKS ? tiles : SORT_SURVEY_BLOCKS;
        for (u32 k = 0; k < plan.num_keys; k++) {
            const u32 nbytes = sort_candidate_bytes(plan.form[k], plan.bits[k]);
            u32* const gh = ghist + 256 * (size_t)plan.first_pos[k];
            Fr* const canon = (Fr*)(base + plan.off_canon[k]);
            bytes[k] = (const uint8_t*)d_keys[k];
            stride[k] = 32;
            if (plan.form[k] == H2_ASSIGNED_FORM_COMPACT) {
                stride[k] = 8;
                hipLaunchKernelGGL(k_sort_survey<H2_ASSIGNED_FORM_COMPACT>, dim3(grid), dim3(256), 0, stream, d_keys[k], canon, n,
                                   tiles, nbytes, plan.bits[k], k, gh, misc);
            } else if (plan.form[k] == H2_ASSIGNED_FORM_MONTGOMERY) {
                bytes[k] = (const uint8_t*)canon;
                hipLaunchKernelGGL(k_sort_survey<H2_ASSIGNED_FORM_MONTGOMERY>, dim3(grid), dim3(256), 0, stream, d_keys[k], canon, n,
                                   tiles, nbytes, plan.bits[k], k, gh, misc);
            } else {
                hipLaunchKernelGGL(k_sort_survey<H2_ASSIGNED_FORM_CANONICAL>, dim3(grid), dim3(256), 0, stream, d_keys[k], canon, n,
                                   tiles, nbytes, plan.bits[k], k, gh, misc);
            }
        }
    }
    hipLaunchKernelGGL(k_sort_decide, dim3(1), dim3(256), 0, stream, (const u32*)ghist, misc, d_status, n ? plan.num_pos : 0u);
    if (n) {
        for (u32 p = 0; p < plan.num_pos; p++) {
            const SortPos at = plan.pos[p];
            hipLaunchKernelGGL(k_sort_hist, dim3(tiles), dim3(256), 0, stream, bytes[at.key] + at.byte, stride[at.key],
                               (const u32*)perm[0], (const u32*)perm[1], digits, hist, (const u32*)misc, p, n, tiles);
            sort_scan(hist, plan.hist_words, scan, misc, p, stream);
            hipLaunchKernelGGL(k_sort_scatter, dim3(tiles), dim3(256), 0, stream, (const u32*)perm[0], (const u32*)perm[1], perm[0],
                               perm[1], (const uint8_t*)digits, (const u32*)hist, (const u32*)misc, p, n, tiles);
        }
        const u32 grid = (u32)sort_ceil_div(n, 256);
        if (perm_width == 4)
            hipLaunchKernelGGL(k_sort_emit<u32>, dim3(grid), dim3(256), 0, stream, (const u32*)perm[0], (const u32*)perm[1],
                               (const u32*)misc, (u32*)d_perm, n);
        else
            hipLaunchKernelGGL(k_sort_emit<uint64_t>, dim3(grid), dim3(256), 0, stream, (const u32*)perm[0], (const u32*)perm[1],
                               (const u32*)misc, (uint64_t*)d_perm, n);
    }
    H2_HIP(hipGetLastError());
    return H2_OK;
}

int sort_gather_launch(const void* d_in, const uint32_t* d_perm, void* d_out, size_t n, hipStream_t stream) {
    if (n == 0) return H2_OK;
    hipLaunchKernelGGL(k_sort_gather, dim3((u32)sort_ceil_div(n, 256)), dim3(256), 0, stream, (const Fr*)d_in, d_perm, (Fr*)d_out,
                       (u32)n);
    H2_HIP(hipGetLastError());
    return H2_OK;
}

}  // namespace h2
