// rangecheck.hip -- what create_proof does to the witness of every `advice_column_range` after synthesis
// (plonk/prover.rs:1699-1783 and `sort`, :164-200): every value of the range is planted in the unused tail of the
// range-checked column, and the companion column becomes the counting sort of the usable rows.  The reference (and
// prover.complete_range_check_witness) do this on the host; here any number of (origin, companion) pairs of one circuit
// instance are completed by three launches on a stream:
//   k_rc_hist   reads the origin once: checks every usable row (in range, no high limb; the cells about to be planted unused
//               when synthesis did not say) and counts it -- the cells of the planted tail are counted as the values they
//               WILL hold, so nothing is written before every check has passed
//   k_rc_scan   one workgroup per pair: decides the pair's status, then turns its counters into exclusive offsets
//   k_rc_write  a pair whose status is OK: plants the tail of the origin and writes the companion's usable rows, each row
//               finding its bin in the offsets (a workgroup first brackets the bins of its 256 rows)
// A column is read and written in ITS form: canonical (n, 4) u64, Montgomery (n, 4) u64 or compact 1-D u64.
// Counters: a range of up to RC_LDS_BINS values is counted in LDS, workgroup by workgroup, and flushed once; a wider one
// (0 ..= 0xFFFF: 256 KiB of u32 counters, more than a CU's LDS) goes to global counters.  Either way the lanes of a wave
// that hit the bin of its first active lane add as ONE atomic (two rounds, as logup.hip): a column of equal rows, or one
// padded with zeros, costs a wave one or two atomics instead of 64 on one address.
#include <cstring>

#include "rangecheck.hpp"

namespace h2 {

namespace {

// (H2_RANGE_CHECK_FORM_CANONICAL is what is left)
constexpr uint32_t RC_MONTGOMERY = H2_RANGE_CHECK_FORM_MONTGOMERY, RC_COMPACT = H2_RANGE_CHECK_FORM_COMPACT;
constexpr uint32_t RC_LDS_BINS = 8192;        // at most 32 KiB of counters per workgroup: five workgroups a CU
constexpr uint32_t RC_SCAN_TILE = 256 * 16;   // k_rc_scan: 16 counters per lane and step
constexpr int RC_PAIRS_PER_LAUNCH = 8;
constexpr uint32_t RC_NONE = 0xffffffffu;
// status words 4 .. 7 of a pair: the first row of each kind, filled by k_rc_hist and judged by k_rc_scan
constexpr int ST_IN_USE = 4, ST_RANGE = 5, ST_NOT_PLANTED = 6, ST_NOT_ZERO = 7;

struct RcPair {
    void* origin;
    void* companion;
    uint64_t vmin, vmax, step;
    uint32_t* counts;      // nbins counters, the end sentinel and the padding of the last scan tile
    uint32_t* status;      // H2_RANGE_CHECK_STATUS_WORDS words
    uint32_t oform, cform;
    uint32_t lo, nvals;    // the planted rows are [lo, lo + nvals) = [lo, usable)
    uint32_t nbins, words;
    uint32_t pre, pre_row; // a status known before any row is read (NO_FIT, UNSUPPORTED) and its row
    uint32_t check_target; // first_unassigned unknown: the planted cells and the one below must be unused
    uint32_t index;
};
struct RcArgs {
    RcPair p[RC_PAIRS_PER_LAUNCH];
    uint32_t usable;
};

// -> the low 64 bits of a cell; `high`: something above them is set
__device__ __forceinline__ uint64_t rc_load(const void* col, uint32_t form, uint32_t r, bool& high) {
    if (form == RC_COMPACT) {
        high = false;
        return ((const uint64_t*)col)[r];
    }
    Fr v = fp_load((const Fr*)col + r);
    if (form == RC_MONTGOMERY) v = fp_from_mont(v);
    high = (v.l[2] | v.l[3] | v.l[4] | v.l[5] | v.l[6] | v.l[7]) != 0;
    return (uint64_t)v.l[0] | ((uint64_t)v.l[1] << 32);
}

__device__ __forceinline__ void rc_store(void* col, uint32_t form, uint32_t r, uint64_t x) {
    if (form == RC_COMPACT) {
        ((uint64_t*)col)[r] = x;
        return;
    }
    Fr v = fp_zero<FrParams>();
    v.l[0] = (uint32_t)x;
    v.l[1] = (uint32_t)(x >> 32);
    if (form == RC_MONTGOMERY) v = fp_to_mont(v);
    fp_store((Fr*)col + r, v);
}

// the value planted in row r of [lo, usable): range_check_assigner's values in descending row order, vmin in the last row
__device__ __forceinline__ uint64_t rc_planted(const RcPair& p, uint32_t r) {
    const uint32_t j = p.nvals - 1 - (r - p.lo);
    return j == p.nvals - 1 ? p.vmax : p.vmin + (uint64_t)j * p.step;
}

// count[bin] += 1 for the valid lanes of a wave; every lane of the wave must arrive
__device__ __forceinline__ void rc_wave_count(uint32_t* count, bool valid, uint32_t bin) {
    const uint32_t lane = threadIdx.x & 63;
    uint64_t active = __ballot(valid);
#pragma unroll
    for (int round = 0; round < 2; round++) {
        if (active == 0) break;
        const int leader = __ffsll((unsigned long long)active) - 1;
        const uint32_t k = __shfl(bin, leader, 64);
        const uint64_t same = __ballot(valid && bin == k) & active;
        if ((int)lane == leader) atomicAdd(&count[k], (uint32_t)__popcll(same));
        active &= ~same;
    }
    if ((active >> lane) & 1) atomicAdd(&count[bin], 1u);
}

// *word = min(*word, r) for the lanes of a wave that `hit`; every lane of the wave must arrive.  Rows ascend with the lane, so
// the first lane that hit holds the wave's minimum and is the only one to send it, and not even that when the word is already
// lower (it only ever falls, so a stale read costs an atomic and no more).  A fresh column has EVERY cell of its planted tail
// "not planted yet": lane by lane that is 32 768 atomics on one address for 0 ..= 0xFFFF, which run one after the other.
__device__ __forceinline__ void rc_wave_min(uint32_t* word, bool hit, uint32_t r) {
    const uint64_t hits = __ballot(hit);
    if (hits == 0) return;
    if ((int)(threadIdx.x & 63) == __ffsll((unsigned long long)hits) - 1 &&
        __hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > r)
        atomicMin(word, r);
}

// LDS: the counters of the widest pair of the launch that counts in LDS (dynamic, up to RC_LDS_BINS words) -- none when every
// pair counts in global memory, so that path keeps its full occupancy
__global__ void __launch_bounds__(256) k_rc_hist(RcArgs a) {
    extern __shared__ uint32_t s_count[];
    const RcPair& p = a.p[blockIdx.y];
    if (p.pre) return;
    const uint32_t usable = a.usable;
    const bool in_lds = p.nbins <= RC_LDS_BINS;
    if (in_lds) {
        for (uint32_t b = threadIdx.x; b < p.nbins; b += 256) s_count[b] = 0;
        __syncthreads();
    }
    uint32_t* count = in_lds ? s_count : p.counts;
    // the trip count is the same for every lane of a workgroup: rc_wave_count needs whole waves
    for (uint32_t base = blockIdx.x * 256; base < usable; base += gridDim.x * 256) {
        const uint32_t r = base + threadIdx.x;
        bool valid = r < usable;
        bool in_use = false, not_planted = false, not_zero = false, outside = false;
        uint64_t v = 0;
        if (valid) {
            const bool tail = r >= p.lo;
            if (tail) v = rc_planted(p, r);
            if (!tail || p.check_target) {
                bool high;
                const uint64_t x = rc_load(p.origin, p.oform, r, high);
                if (p.check_target && r + 1 >= p.lo) {
                    // the planted cells hold nothing but zeros, or exactly the planted values (the same columns proved again);
                    // the cell below them is zero
                    if (high || (!tail && x != 0) || (tail && x != v && x != 0)) in_use = true;
                    else if (tail && x != v) not_planted = true;
                    else if (tail && x != 0) not_zero = true;
                }
                if (!tail) {
                    v = x;
                    if (high || x < p.vmin || x > p.vmax) outside = true, valid = false;
                }
            }
        }
        if (p.check_target && base + 256 >= p.lo) {      // (the same for every lane of the workgroup)
            rc_wave_min(&p.status[ST_IN_USE], in_use, r);
            rc_wave_min(&p.status[ST_NOT_PLANTED], not_planted, r);
            rc_wave_min(&p.status[ST_NOT_ZERO], not_zero, r);
        }
        rc_wave_min(&p.status[ST_RANGE], outside, r);
        rc_wave_count(count, valid, (uint32_t)(v - p.vmin));
    }
    if (in_lds) {
        __syncthreads();
        for (uint32_t b = threadIdx.x; b < p.nbins; b += 256) {
            const uint32_t c = s_count[b];
            if (c) atomicAdd(&p.counts[b], c);
        }
    }
}

// One workgroup per pair.  Status words 0 .. 3: {code, first offending row (or 0xffffffff), pair index, 0}.
__global__ void __launch_bounds__(256) k_rc_scan(RcArgs a) {
    __shared__ uint32_t s_wave[4];
    __shared__ uint32_t s_code;
    const RcPair& p = a.p[blockIdx.y];
    const uint32_t t = threadIdx.x, lane = t & 63, wave = t >> 6;
    if (t == 0) {
        uint32_t* st = p.status;
        uint32_t code = p.pre, row = p.pre_row;
        if (!code) {
            const uint32_t in_use = st[ST_IN_USE], range = st[ST_RANGE], np_ = st[ST_NOT_PLANTED], nz = st[ST_NOT_ZERO];
            if (in_use != RC_NONE) code = H2_RANGE_CHECK_IN_USE, row = in_use;
            else if (np_ != RC_NONE && nz != RC_NONE) code = H2_RANGE_CHECK_IN_USE, row = np_ < nz ? np_ : nz;   // half planted
            else if (range != RC_NONE) code = H2_RANGE_CHECK_OUT_OF_RANGE, row = range;
            else row = RC_NONE;
        }
        st[0] = code;
        st[1] = row;
        st[2] = p.index;
        st[3] = 0;
        s_code = code;
    }
    __syncthreads();
    if (s_code) return;
    uint32_t carry = 0;
    uint4* cells = (uint4*)p.counts;
    for (uint32_t tile = 0; tile < p.words; tile += RC_SCAN_TILE) {
        uint4* mine = cells + (tile >> 2) + 4 * t;       // 16 consecutive counters
        uint4 q[4];
#pragma unroll
        for (int i = 0; i < 4; i++) q[i] = mine[i];
        uint32_t sum = 0;
#pragma unroll
        for (int i = 0; i < 4; i++) sum += q[i].x + q[i].y + q[i].z + q[i].w;
        uint32_t incl = sum;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const uint32_t o = (uint32_t)__shfl_up((int)incl, off, 64);
            if ((int)lane >= off) incl += o;
        }
        if (lane == 63) s_wave[wave] = incl;
        __syncthreads();
        uint32_t before = carry, total = 0;
#pragma unroll
        for (int w = 0; w < 4; w++) {
            if (w < (int)wave) before += s_wave[w];
            total += s_wave[w];
        }
        uint32_t run = before + incl - sum;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            uint4 o;
            o.x = run; run += q[i].x;
            o.y = run; run += q[i].y;
            o.z = run; run += q[i].z;
            o.w = run; run += q[i].w;
            mine[i] = o;
        }
        carry += total;
        __syncthreads();
    }
}

// the bin of row r: the last b in [first, last] with off[b] <= r (off[first] <= r < off[last + 1] on entry)
__device__ __forceinline__ uint32_t rc_find(const uint32_t* off, uint32_t first, uint32_t last, uint32_t r) {
    while (first < last) {
        const uint32_t mid = (first + last) >> 1;
        if (off[mid + 1] <= r) first = mid + 1;
        else last = mid;
    }
    return first;
}

__global__ void __launch_bounds__(256) k_rc_write(RcArgs a) {
    const RcPair& p = a.p[blockIdx.y];
    if (p.pre || p.status[0]) return;
    const uint32_t usable = a.usable;
    const uint32_t* off = p.counts;          // exclusive offsets; off[nbins] = usable
    for (uint32_t base = blockIdx.x * 256; base < usable; base += gridDim.x * 256) {
        const uint32_t end = base + 255 < usable - 1 ? base + 255 : usable - 1;
        // the bins of the workgroup's first and last row, by every lane on the same addresses
        const uint32_t b0 = rc_find(off, 0, p.nbins - 1, base), b1 = rc_find(off, b0, p.nbins - 1, end);
        const uint32_t r = base + threadIdx.x;
        if (r >= usable) continue;
        rc_store(p.companion, p.cform, r, p.vmin + rc_find(off, b0, b1, r));
        if (r >= p.lo) rc_store(p.origin, p.oform, r, rc_planted(p, r));
    }
}

uint32_t rc_grid(size_t usable) {
    const size_t blocks = (usable + 255) / 256;
    return (uint32_t)(blocks < 2048 ? (blocks ? blocks : 1) : 2048);
}

}  // namespace

size_t range_check_pair_words(uint64_t vmin, uint64_t vmax) {
    if (vmin > vmax || vmax - vmin >= RC_MAX_WIDTH) return 0;
    const size_t words = (size_t)(vmax - vmin) + 2;       // the bins and the end sentinel
    return (words + RC_SCAN_TILE - 1) / RC_SCAN_TILE * RC_SCAN_TILE;
}

size_t range_check_scratch_bytes(const uint64_t* vmin, const uint64_t* vmax, size_t pairs) {
    size_t words = 64;
    for (size_t i = 0; vmin && vmax && i < pairs; i++) words += range_check_pair_words(vmin[i], vmax[i]);
    return words * sizeof(uint32_t);
}

const char* range_check_validate(void* const* d_origins, void* const* d_companions, const uint32_t* origin_forms,
                                 const uint32_t* companion_forms, const uint64_t* vmin, const uint64_t* vmax, const uint64_t* step,
                                 size_t pairs, size_t usable, size_t n, const void* d_status, const void* d_scratch,
                                 size_t scratch_bytes) {
    if (!d_origins) return "d_origins is null";
    if (!d_companions) return "d_companions is null";
    if (!origin_forms) return "origin_forms is null";
    if (!companion_forms) return "companion_forms is null";
    if (!vmin) return "vmin is null";
    if (!vmax) return "vmax is null";
    if (!step) return "step is null";
    if (!d_status) return "d_status is null";
    if (!d_scratch) return "d_scratch is null";
    if (n == 0 || (n & (n - 1)) || n >= 0x7fffffffu) return "n is not a power of two below 2^31";
    if (usable > n) return "usable_rows exceeds n";
    if ((uintptr_t)d_status % 4 || (uintptr_t)d_scratch % 16) return "d_status / d_scratch is misaligned";
    for (size_t i = 0; i < pairs; i++) {
        if (!d_origins[i]) return "d_origins holds a null pointer";
        if (!d_companions[i]) return "d_companions holds a null pointer";
        if (d_origins[i] == d_companions[i]) return "a column is its own companion";
        if (origin_forms[i] > RC_COMPACT) return "origin_forms holds an unknown form code";
        if (companion_forms[i] > RC_COMPACT) return "companion_forms holds an unknown form code";
        if ((uintptr_t)d_origins[i] % (origin_forms[i] == RC_COMPACT ? 8 : 16) ||
            (uintptr_t)d_companions[i] % (companion_forms[i] == RC_COMPACT ? 8 : 16))
            return "a column is misaligned for its form";
        if (vmin[i] > vmax[i]) return "vmin exceeds vmax";
        if (step[i] == 0) return "step is zero";
    }
    if (scratch_bytes < range_check_scratch_bytes(vmin, vmax, pairs)) return "scratch too small (h2_range_check_scratch_bytes)";
    return nullptr;
}

int range_check_complete_launch(void* const* d_origins, void* const* d_companions, const uint32_t* origin_forms,
                                const uint32_t* companion_forms, const uint64_t* vmin, const uint64_t* vmax, const uint64_t* step,
                                const uint64_t* first_unassigned, size_t pairs, size_t usable, size_t n, uint32_t* d_status,
                                void* d_scratch, hipStream_t stream) {
    (void)n;
    if (pairs == 0) return H2_OK;
    H2_HIP(hipMemsetAsync(d_status, 0xff, pairs * H2_RANGE_CHECK_STATUS_WORDS * sizeof(uint32_t), stream));
    uint32_t* next = (uint32_t*)d_scratch;
    for (size_t first = 0; first < pairs; first += RC_PAIRS_PER_LAUNCH) {
        RcArgs a;
        memset(&a, 0, sizeof a);
        a.usable = (uint32_t)usable;
        const size_t count = pairs - first < (size_t)RC_PAIRS_PER_LAUNCH ? pairs - first : (size_t)RC_PAIRS_PER_LAUNCH;
        uint32_t* const begin = next;
        bool any = false;
        uint32_t lds_bins = 0;
        for (size_t j = 0; j < count; j++) {
            const size_t i = first + j;
            RcPair& p = a.p[j];
            p.origin = d_origins[i];
            p.companion = d_companions[i];
            p.vmin = vmin[i], p.vmax = vmax[i], p.step = step[i];
            p.oform = origin_forms[i], p.cform = companion_forms[i];
            p.status = d_status + i * H2_RANGE_CHECK_STATUS_WORDS;
            p.index = (uint32_t)i;
            p.pre_row = RC_NONE;
            const uint64_t fu = first_unassigned ? first_unassigned[i] : H2_RANGE_CHECK_UNASSIGNED_UNKNOWN;
            p.check_target = fu == H2_RANGE_CHECK_UNASSIGNED_UNKNOWN;
            const uint64_t width = p.vmax - p.vmin;
            if (width >= RC_MAX_WIDTH) {
                p.pre = H2_RANGE_CHECK_UNSUPPORTED;
                continue;
            }
            // range_check_assigner: vmin, vmin + step, ... below vmax, then vmax
            const uint64_t nvals = width / p.step + (width % p.step != 0) + 1;
            p.nbins = (uint32_t)width + 1;
            p.words = (uint32_t)range_check_pair_words(p.vmin, p.vmax);
            p.counts = next;
            next += p.words;
            // the reference asserts first_unassigned_offset <= lo - 1 (prover.rs:1731); the cell below the planted ones is spare
            if (nvals + 1 > usable || (!p.check_target && fu >= usable - nvals)) {
                p.pre = H2_RANGE_CHECK_NO_FIT;
                if (!p.check_target) p.pre_row = (uint32_t)(fu < RC_NONE ? fu : RC_NONE);
                continue;
            }
            p.nvals = (uint32_t)nvals;
            p.lo = (uint32_t)(usable - nvals);
            if (p.nbins <= RC_LDS_BINS && p.nbins > lds_bins) lds_bins = p.nbins;
            any = true;
        }
        if (next != begin) H2_HIP(hipMemsetAsync(begin, 0, (size_t)(next - begin) * sizeof(uint32_t), stream));
        const dim3 grid(rc_grid(usable), (unsigned)count);
        if (any) hipLaunchKernelGGL(k_rc_hist, grid, dim3(256), lds_bins * sizeof(uint32_t), stream, a);
        hipLaunchKernelGGL(k_rc_scan, dim3(1, (unsigned)count), dim3(256), 0, stream, a);
        if (any) hipLaunchKernelGGL(k_rc_write, grid, dim3(256), 0, stream, a);
        H2_HIP(hipGetLastError());
    }
    return H2_OK;
}

}  // namespace h2
