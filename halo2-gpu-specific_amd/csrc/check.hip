// check.hip -- the checks of MockProver::verify (dev.rs:932-1340) over a witness already on the device.
//   k_check_nonzero_rows  compacts the rows < usable whose screened gate value (all gate polynomials Horner-folded in a
//                         random y: one base-domain evaluate_h) is non-zero into a row list
//   k_check_gate_rows     the evaluator program's interpreter (evalh_interp.hpp) on the listed rows only, one row per lane:
//                         every gate polynomial tested on its own
//   k_check_lookup        probes one compressed input column in the slot table of the compressed table (logup.hip's);
//                         launched input by input in (set, input) order, a row keeps its first miss (dev.rs:1170-1177)
//   k_check_shuffle_*     counts both sides' compressed values in one hash table, then reports the input rows whose value
//                         is counted differently (check.hpp: how this differs from the reference)
//   k_check_copies        value(c, r) against value(mapping(c, r)) for every permutation column and row (dev.rs:1272-1310)
// Every failure goes through check_append (append.hpp; check.hpp: the append scheme).
#include <algorithm>

#include "append.hpp"
#include "check.hpp"
#include "common.hpp"
#include "evalh_interp.hpp"
#include "logup.hpp"
#include "ntt.hpp"

namespace h2 {

__global__ void __launch_bounds__(256) k_check_nonzero_rows(const Fr* values, uint32_t usable, uint32_t* rows,
                                                            unsigned long long* row_count) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const bool take = i < usable && !fp_is_zero(fp_load(values + i));
    const unsigned long long slot = wave_slot(take, row_count);
    if (take) rows[slot] = i;        // at most `usable` rows are taken: the list never overflows
}

// Grid-stride over the listed rows in whole waves, so that every lane of a wave reaches the same appends.
__global__ void __launch_bounds__(256) k_check_gate_rows(EvalhProgram p, Fr* inter, const uint32_t* rows,
                                                         const unsigned long long* row_count, uint32_t kind,
                                                         unsigned long long* count, h2_check_record* out,
                                                         unsigned long long cap) {
    const size_t nthreads = (size_t)gridDim.x * blockDim.x;
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const unsigned long long listed = *row_count;
    Fr* my = inter + t;
    for (size_t base = t & ~(size_t)63; base < listed; base += nthreads) {
        const size_t i = base + (t & 63);
        const bool valid = i < listed;
        const uint32_t row = valid ? rows[i] : 0;
        Interp in{p, my, nthreads, row};
        if (valid) {
            for (uint32_t c = 0; c < p.n_calcs; c++) {
                Fr r = in.eval(p.calcs[c]);
                fp_store(my + (size_t)c * nthreads, r);
                in.last = r;
                in.last_index = c;
            }
        }
        for (uint32_t part = 0; part < p.n_value_parts; part++) {
            const bool fail = valid && !fp_is_zero(in.get(p.value_parts[part]));
            check_append(fail, kind, part, 0, row, count, out, cap);
        }
    }
}

// `failed`: one byte per row, set by the first input of the row that misses (launches of one lookup are stream-ordered)
__global__ void __launch_bounds__(256) k_check_lookup(const Fr* table, const Fr* input, uint32_t usable, uint32_t mask,
                                                      const uint32_t* slots, uint8_t* failed, uint32_t kind, uint32_t index,
                                                      uint32_t tag, unsigned long long* count, h2_check_record* out,
                                                      unsigned long long cap) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    bool miss = false;
    if (i < usable && !failed[i]) {
        const Fr key = fp_load(input + i);
        uint32_t h = key_hash(key) & mask;
        miss = true;
        for (;;) {
            const uint32_t cur = slots[h];
            if (cur == SLOT_EMPTY) break;
            if (fp_eq(fp_load(table + cur), key)) {
                miss = false;
                break;
            }
            h = (h + 1) & mask;
        }
        if (miss) failed[i] = 1;
    }
    check_append(miss, kind, index, tag, i, count, out, cap);
}

// The shuffle table: `cap` u32 slots, each SLOT_EMPTY or a reference to a row (input row r = r, shuffle row r = usable + r),
// and two u32 counters per slot (input side, shuffle side).
__device__ __forceinline__ Fr shuffle_key(const Fr* input, const Fr* shuffle, uint32_t usable, uint32_t ref) {
    return ref < usable ? fp_load(input + ref) : fp_load(shuffle + (ref - usable));
}

__global__ void __launch_bounds__(256) k_check_shuffle_count(const Fr* input, const Fr* shuffle, uint32_t usable, uint32_t side,
                                                             uint32_t mask, uint32_t* slots, uint32_t* counters) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const bool valid = i < usable;
    uint32_t hit = SLOT_EMPTY;
    if (valid) {
        const uint32_t ref = side ? usable + i : i;
        const Fr key = shuffle_key(input, shuffle, usable, ref);
        uint32_t h = key_hash(key) & mask;
        for (;;) {
            uint32_t cur = __atomic_load_n(&slots[h], __ATOMIC_RELAXED);
            if (cur == SLOT_EMPTY) cur = atomicCAS(&slots[h], SLOT_EMPTY, ref);
            if (cur == SLOT_EMPTY || fp_eq(shuffle_key(input, shuffle, usable, cur), key)) {
                hit = h;
                break;
            }
            h = (h + 1) & mask;
        }
    }
    // counters[2 hit + side] += 1, aggregated over the lanes of a wave that hit the slot of the first active lane (two
    // rounds: a padded column repeats one value), the rest individually -- as k_logup_count
    const uint32_t lane = threadIdx.x & 63;
    unsigned long long active = __ballot(valid);
#pragma unroll
    for (int round = 0; round < 2; round++) {
        if (active == 0) break;
        const int leader = __ffsll(active) - 1;
        const uint32_t k = __shfl(hit, leader, 64);
        const unsigned long long same = __ballot(valid && hit == k) & active;
        if ((int)lane == leader) atomicAdd(&counters[2 * (size_t)k + side], (uint32_t)__popcll(same));
        active &= ~same;
    }
    if ((active >> lane) & 1) atomicAdd(&counters[2 * (size_t)hit + side], 1u);
}

__global__ void __launch_bounds__(256) k_check_shuffle_report(const Fr* input, const Fr* shuffle, uint32_t usable, uint32_t mask,
                                                              const uint32_t* slots, const uint32_t* counters, uint32_t kind,
                                                              uint32_t group, uint32_t unit, unsigned long long* count,
                                                              h2_check_record* out, unsigned long long cap) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    bool fail = false;
    if (i < usable) {
        const Fr key = fp_load(input + i);
        uint32_t h = key_hash(key) & mask;
        for (;;) {      // every input value was inserted: the probe ends at its slot
            const uint32_t cur = slots[h];
            if (cur == SLOT_EMPTY || fp_eq(shuffle_key(input, shuffle, usable, cur), key)) break;
            h = (h + 1) & mask;
        }
        fail = slots[h] == SLOT_EMPTY || counters[2 * (size_t)h] != counters[2 * (size_t)h + 1];
    }
    check_append(fail, kind, group, unit, i, count, out, cap);
}

__global__ void __launch_bounds__(256) k_check_copies(const Fr* const* columns, uint32_t n_columns, const uint32_t* map_col,
                                                      const uint32_t* map_row, uint32_t n, uint32_t kind,
                                                      unsigned long long* count, h2_check_record* out, unsigned long long cap) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t total = (size_t)n_columns * n;
    bool fail = false;
    uint32_t c = 0, r = 0;
    if (i < total) {
        c = (uint32_t)(i / n);
        r = (uint32_t)(i - (size_t)c * n);
        const uint32_t mc = map_col[i], mr = map_row[i];
        // a mapping that leaves the columns is a failure of its cell, not a read out of bounds
        fail = mc >= n_columns || mr >= n || !fp_eq(fp_load(columns[c] + r), fp_load(columns[mc] + mr));
    }
    check_append(fail, kind, c, 0, r, count, out, cap);
}

// ------------------------------------------------------------------------------------------------- launchers
static uint32_t shuffle_capacity(size_t usable) { return logup_table_capacity(2 * usable); }   // both sides' rows
static size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

size_t check_scratch_bytes(size_t n) {
    const size_t lookup = align256((size_t)logup_table_capacity(n) * 4) + align256(n);
    const size_t shuffle = align256((size_t)shuffle_capacity(n) * 4) + (size_t)shuffle_capacity(n) * 8;
    return std::max(lookup, shuffle);
}

static int bad_sizes(const char* what) {
    set_last_error(std::string(what) + ": bad sizes");
    return H2_ERR_INVALID;
}

int check_nonzero_rows_launch(const Fr* d_values, size_t usable, uint32_t* d_rows, uint64_t* d_row_count, hipStream_t stream) {
    if (usable >= 0x7fffffffu) return bad_sizes("h2_dev_check_nonzero_rows");
    if (usable)
        hipLaunchKernelGGL(k_check_nonzero_rows, dim3((unsigned)((usable + 255) / 256)), dim3(256), 0, stream, d_values,
                           (uint32_t)usable, d_rows, (unsigned long long*)d_row_count);
    H2_HIP(hipGetLastError());
    return H2_OK;
}

// every value source of the program names something that exists: the interpreter reads what the indices say
static bool sources_ok(const h2_evalh_desc* d, const h2_value_source& v) {
    switch (v.kind) {
        case H2_VS_CONSTANT: return v.index < d->n_constants;
        case H2_VS_INTERMEDIATE: return v.index < d->n_calculations;
        case H2_VS_FIXED: return v.index < d->n_fixed && v.rot < d->n_rotations;
        case H2_VS_ADVICE: return v.index < d->n_advice && v.rot < d->n_rotations;
        case H2_VS_INSTANCE: return v.index < d->n_instance && v.rot < d->n_rotations;
        default: return false;
    }
}

int check_gates_args(const h2_evalh_desc* d) {
    if (d->extended_k != d->k || d->k > 28 || d->n_perm_sets || d->n_lookups || d->n_shuffles || d->reserved != nullptr) {
        set_last_error("h2_dev_check_gates: the descriptor must be a gate program on the base domain (extended_k == k, no "
                       "permutation, lookup or shuffle part)");
        return H2_ERR_INVALID;
    }
    if ((d->n_constants && !d->constants) || (d->n_rotations && !d->rotations) || (d->n_calculations && !d->calculations) ||
        (d->n_value_parts && !d->value_parts) || (d->n_fixed && !d->fixed) || (d->n_advice && !d->advice) ||
        (d->n_instance && !d->instance)) {
        set_last_error("h2_dev_check_gates: null program array");
        return H2_ERR_INVALID;
    }
    for (uint32_t i = 0; i < d->n_calculations; i++) {
        const h2_calculation& c = d->calculations[i];
        const bool unary = c.op == H2_CALC_NEGATE || c.op == H2_CALC_ADD_CHALLENGE || c.op == H2_CALC_STORE;
        if (c.op > H2_CALC_STORE || !sources_ok(d, c.a) || (!unary && !sources_ok(d, c.b))) {
            set_last_error("h2_dev_check_gates: calculation " + std::to_string(i) + " reads outside the program");
            return H2_ERR_INVALID;
        }
    }
    for (uint32_t i = 0; i < d->n_value_parts; i++)
        if (!sources_ok(d, d->value_parts[i])) {
            set_last_error("h2_dev_check_gates: value part " + std::to_string(i) + " reads outside the program");
            return H2_ERR_INVALID;
        }
    for (uint32_t i = 0; i < d->n_fixed; i++)
        if (!d->fixed[i]) return bad_sizes("h2_dev_check_gates: null fixed column");
    for (uint32_t i = 0; i < d->n_advice; i++)
        if (!d->advice[i]) return bad_sizes("h2_dev_check_gates: null advice column");
    for (uint32_t i = 0; i < d->n_instance; i++)
        if (!d->instance[i]) return bad_sizes("h2_dev_check_gates: null instance column");
    return H2_OK;
}

int check_gates_launch(DeviceCtx* ctx, const h2_evalh_desc* d, const uint32_t* d_rows, const uint64_t* d_row_count,
                       uint32_t circuit, uint64_t* d_count, h2_check_record* d_records, size_t cap, hipStream_t stream) {
    if (int rc = check_gates_args(d)) return rc;
    if (d->n_value_parts == 0) return H2_OK;

    const size_t n = (size_t)1 << d->k;
    const unsigned threads = 256, blocks = (unsigned)std::min<size_t>(256, (n + threads - 1) / threads);
    const size_t nthreads = (size_t)blocks * threads;
    const size_t need = 1024 + (size_t)d->n_constants * 32 + (size_t)d->n_rotations * 4 +
                        (size_t)d->n_calculations * sizeof(h2_calculation) + (size_t)d->n_value_parts * sizeof(h2_value_source) +
                        ((size_t)d->n_fixed + d->n_advice + d->n_instance) * 8 + 16 * 16;
    const size_t inter_bytes = (size_t)(d->n_calculations ? d->n_calculations : 1) * nthreads * sizeof(Fr);
    // the interpreter's work space is the library's (as h2_dev_evaluate_h's): per device, under its lock
    std::lock_guard<std::mutex> g(ctx->mu);
    char* block = (char*)ctx->evalh_scratch.lend(align256(need) + inter_bytes, stream);
    const EvalhProgram p = evalh_stage_program(ctx, d, block, need, stream);   // (a gate program: its lookup and shuffle parts are empty)
    hipLaunchKernelGGL(k_check_gate_rows, dim3(blocks), dim3(threads), 0, stream, p, (Fr*)(block + align256(need)), d_rows,
                       (const unsigned long long*)d_row_count, (uint32_t)H2_CHECK_GATE | circuit << 8,
                       (unsigned long long*)d_count, d_records, (unsigned long long)cap);
    H2_HIP(hipGetLastError());
    ctx->evalh_scratch.lent(stream);
    return H2_OK;
}

int check_columns_args(const char* what, size_t usable, size_t n, size_t scratch_bytes) {
    if (usable > n || n >= 0x7fffffffu) return bad_sizes(what);
    if (scratch_bytes < check_scratch_bytes(n)) {
        set_last_error(std::string(what) + ": scratch too small (h2_check_scratch_bytes)");
        return H2_ERR_INVALID;
    }
    return H2_OK;
}

int check_copies_args(size_t n_columns, size_t n) {
    if (n >= 0x7fffffffu || n_columns >= 0x10000u || (n_columns * n + 255) / 256 > 0x7fffffffu) return bad_sizes("h2_dev_check_copies");
    return H2_OK;
}

int check_lookup_launch(const Fr* d_table, const Fr* const* d_inputs, const uint32_t* tags, size_t n_inputs, size_t usable,
                        size_t n, uint32_t lookup_index, uint32_t circuit, void* d_scratch, size_t scratch_bytes, uint64_t* d_count,
                        h2_check_record* d_records, size_t cap, hipStream_t stream) {
    if (int rc = check_columns_args("h2_dev_check_lookup", usable, n, scratch_bytes)) return rc;
    if (!usable || !n_inputs) return H2_OK;
    const uint32_t slots_cap = logup_table_capacity(usable);
    uint32_t* slots = (uint32_t*)d_scratch;
    uint8_t* failed = (uint8_t*)d_scratch + align256((size_t)slots_cap * 4);
    logup_build_launch(d_table, usable, slots, slots_cap, stream);
    H2_HIP(hipMemsetAsync(failed, 0, usable, stream));
    const unsigned blocks = (unsigned)((usable + 255) / 256);
    for (size_t j = 0; j < n_inputs; j++)
        hipLaunchKernelGGL(k_check_lookup, dim3(blocks), dim3(256), 0, stream, d_table, d_inputs[j], (uint32_t)usable, slots_cap - 1,
                           slots, failed, (uint32_t)H2_CHECK_LOOKUP | circuit << 8, lookup_index, tags[j],
                           (unsigned long long*)d_count, d_records, (unsigned long long)cap);
    H2_HIP(hipGetLastError());
    return H2_OK;
}

int check_shuffle_launch(const Fr* d_input, const Fr* d_shuffle, size_t usable, size_t n, uint32_t group, uint32_t unit,
                         uint32_t circuit, void* d_scratch, size_t scratch_bytes, uint64_t* d_count, h2_check_record* d_records,
                         size_t cap, hipStream_t stream) {
    if (int rc = check_columns_args("h2_dev_check_shuffle", usable, n, scratch_bytes)) return rc;
    if (!usable) return H2_OK;
    const uint32_t slots_cap = shuffle_capacity(usable), mask = slots_cap - 1;
    uint32_t* slots = (uint32_t*)d_scratch;
    uint32_t* counters = (uint32_t*)((char*)d_scratch + align256((size_t)slots_cap * 4));
    H2_HIP(hipMemsetAsync(slots, 0xff, (size_t)slots_cap * 4, stream));
    H2_HIP(hipMemsetAsync(counters, 0, (size_t)slots_cap * 8, stream));
    const unsigned blocks = (unsigned)((usable + 255) / 256);
    for (uint32_t side = 0; side < 2; side++)
        hipLaunchKernelGGL(k_check_shuffle_count, dim3(blocks), dim3(256), 0, stream, d_input, d_shuffle, (uint32_t)usable, side,
                           mask, slots, counters);
    hipLaunchKernelGGL(k_check_shuffle_report, dim3(blocks), dim3(256), 0, stream, d_input, d_shuffle, (uint32_t)usable, mask,
                       slots, counters, (uint32_t)H2_CHECK_SHUFFLE | circuit << 8, group, unit, (unsigned long long*)d_count,
                       d_records, (unsigned long long)cap);
    H2_HIP(hipGetLastError());
    return H2_OK;
}

int check_copies_launch(const Fr* const* d_columns, size_t n_columns, const uint32_t* d_map_col, const uint32_t* d_map_row,
                        size_t n, uint32_t circuit, uint64_t* d_count, h2_check_record* d_records, size_t cap, hipStream_t stream) {
    if (int rc = check_copies_args(n_columns, n)) return rc;
    const size_t total = n_columns * n;
    if (total)
        hipLaunchKernelGGL(k_check_copies, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, d_columns,
                           (uint32_t)n_columns, d_map_col, d_map_row, (uint32_t)n, (uint32_t)H2_CHECK_COPY | circuit << 8,
                           (unsigned long long*)d_count, d_records, (unsigned long long)cap);
    H2_HIP(hipGetLastError());
    return H2_OK;
}

}  // namespace h2
