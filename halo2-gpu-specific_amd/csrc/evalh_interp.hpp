// evalh_interp.hpp -- the interpreter of an evaluate_h program (evalh_interp.hip's fallback kernels) and the host staging
// arena that mirrors its program arrays to the device; shared with check.hip, which runs the same program row by row.
#pragma once
#include <cstring>
#include <stdexcept>
#include <vector>

#include "common.hpp"
#include "evalh_desc.hpp"
#include "ntt.hpp"

namespace h2 {

struct EvalhProgram {  // everything the kernels need, device pointers
    const Fr* constants;
    const int32_t* rotations;
    const h2_calculation* calcs;
    const h2_value_source* value_parts;
    const h2_calculation* lookup_calcs;
    const uint32_t* lookup_sets;
    const h2_calculation* shuffle_calcs;
    const Fr* const* fixed;
    const Fr* const* advice;
    const Fr* const* instance;
    uint32_t n_calcs, n_value_parts, n_lookups, n_shuffles;
    uint32_t extended_k, rot_scale;
    size_t row_begin, row_end;   // rows to evaluate
    Fr y, beta, gamma, theta;
};

__device__ __forceinline__ size_t rot_idx(size_t idx, int32_t rot, uint32_t rot_scale, uint32_t extended_k) {
    // (idx + rot * rot_scale) mod 2^extended_k  (get_rotation_idx, evaluation.rs:40-42)
    long long v = (long long)idx + (long long)rot * (long long)rot_scale;
    return (size_t)(v & (((long long)1 << extended_k) - 1));
}

struct Interp {
    const EvalhProgram& p;
    const Fr* inter;  // this thread's column of the intermediates array
    size_t stride;    // distance between consecutive intermediates of one thread
    size_t idx;
    // the most recent intermediate stays in registers: expression trees flattened depth-first consume the previous
    // result in the very next calculation most of the time, which then skips the round trip through memory
    uint32_t last_index = 0xffffffffu;
    Fr last{};

    __device__ __forceinline__ Fr get(const h2_value_source& v) const {
        switch (v.kind) {
            case H2_VS_CONSTANT: return fp_load(p.constants + v.index);
            case H2_VS_INTERMEDIATE:
                if (v.index == last_index) return last;
                return fp_load(inter + (size_t)v.index * stride);
            case H2_VS_FIXED: return fp_load(p.fixed[v.index] + rot_idx(idx, p.rotations[v.rot], p.rot_scale, p.extended_k));
            case H2_VS_ADVICE: return fp_load(p.advice[v.index] + rot_idx(idx, p.rotations[v.rot], p.rot_scale, p.extended_k));
            default: return fp_load(p.instance[v.index] + rot_idx(idx, p.rotations[v.rot], p.rot_scale, p.extended_k));
        }
    }

    __device__ __forceinline__ Fr eval(const h2_calculation& k) const {
        Fr a = get(k.a);
        switch (k.op) {
            case H2_CALC_ADD: return fp_add(a, get(k.b));
            case H2_CALC_SUB: return fp_sub(a, get(k.b));
            case H2_CALC_MUL: return fp_mul(a, get(k.b));
            case H2_CALC_NEGATE: return fp_neg(a);
            case H2_CALC_LC_CHALLENGE: {
                Fr x = (k.challenge == H2_CHALLENGE_BETA) ? p.beta : p.gamma;
                if (k.power > 1) x = fp_pow_u32(x, k.power);
                return fp_mul(fp_add(a, x), get(k.b));
            }
            case H2_CALC_LC_THETA: return fp_add(fp_mul(a, p.theta), get(k.b));
            case H2_CALC_ADD_CHALLENGE: return fp_add(a, (k.challenge == H2_CHALLENGE_BETA) ? p.beta : p.gamma);
            default: return a;  // Store
        }
    }
};

// ---------------------------------------------------------------- host driver
struct Arena {  // bump allocator over one host staging block (`cap` bytes) mirrored to one device block
    char* host = nullptr;
    size_t cap = 0;
    char* dev = nullptr;
    size_t off = 0;
    template <class T>
    const T* put(const T* src, size_t count) {
        off = (off + 15) & ~(size_t)15;
        size_t bytes = count * sizeof(T);
        if (off + bytes > cap) throw std::runtime_error("evaluate_h program: internal staging overflow");
        if (bytes) memcpy(host + off, src, bytes);
        const T* d = reinterpret_cast<const T*>(dev + off);
        off += bytes;
        return d;
    }
};

// the pointer tables the argument kernels (k_evalh_perm, k_evalh_lookup) read, staged next to the program
struct EvalhArgTables {
    const Fr* const* perm_z;
    const Fr* const* perm_cols;   // the column of each permutation column (evaluation.rs:1060-1064)
    const Fr* const* perm_sigma;
    const Fr* const* lookup_z;
};

// Mirrors the program arrays and column pointer tables of a validated descriptor (evalh_desc.hpp) into `block` (device, `need`
// bytes: the caller's own formula) and returns the program over them, every member but the row range filled.  With `args`
// the argument kernels' tables follow.  The caller holds ctx's lock (the block and the staging memory are the slot's).
// The copy is QUEUED when this returns, not made: the host side is the slot's page-locked staging block, so `stream` is not
// waited for -- only the copy that read the staging block last (the previous call's, usually long done).
inline EvalhProgram evalh_stage_program(DeviceCtx* ctx, const h2_evalh_desc* d, char* block, size_t need, hipStream_t stream,
                                        EvalhArgTables* args = nullptr) {
    if (ctx->evalh_staged) H2_HIP(hipEventSynchronize(ctx->evalh_staged));
    Arena ar;
    ar.host = (char*)ctx->evalh_stage.get(need);
    ar.cap = need;
    ar.dev = block;
    auto put_table = [&](uint32_t table) {
        return (const Fr* const*)ar.put(evalh_table(d, table), evalh_table_count(d, table));
    };
    EvalhProgram p{};
    p.constants = (const Fr*)ar.put(d->constants, (size_t)d->n_constants * 4);
    p.rotations = ar.put(d->rotations, d->n_rotations);
    p.calcs = ar.put(d->calculations, d->n_calculations);
    p.value_parts = ar.put(d->value_parts, d->n_value_parts);
    p.lookup_calcs = ar.put(d->lookup_calcs, evalh_lookup_calc_count(d));
    p.lookup_sets = ar.put(d->lookup_sets, d->n_lookups);
    p.shuffle_calcs = ar.put(d->shuffle_calcs, 2 * (size_t)d->n_shuffles);
    p.fixed = put_table(evgen::T_FIXED);
    p.advice = put_table(evgen::T_ADVICE);
    p.instance = put_table(evgen::T_INSTANCE);
    if (args) {
        args->perm_z = put_table(evgen::T_PERM_Z);
        args->perm_sigma = put_table(evgen::T_PERM_SIGMA);
        std::vector<const uint64_t*> cols(d->n_perm_columns);
        for (uint32_t j = 0; d->n_perm_sets && j < d->n_perm_columns; j++) {
            const uint32_t ty = d->perm_col_type[j];
            cols[j] = evalh_column(d, ty == H2_ANY_ADVICE ? evgen::T_ADVICE : (ty == H2_ANY_FIXED ? evgen::T_FIXED : evgen::T_INSTANCE),
                                   d->perm_col_index[j]);
        }
        args->perm_cols = (const Fr* const*)ar.put(cols.data(), cols.size());
        args->lookup_z = put_table(evgen::T_LOOKUP_Z);
    }
    H2_HIP(hipMemcpyAsync(block, ar.host, ar.off, hipMemcpyHostToDevice, stream));
    if (!ctx->evalh_staged) H2_HIP(hipEventCreateWithFlags(&ctx->evalh_staged, hipEventDisableTiming));
    H2_HIP(hipEventRecord(ctx->evalh_staged, stream));
    p.n_calcs = d->n_calculations;
    p.n_value_parts = d->n_value_parts;
    p.n_lookups = d->n_lookups;
    p.n_shuffles = d->n_shuffles;
    p.extended_k = d->extended_k;
    p.rot_scale = 1u << (d->extended_k - d->k);
    p.y = fr_from_u64x4(d->y);
    p.beta = fr_from_u64x4(d->beta);
    p.gamma = fr_from_u64x4(d->gamma);
    p.theta = fr_from_u64x4(d->theta);
    return p;
}

}  // namespace h2
