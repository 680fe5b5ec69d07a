// evalh_interp.hpp -- the interpreter of an evaluate_h program (evalh.hip's fallback kernels) and the host staging
// arena that mirrors its program arrays to the device; shared with check.hip, which runs the same program row by row.
#pragma once
#include <cstring>
#include <vector>

#include "common.hpp"

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
struct Arena {  // bump allocator over one host staging block mirrored to one device block
    std::vector<char> host;
    char* dev = nullptr;
    size_t off = 0;
    template <class T>
    const T* put(const T* src, size_t count) {
        off = (off + 15) & ~(size_t)15;
        size_t bytes = count * sizeof(T);
        if (host.size() < off + bytes + 16) host.resize(off + bytes + 16);
        if (bytes) memcpy(host.data() + off, src, bytes);
        const T* d = reinterpret_cast<const T*>(dev + off);
        off += bytes;
        return d;
    }
};

}  // namespace h2
