// evalh_interp.hip -- the quotient numerator h(X) on the extended coset, Evaluator::evaluate_h, by interpreter kernels.
//
// Reference: CPU twin plonk/evaluation.rs:778-1226; cuda driver plonk/evaluation.rs:1229-1985, which
// walks ProveExpression trees launching one elementwise kernel per AST node (evaluation_gpu.rs:594-803)
// and re-derives extended cosets on demand through a 5-entry cache.  Here every coset stays resident
// (288 GB of HBM) and the whole gate program runs in ONE pass over the extended domain:
//   k_evalh_expr     per index: interpret the flattened `Calculation` program (evaluation.rs:95-266),
//                    Horner-accumulate the gate value parts in y (:891-901), and emit the lookup /
//                    shuffle compressed expressions (:903-997)
//   k_evalh_perm     permutation argument terms (:1004-1085; cuda kernels eval_h_permutation_part1/2/
//                    left_prepare/left_right/part3, :1341-1486) fused into one kernel
//   k_evalh_lookup   logup terms (:1138-1182; cuda eval_h_logup / _z / _extra, :1655-1788)
//   k_evalh_shuffle  shuffle terms (:1197-1219; cuda eval_h_shuffles, :1935-1952)
// Intermediates of the interpreter live in a [calculation][thread] global array (coalesced, L2-resident);
// the program itself is read with wave-uniform (scalar) loads, so there is no divergence.
// These four kernels are the fallback: a program is normally run as kernels GENERATED for it (evalh_gen.cpp: straight-line
// code, intermediates in registers, all terms in one or a few launches), built by hipRTC on first use -- evalh_plan.hip.
#include <algorithm>

#include "common.hpp"
#include "evalh.hpp"
#include "evalh_interp.hpp"
#include "ntt.hpp"

namespace h2 {

// lookup tables layout: [slot][idx], slots per lookup t: table, product_0, sum_0, product_1, sum_1, ...
// (slot base of lookup t = sum_{t' < t} (1 + 2 * sets[t'])) -- the same order as lookup_calcs
__global__ void __launch_bounds__(256) k_evalh_expr(EvalhProgram p, Fr* inter, Fr* values, Fr* lk_out, Fr* sh_out) {
    const size_t size = (size_t)1 << p.extended_k;
    const size_t nthreads = (size_t)gridDim.x * blockDim.x;
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    Fr* my = inter + t;
    for (size_t idx = p.row_begin + t; idx < p.row_end; idx += nthreads) {
        Interp in{p, my, nthreads, idx};
        for (uint32_t i = 0; i < p.n_calcs; i++) {
            Fr r = in.eval(p.calcs[i]);
            fp_store(my + (size_t)i * nthreads, r);
            in.last = r;
            in.last_index = i;
        }
        Fr value = fp_zero<FrParams>();
        for (uint32_t i = 0; i < p.n_value_parts; i++) value = fp_add(fp_mul(value, p.y), in.get(p.value_parts[i]));
        fp_store(values + idx, value);
        uint32_t slot = 0;
        for (uint32_t lk = 0; lk < p.n_lookups; lk++) {
            uint32_t cnt = 1 + 2 * p.lookup_sets[lk];
            for (uint32_t j = 0; j < cnt; j++, slot++) fp_store(lk_out + (size_t)slot * size + idx, in.eval(p.lookup_calcs[slot]));
        }
        for (uint32_t i = 0; i < 2 * p.n_shuffles; i++) fp_store(sh_out + (size_t)i * size + idx, in.eval(p.shuffle_calcs[i]));
    }
}

struct PermArgs {
    Fr* values;
    const Fr* const* perm_z;
    const Fr* const* perm_cols;   // resolved column coset per permutation column
    const Fr* const* perm_sigma;
    const Fr *l0, *l_last, *l_active_row;
    const Fr *tw_lo, *tw_hi;      // extended_omega^i tables (NTT plan)
    uint32_t n_sets, n_columns, chunk_len, extended_k, rot_scale;
    int32_t last_rotation;
    size_t row_begin, row_end;
    Fr y, beta, gamma, delta, delta_start;  // delta_start = beta * ZETA
};

__global__ void __launch_bounds__(256) k_evalh_perm(PermArgs a) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    const Fr one = fp_one<FrParams>();
    for (size_t idx = a.row_begin + (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < a.row_end; idx += stride) {
        const size_t r_next = rot_idx(idx, 1, a.rot_scale, a.extended_k);
        const size_t r_last = rot_idx(idx, a.last_rotation, a.rot_scale, a.extended_k);
        Fr value = fp_load(a.values + idx);
        const Fr l0 = fp_load(a.l0 + idx);
        {   // l_0(X) * (1 - z_0(X))
            Fr z0 = fp_load(a.perm_z[0] + idx);
            value = fp_add(fp_mul(value, a.y), fp_mul(fp_sub(one, z0), l0));
            // l_last(X) * (z_l(X)^2 - z_l(X))
            Fr zl = fp_load(a.perm_z[a.n_sets - 1] + idx);
            value = fp_add(fp_mul(value, a.y), fp_mul(fp_sub(fp_sqr(zl), zl), fp_load(a.l_last + idx)));
        }
        for (uint32_t s = 1; s < a.n_sets; s++) {  // l_0(X) * (z_i(X) - z_{i-1}(w^last X))
            Fr d = fp_sub(fp_load(a.perm_z[s] + idx), fp_load(a.perm_z[s - 1] + r_last));
            value = fp_add(fp_mul(value, a.y), fp_mul(d, l0));
        }
        // beta_term = extended_omega^idx
        Fr beta_term;
        if (a.extended_k <= 12) {
            beta_term = fp_load(a.tw_lo + idx);
        } else {
            beta_term = fp_mul(fp_load(a.tw_lo + (idx & 4095)), fp_load(a.tw_hi + (idx >> 12)));
        }
        Fr current_delta = fp_mul(a.delta_start, beta_term);
        const Fr lar = fp_load(a.l_active_row + idx);
        for (uint32_t s = 0; s < a.n_sets; s++) {
            uint32_t c0 = s * a.chunk_len, c1 = c0 + a.chunk_len;
            if (c1 > a.n_columns) c1 = a.n_columns;
            Fr left = fp_load(a.perm_z[s] + r_next), right = fp_load(a.perm_z[s] + idx);
            for (uint32_t j = c0; j < c1; j++) {
                Fr v = fp_load(a.perm_cols[j] + idx);
                Fr sg = fp_load(a.perm_sigma[j] + idx);
                left = fp_mul(left, fp_add(fp_add(v, fp_mul(a.beta, sg)), a.gamma));
                right = fp_mul(right, fp_add(fp_add(v, current_delta), a.gamma));
                current_delta = fp_mul(current_delta, a.delta);
            }
            value = fp_add(fp_mul(value, a.y), fp_mul(fp_sub(left, right), lar));
        }
        fp_store(a.values + idx, value);
    }
}

struct LookupArgs {
    Fr* values;
    const Fr* const* zs;     // sets_len z cosets of this lookup
    const Fr* m;
    const Fr* table;         // lk_out slots of this lookup: table, product_0, sum_0, product_1, ...
    const Fr *l0, *l_last, *l_active_row;
    uint32_t sets_len, extended_k, rot_scale;
    int32_t last_rotation;
    size_t row_begin, row_end;
    Fr y;
};

__global__ void __launch_bounds__(256) k_evalh_lookup(LookupArgs a) {
    const size_t size = (size_t)1 << a.extended_k;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t idx = a.row_begin + (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < a.row_end; idx += stride) {
        const size_t r_next = rot_idx(idx, 1, a.rot_scale, a.extended_k);
        const size_t r_last = rot_idx(idx, a.last_rotation, a.rot_scale, a.extended_k);
        Fr value = fp_load(a.values + idx);
        const Fr l0 = fp_load(a.l0 + idx), lar = fp_load(a.l_active_row + idx);
        const Fr z0 = fp_load(a.zs[0] + idx);
        value = fp_add(fp_mul(value, a.y), fp_mul(z0, l0));
        value = fp_add(fp_mul(value, a.y), fp_mul(fp_load(a.zs[a.sets_len - 1] + idx), fp_load(a.l_last + idx)));
        {
            Fr table = fp_load(a.table + idx);
            Fr prod = fp_load(a.table + size + idx), sum = fp_load(a.table + 2 * size + idx);
            Fr d = fp_sub(fp_load(a.zs[0] + r_next), z0);
            Fr t = fp_mul(fp_add(fp_mul(d, table), fp_load(a.m + idx)), prod);
            t = fp_sub(t, fp_mul(table, sum));
            value = fp_add(fp_mul(value, a.y), fp_mul(t, lar));
        }
        for (uint32_t i = 1; i < a.sets_len; i++) {
            Fr d = fp_sub(fp_load(a.zs[i] + idx), fp_load(a.zs[i - 1] + r_last));
            value = fp_add(fp_mul(value, a.y), fp_mul(d, l0));
        }
        for (uint32_t i = 1; i < a.sets_len; i++) {
            Fr d = fp_sub(fp_load(a.zs[i] + r_next), fp_load(a.zs[i] + idx));
            Fr t = fp_sub(fp_mul(d, fp_load(a.table + (size_t)(1 + 2 * i) * size + idx)),
                          fp_load(a.table + (size_t)(2 + 2 * i) * size + idx));
            value = fp_add(fp_mul(value, a.y), fp_mul(t, lar));
        }
        fp_store(a.values + idx, value);
    }
}

struct ShuffleArgs {
    Fr* values;
    const Fr* z;
    const Fr *input, *shuffle;
    const Fr *l0, *l_last, *l_active_row;
    uint32_t extended_k, rot_scale;
    size_t row_begin, row_end;
    Fr y;
};

__global__ void __launch_bounds__(256) k_evalh_shuffle(ShuffleArgs a) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    const Fr one = fp_one<FrParams>();
    for (size_t idx = a.row_begin + (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < a.row_end; idx += stride) {
        const size_t r_next = rot_idx(idx, 1, a.rot_scale, a.extended_k);
        Fr value = fp_load(a.values + idx);
        const Fr z = fp_load(a.z + idx);
        value = fp_add(fp_mul(value, a.y), fp_mul(fp_sub(one, z), fp_load(a.l0 + idx)));
        value = fp_add(fp_mul(value, a.y), fp_mul(fp_sub(fp_sqr(z), z), fp_load(a.l_last + idx)));
        Fr t = fp_sub(fp_mul(fp_load(a.z + r_next), fp_load(a.shuffle + idx)), fp_mul(z, fp_load(a.input + idx)));
        value = fp_add(fp_mul(value, a.y), fp_mul(t, fp_load(a.l_active_row + idx)));
        fp_store(a.values + idx, value);
    }
}

// ---------------------------------------------------------------- host driver
// Rows [row_begin, row_end) of a validated descriptor (evalh_desc.hpp) on the four kernels above; the caller holds ctx's lock
// (the work space is the slot's).
int evalh_interpret(DeviceCtx* ctx, const h2_evalh_desc* d, Fr* d_values, size_t row_begin, size_t row_end, hipStream_t stream) {
    const size_t size = (size_t)1 << d->extended_k, rows = row_end - row_begin;
    // ---- stage the program and pointer tables (a few KB) into one device block
    const size_t n_lookup_calcs = evalh_lookup_calc_count(d), n_lookup_z = evalh_lookup_z_count(d);
    size_t need = 4096 + d->n_constants * 32 + d->n_rotations * 4 + (d->n_calculations + n_lookup_calcs + 2 * d->n_shuffles) * sizeof(h2_calculation) +
                  d->n_value_parts * sizeof(h2_value_source) + d->n_lookups * 4 +
                  ((size_t)d->n_fixed + d->n_advice + d->n_instance + d->n_perm_sets + 2 * (size_t)d->n_perm_columns + n_lookup_z +
                   d->n_lookups + d->n_shuffles) * 8 + 64 * 16;
    // ---- work space: interpreter intermediates + lookup / shuffle compressed expressions
    // (one lane per row up to 2048 workgroups, a grid-stride loop beyond: k_evalh_expr's intermediates are [calculation][lane], so
    //  the work space follows the rows of the call -- 16 rows of a 1650-calculation program used to borrow 26 GiB)
    const unsigned threads = 256, blocks = (unsigned)std::max<size_t>(1, std::min<size_t>(256 * 8, (rows + threads - 1) / threads));
    const size_t nthreads = (size_t)blocks * threads;
    size_t inter_bytes = (size_t)(d->n_calculations ? d->n_calculations : 1) * nthreads * sizeof(Fr);
    size_t lk_bytes = n_lookup_calcs ? n_lookup_calcs * size * sizeof(Fr) : 256;
    size_t sh_bytes = d->n_shuffles ? 2 * (size_t)d->n_shuffles * size * sizeof(Fr) : 256;
    auto align = [](size_t v) { return (v + 255) & ~(size_t)255; };
    size_t total = align(need) + align(inter_bytes) + align(lk_bytes) + align(sh_bytes);
    char* block = (char*)ctx->evalh_scratch.lend(total, stream);  // (the previous borrower's kernels may still be queued elsewhere)
    Fr* d_inter = (Fr*)(block + align(need));
    Fr* d_lk = (Fr*)((char*)d_inter + align(inter_bytes));
    Fr* d_sh = (Fr*)((char*)d_lk + align(lk_bytes));

    EvalhArgTables tab{};
    EvalhProgram p = evalh_stage_program(ctx, d, block, need, stream, &tab);
    p.row_begin = row_begin;
    p.row_end = row_end;
    const uint32_t rot_scale = p.rot_scale;

    const int32_t last_rotation = -((int32_t)d->blinding_factors + 1);
    PlanRef pl;  // the power tables of extended_omega: pinned until the kernels that read them are launched
    if (d->n_perm_sets) pl = ntt_get_plan(ctx, d->extended_k, d->extended_omega, stream);
    {
        hipLaunchKernelGGL(k_evalh_expr, dim3(blocks), dim3(threads), 0, stream, p, d_inter, d_values, d_lk, d_sh);
    }

    unsigned eblocks = (unsigned)std::min<size_t>((rows + 255) / 256, 0x7fffffffu);
    if (d->n_perm_sets) {
        PermArgs a{};
        a.row_begin = row_begin;
        a.row_end = row_end;
        a.values = d_values;
        a.perm_z = tab.perm_z;
        a.perm_cols = tab.perm_cols;
        a.perm_sigma = tab.perm_sigma;
        a.l0 = (const Fr*)d->l0;
        a.l_last = (const Fr*)d->l_last;
        a.l_active_row = (const Fr*)d->l_active_row;
        a.tw_lo = pl->tw_lo;
        a.tw_hi = pl->tw_hi;
        a.n_sets = d->n_perm_sets;
        a.n_columns = d->n_perm_columns;
        a.chunk_len = d->chunk_len;
        a.extended_k = d->extended_k;
        a.rot_scale = rot_scale;
        a.last_rotation = last_rotation;
        a.y = p.y;
        a.beta = p.beta;
        a.gamma = p.gamma;
        a.delta = fr_from_u64x4(d->delta);
        a.delta_start = fp_mul(p.beta, fr_from_u64x4(d->zeta));  // evaluation.rs:1012
        hipLaunchKernelGGL(k_evalh_perm, dim3(eblocks), dim3(256), 0, stream, a);
    }
    size_t zoff = 0, slot = 0;
    for (uint32_t lk = 0; lk < d->n_lookups; lk++) {
        LookupArgs a{};
        a.row_begin = row_begin;
        a.row_end = row_end;
        a.values = d_values;
        a.zs = tab.lookup_z + zoff;
        a.m = (const Fr*)d->lookup_m[lk];
        a.table = d_lk + slot * size;
        a.l0 = (const Fr*)d->l0;
        a.l_last = (const Fr*)d->l_last;
        a.l_active_row = (const Fr*)d->l_active_row;
        a.sets_len = d->lookup_sets[lk];
        a.extended_k = d->extended_k;
        a.rot_scale = rot_scale;
        a.last_rotation = last_rotation;
        a.y = p.y;
        hipLaunchKernelGGL(k_evalh_lookup, dim3(eblocks), dim3(256), 0, stream, a);
        zoff += d->lookup_sets[lk];
        slot += 1 + 2 * (size_t)d->lookup_sets[lk];
    }
    for (uint32_t sh = 0; sh < d->n_shuffles; sh++) {
        ShuffleArgs a{};
        a.row_begin = row_begin;
        a.row_end = row_end;
        a.values = d_values;
        a.z = (const Fr*)d->shuffle_z[sh];
        a.input = d_sh + (size_t)(2 * sh) * size;
        a.shuffle = d_sh + (size_t)(2 * sh + 1) * size;
        a.l0 = (const Fr*)d->l0;
        a.l_last = (const Fr*)d->l_last;
        a.l_active_row = (const Fr*)d->l_active_row;
        a.extended_k = d->extended_k;
        a.rot_scale = rot_scale;
        a.y = p.y;
        hipLaunchKernelGGL(k_evalh_shuffle, dim3(eblocks), dim3(256), 0, stream, a);
    }
    H2_HIP(hipGetLastError());
    ctx->evalh_scratch.lent(stream);
    return H2_OK;
}

}  // namespace h2
