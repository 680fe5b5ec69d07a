// values.hpp -- the fused evaluator of witness arithmetic (values.py: Value; DESIGN.md 3b, "Computing a witness"): a
// straight-line program of field operations over m rows, one lane per row (h2_dev_values_eval) or one row after another on
// the host (h2_values_eval).  The argument checks and the lowering (values_host.cpp) are the only thing between a caller's
// program and the kernel's LDS and global accesses; the kernel and the host twin then run the SAME function, val_run_row, on
// the same lowered program, so their results agree bit for bit (the kernel of a program without integer ops is the
// instantiation that leaves the integer steps out; a step both have is the same code).
// Inside a program a value is a FIELD value, a reduced Montgomery residue, or an INTEGER, the canonical representative in
// [0, r) as plain words; the lowering tracks which and refuses a mismatch, the kernel does not look.  The lowered program has
// ONE multiplier site, fp_reduce_once(fp_mul_wide(x, y)), which takes any x < 2^256 and a reduced y: a product (x, y), a
// square (x, x), a leaf conversion (raw words, R^2), a canonical output or TO_INT (x, 1), TO_FIELD (x, R^2) and TO_INT of a
// canonical leaf (raw words, R: the words mod r) all go through it.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "../../include/halo2_hip.h"
#include "field.hpp"

namespace h2 {

constexpr uint32_t VAL_MAX_LEAVES = 16, VAL_MAX_OPS = 128, VAL_MAX_CONSTS = 16, VAL_MAX_OUTPUTS = 4;
// 6 slots: one in registers, five of 8 KiB per workgroup in LDS (DESIGN.md has the register count this was settled against)
constexpr uint32_t VAL_SLOTS = 6, VAL_THREADS = 256, VAL_MAX_BLOCKS = 1024;
constexpr uint32_t VAL_MAX_STEPS = VAL_MAX_OPS + VAL_MAX_OUTPUTS;
// the lowered program's own constants, after the caller's: R^2 (a leaf conversion, TO_FIELD), the integer 1 (a canonical
// output, TO_INT) and R mod r (TO_INT of a canonical leaf: raw words * R * R^-1)
constexpr uint32_t VAL_CONST_RR = VAL_MAX_CONSTS, VAL_CONST_RAW_ONE = VAL_MAX_CONSTS + 1, VAL_CONST_MONT_ONE = VAL_MAX_CONSTS + 2,
                   VAL_CONSTS = VAL_MAX_CONSTS + 3;

// operand of a lowered step: kind << 8 | index.  RAW_LEAF (lowered only): the leaf's words as they stand, no conversion
constexpr uint32_t VAL_K_LEAF = 0, VAL_K_CONST = 1, VAL_K_SLOT = 2, VAL_K_LAST = 3, VAL_K_RAW_LEAF = 4;
constexpr uint8_t VAL_NONE = 0xff;
constexpr uint8_t VAL_OP_COPY = 0xfe;  // lowered only: r = a (an output that needs no product, TO_INT of a compact leaf)

struct ValLeaf {
    const void* p;     // element `first` of the caller's buffer
    uint64_t stride;   // elements between rows
    uint32_t form;
    uint32_t pad;
};
struct ValStep {
    uint8_t op;
    uint8_t dst;       // slot, or VAL_NONE: the result is read from `last` only, or stored only
    uint8_t store;     // output index, or VAL_NONE
    uint8_t n;         // operands
    uint16_t opnd[3];  // EXTRACT: n = 1, opnd[1] = lo, opnd[2] = the number of bits
    uint16_t pad;
};
struct ValProgram {
    Fr konst[VAL_CONSTS];
    ValLeaf leaf[VAL_MAX_LEAVES];
    void* out[VAL_MAX_OUTPUTS];   // element `first` of each output
    ValStep step[VAL_MAX_STEPS];
    uint32_t num_steps;
    uint32_t has_integer;         // an op code from 16 on: the program runs val_run_row<true>
    uint32_t pad[2];
};

H2_DEV Fr val_load32(const void* p) {
#if defined(__HIP_DEVICE_COMPILE__)
    return fp_load((const Fr*)p);
#else
    Fr r;                     // host buffers are 8-byte aligned only
    memcpy(r.l, p, 32);
    return r;
#endif
}
H2_DEV void val_store32(void* p, const Fr& v) {
#if defined(__HIP_DEVICE_COMPILE__)
    fp_store((Fr*)p, v);
#else
    memcpy(p, v.l, 32);
#endif
}

// the raw words of row `row` of a leaf
H2_DEV Fr val_leaf_words(const ValLeaf& l, size_t row) {
    const size_t e = row * l.stride;
    if (l.form == H2_ASSIGNED_FORM_COMPACT) {
        uint64_t x;
#if defined(__HIP_DEVICE_COMPILE__)
        x = ((const uint64_t*)l.p)[e];
#else
        memcpy(&x, (const char*)l.p + 8 * e, 8);
#endif
        Fr v = fp_zero<FrParams>();
        v.l[0] = (uint32_t)x;
        v.l[1] = (uint32_t)(x >> 32);
        return v;
    }
    return val_load32((const char*)l.p + 32 * e);
}

// the 32-bit word at bit offset s (0 .. 31) of hi:lo
H2_DEV uint32_t val_funnel(uint32_t hi, uint32_t lo, uint32_t s) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_alignbit(hi, lo, s);
#else
    return (uint32_t)(((uint64_t)hi << 32 | lo) >> s);
#endif
}

// (v >> lo) mod 2^n, 0 <= lo <= 255, 1 <= n <= 256.  lo and n come from the program: the word shift is three scalar
// branches over statically indexed words (no indexed private copy), the bit shift a funnel over adjacent words
H2_DEV Fr val_extract(Fr v, uint32_t lo, uint32_t n) {
    const uint32_t words = lo >> 5, bits = lo & 31;
    if (words & 4) {
#pragma unroll
        for (int i = 0; i < 8; i++) v.l[i] = i + 4 < 8 ? v.l[i + 4] : 0;
    }
    if (words & 2) {
#pragma unroll
        for (int i = 0; i < 8; i++) v.l[i] = i + 2 < 8 ? v.l[i + 2] : 0;
    }
    if (words & 1) {
#pragma unroll
        for (int i = 0; i < 8; i++) v.l[i] = i + 1 < 8 ? v.l[i + 1] : 0;
    }
    Fr r;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const uint32_t w = val_funnel(i + 1 < 8 ? v.l[i + 1] : 0, v.l[i], bits);
        const uint32_t keep = n > 32u * i ? n - 32u * i : 0;   // bits of word i that stay
        r.l[i] = keep >= 32 ? w : w & ((1u << keep) - 1);
    }
    return r;
}

// 1 if a < b as 256-bit integers, else 0
H2_DEV uint32_t val_less(const Fr& a, const Fr& b) {
    uint32_t borrow = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const uint64_t t = (uint64_t)a.l[i] - b.l[i] - borrow;
        borrow = (uint32_t)(t >> 32) & 1;
    }
    return borrow;
}

// EXTRACT (lo, n), LT, AND, OR, XOR of integers below r
H2_DEV Fr val_integer_op(uint32_t op, const Fr& a, const Fr& b, uint32_t lo, uint32_t n) {
    Fr r = a;
    switch (op) {
        case H2_VALUES_EXTRACT: r = val_extract(a, lo, n); break;
        case H2_VALUES_LT:
            r = fp_zero<FrParams>();
            r.l[0] = val_less(a, b);
            break;
        case H2_VALUES_AND:
#pragma unroll
            for (int i = 0; i < 8; i++) r.l[i] = a.l[i] & b.l[i];  // <= a < r
            break;
        case H2_VALUES_OR:
#pragma unroll
            for (int i = 0; i < 8; i++) r.l[i] = a.l[i] | b.l[i];
            r = fp_reduce_once(r);  // a, b < r < 2^254: a | b < 2^254 < 2 r
            break;
        default:
#pragma unroll
            for (int i = 0; i < 8; i++) r.l[i] = a.l[i] ^ b.l[i];
            r = fp_reduce_once(r);
            break;
    }
    return r;
}

// One row of a lowered (validated) program.  `slots`: load(i) / store(i, v) of this row's slot i.  Everything that steers
// the control flow comes from the program, which is the same for every row: on the device the branches are uniform.
// INTS = false leaves out what only a program with an op code from 16 on reaches (P.has_integer): the kernel of the field
// programs is then, instruction for instruction, the kernel there was before there were integers -- with the integer steps
// in, the allocator moves the field steps' values about more, and they were measured 4 to 9 % slower.
template <bool INTS, class Slots>
H2_DEV void val_run_row(const ValProgram& P, size_t row, Slots& slots) {
    Fr last = fp_zero<FrParams>();
    for (uint32_t s = 0; s < P.num_steps; s++) {
        const ValStep st = P.step[s];
        if (INTS && st.op >= H2_VALUES_EXTRACT && st.op <= H2_VALUES_XOR) {
            // An integer step, apart from the field steps below.  Its operands are slots or `last` (the lowering refuses leaves and constants), it has no
            // product, and it stores nothing (an output is a step of its own)
            const Fr ia = st.opnd[0] >> 8 == VAL_K_SLOT ? slots.load(st.opnd[0] & 0xff) : last;
            Fr ib = ia;
            if (st.n > 1) ib = st.opnd[1] >> 8 == VAL_K_SLOT ? slots.load(st.opnd[1] & 0xff) : last;
            last = val_integer_op(st.op, ia, ib, st.opnd[1], st.opnd[2]);
            if (st.dst != VAL_NONE) slots.store(st.dst, last);
            continue;
        }
        Fr a = fp_zero<FrParams>(), b = a, c = a, r = a;
        // micro-steps 0..2 fetch (and convert) the operands, 3 is the product of the operation itself: one multiplier site
#pragma unroll 1
        for (uint32_t k = 0; k < 4; k++) {
            Fr x, y;
            bool mul;
            if (k < 3) {
                if (k >= st.n) continue;
                const uint32_t word = k == 0 ? st.opnd[0] : k == 1 ? st.opnd[1] : st.opnd[2];  // no indexed private copy
                const uint32_t kind = word >> 8, idx = word & 0xff;
                mul = false;
                y = P.konst[VAL_CONST_RR];
                if (kind == VAL_K_LEAF || (INTS && kind == VAL_K_RAW_LEAF)) {
                    x = val_leaf_words(P.leaf[idx], row);
                    mul = (!INTS || kind == VAL_K_LEAF) && P.leaf[idx].form != H2_ASSIGNED_FORM_MONTGOMERY;
                } else if (kind == VAL_K_CONST) {
                    x = P.konst[idx];
                } else if (kind == VAL_K_SLOT) {
                    x = slots.load(idx);
                } else {
                    x = last;
                }
            } else {
                mul = st.op == H2_VALUES_MUL || st.op == H2_VALUES_SQR;
                x = a;
                y = st.op == H2_VALUES_SQR ? a : b;
            }
            if (mul) x = fp_reduce_once(fp_mul_wide(x, y));
            if (k == 0) a = x;
            else if (k == 1) b = x;
            else if (k == 2) c = x;
            else r = x;
        }
        switch (st.op) {
            case H2_VALUES_ADD: r = fp_add(a, b); break;
            case H2_VALUES_SUB: r = fp_sub(a, b); break;
            case H2_VALUES_NEG: r = fp_neg(a); break;
            case H2_VALUES_SELECT: r = fp_is_zero(a) ? c : b; break;
            case H2_VALUES_ISZERO: r = fp_is_zero(a) ? fp_one<FrParams>() : fp_zero<FrParams>(); break;
            default: break;  // MUL, SQR: r is the product; COPY: r = a, the product's first operand
        }
        last = r;
        if (st.dst != VAL_NONE) slots.store(st.dst, r);
        if (st.store != VAL_NONE) val_store32((char*)P.out[st.store] + 32 * row, r);
    }
}

// The argument checks and the lowering: nullptr and *P filled when the call is usable, else what is wrong (a static string
// or one held in thread-local storage).  `device`: 32-byte elements must be 16-byte aligned (8 on the host).  m > 0.
const char* values_lower(const h2_values_leaf* leaves, size_t num_leaves, const uint64_t* constants, size_t num_constants,
                         const h2_values_op* ops, size_t num_ops, const h2_values_output* outputs, size_t num_outputs, size_t m,
                         bool device, ValProgram* P);
void values_caps(h2_values_caps* out);
// the host twin: a lowered program, row after row
void values_eval_host(const ValProgram& P, size_t m);

#ifdef __HIPCC__
// a lowered program; asynchronous on `stream`
int values_eval_launch(const ValProgram& P, size_t m, hipStream_t stream);
#endif

}  // namespace h2
