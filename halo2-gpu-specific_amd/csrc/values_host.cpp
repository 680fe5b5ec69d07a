// values_host.cpp -- the fused evaluator's argument checks, the lowering of a caller's program to the steps the kernel runs,
// and the host twin (values.hpp): host C++ only, over the host pass of field.hpp (tests/values_host_main.cpp builds it with
// g++ alone, under the sanitizers).
#include "values.hpp"

#include <stdio.h>

namespace h2 {

namespace {

thread_local char g_what[160];

const char* whatf(const char* fmt, unsigned long a, unsigned long b = 0) {
    snprintf(g_what, sizeof g_what, fmt, a, b);
    return g_what;
}

struct Range {
    uintptr_t lo, hi;  // bytes [lo, hi)
};
bool overlap(const Range& a, const Range& b) { return a.lo < b.hi && b.lo < a.hi; }

constexpr uint64_t VAL_MAX_ELEMS = (uint64_t)1 << 56;  // of a buffer: 32 * len and every index product stay inside 64 bits

uint32_t operands_of(uint32_t op) {
    switch (op) {
        case H2_VALUES_ADD:
        case H2_VALUES_SUB:
        case H2_VALUES_MUL: return 2;
        case H2_VALUES_SQR:
        case H2_VALUES_NEG:
        case H2_VALUES_ISZERO: return 1;
        case H2_VALUES_SELECT: return 3;
        case H2_VALUES_TO_INT:
        case H2_VALUES_TO_FIELD:
        case H2_VALUES_EXTRACT: return 1;  // b and c of an EXTRACT are plain numbers
        case H2_VALUES_LT:
        case H2_VALUES_AND:
        case H2_VALUES_OR:
        case H2_VALUES_XOR: return 2;
        default: return 0;
    }
}

// what a value is: VAL_ANY in a requirement takes either
enum : uint8_t { VAL_FIELD = 0, VAL_INT = 1, VAL_ANY = 2 };

// the kind an operand of `op` must have (SELECT: a takes either; b against c is checked apart)
uint8_t wants(uint32_t op) {
    switch (op) {
        case H2_VALUES_ISZERO:
        case H2_VALUES_SELECT: return VAL_ANY;
        case H2_VALUES_TO_FIELD:
        case H2_VALUES_EXTRACT:
        case H2_VALUES_LT:
        case H2_VALUES_AND:
        case H2_VALUES_OR:
        case H2_VALUES_XOR: return VAL_INT;
        default: return VAL_FIELD;
    }
}

// "slot 2 holds" / "the last result is" / "leaf 1 is" / "constant 0 is"
void holder(char* out, size_t room, uint32_t word) {
    const unsigned kind = word >> 24, idx = word & 0xffffffu;
    if (kind == H2_VALUES_SLOT) snprintf(out, room, "slot %u holds", idx);
    else if (kind == H2_VALUES_LAST) snprintf(out, room, "the last result is");
    else snprintf(out, room, "%s %u is", kind == H2_VALUES_LEAF ? "leaf" : "constant", idx);
}

}  // namespace

void values_caps(h2_values_caps* out) {
    *out = h2_values_caps{VAL_MAX_LEAVES, VAL_MAX_OPS, VAL_MAX_CONSTS, VAL_MAX_OUTPUTS, VAL_SLOTS, VAL_MAX_BLOCKS, VAL_THREADS, 0};
}

const char* values_lower(const h2_values_leaf* leaves, size_t num_leaves, const uint64_t* constants, size_t num_constants,
                         const h2_values_op* ops, size_t num_ops, const h2_values_output* outputs, size_t num_outputs, size_t m,
                         bool device, ValProgram* P) {
    if (num_leaves > VAL_MAX_LEAVES) return whatf("%lu leaves, the cap is %lu", num_leaves, VAL_MAX_LEAVES);
    if (num_ops > VAL_MAX_OPS) return whatf("%lu ops, the cap is %lu", num_ops, VAL_MAX_OPS);
    if (num_constants > VAL_MAX_CONSTS) return whatf("%lu constants, the cap is %lu", num_constants, VAL_MAX_CONSTS);
    if (num_outputs > VAL_MAX_OUTPUTS) return whatf("%lu outputs, the cap is %lu", num_outputs, VAL_MAX_OUTPUTS);
    if (num_leaves && !leaves) return "null leaf table";
    if (num_constants && !constants) return "null constant table";
    if (num_ops && !ops) return "null op table";
    if (num_outputs && !outputs) return "null output table";
    if (m == 0 || m > VAL_MAX_ELEMS) return "m must be between 1 and 2^56";
    const uintptr_t wide = device ? 15 : 7;
    memset((void*)P, 0, sizeof *P);

    Range leaf_range[VAL_MAX_LEAVES];
    for (size_t i = 0; i < num_leaves; i++) {
        const h2_values_leaf& l = leaves[i];
        if (l.form > H2_ASSIGNED_FORM_COMPACT) return whatf("leaf %lu has an unknown form code %lu", i, l.form);
        const uint64_t cell = l.form == H2_ASSIGNED_FORM_COMPACT ? 8 : 32;
        if (!l.ptr) return whatf("leaf %lu has a null pointer", i);
        if (l.ptr & (l.form == H2_ASSIGNED_FORM_COMPACT ? 7 : wide)) return whatf("leaf %lu is misaligned for its form", i);
        if (l.stride == 0 || l.stride > VAL_MAX_ELEMS) return whatf("leaf %lu: the stride must be between 1 and 2^56", i);
        // first + (m - 1) stride < len, without a product that could overflow
        if (l.len > VAL_MAX_ELEMS || l.first >= l.len || (m - 1) > (l.len - 1 - l.first) / l.stride)
            return whatf("leaf %lu reaches beyond its buffer of %lu elements", i, l.len);
        if (l.ptr > UINTPTR_MAX - cell * l.len) return whatf("leaf %lu wraps around the address space", i);
        const uintptr_t lo = (uintptr_t)l.ptr + cell * l.first;
        leaf_range[i] = Range{lo, lo + cell * ((m - 1) * l.stride + 1)};
        P->leaf[i] = ValLeaf{(const void*)lo, l.stride, l.form, 0};
    }
    for (size_t i = 0; i < num_constants; i++) {
        Fr c;
        memcpy(c.l, constants + 4 * i, 32);
        P->konst[i] = fp_to_mont(c);  // any 256-bit integer: reduced here
    }
    for (int i = 0; i < 8; i++) P->konst[VAL_CONST_RR].l[i] = FrParams::RR[i];
    P->konst[VAL_CONST_RAW_ONE].l[0] = 1;
    for (int i = 0; i < 8; i++) P->konst[VAL_CONST_MONT_ONE].l[i] = FrParams::ONE[i];

    // the caller's ops as steps; `writer[s]`: the step that wrote slot s last, or none; `holds[s]`: the kind it left there
    int writer[VAL_SLOTS];
    uint8_t holds[VAL_SLOTS], last_kind = VAL_FIELD;
    for (uint32_t s = 0; s < VAL_SLOTS; s++) writer[s] = -1, holds[s] = VAL_FIELD;
    uint32_t steps = 0;
    auto kind_of = [&](uint32_t word) -> uint8_t {  // of an operand that `operand` accepted
        const uint32_t kind = word >> 24;
        return kind == H2_VALUES_SLOT ? holds[word & 0xffffffu] : kind == H2_VALUES_LAST ? last_kind : (uint8_t)VAL_FIELD;
    };
    auto operand = [&](uint32_t word, size_t i, uint16_t* out) -> const char* {
        const uint32_t kind = word >> 24, idx = word & 0xffffffu;
        if (kind == H2_VALUES_LEAF) {
            if (idx >= num_leaves) return whatf("op %lu reads leaf %lu, which does not exist", i, idx);
            *out = (uint16_t)(VAL_K_LEAF << 8 | idx);
        } else if (kind == H2_VALUES_CONST) {
            if (idx >= num_constants) return whatf("op %lu reads constant %lu, which does not exist", i, idx);
            *out = (uint16_t)(VAL_K_CONST << 8 | idx);
        } else if (kind == H2_VALUES_SLOT) {
            if (idx >= VAL_SLOTS) return whatf("op %lu reads slot %lu, at or above the cap", i, idx);
            if (writer[idx] < 0) return whatf("op %lu reads slot %lu, which was never written", i, idx);
            *out = (uint16_t)((writer[idx] + 1 == (int)steps ? VAL_K_LAST : VAL_K_SLOT) << 8 | idx);
        } else if (kind == H2_VALUES_LAST) {
            if (steps == 0) return whatf("op %lu reads the last result, and there is none", i);
            *out = (uint16_t)(VAL_K_LAST << 8);
        } else {
            return whatf("op %lu has an operand of unknown kind %lu", i, kind);
        }
        return nullptr;
    };
    for (size_t i = 0; i < num_ops; i++) {
        const h2_values_op& o = ops[i];
        const uint32_t n = operands_of(o.op);
        if (n == 0) return whatf("op %lu has an unknown op code %lu", i, o.op);
        const bool kept = o.dst != H2_VALUES_NO_SLOT;
        if (kept && o.dst >= VAL_SLOTS) return whatf("op %lu writes slot %lu, at or above the cap", i, o.dst);
        ValStep& st = P->step[steps];
        st.op = (uint8_t)o.op, st.dst = kept ? (uint8_t)o.dst : VAL_NONE, st.store = VAL_NONE, st.n = (uint8_t)n;
        const uint32_t words[3] = {o.a, o.b, o.c};
        uint8_t result = VAL_FIELD;
        if (o.op >= H2_VALUES_TO_INT) P->has_integer = 1;
        for (uint32_t k = 0; k < n; k++) {
            if (const char* what = operand(words[k], i, &st.opnd[k])) return what;
            const uint8_t want = wants(o.op), have = kind_of(words[k]);
            if (want != VAL_ANY && want != have) {
                char who[48];
                holder(who, sizeof who, words[k]);
                snprintf(g_what, sizeof g_what, "op %lu takes %s in operand %c; %s %s", (unsigned long)i,
                         want == VAL_INT ? "an integer" : "a field value", "abc"[k], who, have == VAL_INT ? "an integer" : "a field value");
                return g_what;
            }
        }
        if (o.op == H2_VALUES_SELECT) {
            if (kind_of(o.b) != kind_of(o.c)) return whatf("op %lu selects between a field value and an integer: b and c must be of one kind", i);
            result = kind_of(o.b);
        } else if (o.op == H2_VALUES_TO_INT) {
            // x * 1 * R^-1; a compact leaf is its own integer, a canonical leaf's raw words * R * R^-1 are the words mod r
            result = VAL_INT;
            const uint32_t form = (o.a >> 24) == H2_VALUES_LEAF ? leaves[o.a & 0xffffffu].form : (uint32_t)H2_ASSIGNED_FORM_MONTGOMERY;
            if (form == H2_ASSIGNED_FORM_COMPACT) {
                st.op = VAL_OP_COPY, st.opnd[0] = (uint16_t)(VAL_K_RAW_LEAF << 8 | (o.a & 0xff));
            } else {
                st.op = H2_VALUES_MUL, st.n = 2;
                if (form == H2_ASSIGNED_FORM_CANONICAL) st.opnd[0] = (uint16_t)(VAL_K_RAW_LEAF << 8 | (o.a & 0xff));
                st.opnd[1] = (uint16_t)(VAL_K_CONST << 8 | (form == H2_ASSIGNED_FORM_CANONICAL ? VAL_CONST_MONT_ONE : VAL_CONST_RAW_ONE));
            }
        } else if (o.op == H2_VALUES_TO_FIELD) {
            st.op = H2_VALUES_MUL, st.n = 2, st.opnd[1] = (uint16_t)(VAL_K_CONST << 8 | VAL_CONST_RR);
        } else if (o.op == H2_VALUES_EXTRACT) {
            if (o.b > 255) return whatf("op %lu extracts from bit %lu: lo must be between 0 and 255", i, o.b);
            if (o.c < 1 || o.c > 256) return whatf("op %lu extracts %lu bits: n must be between 1 and 256", i, o.c);
            result = VAL_INT, st.opnd[1] = (uint16_t)o.b, st.opnd[2] = (uint16_t)o.c;
        } else if (o.op >= H2_VALUES_LT) {
            result = VAL_INT;
        }
        last_kind = result;
        if (kept) writer[o.dst] = (int)steps, holds[o.dst] = result;
        steps++;
    }
    // the outputs: one more step each, at the end -- every load of a row precedes every store of it
    Range out_range[VAL_MAX_OUTPUTS];
    for (size_t i = 0; i < num_outputs; i++) {
        const h2_values_output& o = outputs[i];
        if (o.form > H2_ASSIGNED_FORM_MONTGOMERY) return whatf("output %lu has an unknown form code %lu (canonical or Montgomery)", i, o.form);
        if (!o.ptr) return whatf("output %lu has a null pointer", i);
        if (o.ptr & wide) return whatf("output %lu is misaligned", i);
        if (o.first > VAL_MAX_ELEMS || o.ptr > UINTPTR_MAX - 32 * (o.first + m)) return whatf("output %lu wraps around the address space", i);
        if (o.slot >= VAL_SLOTS) return whatf("output %lu reads slot %lu, at or above the cap", i, o.slot);
        if (writer[o.slot] < 0) return whatf("output %lu reads slot %lu, which was never written", i, o.slot);
        const uintptr_t lo = (uintptr_t)o.ptr + 32 * o.first;
        out_range[i] = Range{lo, lo + 32 * m};
        for (size_t l = 0; l < num_leaves; l++) {
            const bool in_place = leaves[l].form != H2_ASSIGNED_FORM_COMPACT && leaves[l].stride == 1 && leaf_range[l].lo == lo;
            if (overlap(out_range[i], leaf_range[l]) && !in_place) return whatf("output %lu overlaps leaf %lu", i, l);
        }
        for (size_t j = 0; j < i; j++)
            if (overlap(out_range[i], out_range[j])) return whatf("output %lu overlaps output %lu", i, j);
        P->out[i] = (void*)lo;
        ValStep& st = P->step[steps];
        st.dst = VAL_NONE, st.store = (uint8_t)i;
        const uint16_t src = (uint16_t)((writer[o.slot] + 1 == (int)steps ? VAL_K_LAST : VAL_K_SLOT) << 8 | o.slot);
        // a field slot: as it stands (Montgomery) or x * 1 * R^-1; an integer slot: x * R^2 * R^-1 or as it stands
        if ((o.form == H2_ASSIGNED_FORM_MONTGOMERY) == (holds[o.slot] == VAL_FIELD)) {
            st.op = VAL_OP_COPY, st.n = 1, st.opnd[0] = src;
        } else {
            st.op = H2_VALUES_MUL, st.n = 2, st.opnd[0] = src;
            st.opnd[1] = (uint16_t)(VAL_K_CONST << 8 | (holds[o.slot] == VAL_FIELD ? VAL_CONST_RAW_ONE : VAL_CONST_RR));
        }
        steps++;
    }
    P->num_steps = steps;
    // a slot write nobody reads from the slot (every reader takes `last`, or there is none before the next write) is dropped
    for (uint32_t s = 0; s < steps; s++) {
        ValStep& st = P->step[s];
        if (st.dst == VAL_NONE) continue;
        bool read = false;
        for (uint32_t t = s + 1; t < steps && !read; t++) {
            for (uint32_t k = 0; k < P->step[t].n; k++)
                if (P->step[t].opnd[k] == (uint16_t)(VAL_K_SLOT << 8 | st.dst)) read = true;
            if (P->step[t].dst == st.dst) break;
        }
        if (!read) st.dst = VAL_NONE;
    }
    return nullptr;
}

namespace {
struct HostSlots {
    Fr v[VAL_SLOTS];
    Fr load(uint32_t i) const { return v[i]; }
    void store(uint32_t i, const Fr& x) { v[i] = x; }
};
}  // namespace

void values_eval_host(const ValProgram& P, size_t m) {
    HostSlots slots;
    memset((void*)&slots, 0, sizeof slots);
    for (size_t row = 0; row < m; row++) val_run_row<true>(P, row, slots);  // the field steps of <false> are these
}

}  // namespace h2
