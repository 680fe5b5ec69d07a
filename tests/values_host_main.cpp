// values_host_main.cpp -- csrc/values_host.cpp (the fused evaluator's argument checks, lowering and host twin) as a stand-alone
// program for the address and undefined-behaviour sanitizers: random well-formed programs over buffers allocated to the exact
// size their leaves declare, checked against field.hpp's arithmetic applied op by op, and malformed programs, each of which
// has to be refused before anything is read or written.  usage: values_host_main ROUNDS
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "values.hpp"

using namespace h2;

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {
    g_state ^= g_state << 13;
    g_state ^= g_state >> 7;
    g_state ^= g_state << 17;
    return g_state;
}

static Fr from_words(const uint64_t* w) {
    Fr r;
    memcpy(r.l, w, 32);
    return r;
}

static int fail(const char* what, int round) {
    printf("FAILED: %s (round %d)\n", what, round);
    return 1;
}

struct Call {
    std::vector<h2_values_leaf> leaves;
    std::vector<uint64_t> constants;
    std::vector<h2_values_op> ops;
    std::vector<h2_values_output> outputs;
    size_t m = 0;
    const char* lower(ValProgram* P) const {
        return values_lower(leaves.data(), leaves.size(), constants.data(), constants.size() / 4, ops.data(), ops.size(), outputs.data(),
                            outputs.size(), m, false, P);
    }
};

int main(int argc, char** argv) {
    const int rounds = argc > 1 ? atoi(argv[1]) : 100;
    h2_values_caps caps;
    values_caps(&caps);
    for (int round = 0; round < rounds; round++) {
        Call call;
        call.m = 1 + rnd() % 70;
        const size_t m = call.m;
        // leaves: heap buffers of exactly `len` elements
        const size_t num_leaves = 1 + rnd() % caps.leaves;
        std::vector<std::vector<uint64_t>> bufs(num_leaves);
        for (size_t i = 0; i < num_leaves; i++) {
            const uint32_t form = rnd() % 3;
            const uint64_t first = rnd() % 4, stride = 1 + rnd() % 3, len = first + (m - 1) * stride + 1 + rnd() % 2;
            const size_t words = form == H2_ASSIGNED_FORM_COMPACT ? 1 : 4;
            bufs[i].resize(len * words);
            for (size_t e = 0; e < len; e++)
                for (size_t w = 0; w < words; w++) bufs[i][e * words + w] = rnd();
            if (form == H2_ASSIGNED_FORM_MONTGOMERY)  // reduced residues
                for (size_t e = 0; e < len; e++) bufs[i][e * 4 + 3] &= 0x0fffffffffffffffull;
            call.leaves.push_back(h2_values_leaf{(uint64_t)(uintptr_t)bufs[i].data(), first, stride, len, form, 0});
        }
        const size_t num_constants = 1 + rnd() % caps.constants;
        for (size_t i = 0; i < 4 * num_constants; i++) call.constants.push_back(rnd());
        // ops over what exists; the model runs next to the construction, row by row, later
        const size_t num_ops = 1 + rnd() % caps.ops;
        std::vector<bool> written(caps.slots, false);
        for (size_t i = 0; i < num_ops; i++) {
            auto operand = [&]() -> uint32_t {
                for (;;) {
                    const uint32_t kind = rnd() % 4;
                    if (kind == H2_VALUES_LEAF) return kind << 24 | (uint32_t)(rnd() % num_leaves);
                    if (kind == H2_VALUES_CONST) return kind << 24 | (uint32_t)(rnd() % num_constants);
                    if (kind == H2_VALUES_LAST && i > 0) return kind << 24;
                    const uint32_t s = rnd() % caps.slots;
                    if (kind == H2_VALUES_SLOT && written[s]) return kind << 24 | s;
                }
            };
            h2_values_op op{(uint32_t)(rnd() % 7), 0, 0, 0, 0};
            op.a = operand(), op.b = operand(), op.c = operand();
            op.dst = rnd() % 8 == 0 && i + 1 < num_ops ? H2_VALUES_NO_SLOT : (uint32_t)(rnd() % caps.slots);
            if (op.dst != H2_VALUES_NO_SLOT) written[op.dst] = true;
            call.ops.push_back(op);
        }
        std::vector<std::vector<uint64_t>> outs;
        for (uint32_t s = 0; s < caps.slots && outs.size() < caps.outputs; s++) {
            if (!written[s]) continue;
            outs.emplace_back(4 * m, 0x5a5a5a5a5a5a5a5aull);
            call.outputs.push_back(h2_values_output{(uint64_t)(uintptr_t)outs.back().data(), 0, s, (uint32_t)(rnd() % 2)});
        }
        if (call.outputs.empty()) {  // every op was transient but the last: cannot happen, the last op keeps its slot
            return fail("no output", round);
        }
        ValProgram P;
        if (const char* what = call.lower(&P)) return fail(what, round);
        values_eval_host(P, m);
        // the model: Montgomery residues, op by op
        for (size_t row = 0; row < m; row++) {
            std::vector<Fr> slots(caps.slots, fp_zero<FrParams>());
            Fr last = fp_zero<FrParams>();
            auto value = [&](uint32_t word) -> Fr {
                const uint32_t kind = word >> 24, idx = word & 0xffffff;
                if (kind == H2_VALUES_LEAF) {
                    const h2_values_leaf& l = call.leaves[idx];
                    const size_t e = l.first + row * l.stride;
                    if (l.form == H2_ASSIGNED_FORM_COMPACT) {
                        uint64_t w[4] = {bufs[idx][e], 0, 0, 0};
                        return fp_to_mont(from_words(w));
                    }
                    const Fr raw = from_words(&bufs[idx][4 * e]);
                    return l.form == H2_ASSIGNED_FORM_MONTGOMERY ? raw : fp_to_mont(raw);
                }
                if (kind == H2_VALUES_CONST) return fp_to_mont(from_words(&call.constants[4 * idx]));
                return kind == H2_VALUES_SLOT ? slots[idx] : last;
            };
            for (const h2_values_op& op : call.ops) {
                const Fr a = value(op.a);
                Fr r;
                switch (op.op) {
                    case H2_VALUES_ADD: r = fp_add(a, value(op.b)); break;
                    case H2_VALUES_SUB: r = fp_sub(a, value(op.b)); break;
                    case H2_VALUES_MUL: r = fp_mul(a, value(op.b)); break;
                    case H2_VALUES_SQR: r = fp_mul(a, a); break;
                    case H2_VALUES_NEG: r = fp_neg(a); break;
                    case H2_VALUES_SELECT: r = fp_is_zero(a) ? value(op.c) : value(op.b); break;
                    default: r = fp_is_zero(a) ? fp_one<FrParams>() : fp_zero<FrParams>(); break;
                }
                last = r;
                if (op.dst != H2_VALUES_NO_SLOT) slots[op.dst] = r;
            }
            for (size_t o = 0; o < call.outputs.size(); o++) {
                Fr want = slots[call.outputs[o].slot];
                if (call.outputs[o].form == H2_ASSIGNED_FORM_CANONICAL) want = fp_from_mont(want);
                if (memcmp(want.l, &outs[o][4 * row], 32) != 0) return fail("a value differs from the model", round);
            }
        }
        // the same call, broken in one way: refused, and no output touched
        for (auto& o : outs) std::fill(o.begin(), o.end(), 0x5a5a5a5a5a5a5a5aull);
        Call bad = call;
        switch (round % 8) {
            case 0: bad.leaves[0].len = bad.leaves[0].first + (m - 1) * bad.leaves[0].stride; break;     // one element short
            case 1: bad.ops.back().dst = caps.slots; break;
            case 2: bad.ops[0].a = H2_VALUES_SLOT << 24 | (caps.slots - 1); break;                      // never written before op 0
            case 3: bad.ops[0].op = 7; break;
            case 4: bad.leaves[0].form = 3; break;
            case 5: {                                                                                   // inside a leaf's elements
                const h2_values_leaf& l = bad.leaves[0];
                const bool compact = l.form == H2_ASSIGNED_FORM_COMPACT;
                bad.outputs[0].ptr = l.ptr + (compact ? 8 : 32) * l.first + (compact ? 0 : 8);
                break;
            }
            case 6: bad.ops[0].a = H2_VALUES_LAST << 24; break;
            default: bad.leaves[0].stride = 0; break;
        }
        if (!bad.lower(&P)) return fail("a malformed program was accepted", round);
        for (auto& o : outs)
            for (uint64_t w : o)
                if (w != 0x5a5a5a5a5a5a5a5aull) return fail("a refused call wrote", round);
    }
    // m = 0 is the entry points' business (they return before lowering); an empty program with outputs is refused here
    Call empty;
    empty.m = 1;
    uint64_t cell[4];
    empty.outputs.push_back(h2_values_output{(uint64_t)(uintptr_t)cell, 0, 0, 0});
    ValProgram P;
    if (!empty.lower(&P)) return fail("an output of a slot never written was accepted", -1);
    printf("ok %d\n", rounds);
    return 0;
}
