// values_int_host_main.cpp -- the integer half of csrc/values_host.cpp (kinds in the lowering; TO_INT, TO_FIELD, EXTRACT, LT,
// AND, OR, XOR in the host twin) as a stand-alone program for the address and undefined-behaviour sanitizers: the edge tables
// of EXTRACT, LT and the bitwise ops against a bit-by-bit model, then a seeded random walk of well-formed programs that mix the
// kinds, over buffers allocated to the exact size their leaves declare, each followed by the same program broken in one way,
// which has to be refused before anything is read or written.  usage: values_int_host_main ROUNDS
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "values.hpp"

using namespace h2;

static uint64_t g_state = 0xD1B54A32D192ED03ull;
static uint64_t rnd() {
    g_state ^= g_state << 13;
    g_state ^= g_state >> 7;
    g_state ^= g_state << 17;
    return g_state;
}

static int fail(const char* what, int round) {
    printf("FAILED: %s (round %d)\n", what, round);
    return 1;
}

// ---- the model: 256-bit integers, one bit at a time --------------------------------------------------------------------------
struct U256 {
    uint64_t w[4];
};
static bool bit_of(const U256& v, unsigned i) { return i < 256 && (v.w[i / 64] >> (i % 64) & 1); }
static U256 model_extract(const U256& v, unsigned lo, unsigned n) {
    U256 r{{0, 0, 0, 0}};
    for (unsigned i = 0; i < n && i < 256; i++)
        if (bit_of(v, lo + i)) r.w[i / 64] |= (uint64_t)1 << (i % 64);
    return r;
}
static bool model_less(const U256& a, const U256& b) {
    for (int i = 3; i >= 0; i--)
        if (a.w[i] != b.w[i]) return a.w[i] < b.w[i];
    return false;
}
static U256 modulus() {
    U256 r;
    memcpy(r.w, FrParams::MOD, 32);
    return r;
}
static U256 model_reduce_once(const U256& a) {
    const U256 p = modulus();
    if (model_less(a, p)) return a;
    U256 r;
    unsigned borrow = 0;
    for (int i = 0; i < 4; i++) {
        const uint64_t t = a.w[i] - p.w[i], u = t - borrow;
        borrow = (a.w[i] < p.w[i]) || (t < borrow);
        r.w[i] = u;
    }
    return r;
}
static U256 of_fr(const Fr& f) {
    U256 r;
    memcpy(r.w, f.l, 32);
    return r;
}
static Fr to_fr(const U256& v) {
    Fr r;
    memcpy(r.l, v.w, 32);
    return r;
}
static U256 random_below_r() {
    U256 v;
    for (auto& w : v.w) w = rnd();
    v.w[3] &= 0x0fffffffffffffffull;  // below 2^252 < r
    return v;
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

static const uint32_t SLOT = H2_VALUES_SLOT << 24, LEAF = H2_VALUES_LEAF << 24, LAST = H2_VALUES_LAST << 24, CONST = H2_VALUES_CONST << 24;

// the edge tables: canonical leaves x, y (reduced) of exactly m elements; one program per (lo, four n) and one for LT and the bitwise ops
static int edge_tables() {
    const unsigned los[] = {0, 1, 31, 32, 33, 63, 64, 65, 127, 128, 223, 224, 253, 255};
    const unsigned ns[] = {1, 31, 32, 33, 64, 254, 256, 8};
    std::vector<U256> xs, ys;
    const U256 p = modulus();
    U256 pm1 = p;
    pm1.w[0] -= 1;
    const U256 zero{{0, 0, 0, 0}}, one{{1, 0, 0, 0}};
    xs = {zero, one, pm1, pm1, zero, pm1};
    ys = {zero, one, pm1, zero, pm1, one};
    for (unsigned j : {1u, 31u, 32u, 33u, 63u, 64u, 65u, 127u, 128u, 192u, 224u, 252u, 253u}) {
        U256 pow{{0, 0, 0, 0}}, below{{0, 0, 0, 0}};
        pow.w[j / 64] = (uint64_t)1 << (j % 64);
        for (unsigned i = 0; i < j; i++) below.w[i / 64] |= (uint64_t)1 << (i % 64);
        xs.push_back(pow), ys.push_back(below);
        xs.push_back(below), ys.push_back(pow);
    }
    U256 hi{{0, 0, 0, (uint64_t)0x30 << 56}}, lo{{0, 0, 0, (uint64_t)0x0f << 56}};  // below r each, their OR above it
    xs.push_back(hi), ys.push_back(lo);
    for (int i = 0; i < 40; i++) {
        U256 a = random_below_r(), b = a;
        if (i % 3 == 0) b.w[3] ^= (uint64_t)1 << 40;  // differ in the top word only
        if (i % 3 == 1) b.w[0] ^= 1;                  // in the bottom word only
        if (i % 3 == 2) b = random_below_r();
        xs.push_back(a), ys.push_back(b);
    }
    const size_t m = xs.size();
    std::vector<uint64_t> xbuf(4 * m), ybuf(4 * m);
    for (size_t i = 0; i < m; i++) memcpy(&xbuf[4 * i], xs[i].w, 32), memcpy(&ybuf[4 * i], ys[i].w, 32);
    Call base;
    base.m = m;
    base.leaves.push_back(h2_values_leaf{(uint64_t)(uintptr_t)xbuf.data(), 0, 1, m, H2_ASSIGNED_FORM_CANONICAL, 0});
    base.leaves.push_back(h2_values_leaf{(uint64_t)(uintptr_t)ybuf.data(), 0, 1, m, H2_ASSIGNED_FORM_CANONICAL, 0});
    std::vector<std::vector<uint64_t>> outs(4, std::vector<uint64_t>(4 * m));
    ValProgram P;
    for (unsigned lo_bit : los)
        for (int half = 0; half < 2; half++) {
            Call call = base;
            call.ops.push_back(h2_values_op{H2_VALUES_TO_INT, 0, LEAF | 0, 0, 0});
            for (uint32_t i = 0; i < 4; i++) {
                call.ops.push_back(h2_values_op{H2_VALUES_EXTRACT, 1 + i, SLOT | 0, lo_bit, ns[4 * half + i]});
                call.outputs.push_back(h2_values_output{(uint64_t)(uintptr_t)outs[i].data(), 0, 1 + i, H2_ASSIGNED_FORM_CANONICAL});
            }
            if (const char* what = call.lower(&P)) return fail(what, -2);
            values_eval_host(P, m);
            for (size_t row = 0; row < m; row++)
                for (int i = 0; i < 4; i++) {
                    const U256 want = model_extract(xs[row], lo_bit, ns[4 * half + i]);
                    if (memcmp(want.w, &outs[i][4 * row], 32) != 0) return fail("EXTRACT differs from the model", (int)lo_bit);
                }
        }
    Call call = base;
    call.ops = {h2_values_op{H2_VALUES_TO_INT, 0, LEAF | 0, 0, 0},          h2_values_op{H2_VALUES_TO_INT, 1, LEAF | 1, 0, 0},
                h2_values_op{H2_VALUES_LT, 2, SLOT | 0, SLOT | 1, 0},       h2_values_op{H2_VALUES_AND, 3, SLOT | 0, SLOT | 1, 0},
                h2_values_op{H2_VALUES_OR, 4, SLOT | 0, SLOT | 1, 0},       h2_values_op{H2_VALUES_XOR, 5, SLOT | 0, LAST, 0},
                h2_values_op{H2_VALUES_XOR, 5, SLOT | 0, SLOT | 1, 0}};
    for (uint32_t i = 0; i < 4; i++) call.outputs.push_back(h2_values_output{(uint64_t)(uintptr_t)outs[i].data(), 0, 2 + i, H2_ASSIGNED_FORM_CANONICAL});
    if (const char* what = call.lower(&P)) return fail(what, -3);
    values_eval_host(P, m);
    for (size_t row = 0; row < m; row++) {
        const U256 &a = xs[row], &b = ys[row];
        U256 want[4] = {U256{{model_less(a, b), 0, 0, 0}}, a, a, a};
        for (int i = 0; i < 4; i++) want[1].w[i] &= b.w[i], want[2].w[i] |= b.w[i], want[3].w[i] ^= b.w[i];
        want[2] = model_reduce_once(want[2]), want[3] = model_reduce_once(want[3]);
        for (int i = 0; i < 4; i++)
            if (memcmp(want[i].w, &outs[i][4 * row], 32) != 0) return fail("LT / AND / OR / XOR differs from the model", (int)row);
    }
    // (r - 1) | 1 is r, which is 0 (row 5)
    if (outs[2][4 * 5] | outs[2][4 * 5 + 1] | outs[2][4 * 5 + 2] | outs[2][4 * 5 + 3]) return fail("(r - 1) | 1 is not 0", -3);
    return 0;
}

int main(int argc, char** argv) {
    const int rounds = argc > 1 ? atoi(argv[1]) : 100;
    h2_values_caps caps;
    values_caps(&caps);
    if (edge_tables()) return 1;
    for (int round = 0; round < rounds; round++) {
        Call call;
        call.m = 1 + rnd() % 70;
        const size_t m = call.m;
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
        // ops over what exists, of the kind each takes: is_int[s] is the model's own account of what slot s holds
        const size_t num_ops = 2 + rnd() % (caps.ops - 1);
        std::vector<int> holds(caps.slots, -1);  // -1 never written, 0 field, 1 integer
        int last = -1;
        for (size_t i = 0; i < num_ops; i++) {
            auto operand = [&](int want) -> uint32_t {  // want: 0 field, 1 integer, 2 either; 0xffffffff if there is none
                for (int tries = 0; tries < 64; tries++) {
                    const uint32_t kind = rnd() % 4;
                    if (kind == H2_VALUES_LEAF && want != 1) return LEAF | (uint32_t)(rnd() % num_leaves);
                    if (kind == H2_VALUES_CONST && want != 1) return CONST | (uint32_t)(rnd() % num_constants);
                    if (kind == H2_VALUES_LAST && last >= 0 && (want == 2 || want == last)) return LAST;
                    const uint32_t s = rnd() % caps.slots;
                    if (kind == H2_VALUES_SLOT && holds[s] >= 0 && (want == 2 || want == holds[s])) return SLOT | s;
                }
                return 0xffffffffu;
            };
            h2_values_op op{0, 0, 0, 0, 0};
            int result = 0;
            for (;;) {
                const uint32_t codes[] = {H2_VALUES_ADD,    H2_VALUES_SUB,      H2_VALUES_MUL,     H2_VALUES_SQR, H2_VALUES_NEG, H2_VALUES_SELECT,
                                          H2_VALUES_ISZERO, H2_VALUES_TO_INT,   H2_VALUES_TO_INT,  H2_VALUES_TO_FIELD, H2_VALUES_EXTRACT,
                                          H2_VALUES_EXTRACT, H2_VALUES_LT,      H2_VALUES_AND,     H2_VALUES_OR,  H2_VALUES_XOR};
                op.op = codes[rnd() % 16];
                result = op.op >= H2_VALUES_TO_INT && op.op != H2_VALUES_TO_FIELD;
                const int takes = op.op == H2_VALUES_ISZERO || op.op == H2_VALUES_SELECT ? 2 : op.op >= H2_VALUES_TO_FIELD;
                op.a = operand(takes), op.b = operand(takes), op.c = 0;
                if (op.op == H2_VALUES_SELECT) {
                    result = rnd() % 2;
                    op.b = operand(result), op.c = operand(result);
                } else if (op.op == H2_VALUES_EXTRACT) {
                    op.b = rnd() % 256, op.c = 1 + rnd() % 256;
                }
                if (op.a != 0xffffffffu && op.b != 0xffffffffu && op.c != 0xffffffffu) break;
            }
            op.dst = rnd() % 8 == 0 && i + 1 < num_ops ? H2_VALUES_NO_SLOT : (uint32_t)(rnd() % caps.slots);
            if (op.dst != H2_VALUES_NO_SLOT) holds[op.dst] = result;
            last = result;
            call.ops.push_back(op);
        }
        std::vector<std::vector<uint64_t>> outs;
        for (uint32_t s = 0; s < caps.slots && outs.size() < caps.outputs; s++) {
            if (holds[s] < 0) continue;
            outs.emplace_back(4 * m, 0x5a5a5a5a5a5a5a5aull);
            call.outputs.push_back(h2_values_output{(uint64_t)(uintptr_t)outs.back().data(), 0, s, (uint32_t)(rnd() % 2)});
        }
        if (call.outputs.empty()) return fail("no output", round);
        ValProgram P;
        if (const char* what = call.lower(&P)) return fail(what, round);
        values_eval_host(P, m);
        // the model: every value as its integer in [0, r), whatever its kind
        for (size_t row = 0; row < m; row++) {
            std::vector<U256> slots(caps.slots, U256{{0, 0, 0, 0}});
            U256 prev{{0, 0, 0, 0}};
            auto value = [&](uint32_t word) -> U256 {
                const uint32_t kind = word >> 24, idx = word & 0xffffff;
                if (kind == H2_VALUES_LEAF) {
                    const h2_values_leaf& l = call.leaves[idx];
                    const size_t e = l.first + row * l.stride;
                    if (l.form == H2_ASSIGNED_FORM_COMPACT) return U256{{bufs[idx][e], 0, 0, 0}};
                    Fr raw;
                    memcpy(raw.l, &bufs[idx][4 * e], 32);
                    return of_fr(l.form == H2_ASSIGNED_FORM_MONTGOMERY ? fp_from_mont(raw) : fp_from_mont(fp_to_mont(raw)));
                }
                if (kind == H2_VALUES_CONST) {
                    Fr raw;
                    memcpy(raw.l, &call.constants[4 * idx], 32);
                    return of_fr(fp_from_mont(fp_to_mont(raw)));
                }
                return kind == H2_VALUES_SLOT ? slots[idx] : prev;
            };
            auto field2 = [&](const U256& a, const U256& b, uint32_t op) -> U256 {
                const Fr x = fp_to_mont(to_fr(a)), y = fp_to_mont(to_fr(b));
                return of_fr(fp_from_mont(op == H2_VALUES_ADD ? fp_add(x, y) : op == H2_VALUES_SUB ? fp_sub(x, y) : fp_mul(x, y)));
            };
            const U256 zero{{0, 0, 0, 0}}, one{{1, 0, 0, 0}};
            for (const h2_values_op& op : call.ops) {
                const U256 a = value(op.a);
                U256 r = a;  // TO_INT, TO_FIELD: the same integer
                switch (op.op) {
                    case H2_VALUES_ADD:
                    case H2_VALUES_SUB:
                    case H2_VALUES_MUL: r = field2(a, value(op.b), op.op); break;
                    case H2_VALUES_SQR: r = field2(a, a, H2_VALUES_MUL); break;
                    case H2_VALUES_NEG: r = field2(zero, a, H2_VALUES_SUB); break;
                    case H2_VALUES_SELECT: r = memcmp(a.w, zero.w, 32) == 0 ? value(op.c) : value(op.b); break;
                    case H2_VALUES_ISZERO: r = memcmp(a.w, zero.w, 32) == 0 ? one : zero; break;
                    case H2_VALUES_EXTRACT: r = model_extract(a, op.b, op.c); break;
                    case H2_VALUES_LT: r = model_less(a, value(op.b)) ? one : zero; break;
                    case H2_VALUES_AND:
                    case H2_VALUES_OR:
                    case H2_VALUES_XOR: {
                        const U256 b = value(op.b);
                        for (int i = 0; i < 4; i++)
                            r.w[i] = op.op == H2_VALUES_AND ? a.w[i] & b.w[i] : op.op == H2_VALUES_OR ? a.w[i] | b.w[i] : a.w[i] ^ b.w[i];
                        r = model_reduce_once(r);
                        break;
                    }
                    default: break;
                }
                prev = r;
                if (op.dst != H2_VALUES_NO_SLOT) slots[op.dst] = r;
            }
            for (size_t o = 0; o < call.outputs.size(); o++) {
                Fr want = to_fr(slots[call.outputs[o].slot]);
                if (call.outputs[o].form == H2_ASSIGNED_FORM_MONTGOMERY) want = fp_to_mont(want);
                if (memcmp(want.l, &outs[o][4 * row], 32) != 0) return fail("a value differs from the model", round);
            }
        }
        // the same call, broken in one way: refused, and no output touched
        for (auto& o : outs) std::fill(o.begin(), o.end(), 0x5a5a5a5a5a5a5a5aull);
        Call bad = call;
        const uint32_t some_leaf = LEAF | 0;
        switch (round % 8) {
            case 0: bad.ops.push_back(h2_values_op{H2_VALUES_EXTRACT, 0, some_leaf, 0, 8}); break;             // a leaf is a field value
            case 1: bad.ops.push_back(h2_values_op{H2_VALUES_TO_INT, 0, some_leaf, 0, 0}),
                    bad.ops.push_back(h2_values_op{H2_VALUES_ADD, 0, LAST, some_leaf, 0}); break;              // a field op on an integer
            case 2: bad.ops.push_back(h2_values_op{H2_VALUES_TO_INT, 0, some_leaf, 0, 0}),
                    bad.ops.push_back(h2_values_op{H2_VALUES_EXTRACT, 0, LAST, 256, 1}); break;
            case 3: bad.ops.push_back(h2_values_op{H2_VALUES_TO_INT, 0, some_leaf, 0, 0}),
                    bad.ops.push_back(h2_values_op{H2_VALUES_EXTRACT, 0, LAST, 0, 257}); break;
            case 4: bad.ops.push_back(h2_values_op{H2_VALUES_TO_INT, 0, some_leaf, 0, 0}),
                    bad.ops.push_back(h2_values_op{H2_VALUES_SELECT, 0, some_leaf, LAST, some_leaf}); break;   // arms of two kinds
            case 5: bad.ops[0].op = 7 + round % 9; break;                                                        // 7 .. 15
            case 6: bad.ops.push_back(h2_values_op{H2_VALUES_TO_INT, 0, some_leaf, 0, 0}),
                    bad.ops.push_back(h2_values_op{H2_VALUES_EXTRACT, 0, LAST, 0, 0}); break;
            default: bad.ops.push_back(h2_values_op{H2_VALUES_LT, 0, CONST | 0, CONST | 0, 0}); break;          // constants are field values
        }
        if (bad.ops.size() > caps.ops) bad.ops.erase(bad.ops.begin() + 1, bad.ops.begin() + 1 + (bad.ops.size() - caps.ops));
        if (!bad.lower(&P)) return fail("a malformed program was accepted", round);
        for (auto& o : outs)
            for (uint64_t w : o)
                if (w != 0x5a5a5a5a5a5a5a5aull) return fail("a refused call wrote", round);
    }
    printf("ok %d\n", rounds);
    return 0;
}
