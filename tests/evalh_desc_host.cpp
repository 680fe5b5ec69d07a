// evalh_desc_host.cpp -- h2_evalh_desc's counts, column slots, remap and validity rules (csrc/evalh_desc.hpp) without a device:
// g++ -I csrc evalh_desc_host.cpp.  One hand-made descriptor over fake addresses (tests/test_evalh_desc_host.py knows them);
// the command is argv[1], answers are lines on stdout:
//   counts    evalh_lookup_z_count, evalh_lookup_calc_count
//   walk      "table index pointer" for every slot evalh_for_each_column visits, in its order
//   column    "table index pointer" of evalh_column for index 0 .. count (one past the table) of every table
//   remap     the walk of evalh_remap's copy under p -> p + 8 bytes, then calls=, original_unchanged=, others_equal=, then the
//             walk of the original afterwards
//   validate  lines "form mutation" on stdin -> evalh_validate's message for the mutated descriptor, or "ok"
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <string>

#include "evalh_desc.hpp"

using namespace h2;

static const uint64_t* at(uintptr_t a) { return (const uint64_t*)a; }

struct Case {
    const uint64_t* fixed[2] = {at(0x10000), at(0x10100)};
    const uint64_t* advice[3] = {at(0x20000), at(0x20100), at(0x20000)};           // one address twice ...
    const uint64_t* perm_z[2] = {at(0x40000), at(0x40100)};
    const uint64_t* perm_sigma[3] = {at(0x50000), at(0x20000), at(0x50200)};       // ... and once more here
    const uint64_t* lookup_z[4] = {at(0x60000), at(0x60100), at(0x60200), at(0x60300)};
    const uint64_t* lookup_m[2] = {at(0x70000), at(0x70100)};
    const uint64_t* shuffle_z[1] = {at(0x80000)};
    uint32_t lookup_sets[2] = {1, 3};
    uint32_t perm_col_type[3] = {H2_ANY_ADVICE, H2_ANY_FIXED, H2_ANY_ADVICE};
    uint32_t perm_col_index[3] = {0, 1, 2};
    uint64_t constants[4] = {1, 2, 3, 4};
    int32_t rotations[2] = {0, -1};
    h2_evalh_desc d;
    Case() {
        memset(&d, 0, sizeof d);
        d.k = 5, d.extended_k = 7, d.blinding_factors = 5, d.chunk_len = 2;
        d.constants = constants, d.n_constants = 1;
        d.rotations = rotations, d.n_rotations = 2;
        d.n_lookups = 2, d.lookup_sets = lookup_sets;
        d.n_shuffles = 1;
        d.fixed = fixed, d.n_fixed = 2;
        d.advice = advice, d.n_advice = 3;
        d.instance = nullptr, d.n_instance = 0;
        d.l0 = at(0x90000), d.l_last = at(0xa0000), d.l_active_row = nullptr;
        d.n_perm_sets = 2, d.perm_z = perm_z;
        d.n_perm_columns = 3, d.perm_col_type = perm_col_type, d.perm_col_index = perm_col_index, d.perm_sigma = perm_sigma;
        d.lookup_z = lookup_z, d.lookup_m = lookup_m, d.shuffle_z = shuffle_z;
        for (int i = 0; i < 4; i++) d.y[i] = 11 + i, d.beta[i] = 21 + i, d.gamma[i] = 31 + i, d.theta[i] = 41 + i, d.delta[i] = 51 + i,
                                    d.zeta[i] = 61 + i, d.extended_omega[i] = 71 + i;
        d.flags = H2_EVALH_INTERPRET;
    }
};

static void print_walk(const h2_evalh_desc* d) {
    evalh_for_each_column(d, [](evgen::Table t, size_t i, const uint64_t* p) { printf("%u %zu %" PRIxPTR "\n", (unsigned)t, i, (uintptr_t)p); });
}

static void validate() {
    char form[32], what[32];
    while (scanf("%31s %31s", form, what) == 2) {
        Case c;
        h2_evalh_desc* d = &c.d;
        const std::string f = form, m = what;
        const EvalhForm ef = f == "device" ? EVALH_DEVICE : (f == "host" ? EVALH_HOST_EXTENDED : EVALH_HOST_COEFF);
        const uint32_t size = 1u << c.d.extended_k;
        if (m == "null") d = nullptr;
        else if (m == "ek_below_k") c.d.extended_k = c.d.k - 1;
        else if (m == "ek_29") c.d.extended_k = 29;
        else if (m == "chunk_len_0") c.d.chunk_len = 0;
        else if (m == "reserved") c.d.reserved = &c;
        else if (m == "row_outside") c.d.row_begin = size + 1;
        else if (m == "row_range") c.d.row_begin = 0, c.d.row_count = 4;
        else if (m == "perm_index") c.perm_col_index[1] = 2;        // fixed has two columns
        else if (m == "ek_equals_k") c.d.extended_k = c.d.k;
        else if (m == "ek_28") c.d.extended_k = 28;
        else if (m == "row_end_exact") c.d.row_begin = size - 4, c.d.row_count = 4;
        else if (m == "row_count_0") c.d.row_begin = size, c.d.row_count = 0;
        else if (m != "sound") {
            fprintf(stderr, "unknown mutation %s\n", what);
            return;
        }
        const char* msg = evalh_validate(d, "entry", ef);
        printf("%s\n", msg ? msg : "ok");
    }
}

int main(int argc, char** argv) {
    const std::string cmd = argc > 1 ? argv[1] : "";
    Case c;
    if (cmd == "counts") {
        printf("%zu %zu\n", evalh_lookup_z_count(&c.d), evalh_lookup_calc_count(&c.d));
    } else if (cmd == "walk") {
        print_walk(&c.d);
    } else if (cmd == "column") {
        for (uint32_t t = 0; t < evgen::T_COUNT; t++)
            for (size_t i = 0; i <= evalh_table_count(&c.d, t); i++) printf("%u %zu %" PRIxPTR "\n", t, i, (uintptr_t)evalh_column(&c.d, t, i));
    } else if (cmd == "remap") {
        h2_evalh_desc before;
        memcpy(&before, &c.d, sizeof before);
        size_t calls = 0;
        const EvalhRemap r = evalh_remap(&c.d, [&](evgen::Table, const uint64_t* p) {
            calls++;
            return at((uintptr_t)p + 8);
        });
        print_walk(&r.desc);
        // every member that is no column slot: the copy with the original's slots put back is the original
        h2_evalh_desc rest = r.desc;
        rest.fixed = c.d.fixed, rest.advice = c.d.advice, rest.instance = c.d.instance, rest.perm_z = c.d.perm_z;
        rest.perm_sigma = c.d.perm_sigma, rest.lookup_z = c.d.lookup_z, rest.lookup_m = c.d.lookup_m, rest.shuffle_z = c.d.shuffle_z;
        rest.l0 = c.d.l0, rest.l_last = c.d.l_last, rest.l_active_row = c.d.l_active_row;
        printf("calls=%zu original_unchanged=%d others_equal=%d\n", calls, memcmp(&before, &c.d, sizeof before) == 0,
               memcmp(&rest, &c.d, sizeof rest) == 0);
        print_walk(&c.d);   // (the original's pointer tables too)
    } else if (cmd == "validate") {
        validate();
    } else {
        fprintf(stderr, "usage: evalh_desc_host counts|walk|column|remap|validate\n");
        return 2;
    }
    return 0;
}
