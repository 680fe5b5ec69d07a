// sort_host_main.cpp -- csrc/sort_plan.cpp and csrc/sort_host.cpp as a stand-alone program (tests/test_sort_host.py builds it with
// g++ alone under the address and undefined-behaviour sanitizers): the plan's candidate positions, tiles and scratch layout,
// the argument checks, and the host twin against std::stable_sort over canonical integers.  Prints "ok <cases>".
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <array>
#include <random>
#include <string>
#include <vector>

#include "field.hpp"
#include "sort.hpp"

using namespace h2;

static int g_cases = 0;
#define CHECK(cond)                                                  \
    do {                                                             \
        if (!(cond)) {                                               \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            return 1;                                                \
        }                                                            \
        g_cases++;                                                   \
    } while (0)

using Cell = std::array<uint64_t, 4>;

static bool less_cell(const Cell& a, const Cell& b) {
    for (int i = 3; i >= 0; i--)
        if (a[i] != b[i]) return a[i] < b[i];
    return false;
}

static Cell to_mont(const Cell& c) {
    Fr v;
    memcpy(v.l, c.data(), 32);
    v = fp_to_mont(v);
    Cell out;
    memcpy(out.data(), v.l, 32);
    return out;
}

static int plan_checks() {
    const uint32_t C = H2_ASSIGNED_FORM_CANONICAL, M = H2_ASSIGNED_FORM_MONTGOMERY, K = H2_ASSIGNED_FORM_COMPACT;
    // candidate byte positions for every form and promise
    const struct { uint32_t form, bits, bytes; } want[] = {
        {C, 0, 32}, {C, 1, 1}, {C, 8, 1}, {C, 9, 2}, {C, 64, 8}, {C, 254, 32}, {C, 248, 31}, {C, 249, 32},
        {M, 0, 32}, {M, 1, 1}, {M, 8, 1}, {M, 9, 2}, {M, 64, 8}, {M, 254, 32},
        {K, 0, 8},  {K, 1, 1}, {K, 8, 1}, {K, 9, 2}, {K, 64, 8}, {K, 63, 8}, {K, 56, 7},
    };
    for (const auto& w : want) {
        CHECK(sort_candidate_bytes(w.form, w.bits) == w.bytes);
        SortPlan p;
        CHECK(sort_plan(&w.form, &w.bits, 1, 1000, &p) == nullptr);
        CHECK(p.num_pos == w.bytes && p.first_pos[0] == 0);
        for (uint32_t b = 0; b < p.num_pos; b++) CHECK(p.pos[b].key == 0 && p.pos[b].byte == b);
    }
    // several keys: the last key's low byte runs first
    {
        const uint32_t forms[3] = {K, C, M}, bits[3] = {2, 16, 0};
        SortPlan p;
        CHECK(sort_plan(forms, bits, 3, 5, &p) == nullptr);
        CHECK(p.num_pos == 1 + 2 + 32 && p.first_pos[2] == 0 && p.first_pos[1] == 32 && p.first_pos[0] == 34);
        CHECK(p.pos[0].key == 2 && p.pos[0].byte == 0 && p.pos[31].byte == 31 && p.pos[32].key == 1 && p.pos[33].byte == 1 &&
              p.pos[34].key == 0 && p.pos[34].byte == 0);
        CHECK(p.bits[0] == 2 && p.bits[1] == 16 && p.bits[2] == 254);
    }
    // tiles, the scan's levels, the layout
    const size_t T = SORT_TILE;
    CHECK(sort_tiles(0) == 0 && sort_tiles(1) == 1 && sort_tiles(T - 1) == 1 && sort_tiles(T) == 1 && sort_tiles(T + 1) == 2 &&
          sort_tiles(2 * T + 1) == 3);
    const size_t second = (SORT_SCAN_TILE / 256) * T + 1;
    CHECK(sort_scan_levels(256 * sort_tiles(second - 1)) == 1 && sort_scan_levels(256 * sort_tiles(second)) == 2);
    CHECK(sort_scan_tmp_words(256 * sort_tiles(second - 1)) == 64 && sort_scan_tmp_words(256 * sort_tiles(second)) == 128);
    size_t before = 0;
    for (size_t keys = 1; keys <= SORT_MAX_KEYS; keys++) {
        const uint32_t forms[SORT_MAX_KEYS] = {}, bits[SORT_MAX_KEYS] = {};
        size_t last = 0;
        for (size_t n : {(size_t)0, (size_t)1, T - 1, T, T + 1, 3 * T + 77, second, (size_t)1 << 22, ((size_t)1 << 32) - 1}) {
            SortPlan p;
            CHECK(sort_plan(forms, bits, keys, n, &p) == nullptr);
            CHECK(p.total >= last && p.total % 256 == 0 && p.tiles == sort_tiles(n) && p.hist_words == 256 * p.tiles);
            // the blocks lie apart, in this order, each as large as what is written into it
            CHECK(p.off_misc == 0 && p.off_ghist >= SORT_MISC_WORDS * 4 && p.off_perm[0] >= p.off_ghist + SORT_MAX_POS * 1024 &&
                  p.off_perm[1] >= p.off_perm[0] + 4 * n && p.off_digits >= p.off_perm[1] + 4 * n && p.off_hist >= p.off_digits + n &&
                  p.off_scan >= p.off_hist + 4 * p.hist_words && p.off_canon[0] >= p.off_scan + 4 * p.scan_words);
            for (size_t k = 0; k < keys; k++)
                CHECK((k + 1 < keys ? p.off_canon[k + 1] : p.total) >= p.off_canon[k] + 32 * n);
            last = p.total;
            if (n == T) {
                CHECK(p.total > before);
                before = p.total;
            }
        }
    }
    // what the plan refuses
    {
        const uint32_t form = C, bits = 0, bad_form = 3, bits255 = 255, compact = K, bits65 = 65;
        SortPlan p;
        CHECK(std::string(sort_plan(nullptr, &bits, 1, 1, &p)) == "forms is null");
        CHECK(std::string(sort_plan(&form, nullptr, 1, 1, &p)) == "bits is null");
        CHECK(std::string(sort_plan(&form, &bits, 0, 1, &p)).find("num_keys") == 0);
        CHECK(std::string(sort_plan(&form, &bits, SORT_MAX_KEYS + 1, 1, &p)).find("num_keys") == 0);
        CHECK(std::string(sort_plan(&form, &bits, 1, (size_t)1 << 32, &p)) == "n is 2^32 or more");
        CHECK(std::string(sort_plan(&bad_form, &bits, 1, 1, &p)).find("forms[0]") == 0);
        CHECK(std::string(sort_plan(&form, &bits255, 1, 1, &p)) == "bits[0] is above 254");
        CHECK(std::string(sort_plan(&compact, &bits65, 1, 1, &p)) == "bits[0] is above 64");
    }
    return 0;
}

static int twin_checks(uint32_t seed, size_t n) {
    std::mt19937_64 rng(seed);
    // two keys: a primary of three values (compact), a secondary of cells below 2^70 in Montgomery form
    std::vector<uint64_t> primary(n);
    std::vector<Cell> second(n), second_mont(n);
    for (size_t i = 0; i < n; i++) {
        primary[i] = rng() % 3;
        second[i] = Cell{rng(), rng() & 63, 0, 0};
        if (i % 7 == 3 && i) second[i] = second[i - 1];   // ties
        second_mont[i] = to_mont(second[i]);
    }
    std::vector<uint32_t> want(n);
    for (size_t i = 0; i < n; i++) want[i] = (uint32_t)i;
    std::stable_sort(want.begin(), want.end(), [&](uint32_t a, uint32_t b) {
        return primary[a] != primary[b] ? primary[a] < primary[b] : less_cell(second[a], second[b]);
    });
    const void* keys[2] = {primary.data(), second_mont.data()};
    const uint32_t forms[2] = {H2_ASSIGNED_FORM_COMPACT, H2_ASSIGNED_FORM_MONTGOMERY};
    for (uint32_t width : {4u, 8u}) {
        uint32_t bits[2] = {2, 70};
        std::vector<uint64_t> perm(n);   // n indices of either width
        uint32_t status[4];
        SortPlan plan;
        CHECK(sort_validate(keys, forms, bits, 2, n, perm.data(), width, status, false, nullptr, 0, &plan) == nullptr);
        sort_permutation_host(plan, keys, perm.data(), width, status);
        for (size_t i = 0; i < n; i++)
            if ((width == 4 ? ((const uint32_t*)perm.data())[i] : perm[i]) != want[i]) CHECK(!"the twin differs from stable_sort");
        CHECK(status[0] == H2_SORT_OK && status[1] == 0xffffffffu && status[2] == 0xffffffffu);
        CHECK(n < 64 || status[3] == 1 + 9);   // the primary's byte and the nine bytes below 2^70
        // a promise that the secondary breaks: the lowest row above 2^64 is named
        bits[1] = 64;
        size_t first = n;
        for (size_t i = 0; i < n && first == n; i++)
            if (second[i][1]) first = i;
        CHECK(sort_validate(keys, forms, bits, 2, n, perm.data(), width, status, false, nullptr, 0, &plan) == nullptr);
        sort_permutation_host(plan, keys, perm.data(), width, status);
        if (first < n) CHECK(status[0] == H2_SORT_OUT_OF_RANGE && status[1] == first && status[2] == 1);
        std::vector<uint8_t> seen(n, 0);   // still a permutation
        for (size_t i = 0; i < n; i++) {
            const uint64_t row = width == 4 ? ((const uint32_t*)perm.data())[i] : perm[i];
            CHECK(row < n && !seen[row]);
            seen[row] = 1;
        }
    }
    return 0;
}

static int validate_checks() {
    uint64_t cells[8] = {};
    const void* keys[1] = {cells};
    const uint32_t form = H2_ASSIGNED_FORM_CANONICAL, bits = 0;
    uint32_t perm[2], status[4];
    SortPlan p;
    auto msg = [&](const char* m) { return std::string(m ? m : "(usable)"); };
    CHECK(msg(sort_validate(nullptr, &form, &bits, 1, 2, perm, 4, status, false, nullptr, 0, &p)) == "keys is null");
    CHECK(msg(sort_validate(nullptr, &form, &bits, 1, 2, perm, 4, status, true, cells, 1 << 20, &p)) == "d_keys is null");
    CHECK(msg(sort_validate(keys, &form, &bits, 1, 2, perm, 4, nullptr, false, nullptr, 0, &p)) == "status is null");
    CHECK(msg(sort_validate(keys, &form, &bits, 1, 2, nullptr, 4, status, false, nullptr, 0, &p)) == "perm is null");
    CHECK(msg(sort_validate(keys, &form, &bits, 1, 2, perm, 2, status, false, nullptr, 0, &p)) == "perm_width is 2 (4 or 8)");
    CHECK(msg(sort_validate(keys, &form, &bits, 1, 2, perm, 4, status, true, nullptr, 0, &p)) == "d_scratch is null");
    CHECK(msg(sort_validate(keys, &form, &bits, 1, 2, perm, 4, status, true, cells, 64, &p)) == "scratch too small (h2_sort_scratch_bytes)");
    const void* none[1] = {nullptr};
    CHECK(msg(sort_validate(none, &form, &bits, 1, 2, perm, 4, status, false, nullptr, 0, &p)) == "keys[0] is null");
    CHECK(msg(sort_validate(none, &form, &bits, 1, 0, nullptr, 4, status, false, nullptr, 0, &p)) == "(usable)");   // n = 0: nothing is read
    CHECK(msg(sort_validate(keys, &form, &bits, 1, 2, perm, 4, status, false, nullptr, 0, &p)) == "(usable)");
    return 0;
}

int main(int argc, char** argv) {
    const size_t n = argc > 1 ? (size_t)atol(argv[1]) : 300;
    if (plan_checks() || validate_checks()) return 1;
    for (size_t m : {(size_t)0, (size_t)1, (size_t)2, n, (size_t)SORT_TILE + 1})
        if (twin_checks(17 + (uint32_t)m, m)) return 1;
    printf("ok %d\n", g_cases);
    return 0;
}
