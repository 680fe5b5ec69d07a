// sort_plan.cpp -- what a sort decides before anything is enqueued (sort.hpp): the candidate digit positions, the tiles and
// the scratch layout.  Host C++ only, no HIP header: every function is a function of its arguments
// (tests/sort_host_main.cpp builds it with g++ alone, under the sanitizers).
#include "sort.hpp"

#include <stdio.h>

namespace h2 {

namespace {

thread_local char g_what[96];

const char* whatf(const char* fmt, unsigned long a, unsigned long b = 0) {
    snprintf(g_what, sizeof g_what, fmt, a, b);
    return g_what;
}

size_t round256(size_t bytes) { return (bytes + 255) & ~(size_t)255; }

}  // namespace

uint32_t sort_effective_bits(uint32_t form, uint32_t bits) {
    return bits ? bits : form == H2_ASSIGNED_FORM_COMPACT ? 64u : 254u;
}

uint32_t sort_candidate_bytes(uint32_t form, uint32_t bits) { return (sort_effective_bits(form, bits) + 7) / 8; }

size_t sort_tiles(size_t n) { return sort_ceil_div(n, SORT_TILE); }

size_t sort_scan_tmp_words(size_t words) {
    size_t total = 0;
    for (;;) {
        const size_t tiles = words ? sort_ceil_div(words, SORT_SCAN_TILE) : 1;
        total += (tiles + 63) & ~(size_t)63;
        if (tiles == 1) return total;
        words = tiles;
    }
}

uint32_t sort_scan_levels(size_t words) {
    uint32_t levels = 1;
    while (words > SORT_SCAN_TILE) {
        words = sort_ceil_div(words, SORT_SCAN_TILE);
        levels++;
    }
    return levels;
}

const char* sort_plan(const uint32_t* forms, const uint32_t* bits, size_t num_keys, size_t n, SortPlan* out) {
    if (!forms) return "forms is null";
    if (!bits) return "bits is null";
    if (num_keys == 0 || num_keys > SORT_MAX_KEYS) return whatf("num_keys is %lu (1 .. %lu)", num_keys, SORT_MAX_KEYS);
    if (n >> 32) return "n is 2^32 or more";
    SortPlan& p = *out;
    p = SortPlan{};
    p.num_keys = (uint32_t)num_keys;
    p.n = n;
    for (size_t k = 0; k < num_keys; k++) {
        if (forms[k] > H2_ASSIGNED_FORM_COMPACT) return whatf("forms[%lu] is %lu (H2_ASSIGNED_FORM_*)", k, forms[k]);
        const uint32_t most = forms[k] == H2_ASSIGNED_FORM_COMPACT ? 64 : 254;
        if (bits[k] > most) return whatf("bits[%lu] is above %lu", k, most);
        p.form[k] = forms[k];
        p.bits[k] = sort_effective_bits(forms[k], bits[k]);
    }
    uint32_t at = 0;
    for (size_t k = num_keys; k-- > 0;) {   // least significant key first, its low byte first
        p.first_pos[k] = at;
        const uint32_t bytes = sort_candidate_bytes(p.form[k], p.bits[k]);
        for (uint32_t b = 0; b < bytes; b++) p.pos[at++] = SortPos{(uint8_t)k, (uint8_t)b};
    }
    p.num_pos = at;
    p.tiles = sort_tiles(n);
    p.hist_words = 256 * p.tiles;
    p.scan_words = sort_scan_tmp_words(p.hist_words);
    size_t off = 0;
    auto take = [&](size_t bytes) {
        const size_t here = off;
        off += round256(bytes);
        return here;
    };
    p.off_misc = take(SORT_MISC_WORDS * 4);
    p.off_ghist = take((size_t)SORT_MAX_POS * 256 * 4);
    p.off_perm[0] = take(n * 4);
    p.off_perm[1] = take(n * 4);
    p.off_digits = take(n);
    p.off_hist = take(p.hist_words * 4);
    p.off_scan = take(p.scan_words * 4);
    // the canonical copy of a Montgomery column; laid out for every key, so that the bytes needed depend on n and the number of
    // keys alone
    for (size_t k = 0; k < num_keys; k++) p.off_canon[k] = take(n * 32);
    p.total = off;
    return nullptr;
}

}  // namespace h2
