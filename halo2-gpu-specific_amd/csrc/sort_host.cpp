// sort_host.cpp -- the sort's argument checks and its host twin (sort.hpp): host C++ only, over the host pass of field.hpp
// for the one conversion of a Montgomery column (tests/sort_host_main.cpp builds it with g++ alone, under the sanitizers).
// The twin runs the passes the kernels run -- the survey of every candidate byte position, the skip of a position with one
// non-empty bin, a stable counting pass over indices per position that is left -- so its status words are the device's.
#include "sort.hpp"

#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "field.hpp"

namespace h2 {

namespace {

thread_local char g_what[96];

const char* whatf(const char* fmt, unsigned long a) {
    snprintf(g_what, sizeof g_what, fmt, a);
    return g_what;
}

// is the integer of these 32 little-endian bytes 2^bits or more?
bool at_or_above(const uint8_t* cell, uint32_t width, uint32_t bits) {
    for (uint32_t b = bits / 8; b < width; b++) {
        const uint8_t keep = b == bits / 8 ? (uint8_t)(0xffu << (bits % 8)) : 0xff;
        if (cell[b] & keep) return true;
    }
    return false;
}

}  // namespace

const char* sort_validate(const void* const* keys, const uint32_t* forms, const uint32_t* bits, size_t num_keys, size_t n,
                          const void* perm, uint32_t perm_width, const uint32_t* status, bool device, const void* scratch,
                          size_t scratch_bytes, SortPlan* plan) {
    if (!keys) return device ? "d_keys is null" : "keys is null";
    if (const char* what = sort_plan(forms, bits, num_keys, n, plan)) return what;
    if (!status) return device ? "d_status is null" : "status is null";
    if ((uintptr_t)status % 4) return "status is misaligned";
    if (perm_width != 4 && perm_width != 8) return whatf("perm_width is %lu (4 or 8)", perm_width);
    if (device) {
        if (!scratch) return "d_scratch is null";
        if ((uintptr_t)scratch % 16) return "d_scratch is misaligned";
        if (scratch_bytes < plan->total) return "scratch too small (h2_sort_scratch_bytes)";
    }
    if (n == 0) return nullptr;
    if (!perm) return device ? "d_perm is null" : "perm is null";
    if ((uintptr_t)perm % perm_width) return "perm is misaligned";
    for (size_t k = 0; k < num_keys; k++) {
        if (!keys[k]) return whatf("keys[%lu] is null", k);
        const uintptr_t align = forms[k] == H2_ASSIGNED_FORM_COMPACT || !device ? 8 : 16;
        if ((uintptr_t)keys[k] % align) return whatf("keys[%lu] is misaligned", k);
    }
    return nullptr;
}

void sort_permutation_host(const SortPlan& plan, const void* const* keys, void* perm, uint32_t perm_width, uint32_t* status) {
    const size_t n = plan.n;
    status[0] = H2_SORT_OK;
    status[1] = status[2] = 0xffffffffu;
    status[3] = 0;
    if (n == 0) return;
    // the bytes of every key: the column itself, or the canonical copy of a Montgomery one
    std::vector<std::vector<uint8_t>> canon(plan.num_keys);
    const uint8_t* base[SORT_MAX_KEYS];
    uint32_t width[SORT_MAX_KEYS];
    for (uint32_t k = 0; k < plan.num_keys; k++) {
        base[k] = (const uint8_t*)keys[k];
        width[k] = plan.form[k] == H2_ASSIGNED_FORM_COMPACT ? 8 : 32;
        if (plan.form[k] == H2_ASSIGNED_FORM_MONTGOMERY) {
            canon[k].resize(n * 32);
            for (size_t i = 0; i < n; i++) {
                Fr v;
                memcpy(v.l, base[k] + 32 * i, 32);
                v = fp_from_mont(v);
                memcpy(&canon[k][32 * i], v.l, 32);
            }
            base[k] = canon[k].data();
        }
    }
    // the promises: the lowest row that breaks one, and its lowest such key
    for (size_t i = 0; i < n && status[0] == H2_SORT_OK; i++)
        for (uint32_t k = 0; k < plan.num_keys; k++)
            if (at_or_above(base[k] + (size_t)width[k] * i, width[k], plan.bits[k])) {
                status[0] = H2_SORT_OUT_OF_RANGE;
                status[1] = (uint32_t)i;
                status[2] = k;
                break;
            }
    std::vector<uint32_t> cur(n), next(n);
    for (size_t i = 0; i < n; i++) cur[i] = (uint32_t)i;
    std::vector<size_t> count(256);
    for (uint32_t p = 0; p < plan.num_pos; p++) {
        const uint8_t* col = base[plan.pos[p].key] + plan.pos[p].byte;
        const uint32_t w = width[plan.pos[p].key];
        std::fill(count.begin(), count.end(), 0);
        for (size_t i = 0; i < n; i++) count[col[(size_t)w * i]]++;
        uint32_t nonempty = 0;
        for (size_t d = 0; d < 256; d++) nonempty += count[d] != 0;
        if (nonempty <= 1) continue;   // every cell agrees here: nothing moves
        size_t run = 0;
        for (size_t d = 0; d < 256; d++) {
            const size_t c = count[d];
            count[d] = run;
            run += c;
        }
        for (size_t i = 0; i < n; i++) next[count[col[(size_t)w * cur[i]]]++] = cur[i];
        cur.swap(next);
        status[3]++;
    }
    for (size_t i = 0; i < n; i++) {
        if (perm_width == 4) ((uint32_t*)perm)[i] = cur[i];
        else ((uint64_t*)perm)[i] = cur[i];
    }
}

}  // namespace h2
