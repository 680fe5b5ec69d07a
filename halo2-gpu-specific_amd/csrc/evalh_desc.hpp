// evalh_desc.hpp -- h2_evalh_desc stated once: its derived counts, its column slots and its validity rules.
// Host C++ only, no HIP header (tests/evalh_desc_host.cpp builds it with g++ alone).  The slot table below is the only place
// that names the descriptor's eight pointer tables and three single pointers; the generated kernels' argument filler, the
// interpreter's staging and the host drivers (evalh_plan.hip, evalh_interp.hpp, evalh.hip) all read the columns through it.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "evalh_gen.hpp"

namespace h2 {

// z cosets over all lookups / entries of lookup_calcs (per lookup: table, product_0, sum_0, product_1, sum_1, ...)
inline size_t evalh_lookup_z_count(const h2_evalh_desc* d) {
    size_t n = 0;
    for (uint32_t t = 0; t < d->n_lookups; t++) n += d->lookup_sets[t];
    return n;
}
inline size_t evalh_lookup_calc_count(const h2_evalh_desc* d) { return d->n_lookups + 2 * evalh_lookup_z_count(d); }

// Where the columns of one evgen::Table live: a pointer table with its length (count == nullptr: evalh_lookup_z_count), or
// one pointer.
struct EvalhSlot {
    const uint64_t* const* h2_evalh_desc::*table;
    uint32_t h2_evalh_desc::*count;
    const uint64_t* h2_evalh_desc::*single;
};
constexpr EvalhSlot EVALH_SLOTS[evgen::T_COUNT] = {
    {&h2_evalh_desc::fixed, &h2_evalh_desc::n_fixed, nullptr},             // T_FIXED
    {&h2_evalh_desc::advice, &h2_evalh_desc::n_advice, nullptr},           // T_ADVICE
    {&h2_evalh_desc::instance, &h2_evalh_desc::n_instance, nullptr},       // T_INSTANCE
    {&h2_evalh_desc::perm_z, &h2_evalh_desc::n_perm_sets, nullptr},        // T_PERM_Z
    {&h2_evalh_desc::perm_sigma, &h2_evalh_desc::n_perm_columns, nullptr}, // T_PERM_SIGMA
    {&h2_evalh_desc::lookup_z, nullptr, nullptr},                          // T_LOOKUP_Z
    {&h2_evalh_desc::lookup_m, &h2_evalh_desc::n_lookups, nullptr},        // T_LOOKUP_M
    {&h2_evalh_desc::shuffle_z, &h2_evalh_desc::n_shuffles, nullptr},      // T_SHUFFLE_Z
    {nullptr, nullptr, &h2_evalh_desc::l0},                                // T_L0
    {nullptr, nullptr, &h2_evalh_desc::l_last},                            // T_L_LAST
    {nullptr, nullptr, &h2_evalh_desc::l_active_row},                      // T_L_ACTIVE
};

// slots of one table (a single pointer is a table of one); its pointer array (null for a single pointer)
inline size_t evalh_table_count(const h2_evalh_desc* d, uint32_t table) {
    const EvalhSlot& s = EVALH_SLOTS[table];
    return s.single ? 1 : (s.count ? d->*s.count : evalh_lookup_z_count(d));
}
inline const uint64_t* const* evalh_table(const h2_evalh_desc* d, uint32_t table) {
    const EvalhSlot& s = EVALH_SLOTS[table];
    return s.single ? nullptr : d->*s.table;
}
// the pointer in slot (table, index); nullptr when there is no such slot
inline const uint64_t* evalh_column(const h2_evalh_desc* d, uint32_t table, size_t index) {
    if (table >= evgen::T_COUNT || index >= evalh_table_count(d, table)) return nullptr;
    const EvalhSlot& s = EVALH_SLOTS[table];
    return s.single ? d->*s.single : (d->*s.table)[index];
}

// f(table, index, pointer) for every slot, null ones included, in the order fixed, advice, instance, perm_z, perm_sigma,
// lookup_z, lookup_m, shuffle_z, l0, l_last, l_active_row.  The pointer array of an empty table is not read (it may be null).
template <class F>
void evalh_for_each_column(const h2_evalh_desc* d, F&& f) {
    for (uint32_t t = 0; t < evgen::T_COUNT; t++) {
        const size_t n = evalh_table_count(d, t);
        for (size_t i = 0; i < n; i++) f((evgen::Table)t, i, evalh_column(d, t, i));
    }
}

// A copy of `d` with every column slot p replaced by f(table, p) -- null stays null, f is not asked -- and the pointer tables
// that copy points into.  Everything else is `d`'s; `d` is only read.
struct EvalhRemap {
    h2_evalh_desc desc;
    template <class F>
    EvalhRemap(const h2_evalh_desc* d, F&& f) : desc(*d) {
        size_t total = 0;
        for (uint32_t t = 0; t < evgen::T_COUNT; t++) total += evalh_table_count(d, t);
        store_.reserve(total);   // (the copy points into it: it must not move)
        for (uint32_t t = 0; t < evgen::T_COUNT; t++) {
            const EvalhSlot& s = EVALH_SLOTS[t];
            const size_t n = evalh_table_count(d, t), at = store_.size();
            for (size_t i = 0; i < n; i++) {
                const uint64_t* p = evalh_column(d, t, i);
                store_.push_back(p ? f((evgen::Table)t, p) : nullptr);
            }
            if (s.single)
                desc.*s.single = store_[at];
            else
                desc.*s.table = n ? store_.data() + at : nullptr;
        }
    }
    EvalhRemap(const EvalhRemap&) = delete;
    EvalhRemap& operator=(const EvalhRemap&) = delete;

private:
    std::vector<const uint64_t*> store_;
};
template <class F>
EvalhRemap evalh_remap(const h2_evalh_desc* d, F&& f) {
    return EvalhRemap(d, f);
}

// ---- validity
// device: column pointers are device memory, a row range may be given; the two host forms take the whole domain
enum EvalhForm { EVALH_DEVICE, EVALH_HOST_EXTENDED, EVALH_HOST_COEFF };

// What is wrong with `d`, or nullptr when it is sound (the string lives until this thread's next call).  Checked before any
// size is computed from extended_k.  `entry` prefixes the rules every entry point states under its own name (null
// descriptor, k / extended_k, a row range handed to a host form); the others are h2_evaluate_h's for every caller, as they
// were when only the device driver stated them.
inline const char* evalh_validate(const h2_evalh_desc* d, const char* entry, EvalhForm form) {
    static thread_local std::string msg;
    auto say = [&](const char* prefix, const char* what) {
        msg = std::string(prefix) + ": " + what;
        return msg.c_str();
    };
    const char* const dev = "h2_evaluate_h";
    if (!d) return say(entry, "null argument");
    if (d->extended_k < d->k || d->extended_k > 28) return say(entry, "bad k / extended_k");
    if (form != EVALH_DEVICE && d->row_count) return say(entry, "a row range is for the device entry point (h2_dev_evaluate_h)");
    if (d->n_perm_sets && d->chunk_len == 0) return say(dev, "chunk_len must be non-zero when permutation sets are present");
    if (d->reserved != nullptr)
        return say(dev, "`reserved` must be NULL (round 4's caller-supplied kernel slot: the library generates the program's "
                        "kernels itself now, see h2_evalh_prepare)");
    if ((size_t)d->row_begin + d->row_count > (size_t)1 << d->extended_k) return say(dev, "row range outside the domain");
    if (d->n_perm_sets)   // the permutation argument's columns (evaluation.rs:1060-1064) exist
        for (uint32_t j = 0; j < d->n_perm_columns; j++) {
            const uint32_t ty = d->perm_col_type[j];
            const uint32_t table = ty == H2_ANY_ADVICE ? evgen::T_ADVICE : (ty == H2_ANY_FIXED ? evgen::T_FIXED : evgen::T_INSTANCE);
            if (d->perm_col_index[j] >= evalh_table_count(d, table)) return say(dev, "permutation column index out of range");
        }
    return nullptr;
}

}  // namespace h2
