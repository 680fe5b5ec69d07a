// ntt.hpp -- the pass schedule of a transform, NTT plans (twiddle tables per (log_n, omega)) with their per-device table
// cache, and the pass driver.
#pragma once
#include <atomic>
#include <vector>

#include "common.hpp"

namespace h2 {

// ---------------------------------------------------------------- the pass schedule
struct PassShape {
    uint32_t log_c, threads;
    bool radix4;  // two stages per LDS round trip, tabulated twiddles as (plain value, quotient) pairs
    bool fixed;   // the common geometry: 8 bits, tiles of 4 columns, 256 lanes (k_ntt_pass8 when nothing is skipped)
};
// One pass of a 2^log_n transform: everything about it that the size alone decides.  What depends on the call -- the live
// inputs, hence the rows a first pass skips, hence the kernel -- is pass_zskip / pass_kernel (ntt.hip).
struct NttPass {
    uint32_t B;      // width: an R = 2^B point DFT per element group
    uint32_t t_log;  // bits consumed before the pass (log2 of T_p; 0: the first pass)
    uint32_t s_log;  // log2 of its stride S_p = log_n - t_log - B
    bool last;
    PassShape shape;
};
void ntt_split(uint32_t log_n, std::vector<uint32_t>& bits);  // the widths alone
// The passes in order (for log_n = 0 the one pass of width 0 that copies and scales x[0]): the plan builder sizes its
// tables from it, the launcher runs it and h2_ntt_shape reports it.  A pass's prevB / prevT are the B / t_log of those before it.
std::vector<NttPass> ntt_schedule(uint32_t log_n);

// ---------------------------------------------------------------- the per-device cache of plans and their tables
struct NttPlan;
// a device table built on demand: one type for the divisor-scaled high tables, the coset scale tables and the last-pass tables
struct NttTable {
    Fr* ptr = nullptr;
    size_t bytes = 0;
    uint64_t last_use = 0;  // NttCache::clock at the last lookup
    int users = 0;          // NttTablePin holders: between looking the table up and having launched the pass that reads it
};
using NttTableMap = std::map<std::string, NttTable>;

// What every caller on ONE device shares (DeviceShared::ntt).  `mu` guards every member, every plan's table maps, last_misses
// and last_use, and every NttTable's users / last_use; it is never held across a device allocation, a launch or a
// synchronisation.  Callers need no lock of their own: what they hold is pinned (PlanRef, NttTablePin).
struct NttCache {
    std::mutex mu;
    std::map<std::string, NttPlan*> plans;  // (log_n, omega) -> plan
    size_t last_table_bytes = 0;            // of the optional last-pass tables of all plans: what ntt_table_budget bounds
    uint64_t clock = 0;                     // least-recently-used order of plans and tables
};

struct NttPlan {
    NttCache* cache = nullptr;
    uint32_t log_n = 0;
    Fr w;                              // the root of unity the plan was built for (Montgomery form)
    std::vector<NttPass> sched;        // ntt_schedule(log_n)
    Fr* tables = nullptr;              // one allocation: lo | hi | per-pass butterfly tables
    const Fr* tw_lo = nullptr;         // w^i,        i < min(n, 4096)
    const Fr* tw_hi = nullptr;         // w^(i<<12),  i < n >> 12
    // per pass: (w^(n/R))^e, e < R/2 -- as (plain value, floor(value 2^256 / r)) PAIRS, the operands of the constant-operand
    // product fp_mul_const, for the passes with shape.radix4 (transforms >= 2^18)
    std::vector<const Fr*> tw_bfly;
    std::vector<const Fr*> tw_chunk;   // per pass of the fixed geometry: tw_bfly's values as chunk tables (fp_mul_chunk), else nullptr
    std::vector<const Fr*> tw_chunk32; // ... and those of index 0, 4, 8 .. as eight-chunk entries (TwChunk32, 8 KiB), else nullptr
    // per pass: its full inter-pass twiddle set as chunk tables, w^(rho K S) at [(rho << t_log) | K] (the middle pass of a plan
    // of three passes or more), else nullptr.  The pass BEFORE it multiplies by them at its store (PassArgs::nx_tab).
    std::vector<const Fr*> tw_inter;
    size_t table_bytes = 0;            // of `tables` and the per-pass tw_inter tables
    NttTableMap scaled_hi;   // divisor -> tw_hi * divisor (iNTT: 1/n folded into the last pass); kept for the plan's life
    // (generator, divisor) -> two-level table of g^i (coset transforms): 4096 + n/4096 entries.  At most SCALE_TABS_MAX per
    // plan: the public coset entry points take any generator, so the least recently used table nobody holds is dropped
    static constexpr size_t SCALE_TABS_MAX = 32;
    NttTableMap scale_tabs;
    // the last pass's complete inter-pass twiddle set, w^(rho * K) at [(K << B_last) | rho] (2^log_n entries, streamed in
    // the order the pass loads its elements), keyed by the divisor folded into it ("" = none).  These are the large
    // optional tables (32 B x n each): they count against the per-device budget (ntt_table_budget) and the least
    // recently used idle one is evicted when a new one would exceed it; a transform that finds none composes its
    // twiddles from the two-level tables (one more product per element, same values).
    NttTableMap last_direct;
    std::map<std::string, int> last_misses;  // lookups of a key that found no table (a key evicts others from its 2nd miss on)
    std::atomic<int> users{0};         // callers holding the plan (PlanRef): a plan in use is not released
    uint64_t last_use = 0;
};

// a plan handed out by ntt_get_plan stays alive until its PlanRef goes (h2_release_plans skips plans in use)
struct PlanRef {
    NttPlan* pl = nullptr;
    PlanRef() = default;
    explicit PlanRef(NttPlan* p) : pl(p) {}
    PlanRef(PlanRef&& o) noexcept : pl(o.pl) { o.pl = nullptr; }
    PlanRef& operator=(PlanRef&& o) noexcept {  // (what this held goes with `o`)
        std::swap(pl, o.pl);
        return *this;
    }
    ~PlanRef() {
        if (pl) pl->users.fetch_sub(1);
    }
    NttPlan* operator->() const { return pl; }
    NttPlan* get() const { return pl; }
};

// A pinned table (or none): it is neither evicted nor released with its plan until the pin goes -- after the pass that reads
// it has been launched, or when anything on the way there throws.  An evicted table is freed after a device synchronisation.
struct NttTablePin {
    NttCache* cache = nullptr;
    NttTable* tab = nullptr;
    NttTablePin() = default;
    NttTablePin(NttCache* c, NttTable* t) : cache(c), tab(t) {}
    NttTablePin(NttTablePin&& o) noexcept : cache(o.cache), tab(o.tab) { o.tab = nullptr; }
    NttTablePin& operator=(NttTablePin&& o) noexcept {  // (what this held goes with `o`)
        std::swap(cache, o.cache);
        std::swap(tab, o.tab);
        return *this;
    }
    ~NttTablePin() {
        if (tab) {
            std::lock_guard<std::mutex> g(cache->mu);
            tab->users--;
        }
    }
    const Fr* get() const { return tab ? tab->ptr : nullptr; }
};

// Finds or builds the plan and returns it pinned.  Needs no lock of the caller's: the lookup runs under the cache's mutex,
// the tables are built outside it on `stream` and complete before the plan is published (of two racing builders one loses
// and frees its own), and the pin keeps the plan from being released.  A pinned plan's tw_* tables may be read freely.
PlanRef ntt_get_plan(DeviceCtx* ctx, uint32_t log_n, const uint64_t omega[4], hipStream_t stream);
// Frees every plan of ctx's device that no caller holds, with all its tables, after a device synchronisation (the plans'
// device current, no lock held: passes already launched against the tables finish first).
void ntt_release_idle_plans(DeviceCtx* ctx);
// bytes of device memory the plans of ctx's device hold: their own tables and every table built on demand
size_t ntt_plan_bytes(DeviceCtx* ctx);
// per-device budget of the optional last-pass tables: H2_NTT_TABLE_BUDGET (bytes; K / M / G suffixes) or
// h2_set_table_budget; default 1/32 of the device's memory (9 GiB on an MI355X: a k = 24 proof's four tables take 3)
size_t ntt_table_budget(DeviceCtx* ctx);
void ntt_set_table_budget(size_t bytes);
// src (in_len valid elements, zero-extended to 2^log_n) -> dst; tmp = 2^log_n scratch (needed when
// the plan has >= 2 passes).  pre3 / post3: nullable HOST pointers to 3 Fr each (passed by value
// in the kernel arguments): x[i] *= pre3[i % 3] (i % 3 != 0) on load, y[i] *= post3[i % 3] on store.
// scale_tab (ntt_scale_table) with scale_mode 1: x[i] *= g^i on the first pass's load; 2: y[i] *= g^i (* divisor) on the
// final store -- the transforms between coefficients and ONE coset g H of a larger domain, without a separate scaling pass.
void ntt_run(DeviceCtx* ctx, NttPlan* pl, const Fr* src, Fr* dst, Fr* tmp, uint32_t in_len, const Fr* pre3,
             const Fr* post3, hipStream_t stream, const Fr* scale_tab = nullptr, uint32_t scale_mode = 0);
// the two-level table of g^i (* d) of a pinned plan, pinned until the caller has launched what reads it
NttTablePin ntt_scale_table(NttPlan* pl, const Fr& g, const Fr* d, hipStream_t stream);
// `count` transforms of one plan with the same scales, several vectors per launch; tmps[i] = scratch of vector i
void ntt_run_many(DeviceCtx* ctx, NttPlan* pl, const Fr* const* srcs, Fr* const* dsts, Fr* const* tmps, size_t count,
                  uint32_t in_len, const Fr* pre3, const Fr* post3, hipStream_t stream, const Fr* scale_tab = nullptr,
                  uint32_t scale_mode = 0);
Fr fr_from_u64x4(const uint64_t v[4]);
void fr_to_u64x4(const Fr& v, uint64_t out[4]);
// h2_ntt_shape: the passes of a 2^log_n transform over 2^in_log live inputs, 7 words each into out[0 .. 7 * min(passes, cap));
// returns the number of passes.  Reads ntt_schedule and the launcher's own zskip / kernel selectors and knobs.
size_t ntt_shape_query(uint32_t log_n, uint32_t in_log, uint32_t* out, size_t cap);

}  // namespace h2
