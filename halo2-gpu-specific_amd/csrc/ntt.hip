// ntt.hip -- the host side of the multi-pass NTT (the kernels and the decomposition they implement: ntt_pass.hip): the pass
// schedule of a size and what a call adds to it; the per-device cache of plans and of the tables built on demand, with its
// one lock, pins and eviction rules; the pass driver (ntt_run, ntt_run_many).
#include <algorithm>
#include <cstdlib>
#include <memory>
#include <utility>

#include "common.hpp"
#include "ntt.hpp"
#include "ntt_pass.hpp"

namespace h2 {

// ---------------------------------------------------------------- pass schedule
void ntt_split(uint32_t log_n, std::vector<uint32_t>& bits) {
    bits.clear();
    if (log_n == 0) return;
    // as many 8-bit passes as possible, the remainder first (it needs no inter-pass twiddle).  A remainder of ONE bit would
    // be a whole sweep over memory for a single stage (2^25, the extended domain of a k = 24 proof: 1 + 8 + 8 + 8): it is
    // folded into a 9-bit pass at the END instead (8 + 8 + 9: the middle pass keeps its 2^16-entry twiddle table; 512-row
    // tiles of 4 columns, 74 KB of LDS): 2^25 4.61 -> 4.33 ms, 2^17 47 -> 41 us.  Two 9-bit passes pay up to 2^18 (9 + 9:
    // 69 -> 62 us) but not at 2^26 (8 + 9 + 9: 8.98 -> 9.04 ms), three never.
    const uint32_t rem = log_n % 8, q = log_n / 8;
    static const bool nine = !(getenv("H2_NTT_NINE") && atoi(getenv("H2_NTT_NINE")) == 0);
    if (nine && q >= rem && (rem == 1 || (rem == 2 && log_n <= 18))) {
        for (uint32_t p = 0; p < q - rem; p++) bits.push_back(8);
        for (uint32_t p = 0; p < rem; p++) bits.push_back(9);
        return;
    }
    if (rem) bits.push_back(rem);
    for (uint32_t p = 0; p < q; p++) bits.push_back(8);
}

// `avail`: the columns a tile can take -- log2 of the stride (s_log) for the passes before the last, of the DFT count for the last
static PassShape pass_shape(uint32_t L, uint32_t B, uint32_t avail) {
    PassShape sh{};
    uint32_t log_c = (B < 8) ? (10 - B) : 2;  // tile = R rows x C columns, about 1024 elements
    if (avail < log_c) log_c = avail;
    sh.log_c = log_c;
    uint32_t threads = ((1u << B) >> 1) << log_c;
    // four elements per lane, half the threads per tile
    // (transforms below 2^18 are latency-bound chains of a few tiles: more lanes per tile finish them sooner)
    sh.radix4 = B >= 2 && threads >= 128 && L >= 18;
    if (sh.radix4) threads >>= 1;
    if (threads < 64) threads = 64;
    if (threads > 512) threads = 512;
    sh.threads = threads;
    sh.fixed = sh.radix4 && B == 8 && log_c == 2 && threads == 256;
    return sh;
}

std::vector<NttPass> ntt_schedule(uint32_t log_n) {
    std::vector<uint32_t> bits;
    ntt_split(log_n, bits);
    if (bits.empty()) bits.push_back(0);  // n = 1: X[0] = x[0] (times its scales), one lane of the radix-2 kernel
    std::vector<NttPass> sched;
    uint32_t consumed = 0;
    for (size_t p = 0; p < bits.size(); p++) {
        NttPass ps{};
        ps.B = bits[p];
        ps.t_log = consumed;
        ps.s_log = log_n - consumed - ps.B;
        ps.last = p + 1 == bits.size();
        ps.shape = pass_shape(log_n, ps.B, ps.last ? ps.t_log : ps.s_log);
        sched.push_back(ps);
        consumed += ps.B;
    }
    return sched;
}

// Rows of the first pass that zero padding leaves live: in_len = 2^(L - z) of 2^L elements prunes the first min(z, B) stages
// of a first pass that is not also the last (H2_NTT_NO_ZSKIP: none)
static uint32_t pass_zskip(uint32_t L, const NttPass& ps, uint32_t in_len) {
    static const bool no_zskip = getenv("H2_NTT_NO_ZSKIP") != nullptr;
    if (ps.t_log != 0 || ps.last || !in_len || in_len >= (1u << L) || (in_len & (in_len - 1)) != 0 || no_zskip) return 0;
    uint32_t z = 0;
    while ((in_len << z) < (1u << L)) z++;  // padded by 2^z
    return z < ps.B ? z : ps.B;             // in_len = (R >> z) * S rows exactly when z <= B
}

static NttKernel pass_kernel(const NttPass& ps, uint32_t zskip) {
    if (!ps.shape.radix4) return NK_R2;
    if (ps.shape.fixed && zskip == 0) return ps.last ? NK_PASS8 : NK_PASS8_DP;
    return ps.last ? NK_R4 : NK_R4_DP;
}

// The plan of a transform as the launcher will run it (h2_ntt_shape): per pass 7 words -- bits, log_c, threads, radix4,
// fixed, zskip, kernel id.  Host only: nothing is allocated or launched.
size_t ntt_shape_query(uint32_t log_n, uint32_t in_log, uint32_t* out, size_t cap) {
    if (log_n == 0) return 0;  // (the copy of a one-point transform is no pass of a decomposition)
    const std::vector<NttPass> sched = ntt_schedule(log_n);
    for (size_t p = 0; p < sched.size() && p < cap; p++) {
        const NttPass& ps = sched[p];
        const uint32_t zskip = pass_zskip(log_n, ps, 1u << in_log);
        const uint32_t row[7] = {ps.B, ps.shape.log_c, ps.shape.threads, ps.shape.radix4, ps.shape.fixed, zskip,
                                 (uint32_t)pass_kernel(ps, zskip)};
        for (int i = 0; i < 7; i++) out[7 * p + i] = row[i];
    }
    return sched.size();
}

static std::string plan_key(uint32_t log_n, const uint64_t omega[4]) {
    char buf[128];
    snprintf(buf, sizeof buf, "%u:%016llx%016llx%016llx%016llx", log_n, (unsigned long long)omega[3],
             (unsigned long long)omega[2], (unsigned long long)omega[1], (unsigned long long)omega[0]);
    return buf;
}

// the eight limbs of an element, most significant first: the key of a table cached per divisor or generator
static std::string fr_key(const Fr& v) {
    char buf[72];
    snprintf(buf, sizeof buf, "%08x%08x%08x%08x%08x%08x%08x%08x", v.l[7], v.l[6], v.l[5], v.l[4], v.l[3], v.l[2], v.l[1], v.l[0]);
    return buf;
}

Fr fr_from_u64x4(const uint64_t v[4]) {
    Fr r;
    for (int i = 0; i < 4; i++) {
        r.l[2 * i] = (uint32_t)v[i];
        r.l[2 * i + 1] = (uint32_t)(v[i] >> 32);
    }
    return r;
}
void fr_to_u64x4(const Fr& v, uint64_t out[4]) {
    for (int i = 0; i < 4; i++) out[i] = (uint64_t)v.l[2 * i] | ((uint64_t)v.l[2 * i + 1] << 32);
}

// ---------------------------------------------------------------- the table cache
// a device block its builder owns until it is published
struct TableBlock {
    Fr* p = nullptr;
    ~TableBlock() {
        if (p) (void)hipFree(p);
    }
    // the enqueued fills are complete before any other stream can find the table (once per table)
    NttTable publish(size_t bytes, hipStream_t stream) {
        H2_HIP(hipGetLastError());
        H2_HIP(hipStreamSynchronize(stream));
        return NttTable{std::exchange(p, nullptr), bytes};
    }
};

// THE rule for a table that leaves a cache while its plan lives on (or with its plan): it was unhooked under the lock with
// no pin on it, so nobody can launch against it any more; the passes already launched finish -- a device synchronisation,
// with no lock held -- and then it is freed.
static void tables_free(const std::vector<Fr*>& gone) {
    if (gone.empty()) return;
    const hipError_t e = hipDeviceSynchronize();
    for (Fr* t : gone) (void)hipFree(t);
    H2_HIP(e);
}

// the least recently used table of `map` that nobody holds (end(): none)
static NttTableMap::iterator lru_idle(NttTableMap& map) {
    auto lru = map.end();
    for (auto it = map.begin(); it != map.end(); ++it)
        if (it->second.users == 0 && (lru == map.end() || it->second.last_use < lru->second.last_use)) lru = it;
    return lru;
}

// The one way a table is looked up and enters a map of its plan.  Under the lock: find and pin.  On a miss `build()` runs
// OUTSIDE it (it allocates, launches and synchronises its stream: the other callers of the device keep transforming) and
// returns a complete table, or none (ptr == nullptr: the caller does without).  Under the lock again: a racing builder may
// have published the same key -- theirs stays and ours is freed (nobody has seen it) --, else `admit(gone)` applies the
// map's policy (accounting; tables it unhooks to make room go into `gone` and are freed by tables_free) and ours is published.
template <class Build, class Admit>
static NttTablePin table_get(NttCache* c, NttTableMap& map, const std::string& key, Build build, Admit admit) {
    auto pin = [&]() -> NttTable* {  // with c->mu held
        auto it = map.find(key);
        if (it == map.end()) return nullptr;
        it->second.users++;
        it->second.last_use = ++c->clock;
        return &it->second;
    };
    {
        std::lock_guard<std::mutex> g(c->mu);
        if (NttTable* t = pin()) return NttTablePin(c, t);
    }
    NttTable made = build();
    Fr* lost = nullptr;
    std::vector<Fr*> gone;
    NttTablePin out;
    {
        std::lock_guard<std::mutex> g(c->mu);
        NttTable* t = pin();
        if (t) {
            lost = made.ptr;
        } else if (made.ptr) {
            admit(gone);
            map[key] = made;
            t = pin();
        }
        out = NttTablePin(c, t);
    }
    if (lost) (void)hipFree(lost);
    tables_free(gone);
    return out;
}

static std::atomic<size_t> g_budget_override{(size_t)-1};

static size_t parse_bytes(const char* s) {
    char* end = nullptr;
    double v = strtod(s, &end);
    if (end && (*end == 'K' || *end == 'k')) v *= 1024.0;
    if (end && (*end == 'M' || *end == 'm')) v *= 1024.0 * 1024.0;
    if (end && (*end == 'G' || *end == 'g')) v *= 1024.0 * 1024.0 * 1024.0;
    return v <= 0 ? 0 : (size_t)v;
}

void ntt_set_table_budget(size_t bytes) { g_budget_override.store(bytes); }

size_t ntt_table_budget(DeviceCtx* ctx) {
    const size_t o = g_budget_override.load();
    if (o != (size_t)-1) return o;
    static const char* env = getenv("H2_NTT_TABLE_BUDGET");
    if (env) return parse_bytes(env);
    return (size_t)ctx->prop.totalGlobalMem / 32;
}

// Makes room for `need` more bytes of last-pass tables on the device: idle tables of any plan leave in least-recently-used
// order.  Returns false when the budget cannot hold `need` even then.  Call WITHOUT the cache's lock.
// `allow_evict` = false: only room that is already free counts.  A table is an optimisation worth ONE product per element
// per transform; evicting one costs a device-wide synchronisation and rebuilding the other a pass over n elements, so a
// key only displaces resident tables once it has missed twice (a budget of one or two tables under a proof that cycles
// through forward / inverse transforms and their divisors would otherwise rebuild a table on every call).
static bool last_table_make_room(DeviceCtx* ctx, size_t need, bool allow_evict) {
    NttCache* c = ctx->shared->ntt;
    const size_t budget = ntt_table_budget(ctx);
    if (need > budget) return false;
    std::vector<Fr*> gone;
    {
        std::lock_guard<std::mutex> g(c->mu);
        while (allow_evict && c->last_table_bytes + need > budget) {
            NttTableMap* owner = nullptr;
            NttTableMap::iterator victim;
            for (auto& pk : c->plans) {
                NttTableMap& map = pk.second->last_direct;
                const auto it = lru_idle(map);
                if (it != map.end() && (!owner || it->second.last_use < victim->second.last_use)) {
                    owner = &map;
                    victim = it;
                }
            }
            if (!owner) break;
            gone.push_back(victim->second.ptr);
            c->last_table_bytes -= victim->second.bytes;
            owner->erase(victim);
        }
    }
    tables_free(gone);
    std::lock_guard<std::mutex> g(c->mu);
    return c->last_table_bytes + need <= budget;
}

// The last pass of a large transform reads its inter-pass twiddles from a complete table (32 B x n, streamed in the order
// of its loads) instead of composing each from two: one product per element instead of two, on a pass that is bound by
// VALU issue and has the HBM time to spare (2^24: 1.84 -> see DESIGN 3.2).  One table per divisor folded into it (`d`, null:
// none), inside the per-device budget (ntt_table_budget: the least recently used idle table leaves first).  Finds the table
// or builds and publishes it, and returns it pinned; H2_NTT_LAST_TABLE=0, a size outside 2^18 .. 2^H2_NTT_LAST_TABLE_MAX_LOG,
// no room in the budget or a failed allocation return none: the pass then composes its twiddles (lo x hi).
static NttTablePin last_table(DeviceCtx* ctx, NttPlan* pl, uint32_t B, const Fr* d, hipStream_t stream) {
    static const bool enabled = !(getenv("H2_NTT_LAST_TABLE") && atoi(getenv("H2_NTT_LAST_TABLE")) == 0);
    static const uint32_t max_log = getenv("H2_NTT_LAST_TABLE_MAX_LOG") ? (uint32_t)atoi(getenv("H2_NTT_LAST_TABLE_MAX_LOG")) : 26u;
    const uint32_t L = pl->log_n;
    if (!enabled || L < 18 || L > max_log) return NttTablePin();
    NttCache* c = pl->cache;
    const std::string key = d ? fr_key(*d) : std::string();
    const size_t bytes = sizeof(Fr) << L;   // (Montgomery form also under CW: see k_ntt_pass's DP)
    auto build = [&]() -> NttTable {
        bool may_evict;
        {
            std::lock_guard<std::mutex> g(c->mu);
            may_evict = ++pl->last_misses[key] >= 2;   // see last_table_make_room
        }
        TableBlock block;
        if (!last_table_make_room(ctx, bytes, may_evict)) return NttTable();
        if (hipMalloc(&block.p, bytes) != hipSuccess) {
            (void)hipGetLastError();  // no room on the device: this transform composes its twiddles
            block.p = nullptr;
            return NttTable();
        }
        ntt_fill_last(block.p, pl->w, B, L, d, stream);   // (a table is 0.5 .. 2 GiB of powers)
        return block.publish(bytes, stream);
    };
    auto admit = [&](std::vector<Fr*>&) {
        c->last_table_bytes += bytes;
        pl->last_misses[key] = 0;  // evicted later, it has to miss twice again before it displaces others
    };
    return table_get(c, pl->last_direct, key, build, admit);
}

// tw_hi * d: the iNTT's divisor folded into the high twiddle table the last pass composes its inter-pass twiddles from.  One
// per divisor, kept for the plan's life.
static NttTablePin scaled_hi_table(NttPlan* pl, const Fr& d, hipStream_t stream) {
    auto build = [&]() -> NttTable {
        const uint32_t cnt = (1u << pl->log_n) >> LO_BITS;
        TableBlock block;
        H2_HIP(hipMalloc(&block.p, cnt * sizeof(Fr)));
        ntt_fill_scaled(block.p, pl->tw_hi, d, cnt, stream);
        return block.publish(cnt * sizeof(Fr), stream);
    };
    return table_get(pl->cache, pl->scaled_hi, fr_key(d), build, [](std::vector<Fr*>&) {});
}

// The two-level table of g^i (i < 2^log_n) with `d` folded into the high level, cached with the plan: the coset transforms
// of a proof use quotient_poly_degree generators per direction, again and again.  At most SCALE_TABS_MAX per plan: the idle
// least recently used ones make room (over the cap for as long as every table is held).
NttTablePin ntt_scale_table(NttPlan* pl, const Fr& g, const Fr* d, hipStream_t stream) {
    auto build = [&]() -> NttTable {
        const uint32_t n = 1u << pl->log_n;
        const uint32_t lo_count = n < (1u << LO_BITS) ? n : (1u << LO_BITS);
        const uint32_t hi_count = pl->log_n > LO_BITS ? (n >> LO_BITS) : 1u;
        const size_t bytes = ((size_t)(1u << LO_BITS) + hi_count) * sizeof(Fr);
        TableBlock block;
        H2_HIP(hipMalloc(&block.p, bytes));
        Fr* const hi = block.p + (1u << LO_BITS);
        ntt_fill_pow(block.p, g, 1u, lo_count, 0u, stream);
        ntt_fill_pow(hi, g, 1u << LO_BITS, hi_count, 0u, stream);
        if (d) ntt_fill_scaled(hi, hi, *d, hi_count, stream);
        return block.publish(bytes, stream);
    };
    auto admit = [&](std::vector<Fr*>& gone) {
        while (pl->scale_tabs.size() >= NttPlan::SCALE_TABS_MAX) {
            const auto lru = lru_idle(pl->scale_tabs);
            if (lru == pl->scale_tabs.end()) break;
            gone.push_back(lru->second.ptr);
            pl->scale_tabs.erase(lru);
        }
    };
    return table_get(pl->cache, pl->scale_tabs, d ? fr_key(g) + '*' + fr_key(*d) : fr_key(g) + '.', build, admit);
}

// ---------------------------------------------------------------- plans
static void free_plan(NttPlan* pl) {
    if (pl->tables) (void)hipFree(pl->tables);
    for (const Fr* t : pl->tw_inter)
        if (t) (void)hipFree(const_cast<Fr*>(t));
    for (NttTableMap* map : {&pl->scaled_hi, &pl->scale_tabs, &pl->last_direct})
        for (auto& kv : *map) (void)hipFree(kv.second.ptr);
    delete pl;
}

// with cache->mu held: the bytes of everything the plan holds, and whether any of its tables is pinned
static size_t plan_bytes(NttPlan* pl, bool* pinned = nullptr) {
    size_t bytes = pl->table_bytes;
    for (NttTableMap* map : {&pl->scaled_hi, &pl->scale_tabs, &pl->last_direct})
        for (auto& kv : *map) {
            bytes += kv.second.bytes;
            if (pinned && kv.second.users != 0) *pinned = true;
        }
    return bytes;
}

size_t ntt_plan_bytes(DeviceCtx* ctx) {
    NttCache* c = ctx->shared->ntt;
    std::lock_guard<std::mutex> g(c->mu);
    size_t bytes = 0;
    for (auto& kv : c->plans) bytes += plan_bytes(kv.second);
    return bytes;
}

void ntt_release_idle_plans(DeviceCtx* ctx) {
    NttCache* c = ctx->shared->ntt;
    std::vector<NttPlan*> gone;
    {
        std::lock_guard<std::mutex> g(c->mu);
        for (auto it = c->plans.begin(); it != c->plans.end();) {
            NttPlan* pl = it->second;
            bool busy = pl->users.load() != 0;
            plan_bytes(pl, &busy);
            if (busy) {
                ++it;
                continue;
            }
            for (auto& kv : pl->last_direct) c->last_table_bytes -= kv.second.bytes;
            gone.push_back(pl);
            it = c->plans.erase(it);
        }
    }
    if (gone.empty()) return;
    // nobody can reach these plans any more; passes already launched against their tables finish first (tables_free's rule)
    const hipError_t e = hipDeviceSynchronize();
    for (NttPlan* pl : gone) free_plan(pl);
    H2_HIP(e);
}

PlanRef ntt_get_plan(DeviceCtx* ctx, uint32_t log_n, const uint64_t omega[4], hipStream_t stream) {
    NttCache* c = ctx->shared->ntt;
    const std::string key = plan_key(log_n, omega);
    auto pin = [&]() -> NttPlan* {  // with c->mu held
        auto it = c->plans.find(key);
        if (it == c->plans.end()) return nullptr;
        it->second->users.fetch_add(1);
        it->second->last_use = ++c->clock;
        return it->second;
    };
    {
        std::lock_guard<std::mutex> g(c->mu);
        if (NttPlan* found = pin()) return PlanRef(found);
    }

    // built outside the lock, owned here until it is published
    std::unique_ptr<NttPlan, void (*)(NttPlan*)> pl(new NttPlan(), free_plan);
    pl->cache = c;
    pl->log_n = log_n;
    pl->sched = ntt_schedule(log_n);
    const Fr w = pl->w = fr_from_u64x4(omega);
    const uint32_t n = 1u << log_n;
    const uint32_t lo_count = n < (1u << LO_BITS) ? n : (1u << LO_BITS);
    const uint32_t hi_count = log_n > LO_BITS ? (n >> LO_BITS) : 0;
    // one block: lo | hi | per pass its R/2 butterfly twiddles (pairs for a radix-4 pass), then -- the fixed geometry -- the
    // same values as chunk tables; the pair table stays for the general kernel (zero padding is a property of the call)
    auto bfly_entries = [](const NttPass& ps) { return ((1u << ps.B) >> 1) * (ps.shape.radix4 ? 2u : 1u); };
    auto chunk_entries = [](const NttPass& ps) { return ps.shape.fixed ? ((1u << ps.B) >> 1) * TW_CHUNK_FR : 0u; };
    // ... and the values of index 0, 4, 8 .. once more as eight-chunk entries (the stage pairs before the last: TwChunk32)
    auto chunk32_entries = [](const NttPass& ps) { return ps.shape.fixed ? TW_CHUNK32_ENTRIES * TW_CHUNK32_FR : 0u; };
    size_t total = lo_count + hi_count;
    for (const NttPass& ps : pl->sched) total += bfly_entries(ps) + chunk_entries(ps) + chunk32_entries(ps);
    H2_HIP(hipMalloc(&pl->tables, total * sizeof(Fr)));
    pl->table_bytes = total * sizeof(Fr);
    pl->tw_lo = pl->tables;
    pl->tw_hi = pl->tables + lo_count;
    ntt_fill_pow(pl->tables, w, 1u, lo_count, 0u, stream);
    ntt_fill_pow(pl->tables + lo_count, w, 1u << LO_BITS, hi_count, 0u, stream);
    Fr* next = pl->tables + lo_count + hi_count;
    for (const NttPass& ps : pl->sched) {
        const uint32_t half = (1u << ps.B) >> 1, form = ps.shape.radix4 ? 1u : 0u;
        ntt_fill_pow(next, w, n >> ps.B, half, form, stream);
        pl->tw_bfly.push_back(next);
        next += bfly_entries(ps);
        if (ps.shape.fixed) ntt_fill_pow(next, w, n >> ps.B, half, 2u, stream);
        pl->tw_chunk.push_back(ps.shape.fixed ? next : nullptr);
        next += chunk_entries(ps);
        if (ps.shape.fixed) ntt_fill_pow(next, w, (n >> ps.B) * (half / TW_CHUNK32_ENTRIES), TW_CHUNK32_ENTRIES, 3u, stream);
        pl->tw_chunk32.push_back(ps.shape.fixed ? next : nullptr);
        next += chunk32_entries(ps);
        // A middle pass whose whole inter-pass twiddle set has <= 2^16 entries (pass 1 of every plan of three passes or more:
        // t_log is the first pass's width) gets it tabulated, as chunk entries in the order (rho << t_log) | K.  The pass
        // BEFORE it multiplies by them where it stores (pass_args: nx_tab / tw_applied): there a tile reads consecutive
        // entries -- 32 KiB per tile of the fixed geometry, about 0.5 MiB hot per L2 of the 8 MiB a 2^16-entry table takes.
        Fr* tab = nullptr;
        if (ps.t_log != 0 && !ps.last && ps.B + ps.t_log <= 16) {
            const uint32_t cnt = 1u << (ps.B + ps.t_log);
            const size_t bytes = (size_t)cnt * sizeof(TwChunk);
            H2_HIP(hipMalloc(&tab, bytes));
            pl->table_bytes += bytes;
        }
        pl->tw_inter.push_back(tab);
        if (tab) ntt_fill_direct(tab, w, ps.t_log, ps.s_log, log_n, 1u << (ps.B + ps.t_log), 2u, stream);
    }
    H2_HIP(hipGetLastError());
    // the tables are complete before the plan is published: a second caller on another stream (h2_dev_* on a different
    // torch stream, or the host API after a device-API first use) must not launch passes against tables still being
    // written.  Once per (log_n, omega) for the life of the process.
    H2_HIP(hipStreamSynchronize(stream));
    std::lock_guard<std::mutex> g(c->mu);
    // another caller on this device built the same plan meanwhile: the published one stays (this one's tables are complete
    // and nobody else has seen them: freed at once, with `pl`)
    if (NttPlan* raced = pin()) return PlanRef(raced);
    c->plans[key] = pl.get();
    pl.release();
    return PlanRef(pin());
}

// ---------------------------------------------------------------- the pass driver
static void set_scale3(PassArgs& a, const Fr* pre3, const Fr* post3) {
    a.has_pre3 = pre3 != nullptr;
    a.has_post3 = post3 != nullptr;
    a.post3_uniform = post3 && fp_eq(post3[0], post3[1]) && fp_eq(post3[0], post3[2]);
    for (int i = 0; i < 3; i++) {
        if (pre3) a.pre3[i] = pre3[i];
        if (post3) a.post3[i] = post3[i];
    }
}

void ntt_run(DeviceCtx* ctx, NttPlan* pl, const Fr* src, Fr* dst, Fr* tmp, uint32_t in_len, const Fr* pre3,
             const Fr* post3, hipStream_t stream, const Fr* scale_tab, uint32_t scale_mode) {
    ntt_run_many(ctx, pl, &src, &dst, &tmp, 1, in_len, pre3, post3, stream, scale_tab, scale_mode);
}

// The arguments of pass p over `cnt` vectors, but for the tables built on demand.  Buffer chain: pass 0 reads src, the passes
// between run in place on the vector's scratch, the last writes dst (a single pass src -> dst through LDS: a tile is a whole DFT).
static PassArgs pass_args(const NttPlan* pl, size_t p, const Fr* const* srcs, Fr* const* dsts, Fr* const* tmps, uint32_t cnt,
                          uint32_t in_len, const Fr* pre3, const Fr* post3, const Fr* scale_tab, uint32_t scale_mode) {
    const NttPass& ps = pl->sched[p];
    const bool first = p == 0, chain = pl->sched.size() >= 2;
    PassArgs a{};
    a.in = first ? srcs[0] : tmps[0];
    a.out = ps.last ? dsts[0] : tmps[0];
    if (cnt > 1) {
        a.batch = cnt;
        for (uint32_t i = 0; i < cnt; i++) {
            Fr* const work_i = chain ? tmps[i] : nullptr;
            a.in_b[i] = first ? srcs[i] : work_i;
            a.out_b[i] = ps.last ? dsts[i] : work_i;
        }
    }
    a.tw_bfly = pl->tw_bfly[p];
    a.tw_chunk = pl->tw_chunk[p];
    a.tw_chunk32 = pl->tw_chunk32[p];
    a.tw_lo = pl->tw_lo;
    a.tw_hi = pl->tw_hi;
    a.tw_applied = pl->tw_inter[p] != nullptr;
    if (!ps.last && pl->tw_inter[p + 1]) {
        const NttPass& nx = pl->sched[p + 1];
        a.nx_tab = pl->tw_inter[p + 1];
        a.nx_s_log = nx.s_log;
        a.nx_B = nx.B;
        a.nx_t_log = nx.t_log;
    }
    set_scale3(a, first ? pre3 : nullptr, ps.last ? post3 : nullptr);
    a.log_n = pl->log_n;
    a.B = ps.B;
    a.s_log = ps.s_log;
    a.t_log = ps.t_log;
    a.nprev = (uint32_t)p;
    for (size_t q = 0; q < p; q++) {
        a.prevB[q] = pl->sched[q].B;
        a.prevT[q] = pl->sched[q].t_log;
    }
    a.is_last = ps.last ? 1 : 0;
    a.in_len = first ? in_len : (1u << pl->log_n);
    a.log_c = ps.shape.log_c;
    a.sc_lo = scale_tab;
    a.sc_hi = scale_tab ? scale_tab + (1u << LO_BITS) : nullptr;
    a.scale_mode = (scale_tab && ((scale_mode == 1u && first) || (scale_mode == 2u && ps.last))) ? scale_mode : 0u;
    a.zskip = pass_zskip(pl->log_n, ps, in_len);
    a.radix4 = ps.shape.radix4 ? 1u : 0u;
    return a;
}

// `count` transforms of one plan (same size, root, scales): chunks of NTT_BATCH_MAX vectors per launch.  tmps[i]: the
// scratch of vector i (distinct per vector of a chunk; needed when the plan has >= 2 passes).
static void ntt_run_chunk(DeviceCtx* ctx, NttPlan* pl, const Fr* const* srcs, Fr* const* dsts, Fr* const* tmps, uint32_t cnt,
                          uint32_t in_len, const Fr* pre3, const Fr* post3, hipStream_t stream, const Fr* scale_tab,
                          uint32_t scale_mode) {
    for (size_t p = 0; p < pl->sched.size(); p++) {
        const NttPass& ps = pl->sched[p];
        PassArgs a = pass_args(pl, p, srcs, dsts, tmps, cnt, in_len, pre3, post3, scale_tab, scale_mode);
        // the last of several passes: the tables built on demand, pinned until the pass has been launched
        NttTablePin scaled_hi, last_tab;
        if (ps.last && p > 0) {
            if (a.post3_uniform && pl->log_n > LO_BITS) {  // iNTT: the divisor rides on the inter-pass twiddles
                scaled_hi = scaled_hi_table(pl, post3[0], stream);
                a.tw_hi = scaled_hi.get();
                a.hi_scaled = 1;
            }
            last_tab = last_table(ctx, pl, ps.B, a.hi_scaled ? &post3[0] : nullptr, stream);
            a.tw_direct = last_tab.get();
        }
        ntt_pass_launch(ctx->device, pass_kernel(ps, a.zskip), a, cnt, ps.shape.threads, stream);
    }
    H2_HIP(hipGetLastError());
}

void ntt_run_many(DeviceCtx* ctx, NttPlan* pl, const Fr* const* srcs, Fr* const* dsts, Fr* const* tmps, size_t count,
                  uint32_t in_len, const Fr* pre3, const Fr* post3, hipStream_t stream, const Fr* scale_tab,
                  uint32_t scale_mode) {
    for (size_t c0 = 0; c0 < count; c0 += NTT_BATCH_MAX) {
        const uint32_t cnt = (uint32_t)std::min<size_t>(NTT_BATCH_MAX, count - c0);
        ntt_run_chunk(ctx, pl, srcs + c0, dsts + c0, tmps + c0, cnt, in_len, pre3, post3, stream, scale_tab, scale_mode);
    }
}

}  // namespace h2
