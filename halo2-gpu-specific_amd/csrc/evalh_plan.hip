// evalh_plan.hip -- evaluate_h as kernels GENERATED for one program (evalh_gen.cpp: straight-line code, intermediates in
// registers, all terms in one or a few launches): the plans per (program, device) -- built by hipRTC on first use, loaded,
// cached with a bound, unloaded when evicted -- the argument block a stage receives for a descriptor, and the launcher.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstring>
#include <map>
#include <memory>
#include <set>
#include <stdexcept>
#include <vector>

#include "common.hpp"
#include "evalh.hpp"
#include "evalh_desc.hpp"
#include "evalh_gen.hpp"
#include "ntt.hpp"


namespace h2 {
// ---------------------------------------------------------------- generated kernels: plans per (program, device)
struct EvalhPlan {
    evgen::Generated gen;               // stage metadata (sources and code objects dropped after loading)
    std::vector<hipModule_t> modules;
    std::vector<hipFunction_t> functions;
    int device = -1;
    bool uses_omega = false;
    int from_cache = 0;                 // 0 compiled now, 2 from the disk cache (1 = memory is decided by the caller)
    mutable uint64_t last_use = 0;      // g_plan_mu: the cache's clock at the last lookup
    mutable uint32_t users = 0;         // g_plan_mu: EvalhPlanRef holders -- a held plan is never evicted
};

namespace {
struct PlanKey {
    uint64_t h[2];
    int device;
    bool operator<(const PlanKey& o) const {
        if (h[0] != o.h[0]) return h[0] < o.h[0];
        if (h[1] != o.h[1]) return h[1] < o.h[1];
        return device < o.device;
    }
};
std::mutex g_plan_mu;
std::map<PlanKey, std::unique_ptr<EvalhPlan>> g_plans;   // a null entry: generation failed for this program (said once)
// programs some caller is generating / compiling / loading right now, OUTSIDE g_plan_mu (a hipRTC build takes seconds): callers
// of the SAME program wait on the condition variable instead of compiling it again; lookups of every other program -- cache
// hits included, on any device or host-API slot -- go on meanwhile
std::set<PlanKey> g_building;
std::condition_variable g_plan_cv;
std::map<PlanKey, std::chrono::steady_clock::time_point> g_failed_at;   // when a null entry was made: retried after a minute
std::map<PlanKey, std::string> g_failed_why;                              // ... and what the generator or the compiler said
constexpr int FAILED_RETRY_SECONDS = 60;
std::atomic<uint64_t> g_generated_launches{0};
std::atomic<uint64_t> g_plan_evictions{0};
uint64_t g_plan_clock = 0;                               // g_plan_mu

size_t plans_max() {
    static const size_t v = [] {
        const char* e = getenv("H2_EVALH_PLANS_MAX");
        const long n = e ? atol(e) : 0;
        return (size_t)(n > 0 ? n : 128);
    }();
    return v;
}

// g_plan_mu held.  UNHOOKS least-recently-used plans nobody holds until the cache is back at its bound and hands them to the
// caller, who unloads them with `unload_plans` AFTER releasing the lock: a plan's device is drained first (its launches are
// asynchronous and the code object has to outlive them), and that wait must not stall every other lookup.
void evict_plans(const PlanKey& keep, std::vector<std::unique_ptr<EvalhPlan>>& gone) {
    while (g_plans.size() > plans_max()) {
        auto victim = g_plans.end();
        for (auto it = g_plans.begin(); it != g_plans.end(); ++it) {
            if (!(it->first < keep) && !(keep < it->first)) continue;
            if (it->second && it->second->users) continue;
            const uint64_t t = it->second ? it->second->last_use : 0;   // (failed generations first: they hold nothing)
            if (victim == g_plans.end() || t < (victim->second ? victim->second->last_use : 0)) victim = it;
        }
        if (victim == g_plans.end()) return;   // everything else is in use: over the bound until a holder lets go
        if (victim->second) gone.push_back(std::move(victim->second));
        g_failed_at.erase(victim->first);
        g_failed_why.erase(victim->first);
        g_plans.erase(victim);
        g_plan_evictions.fetch_add(1);
    }
}
// no lock held: nobody can reach these plans any more
void unload_plans(std::vector<std::unique_ptr<EvalhPlan>>& gone) {
    for (auto& pl : gone) {
        int current = 0;
        const bool have = hipGetDevice(&current) == hipSuccess;
        if (hipSetDevice(pl->device) == hipSuccess) {
            (void)hipDeviceSynchronize();
            for (hipModule_t m : pl->modules) (void)hipModuleUnload(m);
        }
        if (have) (void)hipSetDevice(current);
    }
    gone.clear();
}

// in-memory identity of a program: two multiply-xorshift lanes over the same bytes program_hash covers (the SHA-256 is
// for the file name on disk, where a collision would load foreign code; here it would at worst pick the wrong cached plan
// of THIS process's own programs, at 2^-128)
struct FastHash {
    uint64_t a = 0x9e3779b97f4a7c15ull, b = 0xc2b2ae3d27d4eb4full;
    void word(uint64_t w) {
        a = (a ^ w) * 0xff51afd7ed558ccdull;
        a ^= a >> 32;
        b = (b + w) * 0x9fb21c651e98df25ull;
        b ^= b >> 29;
    }
    void bytes(const void* p, size_t n) {
        const uint8_t* q = (const uint8_t*)p;
        word(n);
        for (; n >= 8; n -= 8, q += 8) {
            uint64_t w;
            memcpy(&w, q, 8);
            word(w);
        }
        uint64_t w = 0;
        memcpy(&w, q, n);
        word(w);
    }
};

PlanKey plan_key(const h2_evalh_desc* d, const evgen::Options& opt, int device) {
    FastHash h;
    const uint32_t o[] = {opt.group, opt.max_ahead, opt.gap, opt.inline_muls, opt.stage_products, opt.max_regs,
                          (uint32_t)opt.factor, opt.waves, opt.live_budget, opt.lds_args, (uint32_t)opt.mul2, opt.min_group, d->blinding_factors, d->chunk_len, d->n_fixed, d->n_advice,
                          d->n_instance, d->n_perm_sets, d->n_perm_columns, d->n_lookups, d->n_shuffles};
    h.bytes(o, sizeof o);
    h.bytes(d->constants, (size_t)d->n_constants * 32);
    h.bytes(d->rotations, (size_t)d->n_rotations * 4);
    h.bytes(d->calculations, (size_t)d->n_calculations * sizeof(h2_calculation));
    h.bytes(d->value_parts, (size_t)d->n_value_parts * sizeof(h2_value_source));
    h.bytes(d->lookup_sets, (size_t)d->n_lookups * 4);
    h.bytes(d->lookup_calcs, evalh_lookup_calc_count(d) * sizeof(h2_calculation));
    h.bytes(d->shuffle_calcs, 2 * (size_t)d->n_shuffles * sizeof(h2_calculation));
    if (d->n_perm_sets) {
        h.bytes(d->perm_col_type, (size_t)d->n_perm_columns * 4);
        h.bytes(d->perm_col_index, (size_t)d->n_perm_columns * 4);
    }
    return PlanKey{{h.a, h.b}, device};
}

bool generation_enabled() {
    const char* v = getenv("H2_EVALH_JIT");
    return !(v && v[0] == '0');
}
}  // namespace

void evalh_plan_release(const EvalhPlan* plan) {
    std::lock_guard<std::mutex> g(g_plan_mu);
    if (plan->users) plan->users--;
}

uint64_t evalh_plan_evictions() { return g_plan_evictions.load(); }

EvalhPlanRef evalh_plan_get(const h2_evalh_desc* d, int* cached, std::string* why) {
    if (cached) *cached = 0;
    if (!generation_enabled()) return EvalhPlanRef();
    int device = 0;
    H2_HIP(hipGetDevice(&device));
    const evgen::Options opt = evgen::Options::from_env();
    const PlanKey key = plan_key(d, opt, device);
    // one builder per PROGRAM: two callers with the same new program would otherwise both compile it.  The build itself runs
    // without the lock.
    std::unique_lock<std::mutex> g(g_plan_mu);
    for (;;) {
        auto it = g_plans.find(key);
        if (it != g_plans.end()) {
            if (!it->second) {
                // a failed generation is not for ever: a transient failure (a full disk, a compiler that was being replaced)
                // is tried again after a minute
                auto f = g_failed_at.find(key);
                if (f != g_failed_at.end() && std::chrono::steady_clock::now() - f->second > std::chrono::seconds(FAILED_RETRY_SECONDS)) {
                    g_failed_at.erase(f);
                    g_failed_why.erase(key);
                    g_plans.erase(it);
                    continue;
                }
                if (why) *why = g_failed_why[key];
            }
            if (cached) *cached = 1;
            if (const EvalhPlan* hit = it->second.get()) {
                hit->last_use = ++g_plan_clock;
                hit->users++;
            }
            return EvalhPlanRef(it->second.get());
        }
        if (!g_building.count(key)) break;
        g_plan_cv.wait(g);
    }
    g_building.insert(key);
    g.unlock();
    struct Done {   // whatever happens below, the waiters of this program are released
        const PlanKey& key;
        std::unique_lock<std::mutex>& g;
        ~Done() {
            if (!g.owns_lock()) g.lock();
            g_building.erase(key);
            g_plan_cv.notify_all();
        }
    } done{key, g};
    std::unique_ptr<EvalhPlan> plan;
    std::string failure;
    try {
        plan.reset(new EvalhPlan);
        plan->gen = evgen::compile(d, opt);
        plan->device = device;
        plan->from_cache = plan->gen.from_disk ? 2 : 0;
        for (evgen::Stage& st : plan->gen.stages) {
            hipModule_t mod = nullptr;
            H2_HIP(hipModuleLoadData(&mod, st.code.data()));
            plan->modules.push_back(mod);
            hipFunction_t fn = nullptr;
            H2_HIP(hipModuleGetFunction(&fn, mod, evgen::KERNEL_NAME));
            plan->functions.push_back(fn);
            plan->uses_omega = plan->uses_omega || st.uses_omega;
            // (st.code stays for the life of the plan: hipModuleLoadData does not copy the image -- freeing it here ended in
            //  memory faults at the first launch)
            std::string().swap(st.source);
        }
        if (cached) *cached = plan->from_cache;
    } catch (const std::exception& e) {
        fprintf(stderr, "libhalo2_hip: evaluate_h runs on the interpreter kernels for this program: %s\n", e.what());
        failure = e.what();
        plan.reset();
    } catch (const HipError& e) {
        fprintf(stderr, "libhalo2_hip: evaluate_h runs on the interpreter kernels for this program: HIP error %d loading the generated code (%s)\n",
                (int)e.code, e.expr);
        failure = std::string("HIP error loading the generated code (") + e.expr + ")";
        plan.reset();
    }
    g.lock();
    const EvalhPlan* out = plan.get();
    if (out) {
        out->last_use = ++g_plan_clock;
        out->users = 1;
    } else {
        g_failed_at[key] = std::chrono::steady_clock::now();
        g_failed_why[key] = failure;
        if (why) *why = failure;
    }
    g_plans[key] = std::move(plan);
    std::vector<std::unique_ptr<EvalhPlan>> gone;
    evict_plans(key, gone);
    if (!gone.empty()) {
        g.unlock();
        unload_plans(gone);
    }
    return EvalhPlanRef(out);
}

void evalh_plan_info(const EvalhPlan* plan, h2_evalh_info* info) {
    if (!info) return;
    memset(info, 0, sizeof *info);
    if (!plan) return;
    evalh_gen_info(plan->gen, info);
}

void evalh_gen_info(const evgen::Generated& g, h2_evalh_info* info) {
    memset(info, 0, sizeof *info);
    info->stages = (uint32_t)g.stages.size();
    info->terms = g.terms;
    info->products_per_row = g.products_per_row;
    info->fused_pairs_per_row = g.fused_pairs_per_row;
    info->reference_products_per_row = g.reference_products_per_row;
    info->vectors_read = g.vectors_read;
    for (const evgen::Stage& st : g.stages) {
        info->max_registers = std::max(info->max_registers, st.vgprs + st.agprs);
        info->scratch_bytes = std::max(info->scratch_bytes, st.scratch);
    }
    info->from_cache = g.from_disk ? 2 : 0;
}

uint64_t evalh_generated_launches() { return g_generated_launches.load(); }

// The argument block of one generated stage (evalh_gen.hpp: fixed part, uniform scalars, column pointers) for descriptor `d`:
// what the kernel receives by value.  Host arithmetic only -- also behind h2_evalh_stage_args, through which the CPU tests run
// the generated source (compiled for the host) against the oracle.  Returns the block's size; throws on a program / descriptor
// mismatch.
size_t evalh_fill_stage_args(const evgen::Stage& st, const h2_evalh_desc* d, Fr* values, const Fr* tw_lo, const Fr* tw_hi,
                             size_t row_begin, size_t row_end, unsigned char* buf, size_t cap) {
    const Fr y = fr_from_u64x4(d->y), beta = fr_from_u64x4(d->beta), gamma = fr_from_u64x4(d->gamma), theta = fr_from_u64x4(d->theta);
    const Fr delta = fr_from_u64x4(d->delta), delta_start = fp_mul(beta, fr_from_u64x4(d->zeta));  // evaluation.rs:1012
    const size_t ns = std::max<size_t>(st.scalars.size(), 1), nc = std::max<size_t>(st.cols.size(), 1);
    const size_t bytes = evgen::ARGS_FIXED_BYTES + 32 * ns + 8 * nc;
    if (bytes > cap) throw std::runtime_error("h2_evaluate_h: generated stage with oversized arguments");
    memset(buf, 0, bytes);
    struct Fixed {
        Fr* values;
        const Fr* tw_lo;
        const Fr* tw_hi;
        unsigned long long row_begin, row_end;
        unsigned int extended_k, rot_scale;
    } fx{values, tw_lo, tw_hi, (unsigned long long)row_begin, (unsigned long long)row_end, d->extended_k, 1u << (d->extended_k - d->k)};
    static_assert(sizeof(Fixed) == evgen::ARGS_FIXED_BYTES, "argument layout");
    memcpy(buf, &fx, sizeof fx);
    Fr* sc = (Fr*)(buf + evgen::ARGS_FIXED_BYTES);
    std::vector<Fr> delta_pow;  // DELTA^j, grown on demand
    for (size_t i = 0; i < st.scalars.size(); i++) {
        const evgen::ScalarRef& r = st.scalars[i];
        switch (r.kind) {
            case evgen::SC_ONE: sc[i] = fp_one<FrParams>(); break;
            case evgen::SC_CONST: sc[i] = fr_from_u64x4(d->constants + 4 * (size_t)r.arg); break;
            case evgen::SC_Y_POW: sc[i] = fp_pow_u32(y, r.arg); break;
            case evgen::SC_BETA_POW: sc[i] = fp_pow_u32(beta, r.arg); break;
            case evgen::SC_GAMMA_POW: sc[i] = fp_pow_u32(gamma, r.arg); break;
            case evgen::SC_THETA: sc[i] = theta; break;
            default: {  // SC_DELTA_TERM: beta ZETA DELTA^arg
                if (delta_pow.empty()) delta_pow.push_back(fp_one<FrParams>());
                while (delta_pow.size() <= r.arg) delta_pow.push_back(fp_mul(delta_pow.back(), delta));
                sc[i] = fp_mul(delta_start, delta_pow[r.arg]);
            }
        }
    }
    const void** cols = (const void**)(buf + evgen::ARGS_FIXED_BYTES + 32 * ns);
    for (size_t i = 0; i < st.cols.size(); i++) {
        const evgen::ColRef& c = st.cols[i];
        const void* p = evalh_column(d, c.table, c.index);
        if (!p) throw std::runtime_error("h2_evaluate_h: a column the program reads has a null pointer in the descriptor");
        cols[i] = p;
    }
    return bytes;
}

// Fills each stage's argument block and launches it.
void evalh_plan_launch(DeviceCtx* ctx, const EvalhPlan* plan, const h2_evalh_desc* d, Fr* d_values, size_t row_begin, size_t row_end,
                       hipStream_t stream) {
    PlanRef pl;  // the power tables of extended_omega: pinned until the kernels that read them are launched
    if (plan->uses_omega) pl = ntt_get_plan(ctx, d->extended_k, d->extended_omega, stream);
    const Fr *tw_lo = plan->uses_omega ? pl->tw_lo : nullptr, *tw_hi = plan->uses_omega ? pl->tw_hi : nullptr;
    const size_t rows = row_end - row_begin;
    const unsigned blocks = (unsigned)std::min<size_t>((rows + 255) / 256, 0x7fffffffu);
    for (size_t s = 0; s < plan->gen.stages.size(); s++) {
        const evgen::Stage& st = plan->gen.stages[s];
        alignas(16) unsigned char buf[evgen::ARGS_MAX_BYTES];
        const size_t bytes = evalh_fill_stage_args(st, d, d_values, tw_lo, tw_hi, row_begin, row_end, buf, sizeof buf);
        static const bool debug = getenv("H2_JIT_DEBUG") != nullptr;
        if (debug)
            fprintf(stderr, "h2_evalh_gen stage %zu: %u blocks, rows [%zu, %zu), %zu scalars, %zu columns, %zu argument bytes, values %p\n", s,
                    blocks, row_begin, row_end, st.scalars.size(), st.cols.size(), bytes, (void*)d_values);
        if (getenv("H2_JIT_LAUNCH_EXTRA")) {
            size_t arg_bytes = (bytes + 15) & ~(size_t)15;
            void* config[] = {HIP_LAUNCH_PARAM_BUFFER_POINTER, buf, HIP_LAUNCH_PARAM_BUFFER_SIZE, &arg_bytes, HIP_LAUNCH_PARAM_END};
            H2_HIP(hipModuleLaunchKernel(plan->functions[s], blocks, 1, 1, 256, 1, 1, 0, stream, nullptr, config));
        } else {
            void* kargs[] = {buf};  // the kernel's one parameter: the argument block by value (copied at the call)
            H2_HIP(hipModuleLaunchKernel(plan->functions[s], blocks, 1, 1, 256, 1, 1, 0, stream, kargs, nullptr));
        }
        if (debug) H2_HIP(hipStreamSynchronize(stream));
        g_generated_launches.fetch_add(1);
    }
}

}  // namespace h2
