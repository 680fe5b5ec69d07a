// msm.hip -- the MSM drivers: what a call samples, decides and reads back around the pipeline.
//
// Replaces ec-gpu-gen's `SingleMultiexpKernel::multiexp_bound`; the CPU twin that fixes the semantics is
// `multiexp_serial` (arithmetic.rs:20-108): result = sum_i scalar_i * base_i.  Four files:
//   msm_plan.cpp     every decision, as pure host functions of their arguments and the knobs (MsmKnobs): the shapes, the
//                    shapes a call may end up with (msm_cover), the launch plan and its record
//   msm_kernels.hip  the pipeline's kernels (documented there) and msm_enqueue, which starts one planned launch
//   msm_table.hip    the shifted-base tables: registry, build and check kernels
//   msm.hip          this file: dominant-value detection on the sampled scalars, the plan of a column, the host tail,
//                    h2_dev_msm, the fused groups and the two-stream pipeline of h2_dev_msm_batch(_ex)
// Each public entry point reads the environment once (msm_knobs) and passes the knobs down.
#include <algorithm>
#include <cstring>
#include <memory>
#include <type_traits>
#include <vector>

#include "msm.hpp"
#include "msm_kernels.hpp"
#include "msm_table.hpp"

namespace h2 {

// every shape an MSM of n rows may take over the tables registered now (h2_msm_scratch_bytes)
static size_t scratch_need(size_t n, uint32_t max_bits, const MsmKnobs& knobs) {
    const std::vector<TableDesc> tabs = tables_covering(n);
    return msm_cover(n, max_bits, tabs.data(), tabs.size(), knobs).total;
}
// sized for the larger of the two shapes (with the extra window of a dominant scalar), table forms included
size_t msm_scratch_bytes(size_t n, uint32_t max_bits) { return scratch_need(n, max_bits, msm_knobs()); }
void msm_shape_query(size_t n, uint32_t max_bits, uint32_t* c, uint32_t* windows, uint32_t* buckets_per_window) {
    MsmShape s = msm_shape(n, max_bits, false, 0, msm_knobs());
    if (c) *c = s.c;
    if (windows) *windows = s.W;
    if (buckets_per_window) *buckets_per_window = s.nb;
}

// device memory the MSM keeps for `ctx`'s device: shifted-base tables (all: they are keyed by device address) and the
// device copies of registered host SRS ranges
size_t msm_library_bytes(DeviceCtx* ctx) {
    size_t bytes = table_library_bytes();
    std::lock_guard<std::mutex> g2(ctx->shared->mu);
    for (const auto& kv : ctx->resident) bytes += kv.second.len * sizeof(Affine);
    return bytes;
}

// ---------------------------------------------------------------- dominant-scalar detection
struct Hot {
    bool on = false;
    Fr value{};         // Montgomery form, as stored in the column
    uint32_t live = HOT_SAMPLES;  // sampled rows that will cost digits: neither zero nor (when `on`) the dominant value
    const Affine* block_sums = nullptr;  // sums of the BLOCK_ROWS-row blocks of this MSM's bases, when they are tabulated
};

static Hot detect_hot(const Fr* samples, const MsmKnobs& knobs) {
    Hot h;
    uint32_t best = 0;
    for (uint32_t i = 0; i < HOT_SAMPLES; i++) {
        uint32_t cnt = 0;
        for (uint32_t j = 0; j < HOT_SAMPLES; j++) cnt += fp_eq(samples[i], samples[j]) ? 1u : 0u;
        if (cnt > best && !fp_is_zero(samples[i])) {  // zero scalars are free already
            best = cnt;
            h.value = samples[i];
        }
    }
    h.on = best >= HOT_MIN && !knobs.no_hot;
    h.live = 0;
    for (uint32_t i = 0; i < HOT_SAMPLES; i++)
        if (!fp_is_zero(samples[i]) && !(h.on && fp_eq(samples[i], h.value))) h.live++;
    return h;
}

// ---------------------------------------------------------------- drivers
void msm_identity(uint64_t out_xyz[12]) {
    Jacobian j = xyzz_to_jacobian(xyzz_identity());
    memcpy(out_xyz, &j, 96);
}

// host tail: add the G partials of each window, then Horner over the windows
static void msm_host_tail(const MsmShape& s, const Hot& hot, const std::vector<XYZZ>& winpart, uint64_t out_xyz[12],
                          size_t w0 = 0) {  // w0: first window of the column inside a fused shape
    XYZZ acc = xyzz_identity();
    if (s.tab && s.planes) {
        // the window's sum from its bit planes: qm * sum_p 2^p P_p + (the chunks' own weighted sums)
        const XYZZ* P = winpart.data() + w0 + s.Wt;
        for (int p = (int)s.planes - 2; p >= 0; p--) {
            acc = xyzz_double(acc);
            acc = xyzz_add(acc, P[p]);
        }
        for (uint32_t m = s.qm; m > 1; m >>= 1) acc = xyzz_double(acc);
        acc = xyzz_add(acc, P[s.planes - 1]);
    } else if (s.tab) {
        acc = winpart[w0];  // the digits' weights are in the table's points: one window, no Horner
    }
    for (int w = (int)(s.tab ? 0 : s.W) - 1; w >= 0; w--) {
        const uint32_t cw = s.c - ((uint32_t)w >= s.wfull ? 1u : 0u);  // the windows above w sit 2^cw higher
        for (uint32_t k = 0; k < cw; k++) acc = xyzz_double(acc);
        XYZZ ws = xyzz_identity();
        for (uint32_t r = 0; r < s.R; r++) ws = xyzz_add(ws, winpart[w0 + (size_t)r * s.W + w]);  // the row ranges of window w
        acc = xyzz_add(acc, ws);
    }
    if (hot.on) {  // + v * E, E = the extra window's sum (bucket 0 carries weight 1)
        const XYZZ e = winpart[w0 + (s.tab ? 1u : (size_t)s.R * s.W)];
        const Fr v = fp_from_mont(hot.value);
        XYZZ r = xyzz_identity();
        for (int bit = 253; bit >= 0; bit--) {
            r = xyzz_double(r);
            if ((v.l[bit >> 5] >> (bit & 31)) & 1) r = xyzz_add(r, e);
        }
        acc = xyzz_add(acc, r);
    }
    Jacobian j = xyzz_to_jacobian(acc);
    memcpy(out_xyz, &j, 96);
}

// ---------------------------------------------------------------- the plan of one column
// What is decided for ONE MSM of n rows -- msm_device's only column, each column of msm_device_batch_ex -- in three steps
// around the stream synchronisation both drivers have anyway: plan_find_table (host only), plan_probe (enqueues the
// sampling), [synchronise], plan_decide (host only; leaves `hot`, `use_tab` and `shape` ready for column_launch).
struct ColumnPlan {
    const Fr* scalars = nullptr;
    const uint64_t* bases = nullptr;
    uint32_t bits = 0;             // the column's scalar bound
    bool fused = false;            // batch: already committed in a fused group
    ShiftTable tab{}, found{};     // the table worth using for this bound; the table that contains the bases at all
    bool use_tab = false;          // commit in table form
    bool have_tab = false;         // a table of these bases exists (its block sums serve the windowed form too)
    Hot hot;
    MsmShape shape{};

    bool active() const { return bits != 0 && !fused; }   // bound 0: the identity (arithmetic.rs:346)
    const Affine* points() const { return use_tab ? tab.table : (const Affine*)bases; }
};

// the batch's "column i is on the host" event: one still alive when the driver leaves (an H2_HIP that threw) goes with it
struct EventDestroy {
    void operator()(hipEvent_t e) const { (void)hipEventDestroy(e); }
};
using ColumnEvent = std::unique_ptr<std::remove_pointer_t<hipEvent_t>, EventDestroy>;

static void plan_find_table(ColumnPlan& p, size_t n, const MsmKnobs& knobs) {
    if (!p.bits || !p.bases) return;
    p.have_tab = table_find(p.bases, n, knobs, &p.found);
    p.use_tab = p.have_tab && table_considered(p.found.desc, n, p.bits, knobs);
    if (p.use_tab) p.tab = p.found;
}

// 64 sampled scalars decide whether a dominant value gets its own window; next to them the table's copy of the bases is
// compared with the bases (k_table_check).  h_samples (HOT_SAMPLES values) and h_stale: mapped pinned memory of the caller
static void plan_probe(const ColumnPlan& p, size_t n, Fr* h_samples, uint32_t* h_stale, hipStream_t stream) {
    *h_stale = 0;
    sample_launch(p.scalars, n, h_samples, stream);
    if (p.have_tab && !p.fused) table_check_launch((const Affine*)p.bases, p.found.table, n, h_stale, stream);
}

// after the synchronisation that brought the samples and the flag in
static void plan_decide(ColumnPlan& p, size_t n, const Fr* h_samples, const uint32_t* h_stale, const MsmKnobs& knobs) {
    if (p.have_tab && *h_stale) {  // the bases changed under their table (see k_table_check): windowed form, table dropped
        table_drop_containing(p.bases);
        p.use_tab = p.have_tab = false;
    }
    p.hot = detect_hot(h_samples, knobs);
    // the extra window trades W additions per dominant row for one: with one or two windows there is nothing to gain,
    // only a giant bucket to fold and a 254-bit multiplication on the host
    if (p.hot.on && msm_shape(n, p.bits, false, 0, knobs).W <= 2) p.hot.on = false;
    p.use_tab = p.use_tab && table_pays(p.tab.desc, n, p.bits, p.hot.live, knobs);
    if (p.hot.on && p.have_tab && p.found.blocks && (p.use_tab ? (size_t)p.tab.desc.D * p.tab.desc.n : n) < BLOCK_INDEX0)
        p.hot.block_sums = p.found.blocks;
    p.shape = p.use_tab ? msm_shape_table(n, p.bits, p.hot.on, p.tab.desc, knobs) : msm_shape(n, p.bits, p.hot.on, 0, knobs);
}

// a decided column's kernels and the read-back of its window sums into h_win (mapped pinned memory), on one stream
static void column_launch(const ColumnPlan& p, char* scratch, XYZZ* h_win, hipStream_t stream, const MsmKnobs& knobs) {
    const MsmLaunchPlan lp = msm_plan_launch(p.shape, p.bits, p.hot.on, p.hot.block_sums != nullptr, false, 0, knobs);
    msm_enqueue(p.shape, lp, p.scalars, p.hot.value, p.points(), p.hot.block_sums, scratch, stream);
    export_to_host((const XYZZ*)(scratch + p.shape.off_winpart), h_win, exported_points(p.shape), stream);
}
// ... and, once they are in, the column's result
static void column_tail(const ColumnPlan& p, const XYZZ* h_win, uint64_t* out_xyz) {
    std::vector<XYZZ> winpart(h_win, h_win + exported_points(p.shape));
    msm_host_tail(p.shape, p.hot, winpart, out_xyz);
}

static bool entries_fit(size_t n, uint32_t max_bits, const MsmKnobs& knobs) {
    if (n > 0x7fffffffu || msm_cover(n, max_bits, nullptr, 0, knobs).entries >= ((size_t)1 << 32)) {
        set_last_error("h2 msm: n * windows must be < 2^32 (sorted entries are indexed with 32 bits): split the MSM");
        return false;
    }
    return true;
}

int msm_device(DeviceCtx* ctx, const Fr* d_scalars, const uint64_t* d_bases, size_t n, uint32_t max_bits,
               void* d_scratch, size_t scratch_bytes, uint64_t* out_xyz, hipStream_t stream) {
    LaunchScope records;
    if (n == 0 || max_bits == 0) {
        msm_identity(out_xyz);
        return H2_OK;
    }
    const MsmKnobs knobs = msm_knobs();
    if (!entries_fit(n, max_bits, knobs)) return H2_ERR_INVALID;
    ColumnPlan p{d_scalars, d_bases, max_bits};
    plan_find_table(p, n, knobs);
    const size_t need = scratch_need(n, max_bits, knobs);
    if (!d_scratch || scratch_bytes < need) {
        set_last_error("h2 msm: scratch too small (see h2_msm_scratch_bytes)");
        return H2_ERR_INVALID;
    }
    static thread_local PinnedBuf staging;  // per calling thread: this entry point takes no context lock
    Fr* h_samples = (Fr*)staging.get((HOT_SAMPLES + 1) * sizeof(Fr));
    uint32_t* h_stale = (uint32_t*)(h_samples + HOT_SAMPLES);
    plan_probe(p, n, h_samples, h_stale, stream);
    H2_HIP(hipStreamSynchronize(stream));
    plan_decide(p, n, h_samples, h_stale, knobs);
    if (p.shape.total > need) {   // (cannot happen: `need` covers every shape plan_decide chooses from; never run past the buffer)
        set_last_error("h2 msm: internal: the chosen shape needs more scratch than h2_msm_scratch_bytes reported");
        return H2_ERR_INVALID;
    }
    XYZZ* h_win = (XYZZ*)staging.get(exported_points(p.shape) * sizeof(XYZZ));
    column_launch(p, (char*)d_scratch, h_win, stream, knobs);
    H2_HIP(hipStreamSynchronize(stream));
    column_tail(p, h_win, out_xyz);
    return H2_OK;
}

// `cols` MSMs over the SAME bases and with the same scalar bound as ONE pass of the pipeline: column j's windows are
// windows j * (W + 1) ... of a single wide MSM (k_digits reads each column's scalars, everything after it only sees
// more windows), so the fixed costs -- sampling, sort launches, the latency-bound finish / reduce, the synchronisation
// and the read-back -- are paid once for the group instead of once per column.  This is what a witness with many
// narrow columns needs: at 2^18 a single MSM is ~1 ms of mostly fixed latency.
static int msm_device_fused(DeviceCtx* ctx, const Fr* const* d_scalars, uint32_t cols, const uint64_t* d_bases, size_t n,
                            uint32_t bits, char* scratch, uint64_t* const* outs, hipStream_t stream, const MsmKnobs& knobs) {
    LaunchScope records;
    const MsmShape s = msm_shape(n, bits, false, cols, knobs);
    const size_t wp = exported_points(s);
    // the column table (cols pointers, padded to 16 bytes, then cols dominant values) is staged in pinned memory too
    const size_t tab_ptr_bytes = ((size_t)cols * 8 + 15) & ~(size_t)15, tab_bytes = tab_ptr_bytes + (size_t)cols * sizeof(Fr);
    char* pinned = (char*)ctx->pinned.get((size_t)cols * HOT_SAMPLES * sizeof(Fr) + wp * sizeof(XYZZ) + tab_bytes);
    Fr* h_samples = (Fr*)pinned;
    XYZZ* h_win = (XYZZ*)(pinned + (size_t)cols * HOT_SAMPLES * sizeof(Fr));
    char* h_tab = pinned + (size_t)cols * HOT_SAMPLES * sizeof(Fr) + wp * sizeof(XYZZ);
    for (uint32_t j = 0; j < cols; j++) sample_launch(d_scalars[j], n, h_samples + (size_t)j * HOT_SAMPLES, stream);
    H2_HIP(hipStreamSynchronize(stream));
    std::vector<Hot> hots(cols);
    FusedCols fc{};
    memset(h_tab, 0, tab_bytes);
    for (uint32_t j = 0; j < cols; j++) {
        hots[j] = detect_hot(h_samples + (size_t)j * HOT_SAMPLES, knobs);
        if (s.Wc == s.W) hots[j].on = false;  // one or two windows: no dominant-scalar slot
        if (hots[j].on) fc.hot_mask |= 1ull << j;
        ((uint64_t*)h_tab)[j] = (uint64_t)(uintptr_t)d_scalars[j];
        ((Fr*)(h_tab + tab_ptr_bytes))[j] = hots[j].value;
    }
    // ... and goes up through the store kernel, not hipMemcpyAsync: a DMA-engine copy queues behind the bulk transfers in
    // flight (see k_export) -- the first group of a wide witness waited here until the LAST column had crossed PCIe
    // (k = 22, 64 compact columns: 34 ms of a 124 ms advice phase; tools/experiments/busy.sh showed the GPU idle)
    char* d_tab = scratch + s.off_coltab;
    copy16_launch(h_tab, d_tab, tab_bytes / 16, stream);
    fc.scalars = (const Fr* const*)d_tab;
    fc.hot_values = (const Fr*)(d_tab + tab_ptr_bytes);
    const MsmLaunchPlan lp = msm_plan_launch(s, bits, false, false, true, fc.hot_mask, knobs);
    msm_enqueue(s, lp, nullptr, Fr{}, (const Affine*)d_bases, nullptr, scratch, stream, &fc);
    export_to_host((const XYZZ*)(scratch + s.off_winpart), h_win, wp, stream);
    H2_HIP(hipStreamSynchronize(stream));  // (the pinned block is this context's until here)
    std::vector<XYZZ> winpart(h_win, h_win + wp);
    for (uint32_t j = 0; j < cols; j++) msm_host_tail(s, hots[j], winpart, outs[j], (size_t)j * s.Wc);
    return H2_OK;
}

// Batch of MSMs over ONE set of bases (the prover commits every advice / fixed / z column against the
// same g_lagrange: plonk/prover.rs:293-299, :477-487, keygen.rs:288-291).  Consecutive MSMs alternate
// between two streams with their own scratch halves, so the latency-bound tail of one MSM (k_finish,
// k_reduce: about one wave per SIMD) overlaps the ALU-bound hot loop of the next, and the host-side
// window combine of MSM i runs while the GPU works on i+1, i+2.
int msm_device_batch(DeviceCtx* ctx, const Fr* const* d_scalars, size_t count, const uint64_t* d_bases, size_t n,
                     uint32_t max_bits, void* d_scratch, size_t scratch_bytes, uint64_t* out_xyz, hipStream_t stream) {
    return msm_device_batch_ex(ctx, d_scalars, nullptr, nullptr, count, d_bases, n, max_bits, d_scratch, scratch_bytes,
                               out_xyz, stream);
}

// bases_each / bits_each (either may be null): per-column base table and scalar bound -- the prover's batches mix
// g_lagrange with g (the vanishing argument's random polynomial) and 16-bit witness columns with full-width ones
int msm_device_batch_ex(DeviceCtx* ctx, const Fr* const* d_scalars, const uint64_t* const* bases_each,
                        const uint32_t* bits_each, size_t count, const uint64_t* d_bases, size_t n, uint32_t max_bits,
                        void* d_scratch, size_t scratch_bytes, uint64_t* out_xyz, hipStream_t stream) {
    LaunchScope records;
    if (count == 0) return H2_OK;
    const MsmKnobs knobs = msm_knobs();
    std::vector<ColumnPlan> plans(count);
    uint32_t top_bits = 0;
    for (size_t i = 0; i < count; i++) {
        const uint64_t* bases = bases_each && bases_each[i] ? bases_each[i] : d_bases;
        plans[i] = ColumnPlan{d_scalars[i], bases, bits_each ? bits_each[i] : max_bits};
        top_bits = std::max(top_bits, plans[i].bits);
    }
    if (!entries_fit(n, top_bits, knobs)) return H2_ERR_INVALID;  // (no bound at all: one window, 2 n entries, so n alone decides)
    if (n == 0 || top_bits == 0) {
        for (size_t i = 0; i < count; i++) msm_identity(out_xyz + 12 * i);
        return H2_OK;
    }
    // columns that share their base table and their bound are committed as fused groups when the caller's scratch
    // allows it (h2_msm_batch_scratch_bytes); the rest goes through the two-stream pipeline below
    // columns whose bases have a shifted-base table go through the pipeline in table form
    for (ColumnPlan& p : plans) plan_find_table(p, n, knobs);
    if (!knobs.no_fuse) {
        H2_HIP(hipStreamSynchronize(stream));
        for (size_t i = 0; i < count; i++) {
            const ColumnPlan& first = plans[i];
            if (first.fused || first.use_tab || first.bits == 0) continue;
            std::vector<size_t> members{i};
            for (size_t j = i + 1; j < count; j++)
                if (!plans[j].fused && !plans[j].use_tab && plans[j].bits == first.bits && plans[j].bases == first.bases)
                    members.push_back(j);
            const uint32_t limit = fused_group_limit(n, first.bits, knobs);
            for (size_t m0 = 0; m0 < members.size(); m0 += limit) {
                const uint32_t g = (uint32_t)std::min<size_t>(limit, members.size() - m0);
                if (g < 2) break;
                if (msm_shape(n, first.bits, false, g, knobs).total > scratch_bytes) break;  // caller sized the scratch for the pipeline only
                std::vector<const Fr*> sc(g);
                std::vector<uint64_t*> outs(g);
                for (uint32_t t = 0; t < g; t++) {
                    sc[t] = d_scalars[members[m0 + t]];
                    outs[t] = out_xyz + 12 * members[m0 + t];
                    plans[members[m0 + t]].fused = true;
                }
                int rc = msm_device_fused(ctx, sc.data(), g, first.bases, n, first.bits, (char*)d_scratch, outs.data(), stream, knobs);
                if (rc != H2_OK) return rc;
            }
        }
    }
    // a lane's scratch and a column's read-back are sized before the samples are in: for every shape the column may be
    // given (msm_cover: windowed and, where a table may be used, the table form, without and with a dominant scalar)
    // (plan_decide computes the one shape it chooses again: which one that is depends on the samples)
    size_t per = 0, wp_max = 0;
    for (const ColumnPlan& p : plans) {
        if (p.fused) continue;
        const MsmCover c = msm_cover(n, p.bits ? p.bits : 1, &p.tab.desc, p.use_tab ? 1 : 0, knobs);
        per = std::max(per, align_up(c.total, 256));
        wp_max = std::max(wp_max, c.exported);
    }
    if (!d_scratch || scratch_bytes < 2 * per) {
        set_last_error("h2 msm batch: scratch too small (need 2 x h2_msm_scratch_bytes of the widest column, 256-byte aligned)");
        return H2_ERR_INVALID;
    }
    // pinned staging: the sampled scalars of every column, then the per-MSM window partials (async read-back)
    char* pinned = (char*)ctx->pinned.get(count * (HOT_SAMPLES * sizeof(Fr) + wp_max * sizeof(XYZZ) + 16));
    Fr* h_samples = (Fr*)pinned;
    XYZZ* h_win = (XYZZ*)(pinned + count * HOT_SAMPLES * sizeof(Fr));
    uint32_t* h_stale = (uint32_t*)(pinned + count * (HOT_SAMPLES * sizeof(Fr) + wp_max * sizeof(XYZZ)));  // per column
    // pipeline lanes: one stream + one scratch slice each.  Two: a third and fourth lane (H2_MSM_LANES, when the scratch
    // holds them) were measured and do not pay -- 2^18: 0.78 (2) / 0.76 (3) / 0.84 (4) ms per MSM, 2^20: 2.06 / 2.08 / 2.17
    hipStream_t st[4] = {ctx->stream, ctx->copy_stream, ctx->aux_stream[0], ctx->aux_stream[1]};
    size_t lanes = knobs.lanes;
    if (!per || lanes * per > scratch_bytes) lanes = 2;
    // (every column is sampled, the fused and the empty ones too; only the pipeline's columns are decided and launched)
    for (size_t i = 0; i < count; i++) plan_probe(plans[i], n, h_samples + i * HOT_SAMPLES, h_stale + i, stream);
    H2_HIP(hipStreamSynchronize(stream));  // inputs produced on the caller's stream are complete; samples are in
    for (size_t i = 0; i < count; i++)
        if (plans[i].active()) plan_decide(plans[i], n, h_samples + i * HOT_SAMPLES, h_stale + i, knobs);
    std::vector<ColumnEvent> done(count);
    size_t lane_of = 0;
    for (size_t i = 0; i < count; i++) {
        const ColumnPlan& p = plans[i];
        if (!p.active()) continue;
        char* scratch = (char*)d_scratch + (lane_of % lanes) * per;
        hipStream_t q = st[lane_of % lanes];
        lane_of++;
        column_launch(p, scratch, h_win + i * wp_max, q, knobs);
        hipEvent_t e = nullptr;
        H2_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        done[i].reset(e);
        H2_HIP(hipEventRecord(e, q));
    }
    for (size_t i = 0; i < count; i++) {
        const ColumnPlan& p = plans[i];
        if (p.fused) continue;
        if (!done[i]) {
            msm_identity(out_xyz + 12 * i);
            continue;
        }
        H2_HIP(hipEventSynchronize(done[i].get()));
        H2_HIP(hipEventDestroy(done[i].release()));
        column_tail(p, h_win + i * wp_max, out_xyz + 12 * i);
    }
    return H2_OK;
}

// scratch that lets h2_dev_msm_batch(_ex) fuse `count` columns of bound `max_bits` over one base table
size_t msm_batch_scratch_bytes(size_t n, uint32_t max_bits, size_t count) {
    const MsmKnobs knobs = msm_knobs();
    return msm_batch_need(n, max_bits, count, scratch_need(n, max_bits, knobs), knobs);
}

}  // namespace h2
