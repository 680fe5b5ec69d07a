// msm_plan.cpp -- the MSM plan (msm_plan.hpp): plain host C++, no HIP.
#include "msm_plan.hpp"

#include <algorithm>
#include <cstdlib>
#include <utility>

namespace h2 {

MsmKnobs msm_knobs() {
    // an integer knob: `fallback` when it is unset or outside [lo, hi]
    auto env_int = [](const char* name, int lo, int hi, int fallback) {
        const char* env = getenv(name);
        const int v = env ? atoi(env) : fallback;
        return (env && v >= lo && v <= hi) ? v : fallback;
    };
    auto env_is_one = [](const char* name) {  // on when the first character is '1'
        const char* env = getenv(name);
        return env && env[0] == '1';
    };
    auto env_not_zero = [](const char* name) {  // off only when set and atoi == 0
        const char* env = getenv(name);
        return !(env && atoi(env) == 0);
    };
    MsmKnobs k;
    k.slice_log = (uint32_t)env_int("H2_MSM_SLICE_LOG", 1, 10, 0);
    k.window = (uint32_t)env_int("H2_MSM_WINDOW", 2, 18, 0);
    k.reduce_qm = (uint32_t)env_int("H2_MSM_REDUCE_QM", 1, 64, 0);
    k.table_lo = (uint32_t)env_int("H2_MSM_TABLE_LO", 4, 12, 0);
    const char* fuse_log = getenv("H2_MSM_FUSE_LOG");
    k.fuse_log_present = fuse_log != nullptr;
    if (fuse_log && atoi(fuse_log) >= 10 && atoi(fuse_log) <= 28) k.fuse_log = (uint32_t)atoi(fuse_log);
    k.lanes = (uint32_t)env_int("H2_MSM_LANES", 2, 4, 2);
    k.no_table = env_is_one("H2_MSM_NO_TABLE");
    k.no_hot = env_is_one("H2_MSM_NO_HOT");
    k.no_fuse = getenv("H2_MSM_NO_FUSE") != nullptr;
    k.table_force = getenv("H2_MSM_TABLE_FORCE") != nullptr;
    if (const char* env = getenv("H2_MSM_TABLE_MIN_N")) k.table_min_n = (size_t)atoll(env);
    k.table_digits = (uint32_t)env_int("H2_MSM_TABLE_DIGITS", (int)TABLE_MIN_D, (int)TABLE_MAX_D, 0);
    if (const char* env = getenv("H2_MSM_REDUCE_WGS")) k.reduce_wgs = (size_t)std::max(1, atoi(env));
    if (const char* env = getenv("H2_MSM_PLANE_WGS")) k.plane_wgs = (uint32_t)std::max(1, atoi(env));
    k.reduce_planes = env_not_zero("H2_MSM_REDUCE_PLANES");
    k.two_level = env_not_zero("H2_MSM_TWO_LEVEL");
    k.sort_stage = env_not_zero("H2_MSM_SORT_STAGE");
    if (const char* env = getenv("H2_MSM_TWO_LEVEL_MIN_HI")) k.two_level_min_hi = (uint32_t)atoi(env);
    if (const char* env = getenv("H2_MSM_ACC_WAVES")) k.acc_waves = atoi(env) == 5 ? 5u : 4u;
    if (const char* env = getenv("H2_MSM_FINISH_LANE_LOG")) k.finish_lane_from = 1u << atoi(env);
    return k;
}

DigitCut balanced_cut(uint32_t T, uint32_t W) {
    const uint32_t base = T / W, rem = T % W;
    return {rem ? base + 1 : base, rem ? rem : W};
}

TableDesc table_desc(size_t n, uint32_t digits) {
    const DigitCut cut = balanced_cut(255, digits);
    return {n, digits, cut.c, cut.wfull};
}

// slice length: aim at >= 2^18 slices (one resident round of the chip at 4 waves/SIMD), 8 <= S <= 64
uint32_t slice_log(size_t entries, size_t per_bucket, const MsmKnobs& k) {
    uint32_t log_s = 6;
    while (log_s > 3 && (entries >> log_s) < (1u << 18)) log_s--;
    // large MSMs: keep the partials per bucket low (k_finish folds <= FINISH_SERIAL of them per thread, more go through
    // the heavy-bucket path) by lengthening the slices while at least 2^20 of them remain
    while (log_s < 10 && (entries >> (log_s + 1)) >= (1u << 20) && (per_bucket >> log_s) > 2) log_s++;
    return k.slice_log ? k.slice_log : log_s;
}

// the scratch regions of a shape whose counts are set, each aligned to 256 bytes
void msm_layout(MsmShape& s) {
    s.max_items = (s.entries >> s.log_s) + s.nbt + 2;
    size_t o = 0;
    auto take = [&](size_t bytes) { return std::exchange(o, align_up(o + bytes, 256)); };
    s.off_keys = take(s.entries * 4);
    s.off_sorted = take(s.entries * 4);
    s.off_tmp = take(s.entries * 8);
    s.off_pcount = take(((size_t)s.np + 2) * 4);
    s.off_pbase = take(((size_t)s.np + 2) * 4);
    s.off_pcursor = take(((size_t)s.np + 2) * 4);
    s.off_starts = take(((size_t)s.nbt + 2) * 4);
    s.off_heavy = take(((size_t)s.nbt + 2) * 4);
    s.off_partials = take(s.max_items * XYZZ_BYTES);
    s.off_buckets = take((size_t)s.nbt * XYZZ_BYTES);
    s.off_winpart = take(((size_t)s.Wt * (1 + s.RG) + s.planes) * XYZZ_BYTES);  // window sums, then the RG group partials of each
    s.off_rcount = take((size_t)s.Wt * 4);
    s.off_planes = s.planes ? take(((size_t)s.chunks + (size_t)s.planes * s.plane_seg) * XYZZ_BYTES + (size_t)s.planes * 4 + 64) : 0;
    s.off_bflags = take(s.n / 256 + 4);  // one byte per 256-row block: the block is one entry of the dominant-value bucket
    s.off_coltab = take((size_t)(s.cols ? s.cols : 1) * 64);
    // two-level partition: the entries pass through a second 8-byte-per-entry buffer
    s.off_tmpa = s.two_level ? take(s.entries * 8 + (PARTA_GROUPS_MAX * 3 + 4) * 4) : 0;
    s.total = o;
}

MsmShape msm_shape(size_t n, uint32_t max_bits, bool hot, uint32_t cols, const MsmKnobs& k) {
    MsmShape s{};
    max_bits = clamp_bits(max_bits);
    s.n = n;
    // cost model: W * (n + 3 * 2^(c-1)) group additions
    double best = 1e300;
    uint32_t best_c = 4;
    // windows wider than 17 bits lose more in the bucket-proportional kernels than they save in additions (measured at
    // 2^22 / 2^24: c = 17 8.4 / 28.8 ms, c = 18 13.7 / 46.3 ms, c = 20 - / 40.7 ms: k_bucket_sort's partitions get small
    // and numerous, k_reduce walks 2^c * W buckets), so the model only ranks c <= 17
    for (uint32_t c = 2; c <= 17; c++) {
        uint32_t W = (max_bits + 1 + c - 1) / c;
        double cost = (double)W * ((double)n + 3.0 * (double)(1u << (c - 1)));
        if (cost < best) {
            best = cost;
            best_c = c;
        }
    }
    s.c = k.window ? k.window : best_c;  // (<= 18: k_reduce folds <= 128 groups per window)
    s.W = (max_bits + 1 + s.c - 1) / s.c;
    // Balanced windows.  max_bits + 1 bits cut into W digits of c bits leave the top window whatever remains -- 7 bits
    // at c = 13, 2 bits at c = 12, 5 at c = 10: a window whose n digits share a handful of buckets, i.e. one sort
    // partition (one workgroup) and nothing but heavy buckets.  The same W windows get (max_bits + 1) / W bits each
    // instead, the first `wfull` of them one more: widths c and c - 1, every window with >= 2^(c-2) buckets.
    const DigitCut cut = balanced_cut(max_bits + 1, s.W);
    s.c = cut.c;
    s.wfull = cut.wfull;
    s.Wt = s.W + (hot ? 1u : 0u);
    s.R = 1;
    s.range_shift = 31;
    s.cols = cols;
    // every fused column keeps a slot for its dominant-scalar window -- except in shapes of one or two windows, where that
    // window is never used (see msm_device) and would only double the finish / reduce work
    s.Wc = s.W + ((cols && s.W <= 2) ? 0u : 1u);
    if (cols) s.Wt = cols * s.Wc;
    s.Wk = s.Wt;
    s.nb = 1u << (s.c - 1);
    // Row ranges.  A narrow column (booleans, bytes, a 10-bit opcode) has ONE window of a few buckets: one or a handful
    // of sort partitions (= workgroups) for all n entries, thousands of entries per bucket, everything after the sort on
    // the heavy-bucket path.  Its rows are cut into R ranges that act as separate windows -- range r of window w is
    // window r * W + w, with its own buckets and partitions -- and the host adds the R sums of each window.
    if (!cols && n >= (1u << 15)) {
        const uint32_t lo0 = (s.c - 1 < 8) ? (s.c - 1) : 8;
        const uint32_t base_np = s.W << (s.c - 1 - lo0);
        uint32_t R = 1;
        // ... until there are >= 128 partitions and a bucket holds <= 2048 entries on average (k_finish_mid's range of
        // slice partials even when half the buckets go unused, as with booleans), while the buckets stay few against
        // the entries and a range keeps >= 2048 rows -- and the windows, the dominant scalar's included, stay within the
        // 16384 partitions of the sort (2^26 booleans asked for 16385: the lo_bits loop below never ended)
        while ((R * base_np < 128 || n / ((size_t)R * s.W * s.nb) > 2048) && (size_t)2 * R * s.W * s.nb * 4 <= n &&
               (n / (2 * R)) >= 2048 && (size_t)2 * R * s.W + 1 <= 16384)
            R *= 2;
        if (R > 1) {
            uint32_t shift = 11;
            while (((size_t)1 << shift) * R < n) shift++;
            s.range_shift = shift;
            s.R = (uint32_t)((n + ((size_t)1 << shift) - 1) >> shift);
            s.Wt = s.R * s.W + (hot ? 1u : 0u);
        }
    }
    s.nbt = s.Wt * s.nb;
    // k_reduce is a chain of 2 * qm additions per quad: the shortest chains whose workgroups still fit the chip once
    s.qm = REDUCE_QM;
    for (uint32_t qm = 4; qm < REDUCE_QM; qm *= 2) {
        uint32_t rg = (s.nb + REDUCE_T / 4 * qm - 1) / (REDUCE_T / 4 * qm);
        if ((size_t)s.Wt * rg <= k.reduce_wgs && rg <= REDUCE_T / 4) {  // one workgroup per CU: a CU with two runs both at half speed
            s.qm = qm;
            break;
        }
    }
    if (const uint32_t v = k.reduce_qm)
        if ((s.nb + REDUCE_T / 4 * v - 1) / (REDUCE_T / 4 * v) <= REDUCE_T / 4) s.qm = v;
    uint32_t per_group = REDUCE_T / 4 * s.qm;
    s.RG = (s.nb + per_group - 1) / per_group;
    s.G = 1;
    s.entries = n * s.Wk;
    s.log_s = slice_log(s.entries, n / s.nb, k);
    // two-level counting sort: the low bits of a bucket id are resolved inside LDS (k_bucket_sort), the
    // high bits select one of 2^hi_bits partitions per window (k_partition); W << hi_bits <= 16384 so
    // the per-workgroup partition histogram of k_digits fits in 64 KiB of LDS
    s.lo_bits = (s.c - 1 < 8) ? (s.c - 1) : 8;
    while (((size_t)s.Wt << (s.c - 1 - s.lo_bits)) > 16384) s.lo_bits++;
    s.hi_bits = s.c - 1 - s.lo_bits;
    s.np = s.Wt << s.hi_bits;
    msm_layout(s);
    return s;
}

// digits a scalar below 2^max_bits needs: the signed top digit must not carry out, i.e. o_(j+1) >= max_bits + 1
uint32_t table_digits_used(const TableDesc& t, uint32_t max_bits) {
    uint32_t off = 0;
    for (uint32_t j = 0; j < t.D; j++) {
        off += t.c - (j >= t.wfull ? 1u : 0u);
        if (off >= max_bits + 1) return j + 1;
    }
    return t.D;
}

MsmShape msm_shape_table(size_t n, uint32_t max_bits, bool hot, const TableDesc& t, const MsmKnobs& k) {
    MsmShape s{};
    max_bits = clamp_bits(max_bits);
    s.n = n;
    s.tab = 1;
    s.tab_stride = t.n;
    s.c = t.c;
    s.wfull = t.wfull;
    s.W = table_digits_used(t, max_bits);
    s.Wk = s.W + (hot ? 1u : 0u);
    s.Wt = 1 + (hot ? 1u : 0u);
    s.R = 1;
    s.range_shift = 31;
    s.Wc = s.W + 1;
    s.nb = 1u << (s.c - 1);
    // k_reduce: every quad pays a ~(c + c / 2)-step scalar multiplication to lift its chunk, so the chunks are as long
    // as still leaves a workgroup per CU (<= 64 buckets: a chain of 128 additions)
    s.qm = 4;
    while (s.qm < 64 && (s.nb + REDUCE_T / 4 * s.qm - 1) / (REDUCE_T / 4 * s.qm) > 256) s.qm *= 2;
    if (k.reduce_qm) s.qm = k.reduce_qm;
    const uint32_t per_group = REDUCE_T / 4 * s.qm;
    s.RG = (s.nb + per_group - 1) / per_group;
    s.G = 1;
    s.entries = n * s.Wk;
    s.log_s = slice_log(s.entries, s.entries / s.nb, k);
    // sort: 2^8 bins per k_bucket_sort workgroup -- measured at 2^24 with 21-bit bucket ids: 2^8 bins 1.6 ms, 2^10 3.5 ms,
    // 2^12 5.1 ms (placing the bins in sweeps of 256 does not change that: profiles/r2_msm_experiments.txt), k_partition
    // over the remaining 2^13 / 2^11 / 2^9 partitions 3.0 / 2.5 / 2.0 ms -- so up to 2^13 partitions for k_partition
    s.lo_bits = (s.c - 1 < 8) ? (s.c - 1) : 8;
    while (s.c - 1 - s.lo_bits > 13 && s.lo_bits < 12) s.lo_bits++;
    if (const uint32_t v = k.table_lo)
        if (v <= s.c - 1 && s.c - 1 - v <= 13) s.lo_bits = v;
    s.hi_bits = s.c - 1 - s.lo_bits;
    // the dominant-scalar window only ever fills its bucket 0: it gets ONE partition (2^lo_bits buckets) behind window 0's
    s.np = (1u << s.hi_bits) + (hot ? 1u : 0u);
    s.nbt = s.nb + (hot ? (1u << s.lo_bits) : 0u);
    // Reduce by bit planes (msm_kernels.hip, k_reduce_chunks): for power-of-two chunk lengths and at least a workgroup of chunks
    s.planes = 0;
    if (k.reduce_planes && (s.qm & (s.qm - 1)) == 0 && s.nb >= 4 * s.qm) {
        s.chunks = (s.nb + s.qm - 1) / s.qm;
        uint32_t nbits = 0;
        while ((1u << nbits) < s.chunks) nbits++;
        s.planes = nbits + 1;
        // the planes' workgroups together fill three quarters of the chip: plane_seg workgroups per plane, plane_l chunk sums
        // per quad.  Measured (profiles/r5_msm_plane_wgs_sweep.txt): MORE workgroups -- shorter chains per quad -- lose (512:
        // +3..12 % on a single MSM, the segment fold and the launch grow), 128-256 tie for a single MSM and the smaller grids
        // leave more of the chip to the next column's accumulation in a batch (2^16 0.25 -> 0.23 ms per MSM, 2^18 0.54 -> 0.53)
        s.plane_seg = std::max<uint32_t>(1, k.plane_wgs / s.planes);
        const uint32_t half = nbits ? (1u << (nbits - 1)) : 1u;
        while (s.plane_seg > 1 && (s.plane_seg - 1) * (REDUCE_T / 4) >= half) s.plane_seg--;   // no empty workgroups
        s.plane_l = (half + s.plane_seg * (REDUCE_T / 4) - 1) / (s.plane_seg * (REDUCE_T / 4));
    }
    // two-level partition (H2_MSM_TWO_LEVEL=0: the single pass)
    s.two_level = (k.two_level && s.hi_bits >= k.two_level_min_hi && s.hi_bits >= 2 && s.hi_bits <= 14) ? 1u : 0u;
    s.a_bits = s.hi_bits / 2;
    msm_layout(s);
    return s;
}

// digits for a table over n points: fewest additions D * n plus the bucket-proportional tail (k_finish, k_reduce: ~5
// additions' worth per bucket), buckets 2^(c - 1) with c = ceil(255 / D) <= 23
uint32_t table_default_digits(size_t n, const MsmKnobs& k) {
    if (k.table_digits) return k.table_digits;
    double best = 1e300;
    uint32_t best_d = 16;
    for (uint32_t D = 12; D <= TABLE_MAX_D; D++) {
        const uint32_t c = (255 + D - 1) / D;
        // (~4.7 additions' worth per bucket since the bit-plane reduce -- 8 with the running-sum chains before it; measured
        // round 5, single / batch of 8: 2^20 14 digits 1.68 / 1.58 ms, 15 digits 1.78 / 1.64, 13 digits 1.79 / 1.61; 2^18 15
        // digits 0.72, 14 digits 0.80; 2^22 13 digits 5.62, 12 digits 6.09, 14 digits 6.07.  Below 2^18 rows, where the chains
        // of k_finish / k_reduce are latency whatever the bucket count, 4 ranks the measured optimum first: 2^16 16 digits
        // 0.40 ms, 15 digits 0.42)
        const double cost = (double)D * (double)n + (n < ((size_t)1 << 18) ? 4.0 : 4.7) * (double)(1u << (c - 1));
        if (cost < best) {
            best = cost;
            best_d = D;
        }
    }
    return best_d;
}

bool table_considered(const TableDesc& t, size_t n, uint32_t max_bits, const MsmKnobs& k) {
    // below 2^15 scalars the windowed pipeline (and its fused groups) is as fast: 2^14 0.41 vs 0.44 ms
    if (n < k.table_min_n) return false;
    // narrow columns: the plain pipeline's row ranges and fused groups are built for them, and a table saves nothing
    return k.table_force || table_digits_used(t, max_bits) < msm_shape(n, max_bits, false, 0, k).W;
}

// additions: digits x rows, + ~10 additions' worth of k_finish / k_reduce per bucket (measured: 0.8 - 0.9 ns per bucket
// against 0.08 ns per addition in both shapes).  A table built for n rows has 2^21 buckets at 2^24: a column that is 7/8
// one value (a grand product over padding rows) leaves 12 entries per bucket and is better off in 15 windows of 2^16.
bool table_pays(const TableDesc& t, size_t n, uint32_t max_bits, uint32_t live, const MsmKnobs& k) {
    const MsmShape p = msm_shape(n, max_bits, false, 0, k);
    const double rows = (double)n * (double)(live ? live : 1) / (double)HOT_SAMPLES;
    const double plain = (double)p.W * rows + 10.0 * (double)p.Wt * (double)p.nb;
    const double table = (double)table_digits_used(t, max_bits) * rows + 10.0 * (double)(1u << (t.c - 1));
    return k.table_force || table < plain;
}

// largest fused group (<= 64 columns) whose sort still fits the LDS histograms and whose keys stay below 2^28 entries
uint32_t fused_group_limit(size_t n, uint32_t bits, const MsmKnobs& k) {
    const MsmShape one = msm_shape(n, bits, true, 0, k);
    // Fusing pays while a column is dominated by fixed latencies (measured, 8 uniform columns: 2^14 0.26 vs 0.51 ms per
    // MSM, 2^16 0.40 vs 0.69, 2^18 0.90 vs 0.86, 2^20 2.35 vs 2.0); past ~4M (scalar, window) entries per column the
    // two-stream pipeline, which hides every column's host tail under the next column's kernels, is the better shape.
    // Columns with a short scalar bound have one or two windows: the slot every fused column keeps for its
    // dominant-scalar window would double their finish / reduce work -- they stay in the pipeline too.
    const uint32_t fuse_log = k.fuse_log;
    // Short bounds (a few windows): fused only when a column still spreads over >= 16 sort partitions; a column of a few
    // hundred buckets is one partition and nothing but heavy buckets -- the row ranges of the single-column shape are
    // what it needs
    const uint32_t wc = one.W + (one.W <= 2 ? 0u : 1u);
    const uint32_t lo0 = (one.c - 1 < 8) ? (one.c - 1) : 8;
    // (columns of one or two windows -- 16-bit witness cells -- are dominated by the fixed costs of their sort, finish and
    // reduce four times further up: measured at 2^22 rows, 64 such columns, 1.45 -> 1.25 ms per column fused; wide k = 22
    // from a compact witness 384 -> 372 ms)
    const uint32_t fuse_log_w = (one.W <= 2 && !k.fuse_log_present) ? fuse_log + 2 : fuse_log;
    if ((size_t)(one.W + 1) * n > ((size_t)1 << fuse_log_w) || (one.W < 8 && (one.W << (one.c - 1 - lo0)) < 16)) return 1;
    uint32_t best = 1;
    for (uint32_t g = 2; g <= 64; g++) {
        const size_t wt = (size_t)g * wc;
        if (wt * n > ((size_t)1 << 28)) break;
        if (one.c - 1 > 9 && (wt << (one.c - 1 - 9)) > 16384) break;  // lo_bits would exceed 9 (512 bins per partition)
        best = g;
    }
    return best;
}

MsmCover msm_cover(size_t n, uint32_t max_bits, const TableDesc* tabs, size_t ntabs, const MsmKnobs& k) {
    MsmCover c;
    auto take = [&](const MsmShape& s) {
        c.total = std::max(c.total, s.total);
        // (the table form exports its window sum as bit planes: up to 24 points where the windowed form has its W + 1)
        c.exported = std::max(c.exported, exported_points(s));
        c.entries = std::max(c.entries, s.entries);
    };
    for (bool hot : {false, true}) {  // (both: with the dominant-scalar array the slices can come out longer and the partials fewer)
        take(msm_shape(n, max_bits, hot, 0, k));
        for (size_t i = 0; i < ntabs; i++) take(msm_shape_table(n, max_bits, hot, tabs[i], k));
    }
    return c;
}

size_t msm_batch_need(size_t n, uint32_t max_bits, size_t count, size_t single, const MsmKnobs& k) {
    const size_t pipeline = 2 * align_up(single, 256);
    if (count < 2 || n == 0 || max_bits == 0) return pipeline;
    const uint32_t g = (uint32_t)std::min<size_t>(count, fused_group_limit(n, max_bits, k));
    return g >= 2 ? std::max(pipeline, msm_shape(n, max_bits, false, g, k).total) : pipeline;
}

MsmLaunchPlan msm_plan_launch(const MsmShape& s, uint32_t max_bits, bool hot_on, bool block_sums, bool fused, uint64_t hot_mask,
                              const MsmKnobs& k) {
    MsmLaunchPlan p{};
    h2_msm_launch_info& rec = p.rec;
    const bool hot = !fused && hot_on;  // a fused shape has no row ranges, no table and its dominant values per column (hot_mask)
    p.fused = fused;
    p.bflags = hot && block_sums;
    const uint32_t nblk = (uint32_t)((s.n + 255) / 256);
    p.digits_grid_x = nblk < 1024 ? nblk : 1024;  // grid-stride: one LDS histogram flush per workgroup
    p.digits_grid_y = fused ? s.cols : 1u;        // fused: one grid row and one LDS histogram per column
    p.np_col = fused ? s.Wc << s.hi_bits : s.np;
    p.digits_lds = (size_t)p.np_col * 4;
    p.block_rows_end = p.bflags ? s.n / BLOCK_ROWS * BLOCK_ROWS : (size_t)0;
    if (s.tab && s.two_level) {
        rec.partition = H2_MSM_PART_TWO_LEVEL;
        rec.hot_partitioned = s.Wk > s.W ? 1u : 0u;
        p.b_bits = s.hi_bits - s.a_bits;
        p.part_a_grid_x = (uint32_t)((s.n + PART_AB_T - 1) / PART_AB_T);
        p.part_b_grid_x = (uint32_t)(s.entries / PART_AB_T + (1u << s.a_bits) + 1);
        // the dominant-scalar array: one partition behind the 2^hi_bits of window 0, appended as before
        p.part_tile = PART_T_TABLE, p.part_first = s.W, p.part_arrays = s.Wk - s.W;
    } else if (s.tab && s.hi_bits > 10) {
        rec.partition = H2_MSM_PART_16384;
        p.part_tile = PART_T_TABLE, p.part_first = 0, p.part_arrays = s.Wk;
    } else {
        rec.partition = H2_MSM_PART_2048;
        p.part_tile = PART_T, p.part_first = 0, p.part_arrays = s.Wk;
    }
    p.part_grid_x = (uint32_t)((s.n + p.part_tile - 1) / p.part_tile);
    p.part_lds = ((size_t)4 << s.hi_bits) + 4 * (p.part_tile / 256);
    // a partition holding more than 4x its fair share (and at least a few thousand entries) takes the skew path
    rec.skew_threshold = (uint32_t)std::max<size_t>(4 * (s.entries / s.np), 4096);
    rec.hot_partition = hot ? ((s.tab ? 1u : s.R * s.W) << s.hi_bits) : 0xffffffffu;
    // partitions of a large MSM over a table are all about the same size (24-29 000 entries at 2^21 .. 2^24): with room
    // for one of them in LDS the sorted list is written as whole lines (H2_MSM_SORT_STAGE=0: placed directly)
    const size_t avg_part = s.entries / s.np;
    rec.stage_cap = (k.sort_stage && s.tab && avg_part >= 8192 && avg_part + avg_part / 10 <= 32768) ? 32768u : 0u;
    p.sort_lds = ((size_t)4 << s.lo_bits) + (size_t)rec.stage_cap * 4;
    p.hot_wc = fused ? s.Wc : 0u;
    const uint32_t nslices = (uint32_t)((s.entries + (1u << s.log_s) - 1) >> s.log_s);
    p.acc_grid_x = (nslices + 255) / 256;
    // waves per SIMD the accumulation is compiled for: 4 (110 VGPRs, no spills) or 5 (96 VGPRs, 14 spilled): H2_MSM_ACC_WAVES
    rec.acc_waves = k.acc_waves;
    // one lane per bucket from 2^19 buckets on (round 3, same box: 2^22 windowed 6.75 -> 6.61 ms, over a table 5.91 -> 5.76-5.90,
    // 2^24 windowed 23.9 -> 23.7; at 2^17 the forms tie, at 2^16 buckets the quads win by 4-7 %)
    rec.finish = s.nbt >= k.finish_lane_from ? H2_MSM_FINISH_LANES : H2_MSM_FINISH_QUADS;
    p.finish_grid_x = rec.finish == H2_MSM_FINISH_LANES ? (s.nbt + 255) / 256 : (s.nbt + 63) / 64;
    rec.reduce = (s.tab && s.planes) ? H2_MSM_REDUCE_PLANES : H2_MSM_REDUCE_GROUPS;
    p.reduce_groups = (s.chunks + REDUCE_T / 4 - 1) / (REDUCE_T / 4);
    p.reduce_grid_y = s.tab ? 1u : s.Wt;
    rec.form = fused ? H2_MSM_FORM_FUSED : s.tab ? H2_MSM_FORM_TABLE : H2_MSM_FORM_WINDOWED;
    rec.max_bits = clamp_bits(max_bits);
    rec.c = s.c, rec.wfull = s.wfull, rec.W = s.W, rec.Wt = s.Wt, rec.Wk = s.Wk, rec.R = s.R, rec.range_shift = s.range_shift;
    rec.cols = s.cols, rec.Wc = s.Wc, rec.nb = s.nb, rec.nbt = s.nbt, rec.lo_bits = s.lo_bits, rec.hi_bits = s.hi_bits;
    rec.np = s.np, rec.log_s = s.log_s, rec.qm = s.qm, rec.RG = s.RG, rec.planes = s.planes, rec.chunks = s.chunks;
    rec.plane_seg = s.plane_seg, rec.plane_l = s.plane_l, rec.two_level = s.two_level, rec.a_bits = s.a_bits;
    rec.hot_on = (fused ? hot_mask != 0 : hot_on) ? 1u : 0u;
    rec.block_sums = p.bflags ? 1u : 0u;
    rec.hot_mask = fused ? hot_mask : 0ull;
    rec.n = s.n, rec.entries = s.entries;
    rec.off_keys = s.off_keys, rec.off_sorted = s.off_sorted, rec.off_pbase = s.off_pbase, rec.off_starts = s.off_starts;
    rec.off_heavy = s.off_heavy, rec.off_buckets = s.off_buckets, rec.total = s.total;
    return p;
}

}  // namespace h2
