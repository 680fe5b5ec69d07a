// msm_plan_host.cpp -- the MSM plan (csrc/msm_plan.hpp) without a device: g++ -I csrc msm_plan_host.cpp csrc/msm_plan.cpp.
// The knobs come from the environment the program is started in (msm_knobs); queries are lines on stdin, answers lines on
// stdout (tests/test_msm_plan_host.py):
//   records   "form n max_bits cols digits table_n hot_on hot_mask block_sums" -> the launch record the plan produces for
//             that call (every h2_msm_launch_info field but `scratch`, in FIELDS' order), then fused_group_limit(n, max_bits)
//   sizes     "n max_bits count..." -> c, windows, buckets, the scratch of one MSM without tables, the batch scratch per count
//   knobs     (no input) -> every MsmKnobs member as name=value
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <sstream>
#include <string>
#include <vector>

#include "msm_plan.hpp"

using namespace h2;

static void records() {
    const MsmKnobs k = msm_knobs();
    unsigned form, max_bits, cols, digits, hot_on, block_sums;
    unsigned long long n, table_n, hot_mask;
    while (scanf("%u %llu %u %u %u %llu %u %llu %u", &form, &n, &max_bits, &cols, &digits, &table_n, &hot_on, &hot_mask, &block_sums) == 9) {
        const bool fused = form == H2_MSM_FORM_FUSED;
        const MsmShape s = form == H2_MSM_FORM_TABLE ? msm_shape_table(n, max_bits, hot_on != 0, table_desc(table_n, digits), k)
                                                     : msm_shape(n, max_bits, !fused && hot_on, fused ? cols : 0, k);
        const h2_msm_launch_info r = msm_plan_launch(s, max_bits, !fused && hot_on, block_sums != 0, fused, hot_mask, k).rec;
        const uint32_t u32[] = {r.form, r.max_bits, r.c, r.wfull, r.W, r.Wt, r.Wk, r.R, r.range_shift, r.cols, r.Wc, r.nb, r.nbt, r.lo_bits,
                                r.hi_bits, r.np, r.log_s, r.qm, r.RG, r.planes, r.chunks, r.plane_seg, r.plane_l, r.two_level, r.a_bits,
                                r.hot_on, r.block_sums, r.partition, r.hot_partitioned, r.stage_cap, r.skew_threshold, r.hot_partition,
                                r.finish, r.acc_waves, r.reduce};
        const uint64_t u64[] = {r.hot_mask, r.n, r.entries, r.off_keys, r.off_sorted, r.off_pbase, r.off_starts, r.off_heavy, r.off_buckets,
                                r.total};
        for (uint32_t v : u32) printf("%" PRIu32 " ", v);
        for (uint64_t v : u64) printf("%" PRIu64 " ", v);
        printf("%" PRIu32 "\n", fused_group_limit(n, max_bits, k));
    }
}

static void sizes() {
    const MsmKnobs k = msm_knobs();
    char line[1024];
    while (fgets(line, sizeof line, stdin)) {
        std::istringstream in(line);
        unsigned long long n, count;
        unsigned bits;
        if (!(in >> n >> bits)) continue;
        const MsmShape s = msm_shape(n, bits, false, 0, k);
        const size_t single = msm_cover(n, bits, nullptr, 0, k).total;
        printf("%" PRIu32 " %" PRIu32 " %" PRIu32 " %zu", s.c, s.W, s.nb, single);
        while (in >> count) printf(" %zu", msm_batch_need(n, bits, count, single, k));
        printf("\n");
    }
}

static void knobs() {
    const MsmKnobs k = msm_knobs();
    printf("slice_log=%u window=%u reduce_qm=%u table_lo=%u fuse_log=%u fuse_log_present=%d lanes=%u no_table=%d no_hot=%d no_fuse=%d "
           "table_force=%d table_min_n=%zu table_digits=%u reduce_wgs=%zu plane_wgs=%u reduce_planes=%d two_level=%d two_level_min_hi=%u "
           "sort_stage=%d acc_waves=%u finish_lane_from=%u\n",
           k.slice_log, k.window, k.reduce_qm, k.table_lo, k.fuse_log, (int)k.fuse_log_present, k.lanes, (int)k.no_table, (int)k.no_hot,
           (int)k.no_fuse, (int)k.table_force, k.table_min_n, k.table_digits, k.reduce_wgs, k.plane_wgs, (int)k.reduce_planes, (int)k.two_level,
           k.two_level_min_hi, (int)k.sort_stage, k.acc_waves, k.finish_lane_from);
}

int main(int argc, char** argv) {
    const std::string cmd = argc > 1 ? argv[1] : "";
    if (cmd == "records")
        records();
    else if (cmd == "sizes")
        sizes();
    else if (cmd == "knobs")
        knobs();
    else {
        fprintf(stderr, "usage: msm_plan_host records|sizes|knobs\n");
        return 2;
    }
    return 0;
}
