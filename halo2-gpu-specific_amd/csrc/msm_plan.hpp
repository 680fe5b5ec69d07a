// msm_plan.hpp -- what an MSM call decides before anything is enqueued (msm_plan.cpp): the knobs of the environment, the
// shape of the pipeline for n rows and a scalar bound, the shapes a call may end up with, and the launch plan of one shape.
// Host only and free of HIP: every function here is a function of its arguments (msm_knobs() alone reads the environment),
// so tests/msm_plan_host.cpp checks them without a device.  The kernels are in msm_kernels.hip, the shifted-base tables in
// msm_table.hip, the drivers in msm.hip.
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/halo2_hip.h"

namespace h2 {

static constexpr uint32_t FINISH_SERIAL = 32; // partials a single quad folds in k_finish
static constexpr uint32_t SORT_T = 1024;      // threads of a k_bucket_sort workgroup (one partition each)
static constexpr uint32_t HEAVY_SPLIT = 64;   // workgroups sharing one heavy bucket in k_finish_heavy
static constexpr uint32_t MID_MAX = 512;      // partials of a bucket one wave folds in k_finish_mid
static constexpr uint32_t KEY_INVALID = 0xffffffffu;
static constexpr uint32_t SIGN_BIT = 0x80000000u;
static constexpr uint32_t REDUCE_T = 512;    // threads per k_reduce workgroup = 128 quads (two waves per SIMD)
static constexpr uint32_t REDUCE_QM = 32;    // consecutive buckets a quad walks (fewer when that still fits the chip)
static constexpr uint32_t PART_T = 2048;      // entries per k_partition workgroup (256 threads x 8)
static constexpr uint32_t PART_AB_T = 8192;       // entries per workgroup of the two-level partition passes (256 threads x 32)
static constexpr uint32_t PARTA_GROUPS_MAX = 128; // level-A groups (2^a_bits <= 2^7)
static constexpr uint32_t PART_T_TABLE = 16384;  // ... over a shifted-base table with many partitions (256 threads x 64)
static constexpr uint32_t BLOCK_ROWS = 256;           // = the rows a k_digits workgroup takes per step
static constexpr uint32_t BLOCK_INDEX0 = 0x40000000u; // point index of block sum 0 in the sorted entries
static constexpr uint32_t BLOCK_KEY = 0x40000000u;    // key of a row that stands for its whole block (bucket 0)
static constexpr uint32_t TABLE_MAX_D = 32;
static constexpr uint32_t TABLE_MIN_D = 11;  // digits of <= 24 bits: 2^23 buckets
static constexpr uint32_t HOT_SAMPLES = 64;
static constexpr uint32_t HOT_MIN = 16;  // a value on >= 16 of 64 sampled rows gets its own window
// sizes of the device types the scratch is laid out for (static_asserted against Fr, Affine and XYZZ in msm_kernels.hip)
static constexpr size_t FR_BYTES = 32, AFFINE_BYTES = 64, XYZZ_BYTES = 128;

// The H2_MSM_* variables, read once per public entry point (msm_knobs) and passed down.  0 = unset where a variable
// replaces a computed value.
struct MsmKnobs {
    uint32_t slice_log = 0;   // SLICE_LOG 1..10: the slice length, whatever slice_log() computes
    uint32_t window = 0;      // WINDOW 2..18: the window width the cost model would choose
    uint32_t reduce_qm = 0;   // REDUCE_QM 1..64: windowed only while RG <= 128 holds; over a table it replaces the computed value
    uint32_t table_lo = 0;    // TABLE_LO 4..12: lo_bits over a table (when the partitions stay <= 2^13)
    uint32_t fuse_log = 22;   // FUSE_LOG 10..28: a column of more (scalar, window) entries than 2^fuse_log is not fused
    bool fuse_log_present = false;  // ... set at all, valid or not: no + 2 for columns of one or two windows
    uint32_t lanes = 2;       // LANES 2..4: streams of the batch pipeline
    bool no_table = false;    // NO_TABLE=1: ignore every shifted-base table
    bool no_hot = false;      // NO_HOT=1: no dominant-value window
    bool no_fuse = false;     // NO_FUSE present: no fused groups
    bool table_force = false; // TABLE_FORCE present: experiment, tables of more digits than windows and ones that do not pay
    size_t table_min_n = (size_t)1 << 15;  // TABLE_MIN_N: tables are used from this many rows on
    uint32_t table_digits = 0;    // TABLE_DIGITS 11..32: digits of a table built with digits = 0
    size_t reduce_wgs = 256;      // REDUCE_WGS >= 1: k_reduce workgroups that count as filling the chip once
    uint32_t plane_wgs = 192;     // PLANE_WGS >= 1: workgroups of k_reduce_planes
    bool reduce_planes = true;    // REDUCE_PLANES=0: k_reduce over a table's window
    bool two_level = true;        // TWO_LEVEL=0: the single-pass partition over a table
    uint32_t two_level_min_hi = 8;  // TWO_LEVEL_MIN_HI: two-level from this many partition bits on
    bool sort_stage = true;       // SORT_STAGE=0: k_bucket_sort places directly
    uint32_t acc_waves = 4;       // ACC_WAVES=5: k_acc_slice<5>
    uint32_t finish_lane_from = 1u << 19;  // 1 << FINISH_LANE_LOG: buckets from which k_finish_lane runs
};
MsmKnobs msm_knobs();

struct MsmShape {
    uint32_t c, W, nb, nbt, G;  // window bits, digit windows, buckets/window, total buckets, points exported per window (1)
    uint32_t RG, qm;            // k_reduce: workgroups per window (folded on the device by the last one to finish) and
                                // consecutive buckets per quad
    uint32_t Wt;                // windows the pipeline runs: R * W, + 1 when a dominant scalar has its own window (see k_digits)
    uint32_t Wk;                // key arrays k_digits writes (n keys each): W, + 1 with a dominant scalar; cols * Wc when fused
    uint32_t wfull;             // windows 0 .. wfull - 1 are c bits wide, the rest c - 1 (see msm_shape)
    uint32_t R, range_shift;    // row ranges: rows i >> range_shift = r use windows r * W .. r * W + W - 1 (see msm_shape)
    uint32_t cols, Wc;          // fused multi-column shape: `cols` columns x Wc = W + 1 windows each (cols = 0: one MSM)
    uint32_t tab;               // 1: shifted-base table (see msm_table.hip): the W digits of a scalar share ONE window of nb buckets
    size_t tab_stride;          // points per level of the table: digit w of row i adds table[w * tab_stride + i]
    size_t off_coltab;          // fused: per-column scalar pointers (8 B) and dominant values (32 B)
    uint32_t log_s;             // slice length S = 2^log_s entries
    uint32_t lo_bits, hi_bits;  // bucket id = hi (partition inside the window) : lo (bin inside the partition)
    uint32_t np;                // partitions = W << hi_bits
    size_t n, entries, max_items;
    // scratch offsets (bytes)
    size_t off_keys, off_sorted, off_tmp, off_pcount, off_pbase, off_pcursor, off_starts, off_heavy, off_partials,
        off_buckets, off_winpart, off_rcount, off_bflags, off_tmpa, total;
    uint32_t two_level;         // table shape: partition in two coalesced passes (k_part_a / k_part_b), a_bits + b_bits = hi_bits
    uint32_t a_bits;
    // table shape, reduce by bit planes (k_reduce_chunks / k_reduce_planes): `planes` points leave the device per MSM --
    // P_0 .. P_(planes-2) and the sum of the chunks' own weighted sums -- in winpart[Wt ..]; 0 = the classic k_reduce
    uint32_t planes, chunks, plane_l, plane_seg;
    size_t off_planes;          // the chunk sums R[chunks], then the plane partials [planes][plane_seg], then `planes` counters
};

// a shifted-base table as the plan sees it: n points per level, D digits, digit j c bits wide for j < wfull, c - 1 after
struct TableDesc {
    size_t n;
    uint32_t D, c, wfull;
};

inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }
inline uint32_t clamp_bits(uint32_t max_bits) { return max_bits > 254 ? 254u : max_bits ? max_bits : 1u; }

// T bits cut into W digits of T / W bits, the first `wfull` of them one more: widths c and c - 1
struct DigitCut {
    uint32_t c, wfull;
};
DigitCut balanced_cut(uint32_t T, uint32_t W);
TableDesc table_desc(size_t n, uint32_t digits);  // the balanced cut of 255 bits

uint32_t slice_log(size_t entries, size_t per_bucket, const MsmKnobs& k);
void msm_layout(MsmShape& s);
MsmShape msm_shape(size_t n, uint32_t max_bits, bool hot, uint32_t cols, const MsmKnobs& k);
MsmShape msm_shape_table(size_t n, uint32_t max_bits, bool hot, const TableDesc& t, const MsmKnobs& k);
// points that leave the device per MSM
inline size_t exported_points(const MsmShape& s) { return (size_t)s.Wt * s.G + s.planes; }

uint32_t table_digits_used(const TableDesc& t, uint32_t max_bits);
uint32_t table_default_digits(size_t n, const MsmKnobs& k);
// is a table of these bases worth looking at for n rows of this bound (before the samples are in) ...
bool table_considered(const TableDesc& t, size_t n, uint32_t max_bits, const MsmKnobs& k);
// ... and does it beat the windowed shape when about live / HOT_SAMPLES of the rows carry digits?
bool table_pays(const TableDesc& t, size_t n, uint32_t max_bits, uint32_t live, const MsmKnobs& k);
uint32_t fused_group_limit(size_t n, uint32_t bits, const MsmKnobs& k);

// The shapes one MSM of n rows and this bound may be given once its samples are in: windowed or over any of `tabs`, each
// without and with the dominant-value window.  What must hold for all of them: the scratch, the points read back, the
// sorted entries (indexed with 32 bits).
struct MsmCover {
    size_t total = 0, exported = 0, entries = 0;
};
MsmCover msm_cover(size_t n, uint32_t max_bits, const TableDesc* tabs, size_t ntabs, const MsmKnobs& k);
// scratch that lets a batch fuse `count` columns of one bound over one base table; `single`: msm_cover's total for one column
size_t msm_batch_need(size_t n, uint32_t max_bits, size_t count, size_t single, const MsmKnobs& k);

// Everything msm_enqueue (msm_kernels.hip) hands the kernels of one launch that is not an address: the choices, the grids
// and the dynamic LDS sizes.  `rec` is the launch's record (h2_msm_last_launches) but for the scratch address.
struct MsmLaunchPlan {
    h2_msm_launch_info rec;
    bool fused, bflags;          // bflags: whole blocks of the dominant value enter its bucket as one point (k_digits)
    uint32_t digits_grid_x, digits_grid_y, np_col;   // np_col: partitions of one column (fused) or of the launch
    size_t digits_lds, block_rows_end;
    // k_partition<part_tile> over the key arrays part_first .. part_first + part_arrays - 1 (no arrays: not launched)
    uint32_t part_tile, part_first, part_arrays, part_grid_x;
    size_t part_lds;
    uint32_t b_bits, part_a_grid_x, part_b_grid_x;   // two-level: k_part_a / k_part_b
    size_t sort_lds;
    uint32_t hot_wc;             // fused: windows per column when columns own a dominant-value window
    uint32_t acc_grid_x, finish_grid_x;
    uint32_t reduce_groups;      // planes: workgroups of k_reduce_chunks
    uint32_t reduce_grid_y;      // groups: windows k_reduce walks (over a table: one window of nb buckets)
};
MsmLaunchPlan msm_plan_launch(const MsmShape& s, uint32_t max_bits, bool hot_on, bool block_sums, bool fused, uint64_t hot_mask,
                              const MsmKnobs& k);

}  // namespace h2
