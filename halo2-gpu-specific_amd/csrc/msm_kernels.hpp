// msm_kernels.hpp -- what the MSM drivers (msm.hip) start on a stream: one planned launch of the pipeline, the sampling
// of a column, the read-back of the window sums (msm_kernels.hip)
#pragma once
#include "common.hpp"
#include "ec.hpp"
#include "msm_plan.hpp"

namespace h2 {

// `fused`: non-null for the multi-column shape (s.cols columns): device table of scalar pointers, then of dominant
// values, and the bit mask of the columns that have one
struct FusedCols {
    const Fr* const* scalars;
    const Fr* hot_values;
    uint64_t hot_mask;
};

// one per driver: the outermost on the calling thread empties the thread's launch list (h2_msm_last_launches)
struct LaunchScope {
    LaunchScope();
    ~LaunchScope();
};

// Starts the kernels of shape `s` as `p` = msm_plan_launch(s, ...) planned them and appends p.rec, with the scratch
// address, to the thread's launch list.  hot_value: the dominant value (when p.rec.hot_on, not fused); block_sums: the
// tabulated sums of the bases' 256-row blocks (when p.bflags).
void msm_enqueue(const MsmShape& s, const MsmLaunchPlan& p, const Fr* d_scalars, const Fr& hot_value, const Affine* d_bases,
                 const Affine* block_sums, char* scratch, hipStream_t stream, const FusedCols* fused = nullptr);
// HOT_SAMPLES rows of a column -> out (mapped pinned memory)
void sample_launch(const Fr* scalars, size_t n, Fr* out, hipStream_t stream);
// out[b] = the sum of bases[256 b .. 256 b + 255] (msm_table.hip keeps them next to a table; k_acc_slice reads them)
void block_sums_launch(const Affine* bases, size_t nblocks, Affine* out, hipStream_t stream);
// count16 16-byte words through a store kernel (see k_export): device <-> mapped pinned memory, not the DMA engines
void copy16_launch(const void* src, void* dst, size_t count16, hipStream_t stream);
void export_to_host(const XYZZ* d_src, XYZZ* h_dst, size_t count, hipStream_t stream);

}  // namespace h2
