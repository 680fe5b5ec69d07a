// values.hip -- the fused evaluator's kernel (values.hpp; DESIGN.md 3b, "Computing a witness").  One lane per row, 256-lane
// workgroups, a grid-stride loop over the rows.  The lowered program travels in the kernel arguments and is the same for
// every lane: its fetch and decode are scalar loads and scalar branches.  Slot 0 of a lane is a register value; its other
// slots are a column of LDS laid out [slot][limb][lane] -- lane t touches words t, 256 + t, ... only, stride-1 across the wave and never another lane's, so no
// barrier is needed anywhere -- and the most recent result stays in registers (`last`).  Nothing of length m is written
// but the outputs.
#include "common.hpp"
#include "values.hpp"

namespace h2 {

namespace {

// slot 0 is a register value, slots 1 .. VAL_SLOTS - 1 are LDS (the slot index is uniform: a scalar branch)
constexpr uint32_t VAL_LDS_SLOTS = VAL_SLOTS - 1;

struct LdsSlots {
    uint32_t* base;  // this lane's column: &sh[0][0][tid]
    Fr r0;
    __device__ __forceinline__ Fr load(uint32_t i) const {
        if (i == 0) return r0;
        Fr v;
#pragma unroll
        for (int l = 0; l < 8; l++) v.l[l] = base[((i - 1) * 8 + l) * VAL_THREADS];
        return v;
    }
    __device__ __forceinline__ void store(uint32_t i, const Fr& v) {
        if (i == 0) {
            r0 = v;
            return;
        }
#pragma unroll
        for (int l = 0; l < 8; l++) base[((i - 1) * 8 + l) * VAL_THREADS] = v.l[l];
    }
};

// INTS: the program has integer ops (values.hpp, val_run_row); each instantiation has its one multiplier site
template <bool INTS>
__global__ void __launch_bounds__(VAL_THREADS) k_values_eval(const ValProgram P, const size_t m) {
    __shared__ uint32_t sh[VAL_LDS_SLOTS * 8 * VAL_THREADS];
    LdsSlots slots{sh + threadIdx.x, fp_zero<FrParams>()};
    const size_t step = (size_t)gridDim.x * VAL_THREADS;
    for (size_t row = (size_t)blockIdx.x * VAL_THREADS + threadIdx.x; row < m; row += step) val_run_row<INTS>(P, row, slots);
}

}  // namespace

int values_eval_launch(const ValProgram& P, size_t m, hipStream_t stream) {
    if (m == 0) return H2_OK;
    const size_t want = (m + VAL_THREADS - 1) / VAL_THREADS;
    const unsigned blocks = (unsigned)(want < VAL_MAX_BLOCKS ? want : VAL_MAX_BLOCKS);
    if (P.has_integer) hipLaunchKernelGGL(k_values_eval<true>, dim3(blocks), dim3(VAL_THREADS), 0, stream, P, m);
    else hipLaunchKernelGGL(k_values_eval<false>, dim3(blocks), dim3(VAL_THREADS), 0, stream, P, m);
    H2_HIP(hipGetLastError());
    return H2_OK;
}

}  // namespace h2
