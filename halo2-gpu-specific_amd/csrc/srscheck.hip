// srscheck.hip -- screening the points of an SRS (srscheck.hpp).
//   k_g1_check_points  one point per lane: four dwordx4 loads, two limb comparisons against q, three field products
//                      (y^2, x^2, x^2 x) and one comparison.  No LDS, no scratch.  Every lane computes the curve equation
//                      whatever its coordinates are -- the products of a non-canonical coordinate are garbage that nothing
//                      reads -- so a wave never diverges before the append, which all of its lanes reach (tail lanes pass false).
#include "append.hpp"
#include "ec.hpp"
#include "srscheck.hpp"

namespace h2 {
namespace {

constexpr uint32_t SRS_BLOCK = 256;

// a < q as stored limbs: the borrow out of a - q
H2_DEV bool fq_is_canonical(const Fq& a) {
    uint32_t borrow = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const uint64_t t = (uint64_t)a.l[i] - FqParams::MOD[i] - borrow;
        borrow = (uint32_t)(t >> 32) & 1;
    }
    return borrow != 0;
}

int invalid(const char* msg) {
    set_last_error(std::string("h2_dev_g1_check_points: ") + msg);
    return H2_ERR_INVALID;
}

}  // namespace

__global__ void __launch_bounds__(SRS_BLOCK) k_g1_check_points(const Affine* points, uint32_t n, uint32_t table, uint32_t flags,
                                                               unsigned long long* count, h2_check_record* out,
                                                               unsigned long long cap) {
    const uint32_t i = blockIdx.x * SRS_BLOCK + threadIdx.x;      // n <= 2^28 and the grid covers n: no overflow
    bool fail = false;
    uint32_t kind = H2_SRS_OFF_CURVE;
    if (i < n) {
        const Affine p = affine_load(points + i);
        const Fq one = fp_one<FqParams>();
        const Fq rhs = fp_add(fp_mul(fp_sqr(p.x), p.x), fp_add(fp_add(one, one), one));
        const bool on_curve = fp_eq(fp_sqr(p.y), rhs);
        if (!fq_is_canonical(p.x) || !fq_is_canonical(p.y)) {
            fail = true;
            kind = H2_SRS_NONCANONICAL;
        } else if (affine_is_identity(p)) {
            fail = (flags & H2_SRS_FORBID_IDENTITY) != 0;
            kind = H2_SRS_IDENTITY;
        } else {
            fail = !on_curve;
        }
    }
    check_append(fail, kind, table, 0, i, count, out, cap);
}

int g1_check_points_args(const void* d_points, size_t n, uint32_t flags, const uint64_t* d_count,
                         const h2_check_record* d_records, size_t cap) {
    if (n > G1_CHECK_MAX_POINTS) return invalid("more than 2^28 points");
    if (flags & ~(uint32_t)H2_SRS_FORBID_IDENTITY) return invalid("unknown flag");
    if ((n && !d_points) || !d_count || (cap && !d_records)) return invalid("null argument");
    return H2_OK;
}

int g1_check_points_launch(const void* d_points, size_t n, uint32_t table, uint32_t flags, uint64_t* d_count,
                           h2_check_record* d_records, size_t cap, hipStream_t stream) {
    if (int rc = g1_check_points_args(d_points, n, flags, d_count, d_records, cap)) return rc;
    if (n)
        hipLaunchKernelGGL(k_g1_check_points, dim3((unsigned)((n + SRS_BLOCK - 1) / SRS_BLOCK)), dim3(SRS_BLOCK), 0, stream,
                           (const Affine*)d_points, (uint32_t)n, table, flags, (unsigned long long*)d_count, d_records,
                           (unsigned long long)cap);
    H2_HIP(hipGetLastError());
    return H2_OK;
}

}  // namespace h2
