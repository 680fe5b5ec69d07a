// g1mul.hip -- out[i] = [k_i] P_i, one lane per point, every lane its own 254-bit scalar (g1mul.hpp).
//
// Lanes of a wave hold unrelated scalars, so the wave issues every group operation that any of its lanes needs.  A plain
// MSB-first double-and-add (g1ntt.hip's affine_mul_scalar) then issues the addition at nearly every bit: 9 x 255 + 10 x 254 =
// 4.8e3 products per point.  Here the scalar is cut into 85 signed digits of 3 bits, d in [-4, 3], MSB first: three
// doublings and ONE addition of +-T[|d|] per digit against a per-lane table T = {P, 2P, 3P, 4P} held in registers.
//
// Digits without a carry chain: with C = 4 (1 + 8 + ... + 8^84) the plain 3-bit digits d' of k + C are d + 4, since
// k = sum (d'_i - 4) 8^i.  k < r gives k + C < 0.95 x 2^255: 85 digits cover it; bit 255 of k + C is tested all the same and
// weighs [2^255] P, so the schedule is exact for every k + C below 2^256.  The digit is read from the top of the scalar,
// which is then shifted left: static limb indices, the scalar stays out of scratch (as g1ntt.hip's shl1).  T[|d| - 1] is
// picked by compares and selects over registers: an index computed at run time would put the table in scratch.
//
// Products issued per point (ec.hpp: doubling 9, XYZZ addition 14): the scalar out of Montgomery form 1, the table 9 + 14 + 9,
// 84 x 3 doublings after the first digit, 85 additions, the normalisation a^(q-2) with 4 more (254 + 127 + 4):
//   1 + 32 + 9 x 252 + 14 x 85 + 385 = 3876, of which 3491 are the multiplication itself (the double-and-add: 4835 + 385).
// (The first digit's addition meets an empty accumulator and costs no product: 3477 as issued.)
// tools/params_update.py --bench counts the same schedule from the scalars of a run.
//
// Exceptional cases are the complete formulas' of ec.hpp (identity input, zero scalar, acc = +-T[|d|]): the results are exact
// group elements, normalised to the one affine form (identity (0, 0)).
#include "ec.hpp"
#include "g1mul.hpp"

namespace h2 {
namespace {

// limb j of C = sum over i < 85 of 4 x 8^i: bits 2, 5, ..., 254
constexpr uint32_t bias_limb(int j) {
    uint32_t v = 0;
    for (int b = 0; b < 32; b++) {
        const int bit = 32 * j + b;
        if (bit % 3 == 2 && bit < 255) v |= 1u << b;
    }
    return v;
}

// k + C over 256 bits
H2_DEV Fr add_bias(const Fr& k) {
    Fr r;
    uint64_t carry = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        carry += (uint64_t)k.l[i] + bias_limb(i);
        r.l[i] = (uint32_t)carry;
        carry >>= 32;
    }
    return r;
}

// k <<= S over 256 bits, 0 < S < 32 (static limb indices)
template <int S>
H2_DEV void shl(Fr& k) {
#pragma unroll
    for (int i = 7; i > 0; i--) k.l[i] = (k.l[i] << S) | (k.l[i - 1] >> (32 - S));
    k.l[0] <<= S;
}

H2_DEV Fq fq_select(bool c, const Fq& a, const Fq& b) {
    Fq r;
#pragma unroll
    for (int i = 0; i < 8; i++) r.l[i] = c ? a.l[i] : b.l[i];
    return r;
}
H2_DEV XYZZ xyzz_select(bool c, const XYZZ& a, const XYZZ& b) {
    XYZZ r;
    r.x = fq_select(c, a.x, b.x);
    r.y = fq_select(c, a.y, b.y);
    r.zz = fq_select(c, a.zz, b.zz);
    r.zzz = fq_select(c, a.zzz, b.zzz);
    return r;
}

// [k] p for a plain (not Montgomery) scalar k < r
H2_DEV XYZZ g1_mul_digits(const Affine& p, const Fr& k_plain) {
    const XYZZ t1 = xyzz_from_affine(p, false);
    Fr k = add_bias(k_plain);
    const XYZZ t2 = xyzz_double(t1);
    const XYZZ t3 = xyzz_add(t2, t1);
    const XYZZ t4 = xyzz_double(t2);
    XYZZ acc = (k.l[7] >> 31) ? t1 : xyzz_identity();  // bit 255
    shl<1>(k);
#pragma unroll 1
    for (uint32_t digit = 0; digit < G1MUL_DIGITS; digit++) {
#pragma unroll 1
        for (uint32_t j = 0; j < G1MUL_WINDOW; j++) acc = xyzz_double(acc);
        const int d = (int)(k.l[7] >> 29) - 4;
        shl<G1MUL_WINDOW>(k);
        const int m = d < 0 ? -d : d;
        if (m != 0) {
            XYZZ t = xyzz_select(m == 2, t2, t1);
            t = xyzz_select(m == 3, t3, t);
            t = xyzz_select(m == 4, t4, t);
            t.y = fq_select(d < 0, fp_neg(t.y), t.y);
            acc = xyzz_add(acc, t);
        }
    }
    return acc;
}

__global__ void __launch_bounds__(G1MUL_BLOCK) k_g1_mul_each(const Affine* points, const Fr* scalars, size_t n, Affine* out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const XYZZ acc = g1_mul_digits(affine_load(points + i), fp_from_mont(fp_load(scalars + i)));
    const Fq zero = fp_zero<FqParams>();
    if (xyzz_is_identity(acc)) {
        fp_store(&out[i].x, zero);
        fp_store(&out[i].y, zero);
        return;
    }
    // x = X / ZZ, y = Y / ZZZ with one inversion: t = 1 / ZZZ, 1 / ZZ = (ZZ t)^2  (ZZ^3 = ZZZ^2)
    const Fq t = fq_inv_device(acc.zzz);
    const Fq u = fp_mul(acc.zz, t);
    fp_store(&out[i].x, fp_mul(acc.x, fp_sqr(u)));
    fp_store(&out[i].y, fp_mul(acc.y, t));
}

}  // namespace

int g1_mul_each_args(const void* d_points, const void* d_scalars, size_t n, const void* d_out) {
    if (n && (!d_points || !d_scalars || !d_out)) {
        set_last_error("h2_dev_g1_mul_each: null argument");
        return H2_ERR_INVALID;
    }
    if (n > ((size_t)1 << 31)) {  // the grid's block count is 32 bits
        set_last_error("h2_dev_g1_mul_each: more than 2^31 points");
        return H2_ERR_INVALID;
    }
    return H2_OK;
}

int g1_mul_each_launch(const uint64_t* d_points, const Fr* d_scalars, size_t n, uint64_t* d_out, hipStream_t stream) {
    if (n == 0) return H2_OK;
    hipLaunchKernelGGL(k_g1_mul_each, dim3((unsigned)((n + G1MUL_BLOCK - 1) / G1MUL_BLOCK)), dim3(G1MUL_BLOCK), 0, stream,
                       (const Affine*)d_points, d_scalars, n, (Affine*)d_out);
    H2_HIP(hipGetLastError());
    return H2_OK;
}

}  // namespace h2
