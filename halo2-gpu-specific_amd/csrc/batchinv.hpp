// batchinv.hpp -- the workgroup step of Montgomery's trick, shared by k_batch_invert (poly.hip) and k_assigned_resolve
// (assigned.hip): every lane of a 256-lane workgroup brings the product of its own chain, ONE field inversion is done per
// workgroup, and every lane leaves with the inverse of its own product.
// The lanes' chain products are multiplied up by two LDS scans (prefix and suffix, 8 steps each), wave 0 inverts the
// workgroup's total (fp_inv: the binary extended GCD of field.hpp -- the inverting wave's lanes all hold the same value, so its
// branches are uniform: ~105 us instead of the ~230 us of the a^(r-2) chain), and lane t recovers the inverse of its own
// product as total^-1 * (product of the lanes before it) * (product of the lanes after it) -- 18 multiplications per lane
// instead of a private inversion.
#pragma once
#include "common.hpp"

namespace h2 {

__device__ __forceinline__ void binv_put(uint4* lo, uint4* hi, uint32_t i, const Fr& v) {
    lo[i] = make_uint4(v.l[0], v.l[1], v.l[2], v.l[3]);
    hi[i] = make_uint4(v.l[4], v.l[5], v.l[6], v.l[7]);
}
__device__ __forceinline__ Fr binv_get(const uint4* lo, const uint4* hi, uint32_t i) {
    const uint4 x = lo[i], y = hi[i];
    Fr r;
    r.l[0] = x.x; r.l[1] = x.y; r.l[2] = x.z; r.l[3] = x.w;
    r.l[4] = y.x; r.l[5] = y.y; r.l[6] = y.z; r.l[7] = y.w;
    return r;
}

// -> acc^-1 (Montgomery form).  Every lane of a workgroup of 256 must arrive (barriers inside), a lane without a chain with
// acc = 1; no acc may be zero.  sh_lo / sh_hi: 256 uint4 of LDS each, free for other use before and after.
__device__ __forceinline__ Fr block_invert_products(const Fr& acc, uint4* sh_lo, uint4* sh_hi) {
    const uint32_t tid = threadIdx.x;
    // before = product of the chain products of lanes < tid, after = of lanes > tid (Hillis-Steele, inclusive then shifted)
    Fr incl = acc;
    for (uint32_t off = 1; off < 256; off <<= 1) {
        binv_put(sh_lo, sh_hi, tid, incl);
        __syncthreads();
        if (tid >= off) incl = fp_mul(incl, binv_get(sh_lo, sh_hi, tid - off));
        __syncthreads();
    }
    binv_put(sh_lo, sh_hi, tid, incl);
    __syncthreads();
    const Fr before = tid ? binv_get(sh_lo, sh_hi, tid - 1) : fp_one<FrParams>();
    const Fr total = binv_get(sh_lo, sh_hi, 255);
    __syncthreads();
    Fr sfx = acc;
    for (uint32_t off = 1; off < 256; off <<= 1) {
        binv_put(sh_lo, sh_hi, tid, sfx);
        __syncthreads();
        if (tid + off < 256) sfx = fp_mul(sfx, binv_get(sh_lo, sh_hi, tid + off));
        __syncthreads();
    }
    binv_put(sh_lo, sh_hi, tid, sfx);
    __syncthreads();
    const Fr after = tid < 255 ? binv_get(sh_lo, sh_hi, tid + 1) : fp_one<FrParams>();
    __syncthreads();
    if (tid < 64) {  // one wave inverts (its lanes all hold `total`), the others wait at the barrier
        const Fr tinv = fp_inv(total);
        if (tid == 0) binv_put(sh_lo, sh_hi, 0, tinv);
    }
    __syncthreads();
    return fp_mul(fp_mul(binv_get(sh_lo, sh_hi, 0), before), after);
}

// elements per lane and lanes of a batch inversion over n elements: 64 elements a lane when that still fills the chip, down
// to 8 for small inputs (the chain of 3 multiplications per element is pure latency there; the shared inversion costs a lane
// 18 multiplications whatever the chunk); at least one whole workgroup once there are 256 elements
__host__ __device__ inline size_t batch_invert_threads(size_t n) {
    size_t chunk = 64;
    while (chunk > 8 && n / chunk < 65536) chunk /= 2;
    size_t nthreads = (n + chunk - 1) / chunk;
    if (nthreads < 256) nthreads = n < 256 ? n : 256;
    return nthreads;
}

}  // namespace h2
