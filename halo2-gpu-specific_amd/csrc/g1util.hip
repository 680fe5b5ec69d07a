// g1util.hip -- G1 work beside the MSM: synthetic points, point compression, fixed-base multiplication and the
// folds of partial points.  None of it is on the prover's hot path.
#include <cstring>

#include "g1util.hpp"

namespace h2 {

// ---------------------------------------------------------------- synthetic bases (bench / tests)
// n deterministic G1 points by try-and-increment: x = mix(seed, i), y = (x^3 + 3)^((q+1)/4) when that
// is a square root (q = 3 mod 4).  Cofactor 1: every curve point is in G1.  Not part of the prover
// path; it exists so bench.py can build its workload without touching the CPU oracle.
__device__ __forceinline__ uint64_t splitmix64(uint64_t& x) {
    uint64_t z = (x += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

__global__ void __launch_bounds__(256) k_random_points(uint64_t seed, size_t n, Affine* out) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    // (q + 1) / 4, little-endian u32 limbs
    const uint32_t E[8] = {0xb61f3f52u, 0x4f082305u, 0x5a1c72a3u, 0x65e05aa4u,
                           0xa0605617u, 0x6e14116du, 0xb84c680au, 0x0c19139cu};
    uint64_t st = seed ^ (0xd1342543de82ef95ull * (uint64_t)(i + 1));
    Fq x;
    for (int k = 0; k < 4; k++) {
        uint64_t v = splitmix64(st);
        x.l[2 * k] = (uint32_t)v;
        x.l[2 * k + 1] = (uint32_t)(v >> 32);
    }
    x.l[7] &= 0x1fffffffu;  // < 2^253 < q: a valid Montgomery residue
    Fq three = fp_add(fp_add(fp_one<FqParams>(), fp_one<FqParams>()), fp_one<FqParams>());
    for (;;) {
        Fq rhs = fp_add(fp_mul(fp_sqr(x), x), three);
        Fq y = fp_one<FqParams>();
        for (int bit = 253; bit >= 0; bit--) {
            y = fp_sqr(y);
            if ((E[bit >> 5] >> (bit & 31)) & 1) y = fp_mul(y, rhs);
        }
        if (fp_eq(fp_sqr(y), rhs)) {
            if (splitmix64(st) & 1) y = fp_neg(y);
            fp_store(&out[i].x, x);
            fp_store(&out[i].y, y);
            return;
        }
        x = fp_add(x, fp_one<FqParams>());
    }
}

int random_points_launch(uint64_t seed, size_t n, uint64_t* d_out, hipStream_t stream) {
    if (n == 0) return H2_OK;
    hipLaunchKernelGGL(k_random_points, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, seed, n,
                       (Affine*)d_out);
    H2_HIP(hipGetLastError());
    return H2_OK;
}

// ---------------------------------------------------------------- compressed points (Params::{read, write})
// poly/commitment.rs:241-294 stores g and g_lagrange as `to_bytes()` = 32 bytes per point.  Convention (the layout of
// pairing_bn256@30b052f cannot be checked without its sources -- "parity unpinned"): x little-endian, bit 7 of byte 31 =
// parity of canonical y, identity = 32 zero bytes.  Decompression is one square root (y = rhs^((q+1)/4), q = 3 mod 4)
// per point: the reference does it with a rayon `parallelize` over `from_bytes`, here it is one lane per point.
__device__ __forceinline__ Fq fq_sqrt_candidate(const Fq& rhs) {
    // (q + 1) / 4, little-endian u32 limbs
    const uint32_t E[8] = {0xb61f3f52u, 0x4f082305u, 0x5a1c72a3u, 0x65e05aa4u,
                           0xa0605617u, 0x6e14116du, 0xb84c680au, 0x0c19139cu};
    Fq y = fp_one<FqParams>();
    for (int bit = 253; bit >= 0; bit--) {
        y = fp_sqr(y);
        if ((E[bit >> 5] >> (bit & 31)) & 1) y = fp_mul(y, rhs);
    }
    return y;
}

__global__ void __launch_bounds__(256) k_points_decompress(const uint32_t* bytes, size_t n, Affine* out, uint32_t* bad) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Fq x;
    uint32_t any = 0;
#pragma unroll
    for (int k = 0; k < 8; k++) {
        x.l[k] = bytes[8 * i + k];
        any |= x.l[k];
    }
    Fq zero = fp_zero<FqParams>();
    if (any == 0) {  // identity
        fp_store(&out[i].x, zero);
        fp_store(&out[i].y, zero);
        return;
    }
    const uint32_t sign = x.l[7] >> 31;
    x.l[7] &= 0x7fffffffu;
    // x must be a canonical residue (< q)
    bool lt = false, decided = false;
#pragma unroll
    for (int k = 7; k >= 0; k--) {
        if (!decided && x.l[k] != FqParams::MOD[k]) {
            lt = x.l[k] < FqParams::MOD[k];
            decided = true;
        }
    }
    if (!lt) {
        atomicAdd(bad, 1u);
        fp_store(&out[i].x, zero);
        fp_store(&out[i].y, zero);
        return;
    }
    Fq xm = fp_to_mont(x);
    Fq three = fp_add(fp_add(fp_one<FqParams>(), fp_one<FqParams>()), fp_one<FqParams>());
    Fq rhs = fp_add(fp_mul(fp_sqr(xm), xm), three);
    Fq y = fq_sqrt_candidate(rhs);
    if (!fp_eq(fp_sqr(y), rhs)) {  // x is not the abscissa of a curve point
        atomicAdd(bad, 1u);
        fp_store(&out[i].x, zero);
        fp_store(&out[i].y, zero);
        return;
    }
    if ((fp_from_mont(y).l[0] & 1u) != sign) y = fp_neg(y);
    fp_store(&out[i].x, xm);
    fp_store(&out[i].y, y);
}

__global__ void __launch_bounds__(256) k_points_compress(const Affine* pts, size_t n, uint32_t* bytes) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Affine p = affine_load(pts + i);
    Fq x = fp_from_mont(p.x), y = fp_from_mont(p.y);
    if (fp_is_zero(x) && fp_is_zero(y)) {
#pragma unroll
        for (int k = 0; k < 8; k++) bytes[8 * i + k] = 0;
        return;
    }
    x.l[7] |= (y.l[0] & 1u) << 31;
#pragma unroll
    for (int k = 0; k < 8; k++) bytes[8 * i + k] = x.l[k];
}

int points_decompress_launch(const void* d_bytes, size_t n, uint64_t* d_out, uint32_t* d_bad, hipStream_t stream) {
    if (n == 0) return H2_OK;
    H2_HIP(hipMemsetAsync(d_bad, 0, 4, stream));
    hipLaunchKernelGGL(k_points_decompress, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream,
                       (const uint32_t*)d_bytes, n, (Affine*)d_out, d_bad);
    H2_HIP(hipGetLastError());
    uint32_t bad = 0;
    H2_HIP(hipMemcpyAsync(&bad, d_bad, 4, hipMemcpyDeviceToHost, stream));
    H2_HIP(hipStreamSynchronize(stream));
    if (bad) {
        set_last_error("points_decompress: " + std::to_string(bad) + " encoding(s) are not curve points");
        return H2_ERR_INVALID;
    }
    return H2_OK;
}

int points_compress_launch(const uint64_t* d_points, size_t n, void* d_bytes, hipStream_t stream) {
    if (n == 0) return H2_OK;
    hipLaunchKernelGGL(k_points_compress, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream,
                       (const Affine*)d_points, n, (uint32_t*)d_bytes);
    H2_HIP(hipGetLastError());
    return H2_OK;
}

// ---------------------------------------------------------------- fixed-base multiplication (Params::unsafe_setup)
// out[i] = [scalars[i]] B for one base B given as the table T[j] = [2^j] B, j < 254 (affine): the setup's
// g[i] = [s^i] G and g_lagrange[i] = [l_i(s)] G (poly/commitment.rs:67-112, a rayon `parallelize` with one variable-
// base multiplication per point there).  One lane per point: ~127 mixed additions against the shared table (every
// lane reads the same entry: a broadcast), then one Fq inversion (a^(q-2)) to normalise.
__global__ void __launch_bounds__(256) k_fixed_base_mul(const Fr* scalars, const Affine* table, size_t n, Affine* out) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const Fr s = fp_from_mont(fp_load(scalars + i));
    XYZZ acc = xyzz_identity();
#pragma unroll 1
    for (int bit = 0; bit < 254; bit++)
        if ((s.l[bit >> 5] >> (bit & 31)) & 1) acc = xyzz_madd(acc, affine_load(table + bit), false);
    Fq zero = fp_zero<FqParams>();
    if (fp_is_zero(acc.zz)) {  // scalar 0: the identity
        fp_store(&out[i].x, zero);
        fp_store(&out[i].y, zero);
        return;
    }
    // x = X / ZZ, y = Y / ZZZ with one inversion: t = 1 / ZZZ, 1 / ZZ = (ZZ * t)^2  (ZZ^3 = ZZZ^2)
    const Fq t = fq_inv_device(acc.zzz);
    const Fq u = fp_mul(acc.zz, t);
    fp_store(&out[i].x, fp_mul(acc.x, fp_sqr(u)));
    fp_store(&out[i].y, fp_mul(acc.y, t));
}

int fixed_base_mul_launch(const Fr* d_scalars, const uint64_t* d_table, size_t n, uint64_t* d_out, hipStream_t stream) {
    if (n == 0) return H2_OK;
    hipLaunchKernelGGL(k_fixed_base_mul, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, d_scalars,
                       (const Affine*)d_table, n, (Affine*)d_out);
    H2_HIP(hipGetLastError());
    return H2_OK;
}

// ---------------------------------------------------------------- folds of partial points
// Device-side fold of gathered partial points (one proof over several ranks): points[r * count + j] = rank r's partial of
// MSM j (Jacobian, 96 B), out[j] = sum over r in rank order -- the `.reduce(|acc, x| acc + x)` of arithmetic.rs:433-435
// after an all-gather, without bringing world x count points back to the host.  One lane per MSM (count is ~10).
__global__ void __launch_bounds__(64) k_g1_fold(const Jacobian* points, uint32_t world, uint32_t count, Jacobian* out) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= count) return;
    XYZZ acc = xyzz_identity();
    for (uint32_t r = 0; r < world; r++) {
        const Jacobian p = points[(size_t)r * count + j];
        acc = xyzz_add(acc, jacobian_to_xyzz(p));
    }
    out[j] = xyzz_to_jacobian(acc);
}

int g1_fold_launch(const uint64_t* d_points, uint32_t world, uint32_t count, uint64_t* d_out, hipStream_t stream) {
    if (count == 0) return H2_OK;
    hipLaunchKernelGGL(k_g1_fold, dim3((count + 63) / 64), dim3(64), 0, stream, (const Jacobian*)d_points, world, count,
                       (Jacobian*)d_out);
    H2_HIP(hipGetLastError());
    return H2_OK;
}

// host fold of `count` Jacobian points (12 x u64 each) -- the `reduce(|acc, x| acc + x)` of
// arithmetic.rs:434 and the local add after an all-gather of per-rank partial points.
void g1_sum_host(const uint64_t* points, size_t count, uint64_t out_xyz[12]) {
    XYZZ acc = xyzz_identity();
    for (size_t p = 0; p < count; p++) {
        Jacobian j;
        memcpy(&j, points + 12 * p, 96);
        acc = xyzz_add(acc, jacobian_to_xyzz(j));
    }
    Jacobian j = xyzz_to_jacobian(acc);
    memcpy(out_xyz, &j, 96);
}
}  // namespace h2
