// g1ntt.hip -- the NTT over G1 (g1ntt.hpp): Params' Lagrange basis from the powers alone.
//
// Products per butterfly, with ec.hpp's operation counts (doubling 9, XYZZ addition 14): the twiddle w^e is read from the
// plan's two-level tables (one product; none up to 2^12 points) and taken out of Montgomery form (one); [w] B is MSB-first
// double-and-add over the XYZZ operand, 9 (bits(w) - 1) + 14 (popcount(w) - 1); A + wB and A - wB are two additions (28).
// About 9 x 253 + 14 x 126 + 30 = 4.1e3 for a 254-bit twiddle; w = 1 (e = 0, all of stage 0) skips the multiplication.
// The inverse's n^-1 is applied as the points are bit-reversed into the scratch: MSB-first double-and-add against the affine
// input, 9 (bits - 1) + 10 (popcount - 1) per point (mixed additions).  The normalisation spends one a^(q - 2) per point
// (254 squarings + 127 products) and 4 more.  tools/g1_ntt_bench.py counts the same way.
//
// Lanes and twiddles.  Butterfly t of the stage with half-size m = 2^s and nb = n / 2m blocks is position p = t / nb of block
// b = t % nb, twiddle exponent e = p nb = t & -nb.  With nb >= 64 the 64 lanes of a wave are 64 blocks at the same p: the
// twiddle and every branch of the double-and-add are the same on all lanes and the scalar sits in SGPRs
// (k_g1ntt_stage<true>).  The last min(6, log_n) stages have fewer blocks: lanes hold different twiddles and the wave issues
// each doubling and addition that any of its lanes needs (k_g1ntt_stage<false>).
//
// Exceptional cases are the complete formulas' of ec.hpp (identity operands, A = wB, A = -wB): the results are exact group
// elements, normalised to the one affine form (identity (0, 0)).
#include "ec.hpp"
#include "g1ntt.hpp"
#include "ntt.hpp"

namespace h2 {
namespace {

constexpr uint32_t G1NTT_BLOCK = 256;
constexpr uint32_t G1NTT_MAX_LOG = 28;   // the 2-adicity of Fr
constexpr uint32_t TW_LO_BITS = 12;      // the plan's tables: w^e = tw_lo[e & 4095] tw_hi[e >> 12] (ntt.hip LO_BITS)
constexpr uint32_t WAVE_LOG = 6;
// the 2^28-th root of unity of EvaluationDomain::new (BN254 Fr ROOT_OF_UNITY), canonical, little-endian
constexpr uint64_t ROOT_OF_UNITY[4] = {0xd34f1ed960c37c9cull, 0x3215cf6dd39329c8ull, 0x98865ea93dd31f74ull,
                                       0x03ddb9f5166d18b7ull};

int invalid(const char* msg) {
    set_last_error(std::string("h2_dev_g1_ntt: ") + msg);
    return H2_ERR_INVALID;
}

// k <<= 1 over 256 bits.  The scalar loops test bit 255 and shift: static limb indices (a runtime-indexed bit test would put
// the scalar in scratch).
H2_DEV void shl1(Fr& k) {
#pragma unroll
    for (int i = 7; i > 0; i--) k.l[i] = (k.l[i] << 1) | (k.l[i - 1] >> 31);
    k.l[0] <<= 1;
}

// [k] b for a plain (not Montgomery) scalar k, MSB first.  Up to the top set bit the accumulator is the identity, which
// xyzz_double and xyzz_add pass through without a product.
__device__ __forceinline__ XYZZ xyzz_mul_scalar(const XYZZ& b, Fr k) {
    XYZZ acc = xyzz_identity();
#pragma unroll 1
    for (int i = 0; i < 256; i++) {
        acc = xyzz_double(acc);
        if (k.l[7] >> 31) acc = xyzz_add(acc, b);
        shl1(k);
    }
    return acc;
}

// [k] p for an affine p (mixed additions)
__device__ __forceinline__ XYZZ affine_mul_scalar(const Affine& p, Fr k) {
    XYZZ acc = xyzz_identity();
#pragma unroll 1
    for (int i = 0; i < 256; i++) {
        acc = xyzz_double(acc);
        if (k.l[7] >> 31) acc = xyzz_madd(acc, p, false);
        shl1(k);
    }
    return acc;
}

// a^(q - 2): per-lane inversions of different values (fp_inv's branches would serialise across the wave; k_fixed_base_mul
// normalises the same way)
__device__ __forceinline__ Fq fq_inv_pow(const Fq& a) {
    const uint32_t E[8] = {0xd87cfd45u, 0x3c208c16u, 0x6871ca8du, 0x97816a91u,
                           0x8181585du, 0xb85045b6u, 0xe131a029u, 0x30644e72u};  // q - 2
    Fq acc = fp_one<FqParams>();
#pragma unroll 1
    for (int bit = 253; bit >= 0; bit--) {
        acc = fp_sqr(acc);
        if ((E[bit >> 5] >> (bit & 31)) & 1) acc = fp_mul(acc, a);
    }
    return acc;
}

// work[bitrev(i)] = [scale] in[i]   (scaled = 0: the point as it is)
__global__ void __launch_bounds__(G1NTT_BLOCK) k_g1ntt_load(const Affine* in, uint32_t log_n, Fr scale, uint32_t scaled,
                                                             XYZZ* work) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (1u << log_n)) return;
    const Affine p = affine_load(in + i);
    const uint32_t j = log_n ? __brev(i) >> (32 - log_n) : 0u;
    xyzz_store(work + j, scaled ? affine_mul_scalar(p, scale) : xyzz_from_affine(p, false));
}

// one radix-2 stage of half-size 2^s: butterflies t < n / 2
template <bool UNIFORM>
__global__ void __launch_bounds__(G1NTT_BLOCK) k_g1ntt_stage(XYZZ* work, uint32_t log_n, uint32_t s, const Fr* tw_lo,
                                                              const Fr* tw_hi) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (1u << (log_n - 1))) return;
    const uint32_t nb_log = log_n - 1 - s;
    const uint32_t b = t & ((1u << nb_log) - 1);
    uint32_t e = t & ~((1u << nb_log) - 1);
    if (UNIFORM) e = __builtin_amdgcn_readfirstlane(e);  // nb >= 64: one block position per wave
    const uint32_t p = e >> nb_log;
    XYZZ* const pa = work + (((size_t)b << (s + 1)) + p);
    XYZZ* const pb = pa + (1u << s);
    XYZZ wb = xyzz_load(pb);
    if (e != 0) {
        Fr w = log_n <= TW_LO_BITS
                   ? fp_load(tw_lo + e)
                   : fp_mul(fp_load(tw_lo + (e & ((1u << TW_LO_BITS) - 1))), fp_load(tw_hi + (e >> TW_LO_BITS)));
        w = fp_from_mont(w);
        if (UNIFORM) {
#pragma unroll
            for (int i = 0; i < 8; i++) w.l[i] = __builtin_amdgcn_readfirstlane(w.l[i]);
        }
        wb = xyzz_mul_scalar(wb, w);
    }
    const XYZZ a = xyzz_load(pa);
    XYZZ neg = wb;
    neg.y = fp_neg(wb.y);
    xyzz_store(pa, xyzz_add(a, wb));
    xyzz_store(pb, xyzz_add(a, neg));
}

// out[i] = work[i] as affine: x = X / ZZ, y = Y / ZZZ with one inversion (t = 1 / ZZZ, 1 / ZZ = (ZZ t)^2 since ZZ^3 = ZZZ^2)
__global__ void __launch_bounds__(G1NTT_BLOCK) k_g1ntt_normalize(const XYZZ* work, uint32_t log_n, Affine* out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (1u << log_n)) return;
    const XYZZ a = xyzz_load(work + i);
    if (xyzz_is_identity(a)) {
        const Fq zero = fp_zero<FqParams>();
        fp_store(&out[i].x, zero);
        fp_store(&out[i].y, zero);
        return;
    }
    const Fq t = fq_inv_pow(a.zzz);
    const Fq u = fp_mul(a.zz, t);
    fp_store(&out[i].x, fp_mul(a.x, fp_sqr(u)));
    fp_store(&out[i].y, fp_mul(a.y, t));
}

}  // namespace

size_t g1_ntt_scratch_bytes(uint32_t log_n) { return log_n > G1NTT_MAX_LOG ? 0 : sizeof(XYZZ) << log_n; }

int g1_ntt_args(const void* d_in, const void* d_out, uint32_t log_n, int inverse, const void* d_scratch, size_t scratch_bytes) {
    if (log_n > G1NTT_MAX_LOG) return invalid("log_n exceeds the 2-adicity of Fr (28)");
    if (inverse != 0 && inverse != 1) return invalid("inverse must be 0 or 1");
    if (!d_in || !d_out || !d_scratch) return invalid("null argument");
    if (scratch_bytes < g1_ntt_scratch_bytes(log_n)) return invalid("scratch smaller than h2_g1_ntt_scratch_bytes(log_n)");
    return H2_OK;
}

int g1_ntt_launch(DeviceCtx* ctx, const uint64_t* d_in, uint64_t* d_out, uint32_t log_n, bool inverse, void* d_scratch,
                  hipStream_t stream) {
    const uint32_t n = 1u << log_n;
    XYZZ* const work = (XYZZ*)d_scratch;
    // w = ROOT_OF_UNITY^(2^(28 - log_n)) and n^-1, host products in Montgomery form
    Fr w = fp_to_mont(fr_from_u64x4(ROOT_OF_UNITY));
    for (uint32_t i = log_n; i < G1NTT_MAX_LOG; i++) w = fp_sqr(w);
    if (inverse) w = fp_inv(w);
    Fr n_plain = fp_zero<FrParams>();
    n_plain.l[0] = n;
    const Fr n_inv = fp_from_mont(fp_inv(fp_to_mont(n_plain)));  // plain: the scalar loop scans its bits
    const uint32_t scaled = inverse && log_n > 0 ? 1u : 0u;
    const unsigned grid = (n + G1NTT_BLOCK - 1) / G1NTT_BLOCK;
    hipLaunchKernelGGL(k_g1ntt_load, dim3(grid), dim3(G1NTT_BLOCK), 0, stream, (const Affine*)d_in, log_n, n_inv, scaled,
                       work);
    if (log_n >= 1) {
        PlanRef pl;  // twiddles other than 1 exist from 4 points on; the plan stays pinned until the stages are launched
        const Fr* tw_lo = nullptr;
        const Fr* tw_hi = nullptr;
        if (log_n >= 2) {
            uint64_t om[4];
            fr_to_u64x4(w, om);
            pl = ntt_get_plan(ctx, log_n, om, stream);
            tw_lo = pl->tw_lo;
            tw_hi = pl->tw_hi;
        }
        const unsigned half_grid = ((n >> 1) + G1NTT_BLOCK - 1) / G1NTT_BLOCK;
        for (uint32_t s = 0; s < log_n; s++) {
            if (log_n - 1 - s >= WAVE_LOG)
                hipLaunchKernelGGL(k_g1ntt_stage<true>, dim3(half_grid), dim3(G1NTT_BLOCK), 0, stream, work, log_n, s, tw_lo,
                                   tw_hi);
            else
                hipLaunchKernelGGL(k_g1ntt_stage<false>, dim3(half_grid), dim3(G1NTT_BLOCK), 0, stream, work, log_n, s, tw_lo,
                                   tw_hi);
        }
        H2_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(k_g1ntt_normalize, dim3(grid), dim3(G1NTT_BLOCK), 0, stream, (const XYZZ*)work, log_n, (Affine*)d_out);
    H2_HIP(hipGetLastError());
    return H2_OK;
}

}  // namespace h2
