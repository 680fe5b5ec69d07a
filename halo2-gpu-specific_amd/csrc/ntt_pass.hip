// ntt_pass.hip -- the device code of the radix-2^B multi-pass NTT over BN254 Fr for gfx950: the table-fill kernels, the two
// pass kernels and their launcher (ntt_pass.hpp).  The schedule, the plans and the table cache are ntt.hip.
//
// Replaces ec-gpu-gen's `SingleFftKernel::{radix_fft, radix_ifft}` (called from
// /root/reference/halo2_proofs/src/arithmetic.rs:495-534) and the device-resident driver
// `do_fft_core` (plonk/evaluation_gpu.rs:976-1052); semantics are those of the CPU twin
// `best_fft_cpu` (arithmetic.rs:556-645): natural order in, natural order out,
// X[k] = sum_j x[j] * omega^(j*k).
//
// Decomposition (not the reference's): n = R_0 * R_1 * ... * R_{P-1}, R_p = 2^{B_p} <= 2^9.
//   input index   j = sum_p j_p * S_p,   S_p = 2^(L - B_0 - ... - B_p)   (j_0 most significant)
//   output index  k = sum_p k_p * T_p,   T_p = 2^(B_0 + ... + B_{p-1})   (k_0 least significant)
// Pass p replaces digit j_p by k_p *in place* (an R_p-point DFT along stride S_p) after
// multiplying element j_p by omega^(j_p * S_p * K_{p-1}), K_{p-1} = sum_{q<p} k_q T_q.
// The last pass reads R_{P-1} contiguous elements per DFT and scatters to the natural output
// order, so it is out of place; tiles hold C DFTs with consecutive K so both the loads
// (contiguous rows) and the stores (C consecutive outputs) are coalesced.
// One workgroup = one LDS tile of R_p x C elements (32 B each); butterflies are radix-2
// DIT on bit-reversed rows, twiddles w_R^e from a per-pass LDS table.
//
// Fused into the passes (so the reference's separate kernels/loops disappear):
//   * zero padding  (eval_fft_prepare, evaluation_gpu.rs:890-900; domain.rs:280)
//   * zeta-power coset pre-scale (distribute_powers_zeta, domain.rs:382-398)
//   * 1/n and zeta^-1 post-scale (domain.rs:404-409, :341)
#include <stdexcept>

#include "ntt_pass.hpp"

namespace h2 {

// ---------------------------------------------------------------- table generation
// A twiddle table in one of four forms.  pair = 0: out[i] = w, Montgomery form (the operand of fp_mul / fp_mul_wide).
// pair = 1: out[2 i] = w as a PLAIN residue, out[2 i + 1] = floor(w 2^256 / r) -- the operands of fp_mul_const (field.hpp), the
// constant-operand product the passes with CW use for every twiddle they read from a table.
// pair = 2: entry i (sizeof(TwChunk) bytes) = w's chunk residues, limb-major -- the operand of fp_mul_chunk, which the fixed
// pass (k_ntt_pass8) uses for its butterfly twiddles.
// pair = 3: entry i (sizeof(TwChunk32) bytes) = w's eight residues w 2^(32 j) 2^64 mod r, limb-major -- the operand of
// fp_mul_chunk_planes, which k_ntt_pass8 uses for its wave-uniform twiddles.
__device__ __forceinline__ void tw_store(Fr* out, uint32_t i, const Fr& w_mont, uint32_t pair) {
    if (!pair) {
        fp_store(out + i, w_mont);
        return;
    }
    if (pair == 2) {
        TwChunk t;
        fp_chunk_table(w_mont, t);
        uint4* const q = reinterpret_cast<uint4*>(out) + (size_t)i * TW_CHUNK_Q;
#pragma unroll
        for (uint32_t k = 0; k < TW_CHUNK_Q; k++) q[k] = make_uint4(t.w[4 * k], t.w[4 * k + 1], t.w[4 * k + 2], t.w[4 * k + 3]);
        return;
    }
    if (pair == 3) {
        TwChunk32 t;
        fp_chunk_table(w_mont, t);
        uint4* const q = reinterpret_cast<uint4*>(out) + (size_t)i * TW_CHUNK32_Q;
#pragma unroll
        for (uint32_t k = 0; k < TW_CHUNK32_Q; k++) q[k] = make_uint4(t.w[4 * k], t.w[4 * k + 1], t.w[4 * k + 2], t.w[4 * k + 3]);
        return;
    }
    Fr w, q;
    fp_const_pair(w_mont, w, q);
    fp_store(out + 2 * (size_t)i, w);
    fp_store(out + 2 * (size_t)i + 1, q);
}

// out[i] = base^(i * mul)   (i < count)
__global__ void __launch_bounds__(256) k_pow_table(Fr* out, Fr base, uint32_t mul, uint32_t count, uint32_t pair) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    // base^(i*mul): exponent < 2^28 always (order of omega divides 2^28)
    tw_store(out, i, fp_pow_u32(base, i * mul), pair);
}

// out[(rho << kbits) | K] = base^((rho * K << s_log) mod n)   -- the complete inter-pass twiddle set of a pass
__global__ void __launch_bounds__(256) k_direct_table(Fr* out, Fr base, uint32_t kbits, uint32_t s_log, uint32_t log_n,
                                                      uint32_t count, uint32_t pair) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    uint32_t rho = i >> kbits, K = i & ((1u << kbits) - 1);
    uint32_t e = (uint32_t)(((uint64_t)rho * K) << s_log) & ((1u << log_n) - 1);
    tw_store(out, i, fp_pow_u32(base, e), pair);
}

// out[(K << bits) | rho] = base^((rho * K) mod n) (* d when `scale`): the last pass's inter-pass twiddles in load order
__global__ void __launch_bounds__(256) k_last_table(Fr* out, Fr base, uint32_t bits, uint32_t log_n, Fr d, uint32_t scale,
                                                    uint32_t pair) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;  // grid covers 2^log_n exactly (log_n >= 8)
    const uint32_t rho = i & ((1u << bits) - 1), K = i >> bits;
    const uint32_t e = (uint32_t)((uint64_t)rho * K) & ((1u << log_n) - 1);
    Fr w = fp_pow_u32(base, e);
    if (scale) w = fp_mul(w, d);
    tw_store(out, i, w, pair);
}

// out[i] = in[i] * d
__global__ void __launch_bounds__(256) k_scale_table(Fr* out, const Fr* in, Fr d, uint32_t count) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < count) fp_store(out + i, fp_mul(fp_load(in + i), d));
}

// ---------------------------------------------------------------- the pass kernel
__device__ __forceinline__ uint32_t bitrev(uint32_t x, uint32_t bits) {
    return bits == 0 ? 0u : (__brev(x) >> (32 - bits));
}

// hi (digits k_0..k_{p-1}, k_0 most significant) -> K = sum k_q << T_q
__device__ __forceinline__ uint32_t hi_to_K(uint32_t hi, const PassArgs& a) {
    uint32_t K = 0;
    for (int q = (int)a.nprev - 1; q >= 0; q--) {
        uint32_t d = hi & ((1u << a.prevB[q]) - 1);
        hi >>= a.prevB[q];
        K |= d << a.prevT[q];
    }
    return K;
}
__device__ __forceinline__ uint32_t K_to_hi(uint32_t K, const PassArgs& a) {
    uint32_t hi = 0;
    for (uint32_t q = 0; q < a.nprev; q++) {
        uint32_t d = (K >> a.prevT[q]) & ((1u << a.prevB[q]) - 1);
        hi = (hi << a.prevB[q]) | d;
    }
    return hi;
}

__device__ __forceinline__ Fr twiddle_pow(const PassArgs& a, uint32_t e) {
    if (a.log_n <= LO_BITS) return fp_load(a.tw_lo + e);
    Fr lo = fp_load(a.tw_lo + (e & ((1u << LO_BITS) - 1)));
    Fr hi = fp_load(a.tw_hi + (e >> LO_BITS));
    return fp_mul(lo, hi);
}

extern __shared__ __attribute__((aligned(16))) uint4 h2_smem[];

// LDS tiles keep the two 16-byte halves of an element in separate planes: a wave then reads 16 B at a
// 16-B lane stride (conflict-free ds_read_b128) instead of 16 B at a 32-B stride (2-way conflicts).
__device__ __forceinline__ Fr lds_get(const uint4* lo, const uint4* hi, uint32_t i) {
    uint4 a = lo[i], b = hi[i];
    Fr r;
    r.l[0] = a.x; r.l[1] = a.y; r.l[2] = a.z; r.l[3] = a.w;
    r.l[4] = b.x; r.l[5] = b.y; r.l[6] = b.z; r.l[7] = b.w;
    return r;
}
__device__ __forceinline__ void lds_put(uint4* lo, uint4* hi, uint32_t i, const Fr& v) {
    lo[i] = make_uint4(v.l[0], v.l[1], v.l[2], v.l[3]);
    hi[i] = make_uint4(v.l[4], v.l[5], v.l[6], v.l[7]);
}

// Every pass works in the lazy domain of field.hpp -- values below 4p in LDS and between the passes, products by fp_mul_wide
// (no final subtraction), bare additions; canonical residues come back at the last pass's store.
// CW (the radix-4 passes): the butterfly twiddles in LDS are (plain value, quotient) pairs and multiply by fp_mul_const: 115
// multiply-adds per product instead of 136 (field.hpp).  Twiddles COMPOSED at run time (lo x hi of the two-level tables, the
// coset scales, pre3 / post3) stay Montgomery products, and so does the LAST pass's complete table (tw_direct): as pairs it is
// 64 B per element streamed from HBM next to the 64 B of data, and the pass -- 2.1 GB per launch at 2^24 -- stopped following
// its instruction count (590 us either way, profiles/r6_ntt_constw.txt).
// NLAST: a pass before the last, known when the kernel is compiled (the last pass's table, scales and scatter are not in it).
// ST: the pass after this one has its inter-pass twiddles tabulated (PassArgs::nx_tab) and this pass multiplies by them where
// it stores, so that pass loads finished operands (tw_applied).  The product is the same wherever it runs; a first pass waits
// for rows 2 MiB apart and has issue slots to spare, the middle pass is bound by issue (measured).  At the store
// the entries a tile needs are consecutive in the table's own order, which is what makes the chunk form (128 B per entry)
// affordable: store_twiddle below.
__device__ __forceinline__ Fr store_twiddle(const PassArgs& a, const Fr& y, const uint32_t entry) {
    const uint4* const q = reinterpret_cast<const uint4*>(a.nx_tab) + (size_t)entry * TW_CHUNK_Q;
    TwChunk t;
#pragma unroll
    for (uint32_t k = 0; k < TW_CHUNK_Q; k++) {
        const uint4 v = q[k];
        t.w[4 * k] = v.x; t.w[4 * k + 1] = v.y; t.w[4 * k + 2] = v.z; t.w[4 * k + 3] = v.w;
    }
    // any 256-bit y (k_ntt_pass hands on values below 4p) -> below p (1 + 2^-29); fp_chunk_handover, which every store with
    // ST ends with, makes it the canonical residue: what the next pass's first butterflies take as they are (k_ntt_pass8:
    // bare sums, FIRST_PAIR_CANON; k_ntt_pass: fp_lazy_red2p hands them back)
    return fp_mul_chunk(y, t);
}

template <bool RADIX4, bool NLAST = false, bool ST = false>
__global__ void __launch_bounds__(512, 4) k_ntt_pass(PassArgs a) {
    constexpr bool CW = RADIX4;
    static_assert(!ST || NLAST || !RADIX4, "a last pass stores the transform's output");
    const bool is_last = NLAST ? false : a.is_last != 0;
    // x * w for a canonical twiddle w: any x < 2^256 -> a value below 2p
    auto tmul = [](const Fr& x, const Fr& w) -> Fr { return fp_mul_wide(x, w); };
    const uint32_t B = a.B, R = 1u << B, log_c = a.log_c, C = 1u << log_c;
    const uint32_t zskip = a.zskip;
    uint4* t_lo = h2_smem;                  // R*C low halves
    uint4* t_hi = t_lo + (R << log_c);      // R*C high halves
    uint4* w_lo = t_hi + (R << log_c);      // R/2 butterfly twiddles, low / high halves
    uint4* w_hi = w_lo + (R >> 1) + (CW ? 0 : 1);
    // CW: two more planes for the quotients, no padding: a 256 x 4 tile + 128 pairs is 40 KiB exactly, four workgroups per CU
    uint4* q_lo = w_hi + (R >> 1);
    uint4* q_hi = q_lo + (R >> 1);
    // x * (butterfly twiddle i)
    struct Tw {
        Fr w, q;
    };
    auto tw_get = [&](uint32_t i) __attribute__((always_inline)) -> Tw {
        Tw t;
        t.w = lds_get(w_lo, w_hi, i);
        if constexpr (CW) t.q = lds_get(q_lo, q_hi, i);
        return t;
    };
    auto bmul = [](const Fr& x, const Tw& t) __attribute__((always_inline)) -> Fr {
        if constexpr (CW) return fp_mul_const(x, t.w, t.q);
        else return fp_mul_wide(x, t.w);
    };
    const uint32_t nthreads = blockDim.x;  // == max(R/2 * C, 1) (RADIX4: half)
    const uint32_t tid = threadIdx.x;
    const Fr* const in_p = a.batch ? a.in_b[blockIdx.y] : a.in;   // (wave-uniform: scalar loads from the kernel arguments)
    Fr* const out_p = a.batch ? a.out_b[blockIdx.y] : a.out;
    const uint32_t n_mask = (a.log_n >= 32) ? 0xffffffffu : ((1u << a.log_n) - 1);

    for (uint32_t i = tid; i < (R >> 1); i += nthreads) {
        if constexpr (CW) {
            lds_put(w_lo, w_hi, i, fp_load(a.tw_bfly + 2 * i));
            lds_put(q_lo, q_hi, i, fp_load(a.tw_bfly + 2 * i + 1));
        } else {
            lds_put(w_lo, w_hi, i, fp_load(a.tw_bfly + i));
        }
    }

    const uint32_t tile_id = blockIdx.x;
    const uint32_t total = R << log_c;

    // ---- tile geometry
    uint32_t base = 0, K_uniform = 0;
    const uint32_t S = 1u << a.s_log;
    if (!is_last) {
        // tiles: for each hi, for each chunk of C consecutive low positions
        uint32_t chunks_per_hi = S >> log_c;
        uint32_t hi = tile_id / chunks_per_hi, lo0 = (tile_id % chunks_per_hi) << log_c;
        base = (hi << (B + a.s_log)) + lo0;
        K_uniform = hi_to_K(hi, a);
    }

    // ---- load (+ zero pad, coset pre-scale, inter-pass twiddle), bit-reversed rows into LDS.
    // A lane's NE elements are fetched as ONE batch -- every global load (the elements, then their twiddles) is issued
    // before the first product needs one -- so a tile pays one memory latency, not one per element (the rows of an early
    // pass are 2 MiB apart: each of those loads is a DRAM page of its own).
    constexpr uint32_t NE = RADIX4 ? 4 : 2;
    for (uint32_t e0 = tid; e0 < total; e0 += NE * nthreads) {
        uint32_t rho[NE], col[NE], idx[NE], Kk[NE];
        bool live[NE];
        Fr x[NE];
#pragma unroll
        for (uint32_t q = 0; q < NE; q++) {
            const uint32_t e = e0 + q * nthreads;
            if (!is_last) {
                col[q] = e & (C - 1);
                rho[q] = (e >> log_c) & (R - 1);
                idx[q] = base + (rho[q] << a.s_log) + col[q];
                Kk[q] = K_uniform;
            } else {
                rho[q] = e & (R - 1);
                col[q] = (e >> B) & (C - 1);
                Kk[q] = (tile_id << log_c) + col[q];
                idx[q] = (K_to_hi(Kk[q], a) << B) + rho[q];
            }
            // Zero padding by 2^z (coeff_to_extended): the rows rho >= R >> z of the first pass are zero, so its first z
            // stages are butterflies (u, 0) -> (u, u) whatever the twiddle: each loaded element is written to the 2^z rows
            // those stages would copy it to (the low z bits of the bit-reversed row index) and the stage loop starts at z.
            live[q] = e < total && !(zskip && rho[q] >= (R >> zskip));
        }
#pragma unroll
        for (uint32_t q = 0; q < NE; q++) {
            x[q] = fp_zero<FrParams>();
            if (live[q] && idx[q] < a.in_len) x[q] = fp_load(in_p + idx[q]);
        }
        if (a.has_pre3) {
#pragma unroll
            for (uint32_t q = 0; q < NE; q++) {
                const uint32_t m = idx[q] % 3;
                Fr w;
#pragma unroll
                for (int l = 0; l < 8; l++) w.l[l] = m == 1 ? a.pre3[1].l[l] : a.pre3[2].l[l];
                if (m != 0) x[q] = tmul(x[q], w);
            }
        }
        const bool pre_scale = a.scale_mode == 1u && a.nprev == 0;
        if ((a.nprev != 0 && !a.tw_applied) || pre_scale) {
            // omega^(rho * S * K); a unit twiddle (rho = 0 or K = 0) multiplies like any other: the tables hold it
            // (tw_applied: the pass before this one multiplied by it at its store)
            if (!NLAST && a.tw_direct != nullptr && !pre_scale) {   // (the last pass's table)
#pragma unroll
                for (uint32_t q0 = 0; q0 < NE; q0 += 2) {
                    Fr w[2];
#pragma unroll
                    for (uint32_t q = 0; q < 2; q++) w[q] = fp_load(a.tw_direct + ((Kk[q0 + q] << B) | rho[q0 + q]));
#pragma unroll
                    for (uint32_t q = 0; q < 2; q++) x[q0 + q] = tmul(x[q0 + q], w[q]);
                }
            } else if (a.log_n <= LO_BITS && !pre_scale) {
#pragma unroll
                for (uint32_t q = 0; q < NE; q++) {
                    const uint32_t ex = (uint32_t)(((uint64_t)rho[q] * Kk[q]) << a.s_log) & n_mask;
                    x[q] = tmul(x[q], fp_load(a.tw_lo + ex));
                }
            } else {
                // two at a time: 16 twiddle halves in flight next to the elements keeps the kernel within 128 VGPRs
                // (the coset pre-scale of a first pass, g^idx from its own two-level table, runs through the same code)
                const Fr* const two_lo = pre_scale ? a.sc_lo : a.tw_lo;
                const Fr* const two_hi = pre_scale ? a.sc_hi : a.tw_hi;
#pragma unroll
                for (uint32_t q0 = 0; q0 < NE; q0 += 2) {
                    Fr wl[2], wh[2];
#pragma unroll
                    for (uint32_t q = 0; q < 2; q++) {
                        const uint32_t ex = pre_scale ? (idx[q0 + q] & n_mask)
                                                      : ((uint32_t)(((uint64_t)rho[q0 + q] * Kk[q0 + q]) << a.s_log) & n_mask);
                        wl[q] = fp_load(two_lo + (ex & ((1u << LO_BITS) - 1)));
                        wh[q] = fp_load(two_hi + (ex >> LO_BITS));
                    }
#pragma unroll
                    for (uint32_t q = 0; q < 2; q++) x[q0 + q] = tmul(x[q0 + q], fp_mul(wl[q], wh[q]));
                }
            }
        }
#pragma unroll
        for (uint32_t q = 0; q < NE; q++) {
            // (row and column again from e: cheaper than keeping them in registers across the products)
            const uint32_t e = e0 + q * nthreads;
            const uint32_t r_q = is_last ? (e & (R - 1)) : ((e >> log_c) & (R - 1));
            const uint32_t c_q = is_last ? ((e >> B) & (C - 1)) : (e & (C - 1));
            if (e >= total || (zskip && r_q >= (R >> zskip))) continue;
            if (zskip) {
                for (uint32_t m = 0; m < (1u << zskip); m++) lds_put(t_lo, t_hi, ((bitrev(r_q, B) | m) << log_c) + c_q, x[q]);
            } else {
                lds_put(t_lo, t_hi, (bitrev(r_q, B) << log_c) + c_q, x[q]);
            }
        }
    }
    __syncthreads();

    // ---- B radix-2 DIT stages in LDS.  With `radix4` two consecutive stages share one round trip: a lane takes the four
    // rows p, p + h, p + 2h, p + 3h (h = 2^s, bits s and s + 1 of p clear), runs the two stage-s butterflies (one
    // twiddle, index r = p mod h, for both) and the two stage-(s+1) butterflies (indices r and r + h) in registers and
    // writes the four rows back: half the LDS instructions, address arithmetic and barriers of the stage-by-stage loop,
    // the same products on the same operands.
    uint32_t s0 = zskip;
    if constexpr (RADIX4) {
        const uint32_t nunits = total >> 2;
        auto round4 = [&](const uint32_t s) __attribute__((always_inline)) {
            const uint32_t h = 1u << s;
            const uint32_t log_per = (B - 2 + log_c) - s;  // units that share one r: 2^log_per
            const bool by_r = s != 0 && log_per >= 6 && (nthreads & 63) == 0;
            for (uint32_t t = tid; t < nunits; t += nthreads) {
                uint32_t c, r, p;
                if (by_r) {
                    r = t >> log_per;
                    const uint32_t j = t & ((1u << log_per) - 1);
                    c = j & (C - 1);
                    p = ((j >> log_c) << (s + 2)) | r;
                } else {
                    c = t & (C - 1);
                    const uint32_t b = t >> log_c;
                    r = b & (h - 1);
                    p = ((b >> s) << (s + 2)) | r;
                }
                const uint32_t i0 = (p << log_c) + c, step = h << log_c;
                Fr x0 = lds_get(t_lo, t_hi, i0), x1 = lds_get(t_lo, t_hi, i0 + step);
                Fr x2 = lds_get(t_lo, t_hi, i0 + 2 * step), x3 = lds_get(t_lo, t_hi, i0 + 3 * step);
                const bool unit = s == 0 || (by_r && r == 0);  // the twiddles of index r are 1 (wave-uniform test)
                // rows below 4p: the operands of a product go in as they are, the others are brought below 2p
                x0 = fp_lazy_red2p(x0);
                x2 = fp_lazy_red2p(x2);
                if (!unit) {
                    const Tw wa = tw_get(r << (B - 1 - s));
                    x1 = bmul(x1, wa);
                    x3 = bmul(x3, wa);
                } else {
                    x1 = fp_lazy_red2p(x1);
                    x3 = fp_lazy_red2p(x3);
                }
                const Fr y0 = fp_lazy_add_red(x0, x1), y1 = fp_lazy_sub_red(x0, x1);   // below 2p: added to next
                Fr y2 = fp_lazy_add(x2, x3), y3 = fp_lazy_sub(x2, x3);                  // below 4p: multiplied next
                y2 = unit ? fp_lazy_red2p(y2) : bmul(y2, tw_get(r << (B - 2 - s)));
                y3 = bmul(y3, tw_get((r + h) << (B - 2 - s)));
                lds_put(t_lo, t_hi, i0, fp_lazy_add(y0, y2));
                lds_put(t_lo, t_hi, i0 + 2 * step, fp_lazy_sub(y0, y2));
                lds_put(t_lo, t_hi, i0 + step, fp_lazy_add(y1, y3));
                lds_put(t_lo, t_hi, i0 + 3 * step, fp_lazy_sub(y1, y3));
            }
            __syncthreads();
        };
        for (; s0 + 1 < B; s0 += 2) round4(s0);
    }
    const uint32_t nbf = total >> 1;
    for (uint32_t s = s0; s < B; s++) {
        const uint32_t h = 1u << s;
        const uint32_t log_per = (B - 1 + log_c) - s;  // butterflies that share one twiddle index r: 2^log_per
        const bool by_r = s != 0 && log_per >= 6 && (nthreads & 63) == 0;
        for (uint32_t t = tid; t < nbf; t += nthreads) {
            uint32_t c, r, i;
            if (by_r) {
                // early stages: order the butterflies by twiddle index so r is uniform across a wave and the
                // r == 0 waves (twiddle 1) skip the multiplication: 1/2, 1/4, 1/8 ... of stages 1, 2, 3 ...
                r = t >> log_per;
                uint32_t j = t & ((1u << log_per) - 1);
                c = j & (C - 1);
                i = ((j >> log_c) << (s + 1)) | r;
            } else {
                c = t & (C - 1);
                uint32_t b = t >> log_c;
                r = b & (h - 1);
                i = ((b >> s) << (s + 1)) | r;
            }
            const uint32_t iu = (i << log_c) + c, iv = ((i + h) << log_c) + c;
            Fr u = lds_get(t_lo, t_hi, iu), v = lds_get(t_lo, t_hi, iv);
            const bool skip = s == 0 || (by_r && r == 0);
            u = fp_lazy_red2p(u);
            v = skip ? fp_lazy_red2p(v) : bmul(v, tw_get(r << (B - 1 - s)));
            lds_put(t_lo, t_hi, iu, fp_lazy_add(u, v));
            lds_put(t_lo, t_hi, iv, fp_lazy_sub(u, v));
        }
        __syncthreads();
    }

    // ---- store (+ post-scale on the final pass), batched like the loads
    for (uint32_t e0 = tid; e0 < total; e0 += NE * nthreads) {
        Fr y[NE];
        uint32_t idx[NE];
#pragma unroll
        for (uint32_t q = 0; q < NE; q++) {
            const uint32_t e = e0 + q * nthreads;
            const uint32_t c = e & (C - 1), k = (e >> log_c) & (R - 1);
            if (!is_last)
                idx[q] = base + (k << a.s_log) + c;
            else
                idx[q] = ((tile_id << log_c) + c) + (k << a.t_log);
            y[q] = lds_get(t_lo, t_hi, (k << log_c) + c);
        }
        if (is_last && a.scale_mode == 2u) {
            // one at a time: four results are live next to the two table halves and the product
#pragma unroll
            for (uint32_t q = 0; q < NE; q++) {
                const uint32_t i = idx[q] & n_mask;
                const Fr w = fp_mul(fp_load(a.sc_lo + (i & ((1u << LO_BITS) - 1))), fp_load(a.sc_hi + (i >> LO_BITS)));
                y[q] = fp_reduce_once(fp_mul_wide(y[q], w));
            }
        } else if (is_last && a.has_post3 && !a.hi_scaled) {
#pragma unroll
            for (uint32_t q = 0; q < NE; q++) {
                const uint32_t m = idx[q] % 3;
                Fr w;
#pragma unroll
                for (int l = 0; l < 8; l++) w.l[l] = m == 0 ? a.post3[0].l[l] : (m == 1 ? a.post3[1].l[l] : a.post3[2].l[l]);
                y[q] = fp_reduce_once(fp_mul_wide(y[q], w));
            }
        } else if (is_last) {
            // the transform's output is canonical (an intermediate pass hands its values on below 4p: the next pass's
            // inter-pass twiddle product takes them as they are)
#pragma unroll
            for (uint32_t q = 0; q < NE; q++) y[q] = fp_lazy_canon(y[q]);
        }
        if constexpr (ST) {
            // the next pass's inter-pass twiddle, one at a time (an entry is 32 registers next to the four results): C may
            // exceed that pass's stride, so its row rho' is taken per element
#pragma unroll
            for (uint32_t q = 0; q < NE; q++) {
                const uint32_t e = e0 + q * nthreads;
                const uint32_t rho_n = (idx[q] >> a.nx_s_log) & ((1u << a.nx_B) - 1);
                const uint32_t K_n = K_uniform | (((e >> log_c) & (R - 1)) << a.t_log);
                if (e < total) y[q] = store_twiddle(a, y[q], (rho_n << a.nx_t_log) | K_n);
            }
            // (radix 2: every scalar register is in use and the branch would spill two more pairs: the form without one)
            fp_chunk_handover<RADIX4>(y);
        }
#pragma unroll
        for (uint32_t q = 0; q < NE; q++)
            if (e0 + q * nthreads < total) fp_store(out_p + idx[q], y[q]);
    }
}

// ---------------------------------------------------------------- the common pass, tile ends fused
// The radix-4 pass at one fixed geometry (8 bits, 4 columns, 256 lanes, four elements per lane, nothing skipped; one tile
// per workgroup, blockIdx.y the vector; the butterfly twiddles as chunk tables, see below) with the two ends of a tile taken out of LDS.
// The four rows a lane loads are the inputs of ONE unit of the first stage pair, and the four rows a unit of the last stage
// pair produces are the four a lane stores.  So the first pair runs on the loaded registers (after pre3, the coset pre-scale
// and the inter-pass twiddle, as before) and writes its outputs to LDS, and the last pair's outputs go through the
// post-processing to memory from registers: two LDS round trips and two of five barriers per tile less, the same operations
// on the same operands.  Lane -> element maps (unit b of the first pair holds LDS rows 4b .. 4b + 3 = the rows
// rho = bitrev6(b) + 64 q of the tile, x_j with bitrev2(j) = q):
//   passes before the last: lane t takes unit b = t >> 2 of column t & 3 and loads rows bitrev6(b) + 64 q (a row is one
//     128-byte segment whichever lane loads it; the unit's LDS writes are those of the unfused round: 2-way conflicts);
//   last pass: a wave takes one column and lane l the rows l + 64 q of it (2 KiB contiguous per load, tw_direct in the same
//     order), i.e. unit bitrev6(l): its LDS writes are 256 B apart (8-way conflicts per lane group, as the bit-reversed
//     writes of the unfused load phase were).
// The first pair needs ONE butterfly twiddle (index 1 of stage 1, entry 64 of the table) before the tile's first barrier, i.e.
// before the LDS copy of the table is ordered against its readers: that one comes from the table in memory (by scalar loads).
// The butterfly twiddles are chunk tables (fp_mul_chunk: 88 multiply-adds per product instead of fp_mul_const's 115).  The
// stage pairs before the last one read only the entries whose index is a multiple of 4: those 32 are in LDS, as TW_CHUNK_Q
// planes of 16-byte words -- plane l holds limb l of the four residues of every twiddle, what one column of the product's
// sweep reads (lanes with different twiddles: 16-byte stride, conflict-free; the same twiddle: a broadcast).  The last stage
// pair reads all R/2 entries, every lane its own three and once per tile: those come from the table in memory (16 KiB, cache
// resident; 384 bytes per lane next to the 256 bytes of its elements).  Tile planes 32 KiB + 4 KiB: four workgroups per CU
// as with the pair tables -- the whole table in LDS (48 KiB) leaves three, which costs more than the shorter product gains.
// Where every lane of a wave multiplies by the SAME twiddle -- the first stage pair's one twiddle, and all of round4(2), whose
// twiddle index is the wave's index -- the entry is an EIGHT-chunk one (TwChunk32: 80 multiply-adds and 2 low products per
// product) read from its 8 KiB table in memory by scalar loads, plane by plane, into scalar registers: bmul_s below.  The
// same entries from LDS for round4(4) (16 ds_read_b128 per product instead of 8) measured slower: DESIGN.md 3.2.
static constexpr uint32_t PASS8_TW_LDS = 32;   // entries in LDS: indices 0, 4, 8 ..
static constexpr uint32_t PASS8_LDS = ((256u << 2) * 2 + PASS8_TW_LDS * TW_CHUNK_Q) * sizeof(uint4);
static_assert(4 * PASS8_LDS <= 160u * 1024, "four workgroups of k_ntt_pass8 per CU");
// NLAST, ST: k_ntt_pass's.  With ST the product runs on the four results a lane holds after the last stage pair, rows
// (tid >> 2) + 64 q of a tile whose next-pass row rho' is uniform: entries (rho' << 8) | k of that table, 16 consecutive ones
// (2 KiB) per wave and load, the same 256 (32 KiB) for the 64 consecutive tiles of one rho'.
// Loads that depend on nothing are issued before the waits they used to follow (profiles/ntt_tile_ends_isa.txt): at the head
// the word of the LDS table copy, the four elements and the last pass's first two table entries are one batch, waited for
// once; at the tail the store products keep the next entry's first half in flight.
// PLAIN: the plain call -- one vector (no batch), in_len the whole vector, no pre3 / post3 product, no coset scale -- with the
// pass's position known when the kernel is compiled: <true, true> the FIRST pass (canonical data in), <true, false> a MIDDLE
// pass whose twiddles the pass before it applied (canonical too), <false> the LAST pass with its complete table (tw_direct).
// ntt_pass_launch chooses it (pass8_plain); every other call runs the instantiations without it.  The element loads carry no
// mask then, so the wait in front of the LDS fill counts the loads behind it, and the branches of the other calls are gone.
template <bool NLAST, bool ST = false, bool PLAIN = false>
__global__ void __launch_bounds__(256, 4) k_ntt_pass8(PassArgs a) {
    static_assert(!ST || NLAST, "a last pass stores the transform's output");
    constexpr uint32_t B = 8, R = 1u << B, log_c = 2, C = 1u << log_c;
    auto tmul = [](const Fr& x, const Fr& w) -> Fr { return fp_mul_wide(x, w); };
    uint4* t_lo = h2_smem;                  // the planes of k_ntt_pass, at the same offsets
    uint4* t_hi = t_lo + (R << log_c);
    uint4* w_pl = t_hi + (R << log_c);      // the chunk table's entries 0, 4, 8 ..: TW_CHUNK_Q planes of PASS8_TW_LDS words
    const uint4* const tw_tab = reinterpret_cast<const uint4*>(a.tw_chunk);   // the whole table, entry-major
    using Tw = TwChunk;
    auto tw_unpack = [](Tw& t, const uint32_t k, const uint4 v) __attribute__((always_inline)) {
        t.w[4 * k] = v.x; t.w[4 * k + 1] = v.y; t.w[4 * k + 2] = v.z; t.w[4 * k + 3] = v.w;
    };
    static_assert((R >> 1) / PASS8_TW_LDS == 4, "the stage pairs before the last read the indices that are multiples of 4");
    auto tw_get = [&](const uint32_t i, const bool mem) __attribute__((always_inline)) -> Tw {
        Tw t;
#pragma unroll
        for (uint32_t k = 0; k < TW_CHUNK_Q; k++)
            tw_unpack(t, k, mem ? tw_tab[(size_t)i * TW_CHUNK_Q + k] : w_pl[k * PASS8_TW_LDS + (i >> 2)]);
        return t;
    };
    auto bmul = [](const Fr& x, const Tw& t) __attribute__((always_inline)) -> Fr { return fp_mul_chunk(x, t); };
    // x * (twiddle i) for a WAVE-UNIFORM i, a multiple of 4: the same eight-chunk entry from the table in memory through the
    // constant address space, i.e. by scalar loads into scalar registers, which the multiply-adds read as they read the
    // modulus limbs -- no vector register and no LDS read for the twiddle.  `i` has to be a scalar value (from `wave`).
    typedef const __attribute__((address_space(4))) uint32_t* TwScalar;
    const TwScalar tw32_s = (TwScalar)reinterpret_cast<const uint32_t*>(a.tw_chunk32);
    auto bmul_s = [&](const Fr& x, const uint32_t i) __attribute__((always_inline)) -> Fr {
        const TwScalar e = tw32_s + (i >> 2) * (uint32_t)(sizeof(TwChunk32) / sizeof(uint32_t));
        return fp_mul_chunk_planes<1, true>(x, [e](uint32_t (&w)[8], const uint32_t c) __attribute__((always_inline)) {
#pragma unroll
            for (uint32_t k = 0; k < 8; k++) w[k] = e[8 * c + k];
        });
    };
    // stages s and s + 1 on the rows p, p + h, p + 2h, p + 3h (h = 2^s) of one column, in registers, twiddle index r = p mod h:
    // the butterflies of k_ntt_pass's round4 on the same residues; x0 .. x3 come back in row order
    // In two halves, so that the last stage pair can start the loads of what follows it between them.  unit4_mul: everything
    // up to the last product; x0 .. x3 leave as y0, y1 (below 2p), y2 and n3 = -y3 (products: below p (1 + 2^-29); y2 of a
    // unit: below 2p).  unit4_add: the four sums and differences, below 4p.
    // The rows come in STRICTLY below 4p, and x2 is used as it comes: its sum with the product x3' = x3 wa is below
    // 5p + 2^-29 p < 2^256 = 5.29 p, which a product takes as it is (fp_mul_chunk: any 256-bit operand), and so is the
    // difference taken the other way round, x3' - x2 + 4p in (0, 5p + 2^-29 p): n3 = (x3' - x2 + 4p) wc is -y3, and unit4_add
    // subtracts where it added.  One fp_lazy_red2p per unit less than reducing x2 first; the products' results are below
    // p (1 + 2^-29) whatever went in, so the rows written are bounded as before.  (Not for k_ntt_pass: fp_mul_const and
    // fp_mul_wide return values below 2p, and x2 + x3' could reach 6p.)  A unit takes its difference the other way round too,
    // x3 - x2 + 2p of the reduced operands, so that one unit4_add serves both.
    auto unit4_mul = [&](Fr& x0, Fr& x1, Fr& x2, Fr& x3, const uint32_t s, const uint32_t r, const bool unit) __attribute__((always_inline)) {
        const uint32_t h = 1u << s;
        const bool mem = s == B - 2;   // the last stage pair: twiddles of every index
        const bool uni = s == 2;       // r = tid >> 6 is the wave's index (round4 passes `wave`): scalar twiddles
        x0 = fp_lazy_red2p(x0);
        Fr y2, n3;
        if (!unit) {
            if (uni) {
                x1 = bmul_s(x1, r << (B - 1 - s));
                x3 = bmul_s(x3, r << (B - 1 - s));
            } else {
                const Tw wa = tw_get(r << (B - 1 - s), mem);
                x1 = bmul(x1, wa);
                x3 = bmul(x3, wa);
            }
            y2 = fp_lazy_add(x2, x3);            // below 5p + 2^-29 p
            n3 = fp_lazy_sub_from4p(x3, x2);     // in (0, 5p + 2^-29 p)
        } else {
            x1 = fp_lazy_red2p(x1);
            x2 = fp_lazy_red2p(x2);
            x3 = fp_lazy_red2p(x3);
            y2 = fp_lazy_add(x2, x3);            // below 4p
            n3 = fp_lazy_sub(x3, x2);            // in (0, 4p)
        }
        // the last stage pair of a pass before the last (never a unit: x1 is a product): its results go to a product and to
        // nothing else, so y0 and y1 stay unreduced (field.hpp: fp_lazy_last_pair_loose_head / _add have the bounds)
        Fr y0, y1;
        if (NLAST && mem) {
            fp_lazy_last_pair_loose_head(x0, x1, y0, y1);
        } else {
            y0 = fp_lazy_add_red(x0, x1);
            y1 = fp_lazy_sub_red(x0, x1);
        }
        if (uni) {
            y2 = unit ? fp_lazy_red2p(y2) : bmul_s(y2, r << (B - 2 - s));
            n3 = bmul_s(n3, (r + h) << (B - 2 - s));
        } else {
            y2 = unit ? fp_lazy_red2p(y2) : bmul(y2, tw_get(r << (B - 2 - s), mem));
            n3 = bmul(n3, tw_get((r + h) << (B - 2 - s), mem));
        }
        x0 = y0;
        x1 = y1;
        x2 = y2;
        x3 = n3;
    };
    // y0, y1, y2 below 2p, n3 = -y3 below p (1 + 2^-29): rows y0 + y2, y1 + y3, y0 - y2, y1 - y3, each strictly below 4p
    // `loose` (after unit4_mul's loose form only): the same four residues below 2^256, for a product
    auto unit4_add = [](Fr& x0, Fr& x1, Fr& x2, Fr& x3, const bool loose) __attribute__((always_inline)) {
        if (loose) {
            fp_lazy_last_pair_loose_add(x0, x1, x2, x3);
            return;
        }
        const Fr y0 = x0, y1 = x1, y2 = x2, n3 = x3;
        x0 = fp_lazy_add(y0, y2);
        x1 = fp_lazy_sub(y1, n3);
        x2 = fp_lazy_sub(y0, y2);
        x3 = fp_lazy_add(y1, n3);
    };
    // the unit of lane `tid` in the round of stages s, s + 1: first LDS index, twiddle index (k_ntt_pass's round4)
    auto unit_of = [](const uint32_t tid, const uint32_t s, uint32_t& i0, uint32_t& r, bool& unit) __attribute__((always_inline)) {
        const uint32_t h = 1u << s, log_per = (B - 2 + log_c) - s;
        const bool by_r = s != 0 && log_per >= 6;
        uint32_t c, p;
        if (by_r) {
            r = tid >> log_per;
            const uint32_t j = tid & ((1u << log_per) - 1);
            c = j & (C - 1);
            p = ((j >> log_c) << (s + 2)) | r;
        } else {
            c = tid & (C - 1);
            const uint32_t b = tid >> log_c;
            r = b & (h - 1);
            p = ((b >> s) << (s + 2)) | r;
        }
        i0 = (p << log_c) + c;
        unit = s == 0 || (by_r && r == 0);
    };
    const uint32_t tid = threadIdx.x;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // (provably uniform: a scalar register)
    auto round4 = [&](const uint32_t s) __attribute__((always_inline)) {
        uint32_t i0, r;
        bool unit;
        unit_of(tid, s, i0, r, unit);
        if (s == 2) {   // r = tid >> 6: the same value from the scalar register, so that the twiddles' addresses are scalar
            r = wave;
            unit = wave == 0;
        }
        const uint32_t step = (1u << s) << log_c;
        Fr x0 = lds_get(t_lo, t_hi, i0), x1 = lds_get(t_lo, t_hi, i0 + step);
        Fr x2 = lds_get(t_lo, t_hi, i0 + 2 * step), x3 = lds_get(t_lo, t_hi, i0 + 3 * step);
        unit4_mul(x0, x1, x2, x3, s, r, unit);
        unit4_add(x0, x1, x2, x3, false);   // (rows of a tile: strictly below 4p, whatever the pass)
        lds_put(t_lo, t_hi, i0, x0);
        lds_put(t_lo, t_hi, i0 + 2 * step, x2);
        lds_put(t_lo, t_hi, i0 + step, x1);
        lds_put(t_lo, t_hi, i0 + 3 * step, x3);
        __syncthreads();
    };
    const bool is_last = NLAST ? false : (PLAIN || a.is_last != 0);
    const uint32_t n_mask = (a.log_n >= 32) ? 0xffffffffu : ((1u << a.log_n) - 1);

    // The LDS copy of the table's entries 0, 4, 8 ..: one 16-byte word per lane.  Nothing reads it before the tile's first
    // barrier, so only its load is issued here; the word goes to LDS once the tile's element loads are in flight behind it:
    // one memory round trip at the head of a tile, not a table round trip and then an element round trip.  (Without PLAIN the
    // wait in front of that ds_write compiles to vmcnt(0): the element loads are under exec masks, idx < in_len, so how many
    // of them are behind this load is not known statically.  The elements are what the lane needs next in any case.)
    static_assert(PASS8_TW_LDS * TW_CHUNK_Q == 256, "one word of the LDS copy per lane");
    const uint4 w_fill = tw_tab[(size_t)(tid / TW_CHUNK_Q) * 4 * TW_CHUNK_Q + tid % TW_CHUNK_Q];

    // (stage 1's twiddle of index 1 for the first stage pair, entry R / 4, is read from the table in memory as the product
    // runs: bmul_s)

    constexpr uint32_t NE = 4;
    {
        const uint32_t tile_id = blockIdx.x;
        const Fr* const in_p = !PLAIN && a.batch ? a.in_b[blockIdx.y] : a.in;   // (wave-uniform: scalar loads from the kernel arguments)
        Fr* const out_p = !PLAIN && a.batch ? a.out_b[blockIdx.y] : a.out;
        uint32_t base = 0, K_uniform = 0;
        if (!is_last) {
            const uint32_t chunks_per_hi = (1u << a.s_log) >> log_c;
            const uint32_t hi = tile_id / chunks_per_hi, lo0 = (tile_id % chunks_per_hi) << log_c;
            base = (hi << (B + a.s_log)) + lo0;
            if (!(PLAIN && ST)) K_uniform = hi_to_K(hi, a);   // (the plain first pass: no earlier digits)
        }

        // ---- load (+ zero pad, coset pre-scale, inter-pass twiddle): k_ntt_pass's, with the lane -> element map above
        {
            uint32_t rho[NE], col[NE], idx[NE], Kk[NE];
            Fr x[NE];
#pragma unroll
            for (uint32_t q = 0; q < NE; q++) {
                if (!is_last) {
                    col[q] = tid & (C - 1);
                    rho[q] = bitrev(tid >> log_c, B - 2) + (q << (B - 2));
                    idx[q] = base + (rho[q] << a.s_log) + col[q];
                    Kk[q] = K_uniform;
                } else {
                    rho[q] = (tid & 63) + (q << (B - 2));
                    col[q] = tid >> 6;
                    Kk[q] = (tile_id << log_c) + col[q];
                    idx[q] = (K_to_hi(Kk[q], a) << B) + rho[q];
                }
            }
#pragma unroll
            for (uint32_t q = 0; q < NE; q++) {
                if constexpr (PLAIN) {
                    x[q] = fp_load(in_p + idx[q]);
                } else {
                    x[q] = fp_zero<FrParams>();
                    if (idx[q] < a.in_len) x[q] = fp_load(in_p + idx[q]);
                }
            }
            const bool pre_scale = !PLAIN && a.scale_mode == 1u && a.nprev == 0;
            // the last pass's table: its first two entries are requested with the elements, not after pre3
            const bool direct = PLAIN ? !NLAST : (!NLAST && a.nprev != 0 && !a.tw_applied && a.tw_direct != nullptr && !pre_scale);
            // PLAIN: a first or an applied middle pass multiplies by nothing at its load, the last pass by its table
            const bool load_mul = PLAIN ? !NLAST : ((a.nprev != 0 && !a.tw_applied) || pre_scale);
            Fr wd[2];
            if (direct) {
#pragma unroll
                for (uint32_t q = 0; q < 2; q++) wd[q] = fp_load(a.tw_direct + ((Kk[q] << B) | rho[q]));
            }
            __builtin_amdgcn_sched_barrier(0);   // (every load above is issued before the wait below)
            w_pl[(tid % TW_CHUNK_Q) * PASS8_TW_LDS + tid / TW_CHUNK_Q] = w_fill;
            if (!PLAIN && a.has_pre3) {
#pragma unroll
                for (uint32_t q = 0; q < NE; q++) {
                    const uint32_t m = idx[q] % 3;
                    Fr w;
#pragma unroll
                    for (int l = 0; l < 8; l++) w.l[l] = m == 1 ? a.pre3[1].l[l] : a.pre3[2].l[l];
                    if (m != 0) x[q] = tmul(x[q], w);
                }
            }
            if (load_mul) {
                if (direct) {
                    Fr w[2];
#pragma unroll
                    for (uint32_t q = 0; q < 2; q++) w[q] = fp_load(a.tw_direct + ((Kk[2 + q] << B) | rho[2 + q]));
#pragma unroll
                    for (uint32_t q = 0; q < 2; q++) x[q] = tmul(x[q], wd[q]);
#pragma unroll
                    for (uint32_t q = 0; q < 2; q++) x[2 + q] = tmul(x[2 + q], w[q]);
                } else if (a.log_n <= LO_BITS && !pre_scale) {
#pragma unroll
                    for (uint32_t q = 0; q < NE; q++) {
                        const uint32_t ex = (uint32_t)(((uint64_t)rho[q] * Kk[q]) << a.s_log) & n_mask;
                        x[q] = tmul(x[q], fp_load(a.tw_lo + ex));
                    }
                } else {
                    const Fr* const two_lo = pre_scale ? a.sc_lo : a.tw_lo;
                    const Fr* const two_hi = pre_scale ? a.sc_hi : a.tw_hi;
#pragma unroll
                    for (uint32_t q0 = 0; q0 < NE; q0 += 2) {
                        Fr wl[2], wh[2];
#pragma unroll
                        for (uint32_t q = 0; q < 2; q++) {
                            const uint32_t ex = pre_scale ? (idx[q0 + q] & n_mask)
                                                          : ((uint32_t)(((uint64_t)rho[q0 + q] * Kk[q0 + q]) << a.s_log) & n_mask);
                            wl[q] = fp_load(two_lo + (ex & ((1u << LO_BITS) - 1)));
                            wh[q] = fp_load(two_hi + (ex >> LO_BITS));
                        }
#pragma unroll
                        for (uint32_t q = 0; q < 2; q++) x[q0 + q] = tmul(x[q0 + q], fp_mul(wl[q], wh[q]));
                    }
                }
            }
            // x[q] is row 4b + bitrev2(q) of unit b: stages 0 and 1 (every twiddle of stage 0 and index 0 of stage 1 is 1)
            const uint32_t b = is_last ? bitrev(tid & 63, B - 2) : (tid >> log_c);
            const uint32_t i0 = (b << (2 + log_c)) + (is_last ? (tid >> 6) : (tid & (C - 1)));
            // Operands that left the twiddle product above are below 2p as they are, and so are a coset first pass's after its
            // pre-scale.  A first pass that loads the caller's data and nothing else holds canonical residues, below p (the
            // library's contract for every input; the zeros of a padded call are), and so does a pass whose twiddles the pass
            // before it applied at its store (tw_applied: every store with ST ends with fp_chunk_handover, in both kernels): no
            // reduction either, and bare sums in place of the reducing ones (FIRST_PAIR_CANON).  Only with pre3, which leaves
            // every third element as loaded next to two products below 2p, the operands are reduced as before.  Wave-uniform;
            // PLAIN: known when the kernel is compiled.
            const FirstPair form = PLAIN ? (NLAST ? FIRST_PAIR_CANON : FIRST_PAIR_2P)
                                   : a.tw_applied ? FIRST_PAIR_CANON
                                   : (a.nprev != 0 || pre_scale) ? FIRST_PAIR_2P : (a.has_pre3 ? FIRST_PAIR_4P : FIRST_PAIR_CANON);
            fp_lazy_first_pair_mul(x[0], x[2], x[1], x[3], [&](const Fr& d) __attribute__((always_inline)) { return bmul_s(d, R >> 2); }, form);
            lds_put(t_lo, t_hi, i0, x[0]);
            lds_put(t_lo, t_hi, i0 + 2 * C, x[1]);
            lds_put(t_lo, t_hi, i0 + C, x[2]);
            lds_put(t_lo, t_hi, i0 + 3 * C, x[3]);
        }
        __syncthreads();
        round4(2);
        round4(4);

        // ---- last stage pair and store (+ post-scale on the final pass): lane t holds rows (t >> 2) + 64 q of column t & 3
        Fr y[NE];
        // the next pass's inter-pass twiddles (ST): entry q of this lane, 64 << t_log entries apart; rho' from the tile's base:
        // its 4 columns share it (nx_s_log >= 2)
        const uint4* nx_q = nullptr;
        size_t nx_step = 0;
        if constexpr (ST) {
            const uint32_t rho_n = (base >> a.nx_s_log) & ((1u << a.nx_B) - 1);
            const uint32_t K_n = K_uniform | ((tid >> log_c) << a.t_log);
            nx_q = reinterpret_cast<const uint4*>(a.nx_tab) + (size_t)((rho_n << a.nx_t_log) | K_n) * TW_CHUNK_Q;
            nx_step = (size_t)((R / NE) << a.t_log) * TW_CHUNK_Q;
        }
        Tw nx_t;   // ST: the entry of the product that runs next
        {
            uint32_t i0, r;
            bool unit;
            unit_of(tid, 6, i0, r, unit);
#pragma unroll
            for (uint32_t q = 0; q < NE; q++) y[q] = lds_get(t_lo, t_hi, i0 + q * (R << log_c) / NE);
            unit4_mul(y[0], y[1], y[2], y[3], 6, r, unit);
            if constexpr (ST) {
                // the first store product's entry under the pair's last additions
#pragma unroll
                for (uint32_t k = 0; k < TW_CHUNK_Q; k++) tw_unpack(nx_t, k, nx_q[k]);
                __builtin_amdgcn_sched_barrier(0);
            }
            unit4_add(y[0], y[1], y[2], y[3], NLAST);
        }
        uint32_t idx[NE];
#pragma unroll
        for (uint32_t q = 0; q < NE; q++) {
            const uint32_t c = tid & (C - 1), k = (tid >> log_c) + q * (R / NE);
            if (!is_last)
                idx[q] = base + (k << a.s_log) + c;
            else
                idx[q] = ((tile_id << log_c) + c) + (k << a.t_log);
        }
        if (!PLAIN && is_last && a.scale_mode == 2u) {
#pragma unroll
            for (uint32_t q = 0; q < NE; q++) {
                const uint32_t i = idx[q] & n_mask;
                const Fr w = fp_mul(fp_load(a.sc_lo + (i & ((1u << LO_BITS) - 1))), fp_load(a.sc_hi + (i >> LO_BITS)));
                y[q] = fp_reduce_once(fp_mul_wide(y[q], w));
            }
        } else if (!PLAIN && is_last && a.has_post3 && !a.hi_scaled) {
#pragma unroll
            for (uint32_t q = 0; q < NE; q++) {
                const uint32_t m = idx[q] % 3;
                Fr w;
#pragma unroll
                for (int l = 0; l < 8; l++) w.l[l] = m == 0 ? a.post3[0].l[l] : (m == 1 ? a.post3[1].l[l] : a.post3[2].l[l]);
                y[q] = fp_reduce_once(fp_mul_wide(y[q], w));
            }
        } else if (is_last) {
#pragma unroll
            for (uint32_t q = 0; q < NE; q++) y[q] = fp_lazy_canon(y[q]);
        }
        if constexpr (ST) {
            // the next pass's inter-pass twiddle, one product at a time (an entry is 32 registers next to the four results).
            // Under product q the first PF words of entry q + 1 are in flight (what the registers allow); its other words are
            // requested together when product q has freed theirs.  Any 256-bit y (the loose last pair's rows are not below
            // 4p) -> below p (1 + 2^-29), and canonical after fp_chunk_handover: what the next pass's first stage pair adds
            // with bare sums.
            constexpr uint32_t PF = TW_CHUNK_Q / 2;
#pragma unroll
            for (uint32_t q = 0; q < NE; q++) {
                uint4 pf[PF];
                if (q + 1 < NE) {
#pragma unroll
                    for (uint32_t k = 0; k < PF; k++) pf[k] = nx_q[(q + 1) * nx_step + k];
                    __builtin_amdgcn_sched_barrier(0);
                }
                y[q] = fp_mul_chunk(y[q], nx_t);
                if (q + 1 < NE) {
                    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                    for (uint32_t k = PF; k < TW_CHUNK_Q; k++) tw_unpack(nx_t, k, nx_q[(q + 1) * nx_step + k]);
#pragma unroll
                    for (uint32_t k = 0; k < PF; k++) tw_unpack(nx_t, k, pf[k]);
                }
            }
            fp_chunk_handover(y);
            // The store indices once more, from a lane id rebuilt here (the wave's index is a scalar register) that the compiler
            // cannot tie to the one above (the empty statement reads the last product, so it stays behind it): kept from the
            // head of the tile across the hand-over's branch, the indices or the lane id cost spilled registers.
            uint32_t t = (wave << 6) | __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
            asm volatile("" : "+v"(t) : "v"(y[NE - 1].l[7]));
#pragma unroll
            for (uint32_t q = 0; q < NE; q++) idx[q] = base + (((t >> log_c) + q * (R / NE)) << a.s_log) + (t & (C - 1));
        }
#pragma unroll
        for (uint32_t q = 0; q < NE; q++) fp_store(out_p + idx[q], y[q]);
    }
}

// ---------------------------------------------------------------- launchers
using PassFn = void (*)(PassArgs);
static const PassFn pass_fn[H2_NTT_KERNEL_COUNT] = {
    k_ntt_pass8<true>,        // NK_PASS8_DP
    k_ntt_pass8<false>,       // NK_PASS8
    k_ntt_pass<true, true>,   // NK_R4_DP
    k_ntt_pass<true, false>,  // NK_R4
    k_ntt_pass<false>,        // NK_R2
};
// the same kernels with the next pass's twiddles at the store (ST: a.nx_tab), for the ids a pass before the last can have
static const PassFn pass_fn_st[H2_NTT_KERNEL_COUNT] = {
    k_ntt_pass8<true, true>, nullptr, k_ntt_pass<true, true, true>, nullptr, k_ntt_pass<false, false, true>,
};

// the plain call of the fixed pass (k_ntt_pass8's PLAIN), by position
static const PassFn pass8_plain_first = k_ntt_pass8<true, true, true>, pass8_plain_middle = k_ntt_pass8<true, false, true>,
                    pass8_plain_last = k_ntt_pass8<false, false, true>;
static PassFn pass8_plain(NttKernel kernel, const PassArgs& a, uint32_t cnt) {
    if (cnt != 1 || a.batch || a.in_len < (1u << a.log_n) || a.has_pre3 || a.scale_mode != 0) return nullptr;
    if (kernel == NK_PASS8) {
        const bool table = a.nprev != 0 && !a.tw_applied && a.tw_direct != nullptr;   // (an inverse's divisor rides in it: hi_scaled)
        return a.is_last && table && !(a.has_post3 && !a.hi_scaled) ? pass8_plain_last : nullptr;
    }
    if (kernel != NK_PASS8_DP || a.is_last) return nullptr;
    if (a.nx_tab) return a.nprev == 0 ? pass8_plain_first : nullptr;
    return a.nprev != 0 && a.tw_applied ? pass8_plain_middle : nullptr;
}

void ntt_pass_launch(int device, NttKernel kernel, const PassArgs& a, uint32_t cnt, uint32_t threads, hipStream_t stream) {
    const uint32_t R = 1u << a.B, C = 1u << a.log_c;
    const uint32_t ntiles = (1u << a.log_n) / (R * C);
    // tile planes + butterfly twiddles: R/2 values and a pad, or (CW: every kernel but NK_R2) R/2 pairs exactly; k_ntt_pass8 has its own (36 KiB)
    const size_t lds = kernel != NK_R2 ? ((size_t)R * C + R) * sizeof(Fr) : ((size_t)R * C + (R >> 1) + 2) * sizeof(Fr);
    if (lds > 64 * 1024) {  // beyond the default dynamic LDS limit: raise it once (never the 8-bit passes)
        static bool raised[64] = {};  // per device
        if (device < 0 || device >= 64 || !raised[device]) {
            for (const PassFn f : {pass_fn[NK_R4_DP], pass_fn[NK_R4], pass_fn[NK_R2], pass_fn_st[NK_R4_DP], pass_fn_st[NK_R2]})
                H2_HIP(hipFuncSetAttribute((const void*)f, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
            if (device >= 0 && device < 64) raised[device] = true;
        }
    }
    const bool pass8 = kernel == NK_PASS8_DP || kernel == NK_PASS8;
    PassFn fn = a.nx_tab ? pass_fn_st[kernel] : pass_fn[kernel];
    if (const PassFn plain = pass8_plain(kernel, a, cnt)) fn = plain;
    if (!fn) throw std::runtime_error("ntt_pass_launch: a last pass has no next pass to multiply for");
    hipLaunchKernelGGL(fn, dim3(ntiles, cnt), dim3(threads), pass8 ? (size_t)PASS8_LDS : lds, stream, a);
}

static dim3 fill_grid(uint32_t count) { return dim3((count + 255) / 256); }

void ntt_fill_pow(Fr* out, const Fr& base, uint32_t mul, uint32_t count, uint32_t form, hipStream_t stream) {
    if (count) hipLaunchKernelGGL(k_pow_table, fill_grid(count), dim3(256), 0, stream, out, base, mul, count, form);
}

void ntt_fill_direct(Fr* out, const Fr& base, uint32_t kbits, uint32_t s_log, uint32_t log_n, uint32_t count, uint32_t form,
                     hipStream_t stream) {
    hipLaunchKernelGGL(k_direct_table, fill_grid(count), dim3(256), 0, stream, out, base, kbits, s_log, log_n, count, form);
}

void ntt_fill_last(Fr* out, const Fr& base, uint32_t bits, uint32_t log_n, const Fr* d, hipStream_t stream) {
    hipLaunchKernelGGL(k_last_table, fill_grid(1u << log_n), dim3(256), 0, stream, out, base, bits, log_n, d ? *d : base,
                       d ? 1u : 0u, 0u);
}

void ntt_fill_scaled(Fr* out, const Fr* in, const Fr& d, uint32_t count, hipStream_t stream) {
    hipLaunchKernelGGL(k_scale_table, fill_grid(count), dim3(256), 0, stream, out, in, d, count);
}

}  // namespace h2
