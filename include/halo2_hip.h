/*
 * halo2_hip.h -- C ABI of libhalo2_hip.so: the MI355X (gfx950) drop-in for the `cuda`
 * feature of halo2_proofs (DelphinusLab/halo2-gpu-specific).
 *
 * Every entry point replaces one `#[cfg(feature = "cuda")]` call site of the reference
 * (file:line under /root/reference/halo2_proofs/src/, cited per function).  The Rust side
 * keeps its generic signatures and forwards the transmuted slices (exactly what it hands to
 * ec-gpu-gen today, arithmetic.rs:156-161,351-352,391-394,507-508); see INTEGRATION.md.
 *
 * Conventions
 *   Fr            32 B = 4 x u64 little-endian limbs, Montgomery form (R = 2^256)
 *   G1Affine      64 B = {x: Fq, y: Fq} Montgomery, identity = (0, 0)
 *   G1 (result)   96 B = Jacobian {x, y, z: Fq} Montgomery, identity has z = 0
 *   value range   every field element handed to the library is a valid residue image: below the modulus (the
 *                 reference's own Fr / Fq invariant).  The multiplier relies on inputs below 2^254 (it skips the
 *                 carry handling that such inputs cannot trigger); out-of-range limbs give unspecified residues, not
 *                 an error.
 *   return value  0 = H2_OK, non-zero = error; h2_last_error() gives the text.  The
 *                 reference unwrap()s its GPU Results (arithmetic.rs:358,360,509), so the
 *                 Rust shim panics on non-zero.
 *   threading     every function may be called concurrently from any thread (rayon workers);
 *                 host-buffer calls take a device from the blocking pool sized by
 *                 HALO2_PROOFS_N_GPU (plonk/prover.rs:56-74; arithmetic.rs:314-331).  A device serves
 *                 H2_HOST_SLOTS (default 2, 1..4) such calls at a time, each on its own stream and staging, so that
 *                 one caller's transfers overlap another's kernels; 1 = the reference's one operation per device.
 *   h2_dev_*      operate on HIP device pointers on the caller's stream (void* = hipStream_t,
 *                 NULL = the library's stream for the current device): they read their inputs and write their outputs
 *                 at their position in that stream, whatever thread calls and whatever other streams are busy.
 *                 NULL does NOT mean HIP's legacy default stream: the library's stream is non-blocking, so work
 *                 the caller queued on stream 0 is not ordered against it -- pass a stream of your own (every
 *                 call then runs in its order), or bracket the calls with h2_synchronize / hipDeviceSynchronize.
 *                 They return without waiting for the stream, EXCEPT the ones below, which return only when the
 *                 stream has drained up to and including their own work -- they hand a result to host memory, or
 *                 stage host tables that live in the call's frame:
 *                   h2_dev_eval_polynomial, h2_dev_eval_polynomial_batch, h2_dev_max_scalar_bits (host results);
 *                   h2_dev_msm, h2_dev_msm_batch, h2_dev_msm_batch_ex (host results), h2_dev_bases_precompute;
 *                   h2_dev_prefix_product, h2_dev_prefix_sum (the initial value is staged from the frame);
 *                   h2_dev_points_decompress, h2_dev_logup_multiplicity, h2_dev_logup_multiplicity_bits (their status
 *                   is a device result); h2_dev_cells_place, h2_dev_selectors_mark, h2_dev_coverage_mark,
 *                   h2_dev_coverage_check (staged tables); h2_dev_permutation_mapping_phases (timed); h2_dev_download.
 *                 The first call for a new transform size, generator or gate program also waits (it builds and
 *                 publishes tables or compiles), later ones do not.  tests/test_gpu_stream_contract.py pins both lists.
 *                 Scratch the library lends to such a call ("Library memory on caller streams") is ordered
 *                 between streams by the library: two threads may drive two streams of one device at once.
 */
#ifndef HALO2_HIP_H
#define HALO2_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum {
    H2_OK = 0,
    H2_ERR_INVALID = 1,
    H2_ERR_NO_DEVICE = 2,
    H2_ERR_HIP = 3,
    H2_ERR_OOM = 4
};

/* ---- library / device pool ------------------------------------------------------------ */
int h2_version(void);
/* Device::all().len() clipped by HALO2_PROOFS_N_GPU -- plonk/prover.rs:57-70 */
int h2_device_count(void);
const char *h2_last_error(void);
/* blocks until all work queued by this library on every pooled device has finished */
int h2_synchronize(void);

/* ---- device memory the library keeps between calls ---------------------------------------------
 * The reference bounds its device memory by keeping coefficient forms and re-deriving extended cosets through a small
 * cache (plonk/evaluation_gpu.rs:335-468, HALO2_PROOF_GPU_EVAL_CACHE).  Here the caller owns every polynomial; what the
 * LIBRARY holds per device is: NTT plans (twiddle tables, a few MiB per (log_n, omega)), the optional complete last-pass
 * twiddle tables (32 B x n per (plan, divisor): 512 MiB at 2^24), shifted-base tables (h2_dev_bases_precompute), device
 * copies of registered SRS ranges and the host-API staging arenas.
 *  - The last-pass tables live inside a per-device budget: H2_NTT_TABLE_BUDGET in the environment (bytes, K / M / G
 *    suffixes) or h2_set_table_budget; default 1/32 of the device's memory.  When a new table would exceed it, idle
 *    tables leave in least-recently-used order; a transform without a table composes its twiddles (same values).
 *  - h2_release_plans frees every plan (and its tables) that no call is using, on every device: for callers that
 *    cycle through domains or coset generators.  Synchronises the devices.  It also gives back every slot's block of
 *    column vectors of h2_evaluate_h_coeff / h2_quotient_poly_coeff ((2 x distinct columns + a few) x 2^k x 32 B plus two
 *    extended vectors: 6.4 GiB for 16 columns at k = 22; kept between calls because allocating it cost up to 160 ms).
 *  - h2_library_memory_bytes: what the library holds on the current device right now. */
int h2_release_plans(void);
int h2_set_table_budget(size_t bytes);
size_t h2_library_memory_bytes(void);

/* ---- NTT (host buffers) ---------------------------------------------------------------- */
/* best_fft -> gpu_fft: arithmetic.rs:546-554, :495-512.  a: 2^log_n Fr, in place. */
int h2_ntt(uint64_t *a, const uint64_t omega[4], uint32_t log_n);
/* gpu_ifft: arithmetic.rs:515-534 (EvaluationDomain::ifft, poly/domain.rs:400-414).
 * a <- NTT(a, omega_inv) * divisor. */
int h2_intt(uint64_t *a, const uint64_t omega_inv[4], const uint64_t divisor[4], uint32_t log_n);
/* the same out of place: `a` (2^log_n values the caller keeps: the reference clones the column first, plonk/prover.rs:643-646)
 * is only read, the coefficients go to `out`. */
int h2_intt_to(const uint64_t *a, uint64_t *out, const uint64_t omega_inv[4], const uint64_t divisor[4], uint32_t log_n);
/* EvaluationDomain::coeff_to_extended: poly/domain.rs:270-287 (+ distribute_powers_zeta :382-398).
 * coeffs: 2^k Fr (read only); out: 2^extended_k Fr. */
int h2_coeff_to_extended(const uint64_t *coeffs, uint64_t *out, uint32_t k, uint32_t extended_k,
                         const uint64_t g_coset[4], const uint64_t g_coset_inv[4],
                         const uint64_t extended_omega[4]);
/* EvaluationDomain::extended_to_coeff: poly/domain.rs:328-350.  a: 2^extended_k Fr (read only);
 * out: out_len = n * quotient_poly_degree Fr (the truncation of :346-347). */
int h2_extended_to_coeff(const uint64_t *a, uint64_t *out, size_t out_len, uint32_t extended_k,
                         const uint64_t g_coset[4], const uint64_t g_coset_inv[4],
                         const uint64_t extended_omega_inv[4], const uint64_t extended_ifft_divisor[4]);

/* ---- MSM (host buffers) ---------------------------------------------------------------- */
/* gpu_multiexp_single_gpu_with_bound: arithmetic.rs:334-367 (kern.multiexp_bound :360).
 * Only the low max_bits bits of each canonical scalar are used (callers guarantee the rest
 * are zero: plonk/prover.rs:237-254).  max_bits == 0 or n == 0 -> identity (:346, :421). */
int h2_msm(const uint64_t *scalars, const uint64_t *bases, size_t n, uint32_t max_bits, uint64_t out_xyz[12]);
/* gpu_multiexp_bound: arithmetic.rs:413-440 -- contiguous ceil(n/N_GPU) chunks, one pooled
 * device each, partial points summed on the host. */
int h2_msm_multi(const uint64_t *scalars, const uint64_t *bases, size_t n, uint32_t max_bits, uint64_t out_xyz[12]);
/* Resident SRS (an improvement the reference lacks: it re-uploads the bases on every call,
 * arithmetic.rs:354-360).  After h2_bases_register(g, n) every host-buffer MSM whose `bases` range lies
 * inside [g, g + n) uses a device copy uploaded once per device (Params::g / g_lagrange never change,
 * poly/commitment.rs:23-29).  The caller must not modify a registered range before unregistering it.
 * From 2^15 points on the device copy also gets a shifted-base table (see h2_dev_bases_precompute: digits x n x 64 B
 * more device memory, built on first use, freed with the copy) when that fits in half of the free device memory;
 * H2_MSM_TABLES=0 in the environment keeps the copy only. */
int h2_bases_register(const uint64_t *bases, size_t n);
int h2_bases_unregister(const uint64_t *bases);
/* Resident polynomials, the same idea for Fr vectors: the proving key's coefficient forms -- fixed_polys, permutation.polys, l0,
 * l_last (plonk.rs:226-240, made once by keygen_pk, plonk/keygen.rs:330-440) -- are read by EVERY proof: by the evaluator
 * (plonk/evaluation.rs:1229-1241), by the evaluations at x (plonk/prover.rs:731-737) and by the multiopen folds
 * (poly/multiopen/shplonk/prover.rs:110-209, gwc/prover.rs:57-151), and the reference's cuda path uploads them each time.
 * After h2_poly_register(values, n) every host-slice entry point that only READS a vector lying inside [values, values + n)
 * -- h2_evaluate_h_coeff's columns, h2_eval_polynomial, h2_lincomb's operands, h2_kate_division's dividend, h2_eval_op's
 * operands, h2_coeff_to_extended's input -- uses a device copy uploaded once per device (on first use).  The caller must not
 * modify a registered range before h2_poly_unregister, which frees the copies on every device; a stale registration is never
 * served: register / unregister bump a generation and a copy made for another generation (or length) is dropped.  A host may
 * also register a proof's own final polynomials (advice / product coefficient forms) for the rest of that proof.
 * Entry points that WRITE through the pointer (h2_ntt, h2_intt, h2_batch_mont, h2_eval_op's result ...) never consult the
 * registry for it. */
int h2_poly_register(const uint64_t *values, size_t n);
int h2_poly_unregister(const uint64_t *values);
/* Host-side fold of `count` partial results (12 x u64 Jacobian each): the
 * `.reduce(|acc, x| acc + x)` of arithmetic.rs:433-435; also used after an all-gather of per-rank
 * partial points when one MSM is split across processes (one process per GPU). */
int h2_g1_sum(const uint64_t *points_xyz, size_t count, uint64_t out_xyz[12]);
/* The same fold on the device, for the partial points of `count` range-split MSMs gathered from `world` ranks
 * (d_points_xyz[(r * count + j) * 12 ..] = rank r's Jacobian partial of MSM j): d_out_xyz[j] = sum over r in rank order.
 * Keeps the multi-GPU exchange on the device: all-gather (RCCL) -> this kernel -> one read-back of count x 96 B. */
int h2_dev_g1_fold(const void *d_points_xyz, uint32_t world, uint32_t count, void *d_out_xyz, void *stream);
/* gpu_multiexp_bound_and_fft: arithmetic.rs:375-410 (Params::commit_lagrange_and_ifft,
 * poly/commitment.rs:148-170): MSM over `bases` and, sharing the one upload, scalars <-
 * NTT(scalars, omega_inv) * divisor. */
int h2_msm_intt(uint64_t *scalars, const uint64_t *bases, size_t n, uint32_t max_bits,
                const uint64_t omega_inv[4], const uint64_t divisor[4], uint32_t log_n, uint64_t out_xyz[12]);

/* ---- Montgomery conversion (host buffers) ------------------------------------------------ */
/* gpu_mont / gpu_unmont: arithmetic.rs:263-306, :218-261 (kernels batch_mont / batch_unmont).
 * Input ranges: the conversions (and the scalars of every MSM, which are taken out of Montgomery form first) accept ANY
 * 256-bit value and return / use its residue; every other entry point takes field elements as the reference holds them
 * (canonical residues below the modulus, < 2^254: the multiplier's carry analysis relies on it). */
int h2_batch_mont(uint64_t *a, size_t n);
int h2_batch_unmont(uint64_t *a, size_t n);

/* ---- elementwise polynomial kernels (host buffers) ---------------- */
enum {
    H2_OP_MUL_C = 0,    /* res[i] = l[i+l_rot] * c          eval_mul_c   evaluation_gpu.rs:669,1034 */
    H2_OP_SUM_C = 1,    /* res[i] = l[i+l_rot] + c          eval_sum_c   evaluation_gpu.rs:560,668  */
    H2_OP_SUM = 2,      /* res[i] = l[i+l_rot] + r[i+r_rot] eval_sum     evaluation_gpu.rs:279-305  */
    H2_OP_MUL = 3,      /* res[i] = l[i+l_rot] * r[i+r_rot] eval_mul     evaluation_gpu.rs:622-648  */
    H2_OP_SUB = 4,      /* res[i] = l[i+l_rot] - r[i+r_rot] Polynomial - poly.rs:205-217            */
    H2_OP_LCTHETA = 5,  /* res = l*c + r                    eval_lctheta evaluation_gpu.rs:148-163  */
    H2_OP_LCBETA = 6,   /* res = (l + c) * r                eval_lcbeta  evaluation_gpu.rs:202-217  */
    H2_OP_ADDGAMMA = 7, /* res = l + c                      eval_addgamma evaluation_gpu.rs:246-259 */
    H2_OP_CONSTANT = 8  /* res = c                          eval_constant evaluation_gpu.rs:579-585 */
};
/* Rotations are signed element offsets taken modulo size (evaluation.rs:40-42).  res may alias
 * l or r when that operand's rotation is 0 (evaluation_gpu.rs:631-639).  Unused operands NULL. */
int h2_eval_op(int op, uint64_t *res, const uint64_t *l, const uint64_t *r, int32_t l_rot, int32_t r_rot,
               size_t size, const uint64_t c[4]);
/* EvaluationDomain::divide_by_vanishing_poly: poly/domain.rs:354-373: a[i] *= t_evals[i % t_len] */
int h2_divide_by_vanishing_poly(uint64_t *a, size_t size, const uint64_t *t_evaluations, size_t t_len);


/* ---- adjacent numerics the prover runs between the transforms ------------ */
/* eval_polynomial: arithmetic.rs:714-735 (Horner; prover.rs:731-737 evaluates every committed polynomial
 * at x).  out = sum_i poly[i] * point^i.  Synchronous (the result is host memory). */
int h2_eval_polynomial(const uint64_t *poly, size_t n, const uint64_t point[4], uint64_t out[4]);
/* `count` evaluations in one call, polynomial j (n coefficients) at points[4j..4j+4] -> out[4j..4j+4]: what
 * plonk/prover.rs:700-790 computes in a rayon par_iter over eval_polynomial_st.  One launch per fold level over all of them,
 * one copy back; registered polynomials are read on the device, the others go up once each. */
int h2_eval_polynomial_batch(const uint64_t *const *polys, size_t count, size_t n, const uint64_t *points, uint64_t *out);
int h2_dev_eval_polynomial(const void *d_poly, size_t n, const uint64_t point[4], uint64_t out[4], void *stream);
/* `count` evaluations, polynomial j (n coefficients, device) at points[4 j .. 4 j + 3], enqueued back to back with one
 * read-back: the rayon `par_iter` over eval_polynomial_st of plonk/prover.rs:731-737.  d_polys: HOST array of device
 * pointers; out: count x 4 u64 on the host.  Synchronous. */
int h2_dev_eval_polynomial_batch(const void *const *d_polys, size_t count, size_t n, const uint64_t *points,
                                 uint64_t *out, void *stream);
/* batch_invert: arithmetic.rs:840-844 -- every non-zero element replaced by its inverse, zeros kept
 * (ff::BatchInvert).  d_tmp: n Fr of scratch. */
int h2_batch_invert(uint64_t *a, size_t n);
int h2_dev_batch_invert(void *d_a, void *d_tmp, size_t n, void *stream);
/* kate_division: arithmetic.rs:754-773 -- q(X) = a(X) / (X - b) without remainder; a: n coefficients,
 * q: n - 1 (multiopen: gwc/prover.rs:154-160, shplonk/prover.rs).  A blocked affine prefix scan.
 * h2_dev_kate_division: a and q must not overlap (workgroups read a while others write q: H2_ERR_INVALID when
 * [d_a, d_a + n) and [d_q, d_q + n - 1) share an element and n >= 2).  h2_kate_division may be called with q == a: the
 * dividend is uploaded before the quotient comes back. */
int h2_kate_division(const uint64_t *a, size_t n, const uint64_t b[4], uint64_t *q);
int h2_dev_kate_division(const void *d_a, size_t n, const uint64_t b[4], void *d_q, void *stream);
/* Grand-product column: z[0] = init, z[i] = z[i-1] * f[i-1] for i < n (f has n - 1 used entries) -- the
 * serial loops of permutation/prover.rs:151-160 (`z.push(last_z); for row in 1..n { tmp *= modified_values[row-1] }`),
 * shuffle/prover.rs and the logup grand sums' multiplicative twin.  h2_dev_prefix_product: f and z must not overlap
 * (H2_ERR_INVALID when d_f[0, n - 1) and d_z[0, n) share an element and n >= 2). */
int h2_prefix_product(const uint64_t *f, size_t n, const uint64_t init[4], uint64_t *z);
int h2_dev_prefix_product(const void *d_f, size_t n, const uint64_t init[4], void *d_z, void *stream);
/* res[i] = sum_j coeffs[j] * polys[j][i] -- the GWC / SHPLONK batching loops (poly/multiopen/gwc/prover.rs:39-151:
 * `poly_batch = poly_batch * v + poly`, cuda branch eval_mul_c + eval_sum per polynomial; shplonk/prover.rs:110-209)
 * with the challenge powers supplied by the caller.  d_polys: HOST array of `count` device pointers; coeffs:
 * count x 4 u64 on the host.  d_res may alias d_polys[0] only. */
int h2_dev_lincomb(void *d_res, const void *const *d_polys, const uint64_t *coeffs, size_t count, size_t size,
                   void *stream);
/* the same on host buffers (the GWC cuda branch's shape, gwc/prover.rs:57-151: every p_i is uploaded for its
 * eval_mul_c / eval_sum pair): polys = host array of `count` host pointers; one upload per operand, one fused pass. */
int h2_lincomb(uint64_t *res, const uint64_t *const *polys, const uint64_t *coeffs, size_t count, size_t size);

/* The quotient contributions of a multi-point opening in one call (poly/multiopen/shplonk/prover.rs:95-153: every rotation
 * set's linear combination minus its low-degree remainder polynomial, divided by the set's vanishing polynomial, the sets
 * folded by powers of v -- and :205-219 with n_sets = 1: the final quotient l(X) / (X - u)):
 *   out = sum_s (sum_i coeffs[s][i] * polys[s][i](X) - low_s(X)) / prod_j (X - points[s][j])
 * counts / low_counts / point_counts: per set; polys (host pointers to n coefficients each), coeffs, low, points: the sets'
 * entries one after the other.  The caller multiplies v^(R-1-s) into set s's coeffs and low (division is linear).  Operands
 * registered with h2_poly_register are read on the device; everything else stays there too: `out` (n coefficients, the top
 * ones zero as the reference resizes them, :118) crosses PCIe once.  remainders (may be NULL): 4 words per point, what each
 * division left (the value of its dividend at the point: the reference's must_be_zero, :213-214). */
int h2_quotient_sum(uint64_t *out, size_t n, size_t n_sets, const size_t *counts, const uint64_t *const *polys,
                    const uint64_t *coeffs, const size_t *low_counts, const uint64_t *low, const size_t *point_counts,
                    const uint64_t *points, uint64_t *remainders);

/* Permutation argument, the elementwise work on either side of the grand-product scan.
 * keygen (plonk/permutation/keygen.rs:197-238): out[j] = DELTA^{map_col[j]} * omega^{map_row[j]} -- one sigma column
 * in Lagrange form from the cycle mapping (u32 device arrays of n entries). */
int h2_dev_permutation_sigma(void *d_out, const void *d_map_col, const void *d_map_row, size_t n,
                             const uint64_t delta[4], const uint64_t omega[4], void *stream);
/* prover (plonk/permutation/prover.rs:89-128), one call per column of a set:
 *   den[i] (*)= beta * sigma[i] + gamma + value[i];   num[i] (*)= delta_pow * omega^i * beta + gamma + value[i]
 * first != 0 overwrites num / den, otherwise multiplies into them.  delta_pow = DELTA^{column position}.
 * The caller follows with h2_dev_batch_invert(den), an elementwise product and h2_dev_prefix_product. */
/* the same on host buffers (the reference leaves these products to a rayon loop between its GPU calls): value / sigma in --
 * sigma, a proving-key column, is read on the device when registered with h2_poly_register -- num / den out; chunk-pipelined */
int h2_permutation_terms(uint64_t *num, uint64_t *den, const uint64_t *value, const uint64_t *sigma, size_t n,
                         const uint64_t beta[4], const uint64_t gamma[4], const uint64_t delta_pow[4],
                         const uint64_t omega[4], int first);
/* One grand-product column of the permutation argument, whole, for one set of `count` columns (permutation/prover.rs:72-165:
 * the products over the set's columns :92-127, the batch inversion :106, the running product :150-154):
 *   z[0] = init;  z[i+1] = z[i] * prod_j (values[j][i] + beta * delta_pow * delta^j * omega^i + gamma)
 *                                / prod_j (values[j][i] + beta * sigmas[j][i] + gamma),  i + 1 < n
 * values / sigmas: `count` host pointers to n-element vectors (read on the device without an upload when registered with
 * h2_poly_register); delta_pow = DELTA^(index of the set's first column).  Every intermediate stays on the device: the
 * columns cross PCIe once, z once.  The caller then overwrites its blinding rows and takes z[n - (blinding_factors + 1)] as
 * the next set's init (:157-162). */
int h2_permutation_product(uint64_t *z, const uint64_t *const *values, const uint64_t *const *sigmas, size_t count, size_t n,
                           const uint64_t beta[4], const uint64_t gamma[4], const uint64_t delta_pow[4],
                           const uint64_t delta[4], const uint64_t omega[4], const uint64_t init[4]);
int h2_dev_permutation_terms(void *d_num, void *d_den, const void *d_value, const void *d_sigma, size_t n,
                             const uint64_t beta[4], const uint64_t gamma[4], const uint64_t delta_pow[4],
                             const uint64_t omega[4], int first, void *stream);

/* The vanishing argument's blinding polynomial (plonk/vanishing/prover.rs:47-61, a parallel fill of `Scalar::random`
 * draws from thread_rng): element i = ChaCha20 block i under the caller's 256-bit key (counter i, zero nonce); the
 * 64 output bytes are cut into two 253-bit little-endian integers lo, hi and the element is lo + 2^253 hi mod r
 * (506 random bits), stored in Montgomery form.  The key MUST come from a cryptographic source in production
 * (halo2-gpu-specific_amd/rng.py draws it from os.urandom; its seeded mode is for tests); rng.py also holds the host
 * twin the reference prover of the tests draws from. */
int h2_dev_random_fr(const uint8_t key[32], size_t n, void *d_out, void *stream);
/* the same stream of elements into a host vector (one copy down) */
int h2_random_fr(const uint8_t key[32], size_t n, uint64_t *out);

/* a[i] *= g^i for i < n (n <= 2^28): distribute_powers_zeta (poly/domain.rs:382-398) for an arbitrary generator.  With
 * g = zeta * extended_omega^j followed by an n-point h2_dev_ntt it evaluates a coefficient vector on coset j of the
 * extended domain (extended index c i + j, c = 2^(extended_k - k)); with g^-1 after an n-point h2_dev_intt it inverts
 * that.  The multi-GPU proof shards the extended domain by such cosets (one proof over several ranks). */
int h2_dev_distribute_powers(void *d_a, size_t n, const uint64_t g[4], void *stream);

/* Grand-sum column: z[0] = init, z[i] = z[i-1] + f[i-1] for i < n -- the `scan` of plonk/logup/prover.rs:353-367.
 * f and z must not overlap, as for h2_dev_prefix_product. */
int h2_dev_prefix_sum(const void *d_f, size_t n, const uint64_t init[4], void *d_z, void *stream);
/* The multiplicity column of a logup lookup (plonk/logup/prover.rs:104-180): for every row r < usable_rows of each
 * compressed input column, the table row holding that value is credited once; m[row] = credit as a field element
 * (Montgomery), m[row >= usable_rows] = 0 (the caller writes the blinding values there, :217-221).  A duplicated table
 * value collects its credits on its lowest row (the reference's binary search lands on an implementation-defined
 * duplicate; the argument is indifferent).  d_inputs: HOST array of n_inputs device pointers.  Returns H2_ERR_INVALID
 * when an input value is absent from the table (the reference panics).  Synchronous. */
size_t h2_logup_scratch_bytes(size_t n);
/* Host-vector twins (the reference runs these steps as host loops between its GPU calls): the grand-sum scan, a[i] *= g^i,
 * one sigma column from the cycle mapping (u32 host arrays of n entries), the multiplicity column of a lookup (table and
 * inputs: host vectors of n elements, read on the device when registered with h2_poly_register; max_bits_out may be NULL). */
/* One grand-sum column of a logup lookup, whole, for one set of `count` compressed input columns (plonk/logup/prover.rs:243-347:
 * beta + f per input :259-272 / :310-324, batch_invert :266 / :318, the table's term m / (beta + t) :275-290, the scan :330-346):
 *   z[0] = init;  z[i+1] = z[i] + sum_j 1 / (beta + inputs[j][i]) - m[i] / (beta + table[i]),  i + 1 < n
 * table and m: both NULL for a set without the table (the extra input sets), both given for the first set.  Every intermediate
 * stays on the device; registered vectors are read there.  The caller writes its blinding rows into z and carries
 * z[n - (blinding_factors + 1)] into the next set's init (:333-345). */
int h2_logup_grand_sum(uint64_t *z, const uint64_t *const *inputs, size_t count, const uint64_t *table, const uint64_t *m,
                       size_t n, const uint64_t beta[4], const uint64_t init[4]);
int h2_prefix_sum(const uint64_t *f, size_t n, const uint64_t init[4], uint64_t *z);
int h2_distribute_powers(uint64_t *a, size_t n, const uint64_t g[4]);
int h2_permutation_sigma(uint64_t *out, const uint32_t *map_col, const uint32_t *map_row, size_t n,
                         const uint64_t delta[4], const uint64_t omega[4]);
int h2_logup_multiplicity(const uint64_t *table, const uint64_t *const *inputs, size_t n_inputs, size_t usable_rows,
                          size_t n, uint64_t *m, uint32_t *max_bits_out);
int h2_dev_logup_multiplicity(const void *d_table, const void *const *d_inputs, size_t n_inputs, size_t usable_rows,
                              size_t n, void *d_m, void *d_scratch, size_t scratch_bytes, void *stream);
/* h2_dev_logup_multiplicity that also returns the bit length of the LARGEST multiplicity (0 when every count is zero): the
 * bound for m's commitment (find_max_scalar_bits of the usable rows, arithmetic.rs's `max_bits`) without another pass --
 * a range lookup's multiplicities are a few bits wide, not the log2(rows x inputs) their sum allows */
int h2_dev_logup_multiplicity_bits(const void *d_table, const void *const *d_inputs, size_t n_inputs, size_t usable_rows,
                                   size_t n, void *d_m, void *d_scratch, size_t scratch_bytes, uint32_t *max_bits_out,
                                   void *stream);
/* The same counting restricted to the input rows [row_begin, row_end) -- one device's share when the rows of a proof are dealt
 * over several devices -- with the RAW counters out: d_counts = n + 1 u32 (credits per table row, then the number of input
 * values missing from the table).  Integer counts are an RCCL reduction (sum), field elements are not: the ranks all-reduce
 * d_counts, check the last word and turn the first n into the field elements of m(X) with h2_dev_logup_emit (rows >=
 * usable_rows zero).  Asynchronous on `stream`; same scratch as above. */
int h2_dev_logup_counts(const void *d_table, const void *const *d_inputs, size_t n_inputs, size_t usable_rows, size_t n,
                        size_t row_begin, size_t row_end, void *d_counts, void *d_scratch, size_t scratch_bytes, void *stream);
int h2_dev_logup_emit(const void *d_counts, size_t usable_rows, size_t n, void *d_m, void *stream);

/* The witness of `advice_column_range` columns, completed after synthesis as create_proof does on the host
 * (plonk/prover.rs:1699-1783, `sort` :164-200; range_check.rs:40-63 for the values): for each of `pairs` (origin,
 * companion) column pairs of ONE circuit instance, every value of the range -- vmin, vmin + step, ... below vmax, then
 * vmax -- is planted in the origin in descending row order, ending at row usable_rows - 1, and rows [0, usable_rows) of
 * the companion become the counting sort of the origin's; rows >= usable_rows of both are left alone (blinding overwrites
 * them).  Each column is read and written in its own form:
 *   CANONICAL   n x 4 u64, the integer            MONTGOMERY  n x 4 u64, as h2_dev_batch_mont leaves a canonical column
 *   COMPACT     n u64 (as h2_dev_widen_u64 takes them)
 * d_origins, d_companions, the form codes, vmin, vmax, step and first_unassigned are HOST arrays of `pairs` entries; the
 * columns of a call are distinct.  first_unassigned[i] = the first row of origin i that synthesis left unassigned (the
 * reference's assignment tracking, prover.rs:1706-1731), or H2_RANGE_CHECK_UNASSIGNED_UNKNOWN; first_unassigned = NULL
 * means unknown for every pair.
 * Nothing of a pair is written unless all of its checks pass, and a pair that fails does not stop the others.  The outcome
 * is d_status: H2_RANGE_CHECK_STATUS_WORDS u32 per pair = {code, first offending row or 0xffffffff, pair index, 0, and
 * four words of working state}, final when the stream reaches the end of the call:
 *   OK            completed
 *   NO_FIT        the values and one spare cell below them do not fit the usable rows, or first_unassigned reaches into them
 *   IN_USE        first_unassigned unknown, and the cells to be planted and the spare one are neither all zero nor the
 *                 planted values already (the same columns completed again)
 *   OUT_OF_RANGE  a usable row of the origin is outside [vmin, vmax] or has bits above the low 64
 *   UNSUPPORTED   vmax - vmin >= 2^24, past the counting sort's cap (the caller sorts such a column some other way)
 * d_scratch: h2_range_check_scratch_bytes(vmin, vmax, pairs) bytes, 16-byte aligned.  Asynchronous on `stream`.  Returns
 * H2_ERR_INVALID without touching a device, h2_last_error naming the argument, for a null pointer, n not a power of two,
 * usable_rows > n, vmin > vmax, step == 0, an unknown form code, a misaligned column or too small a scratch. */
enum { H2_RANGE_CHECK_FORM_CANONICAL = 0, H2_RANGE_CHECK_FORM_MONTGOMERY = 1, H2_RANGE_CHECK_FORM_COMPACT = 2 };
enum { H2_RANGE_CHECK_OK = 0, H2_RANGE_CHECK_NO_FIT = 1, H2_RANGE_CHECK_IN_USE = 2, H2_RANGE_CHECK_OUT_OF_RANGE = 3,
       H2_RANGE_CHECK_UNSUPPORTED = 4 };
#define H2_RANGE_CHECK_STATUS_WORDS 8
#define H2_RANGE_CHECK_UNASSIGNED_UNKNOWN UINT64_MAX
size_t h2_range_check_scratch_bytes(const uint64_t *vmin, const uint64_t *vmax, size_t pairs);
int h2_dev_range_check_complete(void *const *d_origins, void *const *d_companions, const uint32_t *origin_forms,
                                const uint32_t *companion_forms, const uint64_t *vmin, const uint64_t *vmax,
                                const uint64_t *step, const uint64_t *first_unassigned, size_t pairs, size_t usable_rows,
                                size_t n, void *d_status, void *d_scratch, size_t scratch_bytes, void *stream);

/* The circuit front end's device assembly (synthesis.py): `count` segments of assigned cells placed into resident columns of
 * n rows (n x 4 u64 each) by ONE launch whose work is split by cells, not by segments.  Segment i writes cell j < count of
 * its source to row first_row + j * stride of the column dst.  A source is read in the segment's form:
 *   CANONICAL  count cells of 4 u64, the integers (below the modulus)      COMPACT  count u64 values
 *   BROADCAST  ONE canonical cell, written to every row of the segment
 * and the whole batch is written in out_form: CANONICAL (a witness, as the prover takes it) or MONTGOMERY (as
 * h2_dev_batch_mont leaves a canonical column: keygen's fixed columns).  `segments` is a HOST array, read before the call
 * returns; dst and src are device pointers (sources may be anywhere on the device: staged values or tensors computed there).
 * No two segments of a call may write the same cell (which one wins is undefined: a caller that wants "the later
 * assignment wins" places the earlier one by an earlier call).  Segments with count 0 are skipped.
 * d_scratch: h2_cells_place_scratch_bytes(count) bytes, 16-byte aligned.  Asynchronous on `stream`.  Returns H2_ERR_INVALID
 * without touching a device, h2_last_error naming the reason, for a null or misaligned pointer, an unknown form, stride 0, a
 * segment whose last row is not below n, or too small a scratch. */
enum { H2_PLACE_FORM_CANONICAL = 0, H2_PLACE_FORM_COMPACT = 1, H2_PLACE_FORM_BROADCAST = 2 };
enum { H2_PLACE_OUT_CANONICAL = 0, H2_PLACE_OUT_MONTGOMERY = 1 };
typedef struct {
    void *dst;
    const void *src;
    uint64_t first_row;
    uint64_t stride;
    uint64_t count;
    uint32_t form;
    uint32_t reserved;
} h2_place_segment;
size_t h2_cells_place_scratch_bytes(size_t count);
int h2_dev_cells_place(const h2_place_segment *segments, size_t count, size_t n, uint32_t out_form, void *d_scratch,
                       size_t scratch_bytes, void *stream);

/* Selectors (plonk/circuit.rs:253-311) on the device: the front end keeps every selector's activations as a bitmap and
 * writes the fixed columns `ConstraintSystem::compress_selectors` (plonk/circuit.rs:1603-1734) asks for from the bits.
 * d_bitmaps: num_selectors x ceil(n / 32) u32 words, selector-major; bit r % 32 of word r / 32 of a selector is its row r.
 * The CALLER zeroes them before the first mark.  1 <= num_selectors < 2^16, 1 <= n <= 2^31.
 *   h2_dev_selectors_mark       sets the bit of every row of `count` segments (selector, first_row, stride, count: rows
 *                               first_row + j * stride, j < count) by ONE launch whose work is split by cells.  A row may be
 *                               enabled any number of times, within a call or across calls.  `segments` is a HOST array, read
 *                               before the call returns.  d_scratch: h2_selectors_mark_scratch_bytes(count) bytes, 16-byte
 *                               aligned.
 *   h2_dev_selectors_conflicts  d_matrix (num_selectors^2 bytes, row-major) := 1 where two DIFFERENT selectors share a row
 *                               below n, else 0: exact, symmetric, zero diagonal (the exclusion matrix of
 *                               plonk/circuit/compress_selectors.rs:102-127).
 *   h2_dev_selectors_combine    writes `columns` columns of n rows (n x 4 u64).  Column c has the members
 *                               members[first_member .. first_member + num_members): a row takes the 32-byte `value` of the
 *                               member whose selector is enabled there (the last such member, should several be), else zero.
 *                               The values are written as given: the caller supplies them in out_form (CANONICAL or
 *                               MONTGOMERY, the H2_PLACE_OUT_* numbers), the form the columns are then in.  `plan` and
 *                               `members` are HOST arrays, read before the call returns.
 *   h2_selectors_combine        the same over HOST bitmaps and HOST columns, on the host (tests).
 * The device calls are asynchronous on `stream`.  All return H2_ERR_INVALID without touching a device, h2_last_error naming the
 * reason, for a null or misaligned pointer, n or num_selectors out of range, a selector index >= num_selectors, stride 0, a
 * segment whose last row is not below n, members outside the member table, a value not below the modulus, an unknown form or
 * too small a scratch. */
typedef struct {
    uint32_t selector;
    uint32_t reserved;
    uint64_t first_row;
    uint64_t stride;
    uint64_t count;
} h2_selector_segment;
typedef struct {
    void *dst;
    uint32_t first_member;
    uint32_t num_members;
} h2_selector_column;
typedef struct {
    uint64_t value[4];
    uint32_t selector;
    uint32_t reserved;
} h2_selector_member;
size_t h2_selectors_mark_scratch_bytes(size_t count);
int h2_dev_selectors_mark(const h2_selector_segment *segments, size_t count, size_t n, size_t num_selectors, void *d_bitmaps,
                          void *d_scratch, size_t scratch_bytes, void *stream);
int h2_dev_selectors_conflicts(const void *d_bitmaps, size_t num_selectors, size_t n, void *d_matrix, void *stream);
int h2_dev_selectors_combine(const h2_selector_column *plan, size_t columns, const h2_selector_member *members,
                             size_t num_members, size_t n, size_t num_selectors, const void *d_bitmaps, uint32_t out_form,
                             void *stream);
int h2_selectors_combine(const h2_selector_column *plan, size_t columns, const h2_selector_member *members, size_t num_members,
                         size_t n, size_t num_selectors, const void *bitmaps, uint32_t out_form);

/* Rational cells (`Assigned<F>`, plonk/assigned.rs) resolved to field elements, as poly::batch_invert_assigned
 * (poly.rs:148-173) does for keygen's fixed columns and the fork's assign_advice cell by cell (plonk/prover.rs:1607-1612):
 * for each of `cols` columns of n rows, out[r] = num[r] / den[r], and 0 where den[r] = 0 (`Assigned::evaluate`).  All
 * columns of a call are resolved by one launch (more than fit its arguments: in slices), with one field inversion per
 * workgroup and no scratch: `out` holds the working state, so no out column may overlap a num or den column of the call.
 * d_num, d_den, d_rows, d_out, the form codes and counts are HOST arrays of `cols` entries.  Each column is read in its own
 * form (CANONICAL / MONTGOMERY: 4 u64 per cell, reduced; COMPACT: one u64 per cell, as h2_dev_widen_u64 takes them --
 * the H2_RANGE_CHECK_FORM_* numbers) and every out column is written in out_form, CANONICAL or MONTGOMERY.
 *   dense   d_rows == NULL or d_rows[i] == NULL: d_den[i] has n cells (counts[i] is not read)
 *   sparse  d_rows[i] = counts[i] <= n strictly increasing u32 row indices and d_den[i] has counts[i] cells, the
 *           denominators of those rows (the reference's `Option<F>`); every other row is num[r] in out_form
 * The outcome is d_status, H2_ASSIGNED_STATUS_WORDS u32 per column = {code, number of zero denominators, first row with a
 * zero denominator or 0xffffffff, first bad index into rows or 0xffffffff}, final when the stream reaches the end of the
 * call:
 *   OK        resolved
 *   BAD_ROWS  an entry of rows is not below n or not above its predecessor; nothing was written through it and the
 *             content of the column is unspecified
 * Asynchronous on `stream`.  Returns H2_ERR_INVALID without touching a device, h2_last_error naming the argument, for a
 * null array or element (d_rows[i] may be null; d_den[i] when counts[i] == 0), an unknown form code, n == 0 or n >= 2^32,
 * counts[i] > n, a misaligned column (16 bytes for 4-u64 cells, 8 for compact ones, 4 for rows) or an out column that
 * overlaps a num, den, rows or other out column.  cols == 0 does nothing.
 * h2_assigned_resolve: the same on HOST arrays (8-byte alignment does), status included, through the host-slice call
 * scope; a dense column of page-locked memory is resolved chunk by chunk under its own transfers. */
enum { H2_ASSIGNED_FORM_CANONICAL = 0, H2_ASSIGNED_FORM_MONTGOMERY = 1, H2_ASSIGNED_FORM_COMPACT = 2 };
enum { H2_ASSIGNED_OK = 0, H2_ASSIGNED_BAD_ROWS = 1 };
#define H2_ASSIGNED_STATUS_WORDS 4
int h2_dev_assigned_resolve(const void *const *d_num, const uint32_t *num_forms, const void *const *d_den,
                            const uint32_t *den_forms, const uint32_t *const *d_rows, const uint64_t *counts,
                            void *const *d_out, size_t cols, size_t n, uint32_t out_form, void *d_status, void *stream);
int h2_assigned_resolve(const void *const *num, const uint32_t *num_forms, const void *const *den,
                        const uint32_t *den_forms, const uint32_t *const *rows, const uint64_t *counts, void *const *out,
                        size_t cols, size_t n, uint32_t out_form, uint32_t *status);

/* The permutation argument's cycle mapping from the copy constraints (plonk/permutation/keygen.rs:49-145: the cycles the
 * copies induce, every cycle sorted by (column, row), each cell mapped to its successor and the last to the first), built
 * on the device.  d_copies: `copies` x 4 u32, row-major, each row (left column position, left row, right column position,
 * right row) with column positions below n_columns and rows below n; null is allowed when copies == 0, which gives the
 * identity.  d_map_col, d_map_row: n_columns x n u32 each, column-major (entry c n + r = where cell (c, r) maps to) -- what
 * h2_dev_check_copies reads whole and h2_dev_permutation_sigma reads column by column.  n_columns * n < 2^32.
 * The outcome is d_status, H2_PERM_MAPPING_STATUS_WORDS u32 = {code, index of the lowest offending copy or 0xffffffff},
 * final when the stream reaches the end of the call:
 *   OK             the mapping is complete
 *   OUT_OF_BOUNDS  a copy names a column position >= n_columns or a row >= n; the mapping's content is unspecified
 *   INTERNAL       a bounded loop of the union-find ran out (a defect, never an input); the content is unspecified
 * The mapping is a function of the copies as a SET of pairs: their order, duplicates, orientation and the scheduling of the
 * device leave every byte of it the same, call after call.
 * d_scratch: h2_permutation_mapping_scratch_bytes(n_columns, n, copies) bytes, 16-byte aligned (as d_copies); the function
 * returns 0 for sizes the call refuses.  Asynchronous on `stream`.  Returns H2_ERR_INVALID without touching a device,
 * h2_last_error naming the argument, for a null output, status or scratch pointer, null d_copies with copies > 0,
 * n_columns == 0, n == 0, n_columns * n >= 2^32, a misaligned pointer or too small a scratch.
 * h2_dev_permutation_mapping_phases is the same call timed for tools/keygen_bench.py: phase_ms[0 .. 2] = milliseconds
 * (HIP events) of the components, of compaction + sort and of the successors; it returns when the stream has drained.
 * H2_PERM_MAPPING_SORT_TILE: the (label, cell) pairs a workgroup of the radix sort ranks (tests size their inputs around it). */
enum { H2_PERM_MAPPING_OK = 0, H2_PERM_MAPPING_OUT_OF_BOUNDS = 1, H2_PERM_MAPPING_INTERNAL = 2 };
#define H2_PERM_MAPPING_STATUS_WORDS 2
#define H2_PERM_MAPPING_SORT_TILE 4096
size_t h2_permutation_mapping_scratch_bytes(size_t n_columns, size_t n, size_t copies);
int h2_dev_permutation_mapping(const uint32_t *d_copies, size_t copies, size_t n_columns, size_t n, uint32_t *d_map_col,
                               uint32_t *d_map_row, uint32_t *d_status, void *d_scratch, size_t scratch_bytes, void *stream);
int h2_dev_permutation_mapping_phases(const uint32_t *d_copies, size_t copies, size_t n_columns, size_t n,
                                      uint32_t *d_map_col, uint32_t *d_map_row, uint32_t *d_status, void *d_scratch,
                                      size_t scratch_bytes, float *phase_ms, void *stream);

/* Fixed-base multiplication, the work of Params::unsafe_setup (poly/commitment.rs:56-124: g[i] = [s^i] G,
 * g_lagrange[i] = [l_i(s)] G, one variable-base multiplication per point under `parallelize` there):
 * points[i] = [scalars[i]] B, with B given as d_table[j] = [2^j] B for j < 254 (affine Montgomery, 64 B each);
 * scalars Montgomery Fr, output affine Montgomery ((0,0) for a zero scalar).  Asynchronous on `stream`. */
int h2_dev_fixed_base_mul(const void *d_scalars, const void *d_table, size_t n, void *d_points, void *stream);

/* Compressed G1 points of the SRS file -- Params::{write, read}, poly/commitment.rs:241-294 (`to_bytes` / `from_bytes`
 * per point; the reference decompresses with a rayon `parallelize`).  32 bytes per point: x little-endian, bit 7 of
 * byte 31 = parity of the canonical y, identity = zeros (convention of this build: the encoding of pairing_bn256@30b052f
 * could not be checked).  d_points: n x 64 B affine Montgomery.  Decompress is synchronous and returns H2_ERR_INVALID
 * when an encoding is not a curve point (the reference unwraps `from_bytes`). */
int h2_dev_points_decompress(const void *d_bytes, size_t n, void *d_points, void *stream);
int h2_dev_points_compress(const void *d_points, size_t n, void *d_bytes, void *stream);

/* The NTT over G1: n = 2^log_n points (0 <= log_n <= 28), affine Montgomery (64 B each, identity = (0,0)), natural order
 * in and out.  The Lagrange basis of an SRS from its powers alone -- g_lagrange[i] = [L_i(s)] G from g[i] = [s^i] G, what
 * Params::unsafe_setup computes from s itself (poly/commitment.rs:85-112) -- and its inverse:
 *   inverse = 1:  d_out[i] = n^-1 sum_j w^(-ij) d_in[j]
 *   inverse = 0:  d_out[i] = sum_j w^(ij) d_in[j]
 * w = ROOT_OF_UNITY^(2^(28 - log_n)), the omega of EvaluationDomain::new for 2^log_n rows (poly/domain.rs:44-149).  Every
 * result is the exact group element (identity inputs and cancellations included), normalised to affine.
 * d_scratch: device memory of at least h2_g1_ntt_scratch_bytes(log_n) bytes (128 B per point; 0 for log_n > 28), caller-owned
 * and free again when the work on `stream` has run.  d_out may equal d_in.  Asynchronous on `stream`; the first call for a
 * (log_n, direction) builds the twiddle tables of the field NTT's plan for w (or w^-1) and shares them with it.  Returns
 * H2_ERR_INVALID, without touching the device, for log_n > 28, inverse not 0 or 1, a null pointer or too small a scratch.
 * (The reference has no such entry point: its setup keeps s.) */
size_t h2_g1_ntt_scratch_bytes(uint32_t log_n);
int h2_dev_g1_ntt(const void *d_in, void *d_out, uint32_t log_n, int inverse, void *d_scratch, size_t scratch_bytes,
                  void *stream);

/* A table of points times a column of scalars, point by point: d_out[i] = [d_scalars[i]] d_points[i] for i < n.  The work of
 * an SRS update, g[i] -> [tau^i] g[i] (the reference has no such entry point: its only constructor of an SRS is
 * Params::unsafe_setup).  Points affine Montgomery, 64 B each, identity (0,0); scalars Montgomery Fr, as
 * h2_dev_fixed_base_mul takes them.  Every output is the exact group element normalised to the one affine form; a zero
 * scalar or an identity input gives (0,0).  d_out may equal d_points.  One lane per point over signed 3-bit digits of the
 * scalar (csrc/g1mul.hip).  Asynchronous on `stream`.  H2_ERR_INVALID, without touching the device, for a null pointer with
 * n > 0 or n > 2^31; H2_OK for n = 0. */
int h2_dev_g1_mul_each(const void *d_points, const void *d_scalars, size_t n, void *d_out, void *stream);

/* ---- evaluate_h: the quotient numerator h(X) on the extended coset ------------------------------
 * Evaluator::evaluate_h -- plonk/evaluation.rs:778-1226 (CPU twin) / :1229-1985 (cuda).
 * The Rust side flattens its `Evaluator` (plonk/evaluation.rs:270-296) into this plain descriptor:
 * ValueSource :44-57, Calculation :95-112, value_parts, lookup_results, shuffle_results.  All column
 * pointers are extended cosets (2^extended_k Fr).  One circuit instance (the cuda path asserts it,
 * plonk/evaluation.rs:1259). */
enum { H2_VS_CONSTANT = 0, H2_VS_INTERMEDIATE = 1, H2_VS_FIXED = 2, H2_VS_ADVICE = 3, H2_VS_INSTANCE = 4 };
enum {
    H2_CALC_ADD = 0, H2_CALC_SUB = 1, H2_CALC_MUL = 2, H2_CALC_NEGATE = 3,
    H2_CALC_LC_CHALLENGE = 4, /* (a + challenge^power) * b */
    H2_CALC_LC_THETA = 5,     /* a * theta + b */
    H2_CALC_ADD_CHALLENGE = 6,/* a + challenge */
    H2_CALC_STORE = 7
};
enum { H2_CHALLENGE_BETA = 0, H2_CHALLENGE_GAMMA = 1 };
enum { H2_ANY_ADVICE = 0, H2_ANY_FIXED = 1, H2_ANY_INSTANCE = 2 };

typedef struct {
    uint32_t kind;  /* H2_VS_* */
    uint32_t index; /* constant / intermediate / column index */
    uint32_t rot;   /* index into `rotations` (columns only) */
} h2_value_source;

typedef struct {
    uint32_t op; /* H2_CALC_* */
    h2_value_source a, b;
    uint32_t challenge; /* H2_CHALLENGE_* (LC_CHALLENGE, ADD_CHALLENGE) */
    uint32_t power;     /* LC_CHALLENGE exponent p (p <= 1 means the challenge itself) */
} h2_calculation;

typedef struct {
    uint32_t k, extended_k;
    uint32_t blinding_factors; /* cs.blinding_factors(): last_rotation = -(blinding_factors + 1) */
    uint32_t chunk_len;        /* cs.degree() - 2: permutation columns per product set */
    /* the straight-line program */
    const uint64_t *constants;          uint32_t n_constants;    /* Fr each */
    const int32_t *rotations;           uint32_t n_rotations;
    const h2_calculation *calculations; uint32_t n_calculations;
    const h2_value_source *value_parts; uint32_t n_value_parts;
    /* lookup_results[t] = (table, products[sets], sums[sets]); flattened per lookup as
     * table, product_0, sum_0, product_1, sum_1, ...  (lookup_sets[t] = number of sets >= 1) */
    uint32_t n_lookups; const uint32_t *lookup_sets; const h2_calculation *lookup_calcs;
    /* shuffle_results[i] = (input, shuffle), flattened */
    uint32_t n_shuffles; const h2_calculation *shuffle_calcs;
    /* columns */
    const uint64_t *const *fixed;    uint32_t n_fixed;
    const uint64_t *const *advice;   uint32_t n_advice;
    const uint64_t *const *instance; uint32_t n_instance;
    const uint64_t *l0, *l_last, *l_active_row;
    /* permutation argument: sets[i].permutation_product_coset, p.columns, pk.permutation.cosets */
    uint32_t n_perm_sets;    const uint64_t *const *perm_z;
    uint32_t n_perm_columns; const uint32_t *perm_col_type; const uint32_t *perm_col_index;
    const uint64_t *const *perm_sigma;
    /* logup lookups: z cosets of every set of every lookup (in order), m coset per lookup */
    const uint64_t *const *lookup_z; const uint64_t *const *lookup_m;
    /* shuffles: product coset per shuffle */
    const uint64_t *const *shuffle_z;
    /* challenges and field constants */
    uint64_t y[4], beta[4], gamma[4], theta[4];
    uint64_t delta[4], zeta[4], extended_omega[4]; /* FieldExt::DELTA, ::ZETA, domain.get_extended_omega() */
    /* must be NULL (the slot of round 4's caller-supplied kernel: the library now generates, compiles and caches the
     * program's kernels itself, see h2_evalh_prepare) */
    const void *reserved;
    /* H2_EVALH_INTERPRET: run this call on the interpreter kernels even when generated ones exist (tests compare the two) */
    uint32_t flags;
    /* rows of the domain to evaluate: `values[row_begin .. row_begin + row_count)` are written, nothing else (row_count = 0:
     * the whole domain).  Column values are still read at rotated indices modulo the domain, so the rows
     * [row_begin - (blinding_factors + 1) * rot_scale ..., row_begin + row_count + max rotation * rot_scale) of every column
     * must be valid.  For callers that split one evaluation over several devices by row range. */
    uint32_t row_begin, row_count;
} h2_evalh_desc;
enum { H2_EVALH_INTERPRET = 1 };

/* Host buffers everywhere (descriptor and every pointer in it); values: 2^extended_k Fr out. */
int h2_evaluate_h(const h2_evalh_desc *desc, uint64_t *values);
/* The cuda `Evaluator::evaluate_h`'s own shape (plonk/evaluation.rs:1229-1241: advice / instance as coefficient forms,
 * a proving key without extended cosets, plonk.rs:226-240): every column pointer of the descriptor -- fixed, advice,
 * instance, l0, l_last, perm_z, perm_sigma, lookup_z, lookup_m, shuffle_z -- is a HOST coefficient vector of 2^k Fr;
 * l_active_row is HOST extended values (2^extended_k, as the reference keeps it); values: 2^extended_k Fr out (host).
 * Each distinct vector is uploaded once; the extended domain is visited one coset of the n-th roots of unity at a
 * time, so device memory is (distinct columns) x 2 x 2^k x 32 B + two extended vectors whatever extended_k is -- the
 * memory-bounded route (the reference bounds it with a 5-entry cache of extended FFTs, evaluation_gpu.rs:335-468). */
int h2_evaluate_h_coeff(const h2_evalh_desc *desc, uint64_t *values);
/* The vanishing argument's quotient h(X) in COEFFICIENT form from coefficient forms, in one call: the three steps the
 * reference's cuda path takes on host vectors of 2^extended_k elements -- Evaluator::evaluate_h (plonk/evaluation.rs:1229-1985,
 * the descriptor as for h2_evaluate_h_coeff), EvaluationDomain::divide_by_vanishing_poly (poly/domain.rs:354-373) and
 * extended_to_coeff (:328-350), the latter two in vanishing::Argument::construct (plonk/vanishing/prover.rs:69-112) -- with the
 * numerator's values never leaving the device.  out: out_len = n * quotient_poly_degree coefficients (the truncation of
 * domain.rs:346-347); t_evaluations / t_len as h2_divide_by_vanishing_poly, the scalars as h2_extended_to_coeff. */
int h2_quotient_poly_coeff(const h2_evalh_desc *desc, const uint64_t *t_evaluations, size_t t_len,
                           const uint64_t g_coset[4], const uint64_t g_coset_inv[4],
                           const uint64_t extended_omega_inv[4], const uint64_t extended_ifft_divisor[4],
                           uint64_t *out, size_t out_len);
/* Column / table pointers inside `desc` are DEVICE pointers (the descriptor itself and its program
 * arrays -- constants, rotations, calculations, ... and the pointer tables -- stay in host memory).
 * d_values: 2^extended_k Fr on the device.  Work space is taken from the library's arena. */
int h2_dev_evaluate_h(const h2_evalh_desc *desc, void *d_values, void *stream);

/* The generated form of evaluate_h.  The cuda `Evaluator::evaluate_h` of the reference is self-contained in the host
 * language (plonk/evaluation.rs:1229-1985, plonk/evaluation_gpu.rs:594-803); so is this: the first time a descriptor's
 * program (constants, rotations, calculations, value parts, lookup / shuffle calculations, permutation shape) reaches one
 * of the three entry points above, the library turns it into straight-line HIP -- intermediates in registers, every
 * argument's terms folded in, terms that share a factor (l_0, l_last, l_active_row, a gate selector) summed before the
 * factor multiplies them (exact field arithmetic: the same bits) -- compiles it with hipRTC for gfx950, keeps the code
 * object in memory and in a private directory (H2_JIT_CACHE, default <tmp>/halo2_hip_jit_<uid>) under the hash of the
 * program, and launches it for every later call with the same program.  H2_EVALH_JIT=0 (environment) or
 * H2_EVALH_INTERPRET (per call) keeps the interpreter kernels; so does a machine without libhiprtc.so (one warning on
 * stderr).  Both are HIP paths with identical results.
 *
 * h2_evalh_prepare  does that work ahead of the first proof -- at keygen -- for the CURRENT device (h2_set_device) and
 *                   reports what was built; pointers to columns inside `desc` are not read.
 * h2_evalh_compile  generates and compiles into the caches without touching a device (works on a machine without a GPU).
 * h2_evalh_source   the generated source of stage `stage` (for inspection): copies up to `cap` bytes including the
 *                   terminating NUL into `buf` and stores the full length (without NUL) in *len.
 * All three may be called from several threads at once (rayon workers at keygen), for the same program too.  A cache file
 * carries a SHA-256 trailer: a torn or damaged one is a miss and is rebuilt; every writer renames a file of its own into place.
 * Loaded code objects are kept per (program, device), at most H2_EVALH_PLANS_MAX of them (environment, default 128): the least
 * recently used one is unloaded and comes back from the disk cache when its program is seen again. */
typedef struct {
    uint32_t stages;                     /* kernels the program was cut into (1 unless it is too wide for one) */
    uint32_t terms;                      /* y-folded terms of the numerator: value parts + argument terms */
    uint32_t products_per_row;           /* field products the generated kernels spend per row */
    uint32_t reference_products_per_row; /* ... and the formulas of evaluation.rs:875-1219 as written */
    uint32_t vectors_read;               /* distinct column vectors read per row */
    uint32_t max_registers;              /* VGPRs + AGPRs of the widest stage */
    uint32_t scratch_bytes;              /* per-lane scratch of the worst stage (0 = no spills) */
    uint32_t from_cache;                 /* 1 = memory, 2 = disk, 0 = compiled now */
    uint32_t fused_pairs_per_row;        /* pairs of those products that share one Montgomery reduction (a b + c d: 3/4 of the work) */
} h2_evalh_info;
int h2_evalh_prepare(const h2_evalh_desc *desc, h2_evalh_info *info);
int h2_evalh_compile(const h2_evalh_desc *desc, h2_evalh_info *info);
int h2_evalh_source(const h2_evalh_desc *desc, uint32_t stage, char *buf, size_t cap, size_t *len);
/* The argument block stage `stage` of the generated program receives for THIS descriptor (its column pointers, challenges and
 * constants), `values`, the power tables of extended_omega (tw_lo[i] = omega^i for i < min(2^extended_k, 4096), tw_hi[j] =
 * omega^(4096 j)) and the row range -- exactly the bytes the launch passes by value; host arithmetic only, no device needed.
 * For inspection and for tests: with h2_evalh_source it lets a test compile the generated text for the host and run it against
 * the CPU oracle (tests/test_evalh_host_exec.py).  Copies into `buf` (cap bytes; 0 = only report) and stores the size in *len. */
int h2_evalh_stage_args(const h2_evalh_desc *desc, uint32_t stage, uint64_t *values, const uint64_t *tw_lo, const uint64_t *tw_hi,
                        uint64_t row_begin, uint64_t row_end, void *buf, size_t cap, size_t *len);
/* stages of generated kernels launched so far in this process (a test's proof that they, not the interpreter, ran) */
uint64_t h2_evalh_generated_launches(void);

/* ---- device memory and streams for hosts without a HIP binding of their own ------------------
 * The h2_dev_* entry points below take HIP device pointers and a HIP stream.  A host that already links HIP (or, like
 * the Python harness, borrows torch's allocator and streams) passes its own; a host that does not -- the Rust side of
 * INTEGRATION.md holding `Polynomial` values on the device between calls -- gets what it needs from these: plain
 * hipMalloc / hipFree / hipMemcpyAsync / stream wrappers on the CURRENT device (h2_set_device; device 0 by default).
 * h2_dev_download synchronises `stream` before it returns; h2_dev_upload is asynchronous for pinned host memory
 * (h2_host_alloc_pinned) and otherwise returns when the source has been read. */
int h2_set_device(int device);
int h2_dev_alloc(size_t bytes, void **d_out);
int h2_dev_free(void *d_ptr);
int h2_host_alloc_pinned(size_t bytes, void **out);
int h2_host_free_pinned(void *ptr);
int h2_stream_create(void **stream_out);
int h2_stream_destroy(void *stream);
int h2_stream_synchronize(void *stream);
int h2_dev_upload(void *d_dst, const void *src, size_t bytes, void *stream);
int h2_dev_download(void *dst, const void *d_src, size_t bytes, void *stream);

/* One coset of a larger domain, without a separate scaling pass (the unit of the coset-by-coset quotient: multi-GPU proofs,
 * memory-budgeted proofs, and circuits whose extended domain is more than (degree - 1) n points wide):
 *   h2_dev_coset_ntt   out[i] = sum_t coeffs[t] g^t omega^(i t)  -- coeff_to_extended (poly/domain.rs:270-287) restricted to
 *                      the points g omega^i; g^t is applied on the first pass's load from a cached two-level table.
 *                      d_coeffs is left untouched unless d_out == d_coeffs.
 *   h2_dev_coset_intt  in place: the coefficients of the polynomial of degree < n with the values d_a on g H;
 *                      a[t] *= divisor * g_inv^t fused into the last pass's store (divisor = 1/n).
 * Same values as h2_dev_distribute_powers + h2_dev_ntt / h2_dev_intt + h2_dev_distribute_powers. */
int h2_dev_coset_ntt(const void *d_coeffs, void *d_out, void *d_tmp, uint32_t log_n, const uint64_t g[4],
                     const uint64_t omega[4], void *stream);
int h2_dev_coset_intt(void *d_a, void *d_tmp, uint32_t log_n, const uint64_t g_inv[4], const uint64_t omega_inv[4],
                      const uint64_t divisor[4], void *stream);

/* Several vectors through one transform plan, up to 16 per launch (the columns of a wide witness: plonk/prover.rs:643-646
 * runs them as a par_iter).  A 2^20-point pass alone is one resident round of the chip, every workgroup waiting out its own
 * load -> stages -> store chain; with the tiles of many vectors in one grid the rounds overlap.  d_a / d_coeffs / d_out:
 * HOST arrays of `count` device pointers; d_tmp: min(count, 16) x 2^log_n Fr of scratch (NULL allowed for log_n <= 8).
 * Same values as `count` calls of h2_dev_ntt / h2_dev_intt / h2_dev_coset_ntt. */
int h2_dev_ntt_batch(void *const *d_a, size_t count, void *d_tmp, const uint64_t omega[4], uint32_t log_n, void *stream);
int h2_dev_intt_batch(void *const *d_a, size_t count, void *d_tmp, const uint64_t omega_inv[4], const uint64_t divisor[4],
                      uint32_t log_n, void *stream);
int h2_dev_coset_ntt_batch(const void *const *d_coeffs, void *const *d_out, size_t count, void *d_tmp, uint32_t log_n,
                           const uint64_t g[4], const uint64_t omega[4], void *stream);
/* `count` coefficient vectors of 2^k elements to the extended domain (h2_dev_coeff_to_extended each); d_out[i] != d_coeffs[i];
 * d_tmp: min(count, 16) x 2^extended_k Fr. */
int h2_dev_coeff_to_extended_batch(const void *const *d_coeffs, void *const *d_out, size_t count, void *d_tmp, uint32_t k,
                                   uint32_t extended_k, const uint64_t g_coset[4], const uint64_t g_coset_inv[4],
                                   const uint64_t extended_omega[4], void *stream);

/* ---- device-resident entry points ---------------------------------------------------------- */
/* Same semantics on HIP device pointers.  d_tmp: scratch of 2^log_n Fr (may be NULL for
 * log_n <= 8).  Results land in d_a (in place from the caller's view).
 * Device memory the library keeps per (device, log_n, omega) for the life of the process: the twiddle tables of the
 * transform (a few MiB) and, for 2^18 .. 2^26 points, the last pass's complete twiddle set -- 32 B x 2^log_n, one per
 * divisor it is used with (512 MiB at 2^24; built on first use; the environment variable H2_NTT_LAST_TABLE=0 or a failed
 * allocation leave the smaller two-level tables in use, at one more multiplication per element). */
int h2_dev_ntt(void *d_a, void *d_tmp, const uint64_t omega[4], uint32_t log_n, void *stream);
int h2_dev_intt(void *d_a, void *d_tmp, const uint64_t omega_inv[4], const uint64_t divisor[4], uint32_t log_n,
                void *stream);
int h2_dev_coeff_to_extended(const void *d_coeffs, void *d_out, void *d_tmp, uint32_t k, uint32_t extended_k,
                             const uint64_t g_coset[4], const uint64_t g_coset_inv[4],
                             const uint64_t extended_omega[4], void *stream);
int h2_dev_extended_to_coeff(void *d_a, void *d_tmp, uint32_t extended_k, const uint64_t g_coset[4],
                             const uint64_t g_coset_inv[4], const uint64_t extended_omega_inv[4],
                             const uint64_t extended_ifft_divisor[4], void *stream);
/* MSM over device-resident scalars and bases.  d_scratch/scratch_bytes: device workspace sized by
 * h2_msm_scratch_bytes(n, max_bits).  out_xyz is HOST memory: the call synchronises `stream` to
 * read back the per-window partial sums (<= a few KB) and finishes the window combine on the host. */
/* Scalar distributions: zero scalars cost nothing; a column whose values crowd a few buckets takes the skew path of
 * the sort; a non-zero value found on >= 1/4 of 64 sampled rows (a grand-product column over padding rows) gets a window
 * of its own -- one addition per such row plus one scalar multiplication on the host.  The result is the same group
 * element in every case; h2_msm_scratch_bytes covers the larger layout. */
size_t h2_msm_scratch_bytes(size_t n, uint32_t max_bits);
/* the Pippenger shape the library will use: window bits c, number of windows, buckets per window */
int h2_msm_shape(size_t n, uint32_t max_bits, uint32_t *c, uint32_t *windows, uint32_t *buckets_per_window);
/* What the MSM launcher did, for reporting and for tests.  Part of what one launch runs depends on the sampled scalars (a
 * dominant value, whether a table pays), so it cannot be told from n and the bound: every launch of the pipeline appends
 * one record -- the very values it hands its kernels -- to a list of the calling thread.  The list is emptied when
 * h2_dev_msm / _batch / _batch_ex (or a host-slice MSM that ends in them) is entered, so afterwards it holds that call's
 * launches in launch order: one for h2_dev_msm, one per fused group and then one per remaining column for a batch.  Host
 * only: no device work, no synchronisation, no allocation in the steady state. */
enum { H2_MSM_FORM_WINDOWED = 0, H2_MSM_FORM_TABLE = 1, H2_MSM_FORM_FUSED = 2, H2_MSM_FORM_COUNT = 3 };
enum {
    H2_MSM_PART_2048 = 0,      /* k_partition<2048> over every key array */
    H2_MSM_PART_16384 = 1,     /* k_partition<16384> over every key array (a table with more than 2^10 partitions) */
    H2_MSM_PART_TWO_LEVEL = 2, /* k_part_a + k_part_b over the digit arrays of a table */
    H2_MSM_PART_COUNT = 3
};
enum { H2_MSM_FINISH_QUADS = 0, H2_MSM_FINISH_LANES = 1, H2_MSM_FINISH_COUNT = 2 }; /* k_finish / k_finish_lane */
enum { H2_MSM_REDUCE_GROUPS = 0, H2_MSM_REDUCE_PLANES = 1, H2_MSM_REDUCE_COUNT = 2 }; /* k_reduce / k_reduce_chunks + _planes */
typedef struct {
    uint32_t form;      /* H2_MSM_FORM_* */
    uint32_t max_bits;  /* the bound k_digits was given */
    /* the shape: window bits, windows c bits wide (the rest c - 1), digit windows, windows run, key arrays, row ranges and
     * their shift, fused columns and windows per column, buckets per window and in all, the sort's split of a bucket id,
     * partitions, slice length, k_reduce's chunk length and workgroups per window, the bit-plane reduce, the two-level
     * partition */
    uint32_t c, wfull, W, Wt, Wk, R, range_shift, cols, Wc, nb, nbt, lo_bits, hi_bits, np, log_s, qm, RG;
    uint32_t planes, chunks, plane_seg, plane_l, two_level, a_bits;
    uint32_t hot_on;          /* a dominant value has its own window (fused: any column has) */
    uint32_t block_sums;      /* ... and whole 256-row blocks of it enter as one tabulated point */
    uint32_t partition;       /* H2_MSM_PART_* */
    uint32_t hot_partitioned; /* two-level: the dominant-value array went through k_partition<16384> on its own */
    uint32_t stage_cap;       /* k_bucket_sort stages partitions of up to this many entries in LDS; 0: none */
    uint32_t skew_threshold;  /* ... and counts larger ones with wave-aggregated atomics */
    uint32_t hot_partition;   /* the partition k_copy_hot moves; 0xffffffff: none (fused: see hot_mask) */
    uint32_t finish;          /* H2_MSM_FINISH_* */
    uint32_t acc_waves;       /* k_acc_slice<4> or <5> */
    uint32_t reduce;          /* H2_MSM_REDUCE_* */
    uint64_t hot_mask;        /* fused: the columns with a dominant value */
    uint64_t n, entries;
    uint64_t scratch;         /* device address of the scratch slice, then byte offsets into it */
    uint64_t off_keys, off_sorted, off_pbase, off_starts, off_heavy, off_buckets, total;
} h2_msm_launch_info;
/* Copies the calling thread's records to out[0 .. min(count, cap)) and returns their count, which may exceed cap
 * (out may be null when cap is 0). */
size_t h2_msm_last_launches(h2_msm_launch_info *out, size_t cap);
/* The passes the library will run for a transform of 2^log_n points (best_fft, arithmetic.rs:546) whose first 2^in_log
 * inputs are live and the rest zero padding (in_log == log_n: none), for reporting and for tests: computed by the
 * launcher's own split, geometry and kernel selector under the same once-per-process H2_NTT_* knobs.  Host only.  Writes
 * one entry per pass to out[0 .. cap) and the number of passes to *count; log_n = 0 has none.  log_n > 28,
 * in_log > log_n, a null pointer or cap < *count: H2_ERR_INVALID (*count is set in the last case). */
typedef struct {
    uint32_t bits;    /* width of the pass: 2^bits rows per tile */
    uint32_t log_c;   /* 2^log_c columns per tile */
    uint32_t threads; /* lanes per workgroup */
    uint32_t radix4;  /* two stages per LDS round trip, constant-operand twiddles ((value, quotient) pairs) */
    uint32_t fixed;   /* the common geometry: 8 bits, 4 columns, 256 lanes */
    uint32_t zskip;   /* leading stages pruned by zero padding: min(log_n - in_log, bits) on the first of several passes */
    uint32_t kernel;  /* H2_NTT_KERNEL_* */
} h2_ntt_pass_shape;
enum {
    H2_NTT_KERNEL_PASS8_DP = 0, /* k_ntt_pass8<true>: the common 8-bit pass, not last */
    H2_NTT_KERNEL_PASS8 = 1,    /* k_ntt_pass8<false>: the common 8-bit pass, last */
    H2_NTT_KERNEL_R4_DP = 2,    /* k_ntt_pass<true, true>: another width or padding to skip, from 2^18, not last */
    H2_NTT_KERNEL_R4 = 3,       /* k_ntt_pass<true, false>: the same, last */
    H2_NTT_KERNEL_R2 = 4,       /* k_ntt_pass<false>: every pass below 2^18 */
    H2_NTT_KERNEL_COUNT = 5
};
int h2_ntt_shape(uint32_t log_n, uint32_t in_log, h2_ntt_pass_shape *out, size_t cap, size_t *count);
int h2_dev_msm(const void *d_scalars, const void *d_bases, size_t n, uint32_t max_bits, void *d_scratch,
               size_t scratch_bytes, uint64_t out_xyz[12], void *stream);
/* `count` MSMs over the SAME bases (one per column: plonk/prover.rs:293-299 commits every advice column
 * against g_lagrange; :477-487, :540-549 the z polynomials).  d_scalars: host array of `count` device
 * pointers.  scratch_bytes >= 2 * round_up(h2_msm_scratch_bytes(n, max_bits), 256): consecutive MSMs
 * alternate between two internal streams so one MSM's latency-bound bucket reduction overlaps the next
 * one's accumulation.  out_xyz: count x 12 u64 in HOST memory.  Synchronous. */
int h2_dev_msm_batch(const void *const *d_scalars, size_t count, const void *d_bases, size_t n, uint32_t max_bits,
                     void *d_scratch, size_t scratch_bytes, uint64_t *out_xyz, void *stream);
/* The same pipeline with a base table and a scalar bound PER COLUMN (host arrays of `count` entries): one call commits
 * 16-bit witness columns next to full-width ones (plonk/prover.rs:293-299 computes max_bits per column) and columns over
 * g_lagrange next to one over g.  scratch_bytes >= 2 * max over the columns of round_up(h2_msm_scratch_bytes(n, max_bits_each[i]), 256)
 * (the layout depends on the window size picked for the bound: it is not monotonic in max_bits). */
/* Scratch that lets the batch entry points commit `count` columns sharing one base table and one bound as a FUSED group
 * (their windows become the windows of one wide MSM: sampling, sort launches, finish / reduce latency, synchronisation
 * and read-back are paid once per group -- what a witness of many narrow columns needs).  With less scratch (but at
 * least the 2 x h2_msm_scratch_bytes of the pipeline) the calls still succeed, column by column. */
size_t h2_msm_batch_scratch_bytes(size_t n, uint32_t max_bits, size_t count);
int h2_dev_msm_batch_ex(const void *const *d_scalars, const void *const *d_bases_each, const uint32_t *max_bits_each,
                        size_t count, size_t n, void *d_scratch, size_t scratch_bytes, uint64_t *out_xyz, void *stream);
/* Shifted-base table for a device-resident base set that is committed against repeatedly -- the SRS (`params.g`,
 * `params.g_lagrange`: poly/commitment.rs:148-170 `commit` / `commit_lagrange`; the reference re-uploads them per call,
 * arithmetic.rs:354-360).  Builds T[j][i] = [2^(o_j)] bases[i] for the `digits` (11..32) digit offsets o_j (0 = chosen from n:
 * 12 at 2^24, 14 at 2^20) in library-owned device memory (h2_dev_bases_precompute_bytes: digits x n x 64 B) and
 * remembers it under `d_bases`.  From then on every h2_dev_msm / _batch / _batch_ex whose bases lie inside
 * [d_bases, d_bases + n) and whose bound needs more windows than digits adds all digits of a scalar into ONE shared
 * bucket set: ~20 % fewer point additions at 2^24, one reduction instead of one per window, no host Horner.  The sums
 * of every 256 consecutive bases are tabulated too (n / 256 points): a column whose dominant value fills whole blocks
 * of rows (a grand product over padding rows) adds one point per block instead of 256, in either form.  Same group
 * element (multiexp_serial, arithmetic.rs:20-108).  Call it before sizing scratch with h2_msm_scratch_bytes (over a
 * table the sort keeps a second 8-byte-per-entry buffer: 5.9 GB instead of 4.6 GB at 2^24).  The
 * bases must not change while the table exists (as a guard, every MSM compares 64 sampled base rows with the table's
 * own copy first and drops a table that no longer matches); h2_dev_bases_forget(d_bases) frees it (synchronises the
 * device).
 * H2_MSM_NO_TABLE=1 in the environment ignores all tables.  Synchronous (~0.3 s at 2^24). */
int h2_dev_bases_precompute(const void *d_bases, size_t n, uint32_t digits, void *stream);
int h2_dev_bases_forget(const void *d_bases);
size_t h2_dev_bases_precompute_bytes(size_t n, uint32_t digits);
int h2_dev_eval_op(int op, void *d_res, const void *d_l, const void *d_r, int32_t l_rot, int32_t r_rot, size_t size,
                   const uint64_t c[4], void *stream);
int h2_dev_divide_by_vanishing_poly(void *d_a, size_t size, const void *d_t_evaluations, size_t t_len, void *stream);
int h2_dev_batch_mont(void *d_a, size_t n, void *stream);
int h2_dev_batch_unmont(void *d_a, size_t n, void *stream);
/* Compact witness columns.  The reference hands create_proof 32-byte cells whatever they hold (plonk/prover.rs:255-312:
 * `advice: Vec<Polynomial<C::Scalar, LagrangeCoeff>>`), and its cuda path uploads them as such; most cells of a real trace are
 * booleans, bytes, 16-bit limbs or products of a few of them.  A caller that knows a column fits 64 bits sends 8 bytes per
 * cell (d_src: n x u64 on the device, e.g. copied from pinned host memory) and widens it here to canonical scalars:
 * d_dst[i] = {d_src[i], 0, 0, 0} (n x 32 B; canonical form -- follow with h2_dev_batch_mont as for any uploaded column). */
int h2_dev_widen_u64(const void *d_src, size_t n, void *d_dst, void *stream);
/* find_max_scalar_bits (plonk/prover.rs:237-254) for `count` CANONICAL columns of n scalars resident on the device, in
 * one launch and one synchronisation: out_bits[i] (host) = bit length of the largest value of column i (0 for an all-zero
 * column) -- the `max_bits` of commit_lagrange_with_bound.  d_words: count * 32 bytes of device scratch. */
int h2_dev_max_scalar_bits(const void *const *d_cols, size_t count, size_t n, void *d_words, uint32_t *out_bits,
                           void *stream);

/* ---- checking a witness (MockProver::verify, dev.rs:932-1340) on the device ----------------------------------------------
 * Each failure is one record; kind = H2_CHECK_* | circuit << 8 (the caller's circuit-instance index, < 2^24):
 *   (GATE, part, 0, row)              gate polynomial `part` (gate by gate, then polynomial by polynomial) is non-zero at row
 *   (LOOKUP, lookup, tag, row)        the first compressed input of the row that is absent from the table: tag = set << 16 | input
 *   (SHUFFLE, group, unit, row)       the input value of the row occurs a different number of times among the two sides'
 *                                     usable rows (the reference reports rows of its sorted tuples instead: dev.rs:1209-1262,
 *                                     an order that compression destroys)
 *   (COPY, column, 0, row)            value(column, row) != value(mapping(column, row))
 *   (CELL, gate << 16 | query, region, cell_row)   h2_dev_coverage_check below: a cell an enabled gate reads, unassigned
 * Every entry adds to a caller-zeroed device u64 *d_count and appends to a caller-owned device buffer of `cap` records: one
 * agent-scope atomic per wave, a record written only when its slot is < cap -- the count is exact after the buffer fills,
 * which records were kept then is not specified.  One buffer may collect every check of a witness: one download.
 * Rows checked: the usable rows (< usable_rows) for gates, lookups and shuffles; all n rows for copies.
 * A reported failure is always real.  The gate screen (all parts Horner-folded in a random y) and a compressed lookup /
 * shuffle tuple (folded in a random theta) miss a real failure with probability <= (parts or tuple length) x n / r < 2^-200
 * (Schwartz-Zippel); copies and single-column lookups are exact.
 * Every entry is asynchronous on `stream` and returns H2_ERR_INVALID for bad arguments without touching the device. */
typedef struct { uint32_t kind, index, sub, row; } h2_check_record;
enum { H2_CHECK_GATE = 0, H2_CHECK_LOOKUP = 1, H2_CHECK_SHUFFLE = 2, H2_CHECK_COPY = 3, H2_CHECK_CELL = 4 };
/* device scratch (bytes) of h2_dev_check_lookup / h2_dev_check_shuffle for columns of n rows */
size_t h2_check_scratch_bytes(size_t n);
/* The screen's compaction: appends every row r < usable_rows with d_values[r] != 0 to d_rows (room for usable_rows u32) and
 * counts them in the caller-zeroed u64 *d_row_count (the list is in no particular order). */
int h2_dev_check_nonzero_rows(const void *d_values, size_t usable_rows, uint32_t *d_rows, uint64_t *d_row_count, void *stream);
/* The localisation: the gate program of `desc` (extended_k == k, no permutation, lookup or shuffle part; device column pointers,
 * as h2_dev_evaluate_h) interpreted at the d_rows listed by h2_dev_check_nonzero_rows only, every value part tested on its own.
 * Work space is the library's (as h2_dev_evaluate_h's interpreter). */
int h2_dev_check_gates(const h2_evalh_desc *desc, const uint32_t *d_rows, const uint64_t *d_row_count, uint32_t circuit,
                       uint64_t *d_count, h2_check_record *d_records, size_t cap, void *stream);
/* One lookup: the first usable_rows rows of the compressed table d_table against the compressed input columns d_inputs (HOST
 * array of n_inputs device pointers, in (set, input) order) with their HOST tags (set << 16 | input). */
int h2_dev_check_lookup(const void *d_table, const void *const *d_inputs, const uint32_t *tags, size_t n_inputs,
                        size_t usable_rows, size_t n, uint32_t lookup_index, uint32_t circuit, void *d_scratch,
                        size_t scratch_bytes, uint64_t *d_count, h2_check_record *d_records, size_t cap, void *stream);
/* One shuffle unit: its compressed input and shuffle columns. */
int h2_dev_check_shuffle(const void *d_input, const void *d_shuffle, size_t usable_rows, size_t n, uint32_t group, uint32_t unit,
                         uint32_t circuit, void *d_scratch, size_t scratch_bytes, uint64_t *d_count, h2_check_record *d_records,
                         size_t cap, void *stream);
/* The copy constraints: d_columns = DEVICE array of the n_columns permutation columns' device pointers; d_map_col / d_map_row:
 * device u32, n_columns x n each (the cycle mapping, column-major: entry c n + r).  A mapping entry outside the columns is
 * reported as a failure of its cell. */
int h2_dev_check_copies(const void *const *d_columns, size_t n_columns, const uint32_t *d_map_col, const uint32_t *d_map_row,
                        size_t n, uint32_t circuit, uint64_t *d_count, h2_check_record *d_records, size_t cap, void *stream);

/* ---- checking assignments (MockProver's VerifyFailure::CellNotAssigned, dev.rs:959-1000) -------------------------------------
 * Which cells each REGION of an assignment pass assigned, one bit per cell, and every cell an enabled gate reads tested
 * against the bits of the region that enabled it ("Checking assignments").
 *   plane     one (region, column) pair: the rows [row_lo, row_lo + rows) the region spans in that column.  Its bits start at
 *             u32 word `first_word` of ONE bit array of `words` words that holds every plane, each on a word boundary; bit
 *             (r - row_lo) % 32 of word first_word + (r - row_lo) / 32 is row r.  The CALLER zeroes the array before the mark.
 *   segment   `count` assigned cells of a plane, `stride` rows apart from the absolute row `first_row` on.
 *   query     one cell a gate reads, as seen from one region: the region's plane of the cell's column, or
 *             H2_COVERAGE_NO_PLANE where the region has none (every such cell is unassigned), and the rotation, |rotation| < n.
 *             `column` is for whoever reads the table; the library does not look at it.
 *   use       one segment of rows a region enabled a gate on: rows first_row, first_row + stride, ... (`count` of them, all
 *             below n), the gate (< 2^16) and its queries [first_query, first_query + num_queries), num_queries < 2^16.  Rows
 *             that one of the EARLIER uses earlier[first_earlier .. first_earlier + num_earlier) (indices into `uses`, each
 *             below the use's own) holds are skipped: the caller lists there the uses of the same region and gate that may
 *             share a row with this one, so that no failure is reported twice.
 *   h2_dev_coverage_mark   sets the bit of every cell of `count` segments in ONE launch: stride-1 segments word by word (one
 *                          atomic OR per 32 cells), the others cell by cell.
 *   h2_dev_coverage_check  for every row of every use and every query q of its gate: cell_row = (row + n + rotation) mod n;
 *                          unless the query's plane spans cell_row and holds its bit, the record
 *                          (H2_CHECK_CELL, gate << 16 | q - first_query, region, cell_row) is appended to the block of the
 *                          witness checks above (caller-zeroed *d_count, `cap` records), in ONE launch.
 *   h2_coverage_mark / h2_coverage_check   the same over a HOST bit array, count and records, on the host.
 * d_scratch: h2_coverage_scratch_bytes(segments, planes, queries, uses, earlier) bytes, 16-byte aligned (a mark asks with the
 * last four 0, a check with segments 0).  The tables are HOST arrays, read before the call returns; the device calls are
 * asynchronous on `stream`.  All return H2_ERR_INVALID without touching a device, h2_last_error naming the call and the
 * reason, for a null or misaligned pointer, n outside 1 .. 2^31, words above 2^30, stride 0, a segment outside its plane, a
 * plane outside the bit array, a plane, query or earlier index out of range, a gate or a query count of 2^16 or more, a use
 * whose last row is not below n, or too small a scratch. */
#define H2_COVERAGE_NO_PLANE 0xffffffffu
typedef struct {
    uint64_t first_word;
    uint32_t row_lo;
    uint32_t rows;
} h2_coverage_plane;
typedef struct {
    uint32_t plane;
    uint32_t reserved;
    uint64_t first_row;
    uint64_t stride;
    uint64_t count;
} h2_coverage_segment;
typedef struct {
    uint32_t plane;
    uint32_t column;
    int32_t rotation;
    uint32_t reserved;
} h2_coverage_query;
typedef struct {
    uint32_t region;
    uint32_t gate;
    uint32_t first_query;
    uint32_t num_queries;
    uint32_t first_earlier;
    uint32_t num_earlier;
    uint64_t first_row;
    uint64_t stride;
    uint64_t count;
} h2_coverage_use;
size_t h2_coverage_scratch_bytes(size_t segments, size_t planes, size_t queries, size_t uses, size_t earlier);
int h2_dev_coverage_mark(const h2_coverage_plane *planes, size_t num_planes, const h2_coverage_segment *segments, size_t count,
                         void *d_bits, size_t words, void *d_scratch, size_t scratch_bytes, void *stream);
int h2_dev_coverage_check(const h2_coverage_plane *planes, size_t num_planes, const h2_coverage_query *queries,
                          size_t num_queries, const h2_coverage_use *uses, size_t num_uses, const uint32_t *earlier,
                          size_t num_earlier, size_t n, const void *d_bits, size_t words, void *d_scratch, size_t scratch_bytes,
                          uint64_t *d_count, h2_check_record *d_records, size_t cap, void *stream);
int h2_coverage_mark(const h2_coverage_plane *planes, size_t num_planes, const h2_coverage_segment *segments, size_t count,
                     void *bits, size_t words);
int h2_coverage_check(const h2_coverage_plane *planes, size_t num_planes, const h2_coverage_query *queries, size_t num_queries,
                      const h2_coverage_use *uses, size_t num_uses, const uint32_t *earlier, size_t num_earlier, size_t n,
                      const void *bits, size_t words, uint64_t *count, h2_check_record *records, size_t cap);

/* ---- computing a witness: one fused launch per straight-line program (values.hip; DESIGN.md 3b "Computing a witness") ----
 * What `Value<F>` and `Assigned<F>` arithmetic (circuit.rs, plonk/assigned.rs) give a synthesize body, in bulk: one program of
 * field operations evaluated over m rows, one lane per row, with no intermediate of length m in device memory.
 *   leaves     row i of leaf l is element first + i * stride of a buffer of `len` elements at `ptr`, read in its form
 *              (H2_ASSIGNED_FORM_*).  A CANONICAL element may be ANY 256-bit integer and is reduced mod r on load (the
 *              conversion is the wide product, which takes a < 2^256); a MONTGOMERY element must be reduced, as everywhere in
 *              the library; a COMPACT element is one u64.  first + (m - 1) * stride < len is checked, stride >= 1.
 *   constants  num_constants x 4 u64, canonical (any 256-bit integer), converted once on the host
 *   ops        op i computes dst = op(a, b, c) into slot `dst`; an operand is kind << 24 | index with kind LEAF, CONST,
 *              SLOT or LAST (the result of op i - 1, which the kernel keeps in registers; the index is not read).  dst may
 *              be H2_VALUES_NO_SLOT: the result is only there for the next op's LAST.  ADD, SUB, MUL take a, b; SQR, NEG,
 *              ISZERO (1 or 0) take a; SELECT gives b where a != 0, else c.  A slot must have been written by an earlier
 *              op before it is read.
 *   outputs    row i of slot `slot`, as it stands at the END of the program, goes to element first + i of `ptr` (32-byte
 *              elements, contiguous) in `form`, CANONICAL or MONTGOMERY, fully reduced.
 *   kinds      a value inside a program is of one of two kinds: a FIELD value (a reduced Montgomery residue: what every leaf,
 *              every constant and ADD SUB MUL SQR NEG ISZERO give) or an INTEGER, the canonical representative v in [0, r)
 *              as plain 256-bit words, in the same slots.  The codes from 16 on work on integers:
 *                TO_INT    a: field            the integer v (of a CANONICAL leaf holding any 256-bit integer: v mod r; of a
 *                                              COMPACT leaf: the u64 itself, at no product)
 *                TO_FIELD  a: integer          the field element
 *                EXTRACT   a: integer          (v >> lo) mod 2^n; `b` = lo and `c` = n are PLAIN NUMBERS, not operands,
 *                                              0 <= lo <= 255, 1 <= n <= 256
 *                LT        a, b: integers      the integer 1 if v_a < v_b, else 0
 *                AND OR XOR  a, b: integers    the bitwise result, an integer.  OR and XOR of two integers below r can reach
 *                                              r or more; the result is reduced by ONE conditional subtraction of r, which is
 *                                              enough: it is below 2^254, which is below 2 r.  ((r - 1) | 1 = r gives 0.)
 *              ADD SUB MUL SQR NEG take field values only; ISZERO takes either kind and gives the FIELD 1 or 0; SELECT takes
 *              either kind in a, and b and c of one kind, which is the result's.  An integer op takes slots and LAST only:
 *              a leaf or a constant is a field operand and goes through TO_INT first.  An output of an integer slot is a
 *              plain store in CANONICAL form and the product x * R^2 (the residue of the same element) in MONTGOMERY form.
 *              Codes 7 .. 15 are not op codes.
 * Overlap rule: the m elements of an output may not overlap the elements a leaf of the same call reads, nor another output,
 * with ONE exception: a 32-byte leaf of stride 1 whose element i is the very bytes of the output's element i (in place).
 * Every load of a row precedes every store of that row and rows do not talk to each other, so that mapping alone is safe.
 * h2_values_limits: the caps {leaves, ops, constants, outputs, slots} a call may use, and `blocks`, the most workgroups (of
 * `threads` lanes) a launch starts -- beyond blocks * threads rows every lane takes several rows.
 * h2_dev_values_eval is asynchronous on `stream`, does not synchronise the host, and passes the program in the kernel
 * arguments.  h2_values_eval is the same on HOST memory by a host interpreter of the same lowered program on the same
 * reduced representatives: bit-exact with the kernel; it touches no device.  Both return H2_ERR_INVALID, before anything is
 * read or written, h2_last_error naming what is wrong, for a count above its cap, a null or misaligned pointer (16 bytes
 * for 32-byte elements on the device, 8 on the host; 8 for compact), an unknown form or op, a slot index at or above the
 * cap, an operand that names a leaf or constant that does not exist or a slot never written, LAST in the first op, a leaf whose range passes
 * `len`, an operand of the wrong kind ("op 3 takes an integer in operand a; slot 2 holds a field value"), lo or n of an
 * EXTRACT out of range, or an overlap the rule above refuses.  m == 0 succeeds and touches nothing. */
enum { H2_VALUES_ADD = 0, H2_VALUES_SUB = 1, H2_VALUES_MUL = 2, H2_VALUES_SQR = 3, H2_VALUES_NEG = 4, H2_VALUES_SELECT = 5,
       H2_VALUES_ISZERO = 6, H2_VALUES_TO_INT = 16, H2_VALUES_TO_FIELD = 17, H2_VALUES_EXTRACT = 18, H2_VALUES_LT = 19,
       H2_VALUES_AND = 20, H2_VALUES_OR = 21, H2_VALUES_XOR = 22 };
enum { H2_VALUES_LEAF = 0, H2_VALUES_CONST = 1, H2_VALUES_SLOT = 2, H2_VALUES_LAST = 3 };
#define H2_VALUES_NO_SLOT 0xffffffffu
typedef struct {
    uint64_t ptr;
    uint64_t first;
    uint64_t stride;
    uint64_t len;
    uint32_t form;
    uint32_t reserved;
} h2_values_leaf;
typedef struct {
    uint32_t op;
    uint32_t dst;
    uint32_t a;
    uint32_t b;
    uint32_t c;
} h2_values_op;
typedef struct {
    uint64_t ptr;
    uint64_t first;
    uint32_t slot;
    uint32_t form;
} h2_values_output;
typedef struct {
    uint32_t leaves;
    uint32_t ops;
    uint32_t constants;
    uint32_t outputs;
    uint32_t slots;
    uint32_t blocks;
    uint32_t threads;
    uint32_t reserved;
} h2_values_caps;
int h2_values_limits(h2_values_caps *out);
int h2_dev_values_eval(const h2_values_leaf *leaves, size_t num_leaves, const uint64_t *constants, size_t num_constants,
                       const h2_values_op *ops, size_t num_ops, const h2_values_output *outputs, size_t num_outputs, size_t m,
                       void *stream);
int h2_values_eval(const h2_values_leaf *leaves, size_t num_leaves, const uint64_t *constants, size_t num_constants,
                   const h2_values_op *ops, size_t num_ops, const h2_values_output *outputs, size_t num_outputs, size_t m);

/* ---- sorting field elements (csrc/sort.hip; values.py: Value.argsort) -----------------------------------------------------
 * h2_dev_sort_permutation: the stable, lexicographic order of n rows under num_keys (1 .. H2_SORT_MAX_KEYS) key columns, the
 * most significant first.  d_keys is a HOST array of device columns; forms[k] says how column k stores its cells
 * (H2_ASSIGNED_FORM_*: canonical or Montgomery cells of 32 bytes, compact cells of 8) and each cell is read as the integer in
 * [0, r) it stands for -- a canonical cell as the 256-bit integer it holds, which is that integer when the cell is reduced.
 * d_perm[i] (perm_width = 4 or 8 bytes an index) is the row of the i-th smallest tuple; equal tuples keep ascending row order.
 * The result is a function of the input alone: what places a row is a prefix sum or a ballot rank, never an atomic's arrival.
 *   bits[k]      the caller's promise key k < 2^bits[k]; 0 = none (254; 64 for a compact column).  Byte positions at and above
 *                the promise are not launched.  A cell that breaks it makes d_status {H2_SORT_OUT_OF_RANGE, the lowest such
 *                row, the lowest such key of that row, passes}; the permutation is then some permutation of 0 .. n - 1.
 *   skipping     one read of the keys fills a histogram of every candidate byte position; a position where all n cells hold
 *                the same byte (exactly one non-empty bin) moves no data.  The decision is taken on the device, in the stream.
 *   d_status     H2_SORT_STATUS_WORDS u32 = {code, row, key, the number of passes that moved data}; row and key are
 *                0xffffffff when the code is H2_SORT_OK.
 *   d_scratch    h2_sort_scratch_bytes(n, num_keys) bytes (sized for Montgomery columns without a promise: enough for any
 *                forms and bits), 16-byte aligned, the caller's: two calls on two streams with two blocks are independent.
 * Asynchronous on `stream`; the host is never synchronised; only d_perm, d_status and d_scratch are written.  n = 0 is a
 * no-op that reports H2_SORT_OK.  Returns H2_ERR_INVALID without touching a device, h2_last_error naming the argument, for a
 * null pointer, num_keys of 0 or above the cap, an unknown form, bits above 254 (64 for compact), n >= 2^32, a misaligned
 * pointer, perm_width other than 4 or 8 and too small a scratch.
 * h2_sort_permutation is the same on HOST memory (cells 8-byte aligned) by the same passes: equal output, equal status.
 * h2_sort_limits: `tile`, the rows a workgroup ranks in a pass; the prefix sum over a pass's 256 x ceil(n / tile) counters
 * takes 2 x tile words a workgroup and a second level once there are more (tests size their inputs around both).
 * h2_sort: the reference's gpu_sort (arithmetic.rs:167-216) as a host-slice call: n Montgomery residues, in place, ascending
 * by the integer in [0, r) each stands for. */
enum { H2_SORT_OK = 0, H2_SORT_OUT_OF_RANGE = 1 };
#define H2_SORT_MAX_KEYS 4
#define H2_SORT_STATUS_WORDS 4
#define H2_SORT_TILE 2048
typedef struct {
    uint32_t tile;
    uint32_t max_keys;
    uint32_t status_words;
    uint32_t reserved;
} h2_sort_caps;
int h2_sort_limits(h2_sort_caps *out);
size_t h2_sort_scratch_bytes(size_t n, size_t num_keys);
int h2_dev_sort_permutation(const void *const *d_keys, const uint32_t *forms, const uint32_t *bits, size_t num_keys, size_t n,
                            void *d_perm, uint32_t perm_width, uint32_t *d_status, void *d_scratch, size_t scratch_bytes,
                            void *stream);
int h2_sort_permutation(const void *const *keys, const uint32_t *forms, const uint32_t *bits, size_t num_keys, size_t n,
                        void *perm, uint32_t perm_width, uint32_t *status);
int h2_sort(uint64_t *values, size_t n);

/* ---- screening the points of an SRS ------------------------------------------------------------------------------------
 * The reference takes the points of its parameters as they come: Params::read unwraps `from_bytes` per point
 * (poly/commitment.rs:262-275) and a table built in memory is never looked at.  h2_dev_g1_check_points tests each of the n
 * affine Montgomery points (64 B each; any n <= 2^28) of d_points, one lane per point.  A point fails in exactly one way,
 * tested in this order:
 *   H2_SRS_NONCANONICAL  x or y, as stored limbs, is >= q
 *   H2_SRS_IDENTITY      the point is (0, 0) -- only with H2_SRS_FORBID_IDENTITY in `flags`; otherwise the identity passes
 *   H2_SRS_OFF_CURVE     y^2 != x^3 + 3 (BN254 G1 has cofactor 1: a point on the curve is in the group)
 * and appends one record {kind, index = table, sub = 0, row = point index} by the scheme of the witness checks above: one
 * agent-scope atomic per wave, a record stored only below `cap`, *d_count exact after the buffer fills.  The count
 * accumulates: a call for g with table = 0 and one for g_lagrange with table = 1 share one buffer and one download.
 * Asynchronous on `stream`.  H2_ERR_INVALID, without touching a device, for a null d_points with n > 0, a null d_count, null
 * records with cap > 0, n > 2^28 or an unknown flag. */
enum { H2_SRS_NONCANONICAL = 0, H2_SRS_IDENTITY = 1, H2_SRS_OFF_CURVE = 2 };
enum { H2_SRS_FORBID_IDENTITY = 1 };
int h2_dev_g1_check_points(const void *d_points, size_t n, uint32_t table, uint32_t flags, uint64_t *d_count,
                           h2_check_record *d_records, size_t cap, void *stream);

/* ---- the verifier's pairing and G2 (host only: no entry below touches a device) ---------------
 * What the reference takes from the pairing_bn256 crate on the verifier side.  G1: 64 B affine Montgomery, identity (0,0).
 * G2 (the twist y^2 = x^3 + 3/(9+u) over Fq2 = Fq[u]/(u^2+1)): 128 B = x.c0, x.c1, y.c0, y.c1 in Montgomery form,
 * identity all zeros.  Every entry validates what it is given and returns H2_ERR_INVALID (never crashes) for a coordinate
 * that is not a canonical residue, a point off its curve and, where said, a G2 point outside the order-r subgroup. */
/* *ok = (prod_i e(P_i, Q_i) == 1), one shared final exponentiation; an identity on either side contributes 1.  The
 * decision of the verifier's `PairMSM`: e(left, [s]G2) e(-right, G2) == 1 (poly/multiopen.rs:29-55 `Decider`,
 * plonk/verifier.rs:496-507, poly/msm.rs:72-101).  G2 points are checked for the subgroup. */
int h2_pairing_check(const uint64_t *g1_xy, const uint64_t *g2_xy, size_t pairs, int *ok);
/* out_xy = [scalar] G2 for the plain (not Montgomery) little-endian scalar < r: the `s_g2` that Params::unsafe_setup
 * writes as additional_data (poly/commitment.rs:113-116).  A scalar of r or above is H2_ERR_INVALID. */
int h2_g2_mul_generator(const uint64_t scalar[4], uint64_t out_xy[16]);
/* out_xy = [scalar] P for a G2 point P in the layout above and a scalar as h2_g2_mul_generator takes it: the step of an SRS
 * update on the G2 side, [s]G2 -> [s tau]G2.  P must be on the twist and in the order-r subgroup (the identity is);
 * otherwise, and for a scalar of r or above, H2_ERR_INVALID.  out_xy may be xy. */
int h2_g2_mul(const uint64_t xy[16], const uint64_t scalar[4], uint64_t out_xy[16]);
/* The 64-byte G2 encoding of the SRS file's additional_data and of ParamsVerifier::{write, read} (poly/commitment.rs:392-433):
 * x.c0 then x.c1, 32 bytes little-endian each, bit 7 of byte 63 = the parity of the canonical y.c0 (of y.c1 when y.c0 is
 * zero), identity = zeros -- the G1 convention above extended to Fq2, and like it a convention of this build.  Compress
 * checks the curve equation; decompress also checks the subgroup. */
int h2_g2_compress(const uint64_t xy[16], uint8_t out[64]);
int h2_g2_decompress(const uint8_t in[64], uint64_t out_xy[16]);

/* ---- synthetic workload (bench.py / tests; not a reference entry point) --------------------- */
/* n deterministic valid G1Affine points (try-and-increment on y^2 = x^3 + 3) into d_out (n x 64 B). */
int h2_dev_random_points(uint64_t seed, size_t n, void *d_out, void *stream);

/* ---- measurement hooks (bench.py) ------------------------------------------------------------ */
/* Wall time in ms of the last timed region recorded with HIP events on `stream`:
 * h2_timer_start / h2_timer_stop bracket any sequence of h2_dev_* calls on that stream. */
int h2_timer_start(void *stream);
int h2_timer_stop(void *stream, float *ms_out);

#ifdef __cplusplus
}
#endif
#endif /* HALO2_HIP_H */
