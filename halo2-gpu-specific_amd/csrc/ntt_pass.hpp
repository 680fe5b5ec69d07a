// ntt_pass.hpp -- what ntt.hip (schedule, plans, table cache) needs of ntt_pass.hip (the device code): the argument block of a
// pass, the kernel ids, the launcher and the table fillers.  Internal to the two files.
#pragma once
#include "common.hpp"

namespace h2 {

static constexpr int NTT_BATCH_MAX = 16;  // vectors per launch of a batched transform (pointers travel in the kernel arguments)
static constexpr int LO_BITS = 12;  // two-level twiddle tables: w^e = lo[e & 4095] * hi[e >> 12]

using TwChunk = FpChunk<2>;   // four chunks of 64 bits: the entries a lane reads for itself, from LDS or from memory
static constexpr uint32_t TW_CHUNK_FR = sizeof(TwChunk) / sizeof(Fr);   // table elements per entry
static constexpr uint32_t TW_CHUNK_Q = sizeof(TwChunk) / sizeof(uint4);  // 16-byte words per entry
// Eight chunks of 32 bits (80 multiply-adds and 2 low products per product instead of 88 and 3) for the twiddles of k_ntt_pass8
// that are the same for a whole wave (its first stage pair, the round of stages 2 and 3): the entries of index 0, 4, 8 .. in a
// table of their own, read by scalar loads, plane by plane, into scalar registers (fp_mul_chunk_planes).  The same form from
// LDS for the per-lane twiddles of stages 4 and 5 measured slower, the whole table in LDS much slower.
using TwChunk32 = FpChunk<1>;
static constexpr uint32_t TW_CHUNK32_ENTRIES = 32;
static constexpr uint32_t TW_CHUNK32_FR = sizeof(TwChunk32) / sizeof(Fr);
static constexpr uint32_t TW_CHUNK32_Q = sizeof(TwChunk32) / sizeof(uint4);

struct PassArgs {
    const Fr* in;
    Fr* out;
    const Fr* tw_bfly;  // R/2 entries: (w^(n/R))^e   (CW kernels: R/2 PAIRS -- plain value, quotient; see tw_store)
    const Fr* tw_chunk;  // k_ntt_pass8: the same R/2 values as chunk tables (tw_store's third form)
    const Fr* tw_chunk32;  // k_ntt_pass8: the values of index 0, 4, 8 .. as eight-chunk entries (tw_store's fourth form)
    const Fr* tw_lo;    // min(n, 4096) entries: w^i
    const Fr* tw_hi;    // n >> 12 entries: w^(i << 12)   (unused when n <= 4096)
    const Fr* tw_direct;  // non-null (a last pass): inter-pass twiddle = tw_direct[(K << B) | rho], its load order (no generation multiply)
    // The inter-pass twiddles of a tabulated middle pass (the plan's tw_inter) are applied where the pass BEFORE it stores:
    // tw_applied (that middle pass): the elements it loads carry their twiddle already, its load multiplies by nothing, and
    // they are CANONICAL residues (every store product ends with fp_chunk_handover): its first stage pair reduces nothing;
    // nx_tab (the pass before it): the next pass's table, chunk entries (tw_store's third form) at [(rho' << nx_t_log) | K'], and
    // that pass's s_log / B / t_log -- the element stored at idx is the next pass's row rho' = (idx >> nx_s_log) & (2^nx_B - 1)
    // and its K' is this pass's K | k << t_log
    uint32_t tw_applied;
    const Fr* nx_tab;
    uint32_t nx_s_log, nx_B, nx_t_log;
    uint32_t hi_scaled;  // tw_hi already carries the uniform post-scale (1/n): never skip, no post multiply
    Fr pre3[3];         // has_pre3: x *= pre3[idx % 3] on the first-pass load (idx % 3 == 0 skipped)
    Fr post3[3];        // has_post3: y *= post3[idx % 3] on the final store
    uint32_t has_pre3, has_post3, post3_uniform;
    uint32_t log_n, B, s_log, t_log;
    uint32_t nprev;       // number of earlier passes
    uint32_t prevB[4];    // their bit widths
    uint32_t prevT[4];    // their T_q logs
    uint32_t is_last, in_len, log_c;
    // generic coset scale (coeff -> one coset of the extended domain and back): sc[i] = g^i = sc_lo[i & 4095] * sc_hi[i >> 12]
    // (sc_hi also carries the iNTT divisor).  scale_mode 1: x[i] *= sc[i] on the first pass's load (the inter-pass twiddle
    // path, which a first pass never uses, does it); 2: y[i] *= sc[i] on the final store
    const Fr* sc_lo;
    const Fr* sc_hi;
    uint32_t scale_mode;
    // several transforms of one plan in ONE launch (blockIdx.y picks the vector): a 2^20-point pass is 1024 tiles, one
    // resident round of the chip in which every workgroup waits out its own load -> stages -> store chain; with the
    // tiles of 8-16 vectors in the grid the rounds overlap (the columns of a wide witness on one coset)
    uint32_t batch;
    const Fr* in_b[NTT_BATCH_MAX];
    Fr* out_b[NTT_BATCH_MAX];
    uint32_t zskip;  // first pass of a zero-padded transform: rows rho >= R >> zskip are zero (see the load loop)
    uint32_t radix4;  // stage loop: two stages per LDS round trip (four elements per lane), launched with R / 4 * C threads
};

// Which kernel a pass runs (the values are h2_ntt_shape's kernel ids, H2_NTT_KERNEL_* in halo2_hip.h): chosen by pass_kernel
// (ntt.hip) only; the launcher indexes pass_fn with it and h2_ntt_shape reports it.
enum NttKernel : uint32_t {
    NK_PASS8_DP = H2_NTT_KERNEL_PASS8_DP,
    NK_PASS8 = H2_NTT_KERNEL_PASS8,
    NK_R4_DP = H2_NTT_KERNEL_R4_DP,
    NK_R4 = H2_NTT_KERNEL_R4,
    NK_R2 = H2_NTT_KERNEL_R2,
};

// One pass over `cnt` vectors on `threads` lanes per tile; the grid and the dynamic LDS follow from the kernel and a.log_n /
// a.B / a.log_c.  `device`: the current one (the LDS limit of the general kernels is raised once per device: 9-bit passes).
// Which instantiation of `kernel` runs is the launcher's choice from `a`: with a.nx_tab the one that multiplies at its store,
// and for the plain call of the fixed pass (one vector of full length, no scale) the one compiled for the pass's position.
void ntt_pass_launch(int device, NttKernel kernel, const PassArgs& a, uint32_t cnt, uint32_t threads, hipStream_t stream);

// Table fillers: one kernel each on `stream` (none for an empty table).  `form`: tw_store's `pair` (ntt_pass.hip), 0 .. 3.
void ntt_fill_pow(Fr* out, const Fr& base, uint32_t mul, uint32_t count, uint32_t form, hipStream_t stream);  // out[i] = base^(i mul)
// out[(rho << kbits) | K] = base^((rho K << s_log) mod n): the complete inter-pass twiddle set of a middle pass (form 2:
// sizeof(TwChunk) bytes per entry)
void ntt_fill_direct(Fr* out, const Fr& base, uint32_t kbits, uint32_t s_log, uint32_t log_n, uint32_t count, uint32_t form,
                     hipStream_t stream);
// out[(K << bits) | rho] = base^((rho K) mod n) (* d when given), 2^log_n Montgomery values (log_n >= 8): the last pass's, in load order
void ntt_fill_last(Fr* out, const Fr& base, uint32_t bits, uint32_t log_n, const Fr* d, hipStream_t stream);
void ntt_fill_scaled(Fr* out, const Fr* in, const Fr& d, uint32_t count, hipStream_t stream);  // out[i] = in[i] * d

}  // namespace h2
