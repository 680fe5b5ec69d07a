// tests/arith_conformance.hip -- the field and G1 primitives of csrc/field.hpp, ec.hpp and ec_quad.hpp, one kernel per primitive,
// run on operand tables that tests/test_arith_conformance.py writes (it also holds every expected value: this file has none).
// TEST INFRASTRUCTURE: it includes the product's headers and adds nothing to the library.  Built three ways from this source:
//   g++ -x c++                                 the host path (4 x u64 CIOS product, portable column scans)
//   hipcc --offload-arch=gfx950                the inline-asm carry chains and the generated schedules (fp_mul_gen.hpp)
//   hipcc --offload-arch=gfx950 -DH2_PORTABLE_MUL   the portable device path
// The quad functions (ec_quad.hpp) and the chunk product with its entry in scalar registers exist in the device builds only.
//
// usage: arith_conformance IN OUT
//   IN : "ACF2", u32 batches, then per batch: char op[32], u32 field (0 Fr, 1 Fq), u32 n, n x (the op's input record)
//   OUT: "ACF2", u32 batches, then per batch: char op[32], u32 field, u32 results (n x lanes), that many x (its output record)
// The records are In / Out, but for the ops that say otherwise (in_t, out_t): a case of a chunk product or of a first stage pair
// carries a whole table entry (InW), and fp_chunk_table writes one (OutW).
// A quad primitive (lanes = 4) runs each case on the four lanes of one quad and writes one result per lane.
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <type_traits>
#include <vector>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#else
// host shim: field.hpp / ec.hpp compiled by g++ (the hipRTC branch of field.hpp supplies the integer types)
#define __HIPCC_RTC__ 1
#define __host__
#define __device__
#define __global__
#define __forceinline__ inline
struct uint4 { unsigned x, y, z, w; };
static inline uint4 make_uint4(unsigned x, unsigned y, unsigned z, unsigned w) { return uint4{x, y, z, w}; }
#endif

#include "field.hpp"
#include "ec.hpp"
#if defined(__HIPCC__)
#include "ec_quad.hpp"
#endif

using namespace h2;

struct alignas(16) In {   // 272 B: eight 256-bit operands, a 32-bit scalar and a flag
    uint32_t v[8][8];
    uint32_t k, flag, pad[2];
};
struct alignas(16) Out {  // 128 B: up to four 256-bit results
    uint32_t r[4][8];
};
struct alignas(16) InW {  // 400 B: four 256-bit operands, a table entry (FpChunk<1>: 64 words, FpChunk<2>: the first 32), k, flag
    uint32_t v[4][8];
    uint32_t t[64];
    uint32_t k, flag, pad[2];
};
struct alignas(16) OutW {  // 256 B: a table entry
    uint32_t r[8][8];
};
static_assert(sizeof(In) == 272 && sizeof(Out) == 128, "record layout");
static_assert(sizeof(InW) == 400 && offsetof(InW, t) == 128 && sizeof(OutW) == 256, "record layout");

// the records of an op: In and Out unless it names others
template <class Op, class = void>
struct in_of { using type = In; };
template <class Op>
struct in_of<Op, std::void_t<typename Op::in_t>> { using type = typename Op::in_t; };
template <class Op, class = void>
struct out_of { using type = Out; };
template <class Op>
struct out_of<Op, std::void_t<typename Op::out_t>> { using type = typename Op::out_t; };
// an op whose waves each read ONE entry, that of the wave's first record, has apply_wave(in, t, y) in place of apply(x, y, lane)
template <class Op, class = void>
struct is_wave_op : std::false_type {};
template <class Op>
struct is_wave_op<Op, std::void_t<decltype(&Op::apply_wave)>> : std::true_type {};

template <class P, class Rec>
H2_DEV Fp<P> ld(const Rec& x, int i) {
    Fp<P> r;
    for (int j = 0; j < 8; j++) r.l[j] = x.v[i][j];
    return r;
}
template <class P, class Rec>
H2_DEV void st(Rec& y, int i, const Fp<P>& a) {
    for (int j = 0; j < 8; j++) y.r[i][j] = a.l[j];
}
template <int CL>
H2_DEV FpChunk<CL> ld_chunk(const InW& x) {
    FpChunk<CL> t;
    for (int i = 0; i < 64 / CL; i++) t.w[i] = x.t[i];
    return t;
}
H2_DEV XYZZ ld_xyzz(const In& x, int i) {
    XYZZ r;
    r.x = ld<FqParams>(x, i);
    r.y = ld<FqParams>(x, i + 1);
    r.zz = ld<FqParams>(x, i + 2);
    r.zzz = ld<FqParams>(x, i + 3);
    return r;
}
H2_DEV Affine ld_affine(const In& x, int i) {
    Affine r;
    r.x = ld<FqParams>(x, i);
    r.y = ld<FqParams>(x, i + 1);
    return r;
}
H2_DEV void st_xyzz(Out& y, const XYZZ& p) {
    st(y, 0, p.x);
    st(y, 1, p.y);
    st(y, 2, p.zz);
    st(y, 3, p.zzz);
}

// ---- one struct per primitive: operands v[0], v[1], ... -> results r[0], r[1], ...
#define FIELD_OP(NAME, EXPR)                                                   \
    template <class P>                                                         \
    struct NAME##_op {                                                         \
        static constexpr int lanes = 1;                                        \
        H2_DEV static void apply(const In& x, Out& y, uint32_t) {              \
            const Fp<P> a = ld<P>(x, 0), b = ld<P>(x, 1), c = ld<P>(x, 2), d = ld<P>(x, 3); \
            (void)a; (void)b; (void)c; (void)d;                                \
            st(y, 0, EXPR);                                                    \
        }                                                                      \
    };
FIELD_OP(fp_add, fp_add(a, b))
FIELD_OP(fp_sub, fp_sub(a, b))
FIELD_OP(fp_neg, fp_neg(a))
FIELD_OP(fp_dbl, fp_dbl(a))
FIELD_OP(fp_reduce_once, fp_reduce_once(a))
FIELD_OP(fp_mul, fp_mul(a, b))
FIELD_OP(fp_sqr, fp_sqr(a))
FIELD_OP(fp_mul2, fp_mul2(a, b, c, d))
FIELD_OP(fp_mul_wide, fp_mul_wide(a, b))
FIELD_OP(fp_mul_const, fp_mul_const(a, b, c))
FIELD_OP(fp_to_mont, fp_to_mont(a))
FIELD_OP(fp_from_mont, fp_from_mont(a))
FIELD_OP(fp_lazy_red2p, fp_lazy_red2p(a))
FIELD_OP(fp_lazy_add, fp_lazy_add(a, b))
FIELD_OP(fp_lazy_sub, fp_lazy_sub(a, b))
FIELD_OP(fp_lazy_add_red, fp_lazy_add_red(a, b))
FIELD_OP(fp_lazy_sub_red, fp_lazy_sub_red(a, b))
FIELD_OP(fp_lazy_canon, fp_lazy_canon(a))
FIELD_OP(fp_inv, fp_inv(a))
FIELD_OP(fp_pow_u32, fp_pow_u32(a, x.k))
FIELD_OP(fp_lazy_sub_off1, fp_lazy_sub_off<1>(a, b))
FIELD_OP(fp_lazy_sub_from4p, fp_lazy_sub_from4p(a, b))
#undef FIELD_OP

template <class P>
struct fp_const_pair_op {
    static constexpr int lanes = 1;
    H2_DEV static void apply(const In& x, Out& y, uint32_t) {
        Fp<P> w, wq;
        fp_const_pair(ld<P>(x, 0), w, wq);
        st(y, 0, w);
        st(y, 1, wq);
    }
};

// ---- the chunk-tabulated products of the NTT and what k_ntt_pass8 builds from them: the entry is the case's own data (x.t)
template <class P>
struct fp_mul_chunk2_op {
    using in_t = InW;
    static constexpr int lanes = 1;
    H2_DEV static void apply(const InW& x, Out& y, uint32_t) { st(y, 0, fp_mul_chunk<2>(ld<P>(x, 0), ld_chunk<2>(x))); }
};
// the eight-chunk entry plane by plane, its words in vector registers (Fr: the planes are generated for it only)
template <int AH>
struct fp_mul_chunk_planes_op {
    using in_t = InW;
    static constexpr int lanes = 1;
    H2_DEV static void apply(const InW& x, Out& y, uint32_t) {
        const uint32_t* e = x.t;
        st(y, 0, fp_mul_chunk_planes<AH, false>(ld<FrParams>(x, 0), [e](uint32_t (&w)[8], const uint32_t c) {
               for (uint32_t k = 0; k < 8; k++) w[k] = e[8 * c + k];
           }));
    }
};
template <class P, int CL>
struct fp_chunk_table_op {
    using out_t = OutW;
    static constexpr int lanes = 1;
    H2_DEV static void apply(const In& x, OutW& y, uint32_t) {
        FpChunk<CL> t;
        fp_chunk_table(ld<P>(x, 0), t);
        for (int i = 0; i < 64 / CL; i++) y.r[i / 8][i % 8] = t.w[i];
    }
};
template <class P, FirstPair FORM>
struct fp_lazy_first_pair_op {
    using in_t = InW;
    static constexpr int lanes = 1;
    H2_DEV static void apply(const InW& x, Out& y, uint32_t) {
        Fp<P> x0 = ld<P>(x, 0), x1 = ld<P>(x, 1), x2 = ld<P>(x, 2), x3 = ld<P>(x, 3);
        fp_lazy_first_pair_of(x0, x1, x2, x3, ld_chunk<2>(x), FORM);
        st(y, 0, x0);
        st(y, 1, x1);
        st(y, 2, x2);
        st(y, 3, x3);
    }
};
template <class P>
struct fp_lazy_last_pair_loose_head_op {
    static constexpr int lanes = 1;
    H2_DEV static void apply(const In& x, Out& y, uint32_t) {
        Fp<P> y0, y1;
        fp_lazy_last_pair_loose_head(ld<P>(x, 0), ld<P>(x, 1), y0, y1);
        st(y, 0, y0);
        st(y, 1, y1);
    }
};
template <class P>
struct fp_lazy_last_pair_loose_add_op {
    static constexpr int lanes = 1;
    H2_DEV static void apply(const In& x, Out& y, uint32_t) {
        Fp<P> x0 = ld<P>(x, 0), x1 = ld<P>(x, 1), x2 = ld<P>(x, 2), x3 = ld<P>(x, 3);
        fp_lazy_last_pair_loose_add(x0, x1, x2, x3);
        st(y, 0, x0);
        st(y, 1, x1);
        st(y, 2, x2);
        st(y, 3, x3);
    }
};
// N = 4, as both pass kernels instantiate it
template <class P, bool BRANCH>
struct fp_chunk_handover_op {
    static constexpr int lanes = 1;
    H2_DEV static void apply(const In& x, Out& y, uint32_t) {
        Fp<P> v[4] = {ld<P>(x, 0), ld<P>(x, 1), ld<P>(x, 2), ld<P>(x, 3)};
        fp_chunk_handover<BRANCH>(v);
        for (int q = 0; q < 4; q++) st(y, q, v[q]);
    }
};
#if defined(__HIPCC__)
// the eight-chunk entry in SCALAR registers, as k_ntt_pass8's bmul_s has it: a wave reads the entry of its first record, through
// the constant address space from an index made uniform, and every lane brings its own x
template <int AH>
struct fp_mul_chunk_splanes_op {
    using in_t = InW;
    static constexpr int lanes = 1;
    __device__ static void apply_wave(const InW* in, uint32_t t, Out& y) {
        typedef const __attribute__((address_space(4))) uint32_t* Scalar;
        constexpr uint32_t REC = sizeof(InW) / sizeof(uint32_t), ENTRY = offsetof(InW, t) / sizeof(uint32_t);
        const uint32_t first = (uint32_t)__builtin_amdgcn_readfirstlane((int)(t >> 6)) << 6;
        const Scalar e = (Scalar) reinterpret_cast<const uint32_t*>(in) + ((size_t)first * REC + ENTRY);
        st(y, 0, fp_mul_chunk_planes<AH, true>(ld<FrParams>(in[t], 0), [e](uint32_t (&w)[8], const uint32_t c) __attribute__((always_inline)) {
#pragma unroll
               for (uint32_t k = 0; k < 8; k++) w[k] = e[8 * c + k];
           }));
    }
};
#endif

// G1 (Fq): a point operand is v[0..3] (XYZZ) or v[0..1] (affine); the second one v[4..7] / v[4..5]
struct xyzz_from_affine_op {
    static constexpr int lanes = 1;
    H2_DEV static void apply(const In& x, Out& y, uint32_t) { st_xyzz(y, xyzz_from_affine(ld_affine(x, 0), x.flag != 0)); }
};
struct xyzz_madd_op {
    static constexpr int lanes = 1;
    H2_DEV static void apply(const In& x, Out& y, uint32_t) { st_xyzz(y, xyzz_madd(ld_xyzz(x, 0), ld_affine(x, 4), x.flag != 0)); }
};
struct xyzz_add_op {
    static constexpr int lanes = 1;
    H2_DEV static void apply(const In& x, Out& y, uint32_t) { st_xyzz(y, xyzz_add(ld_xyzz(x, 0), ld_xyzz(x, 4))); }
};
struct xyzz_double_op {
    static constexpr int lanes = 1;
    H2_DEV static void apply(const In& x, Out& y, uint32_t) { st_xyzz(y, xyzz_double(ld_xyzz(x, 0))); }
};
struct xyzz_double_affine_op {
    static constexpr int lanes = 1;
    H2_DEV static void apply(const In& x, Out& y, uint32_t) {
        st_xyzz(y, xyzz_double_affine(ld<FqParams>(x, 0), ld<FqParams>(x, 1)));
    }
};
struct xyzz_mul_u32_op {
    static constexpr int lanes = 1;
    H2_DEV static void apply(const In& x, Out& y, uint32_t) { st_xyzz(y, xyzz_mul_u32(ld_xyzz(x, 0), x.k)); }
};
struct xyzz_to_jacobian_op {
    static constexpr int lanes = 1;
    H2_DEV static void apply(const In& x, Out& y, uint32_t) {
        const Jacobian j = xyzz_to_jacobian(ld_xyzz(x, 0));
        st(y, 0, j.x);
        st(y, 1, j.y);
        st(y, 2, j.z);
    }
};
struct jacobian_to_xyzz_op {
    static constexpr int lanes = 1;
    H2_DEV static void apply(const In& x, Out& y, uint32_t) {
        Jacobian j;
        j.x = ld<FqParams>(x, 0);
        j.y = ld<FqParams>(x, 1);
        j.z = ld<FqParams>(x, 2);
        st_xyzz(y, jacobian_to_xyzz(j));
    }
};
#if defined(__HIPCC__)
struct xyzz_add_q_op {
    static constexpr int lanes = 4;
    __device__ static void apply(const In& x, Out& y, uint32_t q) { st_xyzz(y, xyzz_add_q(ld_xyzz(x, 0), ld_xyzz(x, 4), q)); }
};
struct xyzz_double_q_op {
    static constexpr int lanes = 4;
    __device__ static void apply(const In& x, Out& y, uint32_t q) { st_xyzz(y, xyzz_double_q(ld_xyzz(x, 0), q)); }
};
struct xyzz_mul_u32_q_op {
    static constexpr int lanes = 4;
    __device__ static void apply(const In& x, Out& y, uint32_t q) { st_xyzz(y, xyzz_mul_u32_q(ld_xyzz(x, 0), x.k, q)); }
};
#endif

// ---- running a table: thread t takes case t / lanes as lane t % lanes (a quad's lanes are t & 3 on the device)
#if defined(__HIPCC__)
#define CK(x)                                                                                   \
    do {                                                                                        \
        hipError_t e_ = (x);                                                                    \
        if (e_ != hipSuccess) {                                                                 \
            fprintf(stderr, "HIP error %s at line %d\n", hipGetErrorString(e_), __LINE__);      \
            return 1;                                                                           \
        }                                                                                       \
    } while (0)

template <class Op>
__global__ __launch_bounds__(256) void k_prim(const typename in_of<Op>::type* in, typename out_of<Op>::type* out, uint32_t n_threads) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_threads) return;
    typename out_of<Op>::type y = {};
    if constexpr (is_wave_op<Op>::value) {
        static_assert(Op::lanes == 1, "one case per lane");
        Op::apply_wave(in, t, y);  // (a block is four whole waves: t >> 6 is the wave's index in the table)
    } else {
        Op::apply(in[t / Op::lanes], y, t % Op::lanes);
    }
    out[t] = y;
}

template <class Op>
static int run(const void* in, void* out, uint32_t n) {
    using I = typename in_of<Op>::type;
    using O = typename out_of<Op>::type;
    const uint32_t threads = n * Op::lanes;
    I* d_in = nullptr;
    O* d_out = nullptr;
    CK(hipMalloc(&d_in, (size_t)n * sizeof(I)));
    CK(hipMalloc(&d_out, (size_t)threads * sizeof(O)));
    CK(hipMemcpy(d_in, in, (size_t)n * sizeof(I), hipMemcpyHostToDevice));
    CK(hipMemset(d_out, 0xA5, (size_t)threads * sizeof(O)));  // a result never written stays this pattern
    hipLaunchKernelGGL(k_prim<Op>, dim3((threads + 255) / 256), dim3(256), 0, 0, d_in, d_out, threads);
    CK(hipGetLastError());
    CK(hipDeviceSynchronize());
    CK(hipMemcpy(out, d_out, (size_t)threads * sizeof(O), hipMemcpyDeviceToHost));
    CK(hipFree(d_in));
    CK(hipFree(d_out));
    return 0;
}
#else
template <class Op>
static int run(const void* in_, void* out_, uint32_t n) {
    using O = typename out_of<Op>::type;
    const typename in_of<Op>::type* in = (const typename in_of<Op>::type*)in_;
    O* out = (O*)out_;
    memset(out, 0xA5, (size_t)n * Op::lanes * sizeof(O));
    for (uint32_t t = 0; t < n * Op::lanes; t++) {
        O y;
        memset(&y, 0, sizeof y);
        Op::apply(in[t / Op::lanes], y, t % Op::lanes);
        out[t] = y;
    }
    return 0;
}
#endif

struct Entry {
    const char* name;
    uint32_t field;  // 0 Fr, 1 Fq
    uint32_t lanes;
    uint32_t in_bytes, out_bytes;  // of one record
    int (*fn)(const void*, void*, uint32_t);
};
#define OP_ENTRY(NAME, FIELD, ...) \
    {NAME, FIELD, __VA_ARGS__::lanes, (uint32_t)sizeof(in_of<__VA_ARGS__>::type), (uint32_t)sizeof(out_of<__VA_ARGS__>::type), run<__VA_ARGS__>}
#define FIELD_ENTRY(NAME) OP_ENTRY(#NAME, 0, NAME##_op<FrParams>), OP_ENTRY(#NAME, 1, NAME##_op<FqParams>)
#define G1_ENTRY(NAME) OP_ENTRY(#NAME, 1, NAME##_op)
static const Entry kEntries[] = {
    FIELD_ENTRY(fp_add), FIELD_ENTRY(fp_sub), FIELD_ENTRY(fp_neg), FIELD_ENTRY(fp_dbl), FIELD_ENTRY(fp_reduce_once),
    FIELD_ENTRY(fp_mul), FIELD_ENTRY(fp_sqr), FIELD_ENTRY(fp_mul2), FIELD_ENTRY(fp_mul_wide), FIELD_ENTRY(fp_mul_const),
    FIELD_ENTRY(fp_const_pair), FIELD_ENTRY(fp_to_mont), FIELD_ENTRY(fp_from_mont), FIELD_ENTRY(fp_lazy_red2p),
    FIELD_ENTRY(fp_lazy_add), FIELD_ENTRY(fp_lazy_sub), FIELD_ENTRY(fp_lazy_add_red), FIELD_ENTRY(fp_lazy_sub_red),
    FIELD_ENTRY(fp_lazy_canon), FIELD_ENTRY(fp_inv), FIELD_ENTRY(fp_pow_u32),
    G1_ENTRY(xyzz_from_affine), G1_ENTRY(xyzz_madd), G1_ENTRY(xyzz_add), G1_ENTRY(xyzz_double), G1_ENTRY(xyzz_double_affine),
    G1_ENTRY(xyzz_mul_u32), G1_ENTRY(xyzz_to_jacobian),
#if defined(__HIPCC__)
    G1_ENTRY(xyzz_add_q), G1_ENTRY(xyzz_double_q), G1_ENTRY(xyzz_mul_u32_q),
#endif
    FIELD_ENTRY(fp_mul_chunk2), FIELD_ENTRY(fp_lazy_sub_off1), FIELD_ENTRY(fp_lazy_sub_from4p),
    FIELD_ENTRY(fp_lazy_last_pair_loose_head), FIELD_ENTRY(fp_lazy_last_pair_loose_add),
    OP_ENTRY("fp_mul_chunk_planes_ah1", 0, fp_mul_chunk_planes_op<1>), OP_ENTRY("fp_mul_chunk_planes_ah2", 0, fp_mul_chunk_planes_op<2>),
    OP_ENTRY("fp_chunk_table1", 0, fp_chunk_table_op<FrParams, 1>), OP_ENTRY("fp_chunk_table1", 1, fp_chunk_table_op<FqParams, 1>),
    OP_ENTRY("fp_chunk_table2", 0, fp_chunk_table_op<FrParams, 2>), OP_ENTRY("fp_chunk_table2", 1, fp_chunk_table_op<FqParams, 2>),
    OP_ENTRY("fp_lazy_first_pair_2p", 0, fp_lazy_first_pair_op<FrParams, FIRST_PAIR_2P>),
    OP_ENTRY("fp_lazy_first_pair_2p", 1, fp_lazy_first_pair_op<FqParams, FIRST_PAIR_2P>),
    OP_ENTRY("fp_lazy_first_pair_4p", 0, fp_lazy_first_pair_op<FrParams, FIRST_PAIR_4P>),
    OP_ENTRY("fp_lazy_first_pair_4p", 1, fp_lazy_first_pair_op<FqParams, FIRST_PAIR_4P>),
    OP_ENTRY("fp_lazy_first_pair_canon", 0, fp_lazy_first_pair_op<FrParams, FIRST_PAIR_CANON>),
    OP_ENTRY("fp_lazy_first_pair_canon", 1, fp_lazy_first_pair_op<FqParams, FIRST_PAIR_CANON>),
    OP_ENTRY("fp_chunk_handover", 0, fp_chunk_handover_op<FrParams, true>), OP_ENTRY("fp_chunk_handover", 1, fp_chunk_handover_op<FqParams, true>),
    OP_ENTRY("fp_chunk_handover_nobranch", 0, fp_chunk_handover_op<FrParams, false>),
    OP_ENTRY("fp_chunk_handover_nobranch", 1, fp_chunk_handover_op<FqParams, false>),
    G1_ENTRY(jacobian_to_xyzz),
#if defined(__HIPCC__)
    OP_ENTRY("fp_mul_chunk_splanes_ah1", 0, fp_mul_chunk_splanes_op<1>), OP_ENTRY("fp_mul_chunk_splanes_ah2", 0, fp_mul_chunk_splanes_op<2>),
#endif
};

static bool read_exact(FILE* f, void* p, size_t bytes) { return bytes == 0 || fread(p, 1, bytes, f) == bytes; }

int main(int argc, char** argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: %s IN OUT\n", argv[0]);
        return 2;
    }
    FILE* fi = fopen(argv[1], "rb");
    FILE* fo = fopen(argv[2], "wb");
    if (!fi || !fo) {
        fprintf(stderr, "cannot open %s or %s\n", argv[1], argv[2]);
        return 2;
    }
    char magic[4];
    uint32_t batches = 0;
    if (!read_exact(fi, magic, 4) || memcmp(magic, "ACF2", 4) || !read_exact(fi, &batches, 4)) {
        fprintf(stderr, "bad input header\n");
        return 2;
    }
    fwrite("ACF2", 1, 4, fo);
    fwrite(&batches, 4, 1, fo);
    uint64_t total = 0;
    for (uint32_t b = 0; b < batches; b++) {
        char op[32];
        uint32_t field = 0, n = 0;
        if (!read_exact(fi, op, 32) || !read_exact(fi, &field, 4) || !read_exact(fi, &n, 4)) {
            fprintf(stderr, "truncated input at batch %u\n", b);
            return 2;
        }
        op[31] = 0;
        const Entry* e = nullptr;
        for (const Entry& c : kEntries)
            if (!strcmp(c.name, op) && c.field == field) e = &c;
        if (!e) {
            fprintf(stderr, "no primitive %s for field %u in this build\n", op, field);
            return 2;
        }
        std::vector<uint4> in(((size_t)n * e->in_bytes + 15) / 16), out(((size_t)n * e->lanes * e->out_bytes + 15) / 16);  // (16-byte aligned)
        if (!read_exact(fi, in.data(), (size_t)n * e->in_bytes)) {
            fprintf(stderr, "truncated input in batch %s\n", op);
            return 2;
        }
        if (n && e->fn(in.data(), out.data(), n)) return 1;
        const uint32_t results = n * e->lanes;
        fwrite(op, 1, 32, fo);
        fwrite(&field, 4, 1, fo);
        fwrite(&results, 4, 1, fo);
        fwrite(out.data(), e->out_bytes, results, fo);
        total += results;
    }
    if (fclose(fo)) {
        fprintf(stderr, "cannot write %s\n", argv[2]);
        return 2;
    }
    fclose(fi);
    printf("arith_conformance: %u batches, %llu results\n", batches, (unsigned long long)total);
    return 0;
}
