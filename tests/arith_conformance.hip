// tests/arith_conformance.hip -- the field and G1 primitives of csrc/field.hpp, ec.hpp and ec_quad.hpp, one kernel per primitive,
// run on operand tables that tests/test_arith_conformance.py writes (it also holds every expected value: this file has none).
// TEST INFRASTRUCTURE: it includes the product's headers and adds nothing to the library.  Built three ways from this source:
//   g++ -x c++                                 the host path (4 x u64 CIOS product, portable column scans)
//   hipcc --offload-arch=gfx950                the inline-asm carry chains and the generated schedules (fp_mul_gen.hpp)
//   hipcc --offload-arch=gfx950 -DH2_PORTABLE_MUL   the portable device path
// The quad functions (ec_quad.hpp) exist in the device builds only.
//
// usage: arith_conformance IN OUT
//   IN : "ACF1", u32 batches, then per batch: char op[32], u32 field (0 Fr, 1 Fq), u32 n, n x In
//   OUT: "ACF1", u32 batches, then per batch: char op[32], u32 field, u32 results (n x lanes), that many x Out
// A quad primitive (lanes = 4) runs each case on the four lanes of one quad and writes one result per lane.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
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
static_assert(sizeof(In) == 272 && sizeof(Out) == 128, "record layout");

template <class P>
H2_DEV Fp<P> ld(const In& x, int i) {
    Fp<P> r;
    for (int j = 0; j < 8; j++) r.l[j] = x.v[i][j];
    return r;
}
template <class P>
H2_DEV void st(Out& y, int i, const Fp<P>& a) {
    for (int j = 0; j < 8; j++) y.r[i][j] = a.l[j];
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
__global__ __launch_bounds__(256) void k_prim(const In* in, Out* out, uint32_t n_threads) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_threads) return;
    Out y;
    for (int i = 0; i < 4; i++)
        for (int j = 0; j < 8; j++) y.r[i][j] = 0;
    Op::apply(in[t / Op::lanes], y, t % Op::lanes);
    out[t] = y;
}

template <class Op>
static int run(const In* in, Out* out, uint32_t n) {
    const uint32_t threads = n * Op::lanes;
    In* d_in = nullptr;
    Out* d_out = nullptr;
    CK(hipMalloc(&d_in, (size_t)n * sizeof(In)));
    CK(hipMalloc(&d_out, (size_t)threads * sizeof(Out)));
    CK(hipMemcpy(d_in, in, (size_t)n * sizeof(In), hipMemcpyHostToDevice));
    CK(hipMemset(d_out, 0xA5, (size_t)threads * sizeof(Out)));  // a result never written stays this pattern
    hipLaunchKernelGGL(k_prim<Op>, dim3((threads + 255) / 256), dim3(256), 0, 0, d_in, d_out, threads);
    CK(hipGetLastError());
    CK(hipDeviceSynchronize());
    CK(hipMemcpy(out, d_out, (size_t)threads * sizeof(Out), hipMemcpyDeviceToHost));
    CK(hipFree(d_in));
    CK(hipFree(d_out));
    return 0;
}
#else
template <class Op>
static int run(const In* in, Out* out, uint32_t n) {
    memset(out, 0xA5, (size_t)n * Op::lanes * sizeof(Out));
    for (uint32_t t = 0; t < n * Op::lanes; t++) {
        Out y;
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
    int (*fn)(const In*, Out*, uint32_t);
};
#define FIELD_ENTRY(NAME) {#NAME, 0, 1, run<NAME##_op<FrParams>>}, {#NAME, 1, 1, run<NAME##_op<FqParams>>}
#define G1_ENTRY(NAME) {#NAME, 1, NAME##_op::lanes, run<NAME##_op>}
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
    if (!read_exact(fi, magic, 4) || memcmp(magic, "ACF1", 4) || !read_exact(fi, &batches, 4)) {
        fprintf(stderr, "bad input header\n");
        return 2;
    }
    fwrite("ACF1", 1, 4, fo);
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
        std::vector<In> in(n);
        std::vector<Out> out((size_t)n * e->lanes);
        if (!read_exact(fi, in.data(), (size_t)n * sizeof(In))) {
            fprintf(stderr, "truncated input in batch %s\n", op);
            return 2;
        }
        if (n && e->fn(in.data(), out.data(), n)) return 1;
        const uint32_t results = n * e->lanes;
        fwrite(op, 1, 32, fo);
        fwrite(&field, 4, 1, fo);
        fwrite(&results, 4, 1, fo);
        fwrite(out.data(), sizeof(Out), results, fo);
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
