// Host harness of tests/test_ntt_lazy_ranges_host.py: the portable bodies of csrc/field.hpp behind the two stage pairs of the
// fixed NTT pass that leave reductions out, compiled by g++.
//   mode 0: fp_lazy_first_pair_canon on four canonical operands (w[2] the pair's one twiddle)
//   mode 1: a stage pair with twiddles, the arithmetic of k_ntt_pass8's unit4_mul + unit4_add (csrc/ntt_pass.hip) call for call:
//           x0 .. x3 are rows as LDS holds them, w[0] = wa, w[1] = wb, w[2] = wc
//   mode 2: the same with x1 and x3 taken as the results x1', x3' of the first two products (so that a test can set them to the
//           products' largest value, which no chosen operand is known to produce)
// Input file: records of (mode u32, pad u32, x0 .. x3 32 bytes each, w[0 .. 2] in Montgomery form 32 bytes each); output file:
// per record the four rows written, then the operands of the last two products (modes 1, 2; zero for mode 0), 32 bytes each.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

// host shim: field.hpp compiled by g++ (the hipRTC branch of field.hpp supplies the integer types)
#define __HIPCC_RTC__ 1
#define __host__
#define __device__
#define __global__
#define __forceinline__ inline
struct uint4 { unsigned x, y, z, w; };
static inline uint4 make_uint4(unsigned x, unsigned y, unsigned z, unsigned w) { return uint4{x, y, z, w}; }

#include "field.hpp"

using namespace h2;
using F = Fp<FrParams>;

struct Rec {
    uint32_t mode, pad;
    uint32_t x[4][8], w[3][8];
};
struct Out {
    uint32_t v[6][8];
};

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 3;
    std::vector<Rec> recs;
    Rec rec;
    while (fread(&rec, sizeof rec, 1, f) == 1) recs.push_back(rec);
    fclose(f);
    FILE* g = fopen(argv[2], "wb");
    if (!g) return 4;
    for (const Rec& in : recs) {
        F x[4], w;
        FpChunk<2> t[3];
        for (int i = 0; i < 4; i++) memcpy(x[i].l, in.x[i], 32);
        for (int i = 0; i < 3; i++) {
            memcpy(w.l, in.w[i], 32);
            fp_chunk_table<2>(w, t[i]);
        }
        F s = fp_zero<FrParams>(), n = fp_zero<FrParams>();
        if (in.mode == 0) {
            fp_lazy_first_pair_canon(x[0], x[1], x[2], x[3], t[2]);
        } else {
            // unit4_mul, the branch with twiddles
            F x0 = fp_lazy_red2p(x[0]), x1 = x[1], x2 = x[2], x3 = x[3];
            if (in.mode == 1) {
                x1 = fp_mul_chunk(x1, t[0]);
                x3 = fp_mul_chunk(x3, t[0]);
            }
            s = fp_lazy_add(x2, x3);
            n = fp_lazy_sub_from4p(x3, x2);
            const F y0 = fp_lazy_add_red(x0, x1), y1 = fp_lazy_sub_red(x0, x1);
            const F y2 = fp_mul_chunk(s, t[1]), n3 = fp_mul_chunk(n, t[2]);
            // unit4_add
            x[0] = fp_lazy_add(y0, y2);
            x[1] = fp_lazy_sub(y1, n3);
            x[2] = fp_lazy_sub(y0, y2);
            x[3] = fp_lazy_add(y1, n3);
        }
        Out out;
        for (int i = 0; i < 4; i++) memcpy(out.v[i], x[i].l, 32);
        memcpy(out.v[4], s.l, 32);
        memcpy(out.v[5], n.l, 32);
        if (fwrite(&out, sizeof out, 1, g) != 1) return 6;
    }
    return fclose(g) == 0 ? 0 : 7;
}
