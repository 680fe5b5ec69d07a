// Host harness of tests/test_ntt_pass_boundaries_host.py: the portable bodies of csrc/field.hpp behind the two ends of the hand-over
// between two NTT passes, compiled by g++.
//   mode 1: the last stage pair of a pass before the last, the arithmetic of k_ntt_pass8's unit4_mul + unit4_add at s = 6
//           (csrc/ntt_pass.hip) call for call: x0 .. x3 are rows as LDS holds them, w[0] = wa, w[1] = wb, w[2] = wc
//   mode 2: the same with the three products given -- x1 = x1', x2 = y2, x3 = n3 -- so that a test can set them to a product's
//           largest value, which no chosen operand is known to produce
//   mode 3: the store product and the hand-over: x0 w[0] by fp_mul_chunk as it is, after fp_chunk_handover with its branch,
//           and after the form without one
// Input file: records of (mode u32, pad u32, x0 .. x3 32 bytes each, w[0 .. 2] in Montgomery form 32 bytes each); output file:
// per record six values of 32 bytes: modes 1, 2 the four rows written, then y0 and y1; mode 3 the three results, then zeros.
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
        F o[6];
        for (int i = 0; i < 6; i++) o[i] = fp_zero<FrParams>();
        if (in.mode == 1 || in.mode == 2) {
            // unit4_mul, the branch with twiddles, NLAST at s = 6
            const F x0 = fp_lazy_red2p(x[0]);
            F x1 = x[1], y2 = x[2], n3 = x[3];
            if (in.mode == 1) {
                x1 = fp_mul_chunk(x[1], t[0]);
                const F x3 = fp_mul_chunk(x[3], t[0]);
                y2 = fp_mul_chunk(fp_lazy_add(x[2], x3), t[1]);
                n3 = fp_mul_chunk(fp_lazy_sub_from4p(x3, x[2]), t[2]);
            }
            F y0, y1;
            fp_lazy_last_pair_loose_head(x0, x1, y0, y1);
            // unit4_add, loose
            o[0] = y0; o[1] = y1; o[2] = y2; o[3] = n3;
            fp_lazy_last_pair_loose_add(o[0], o[1], o[2], o[3]);
            o[4] = y0;
            o[5] = y1;
        } else if (in.mode == 3) {
            o[0] = fp_mul_chunk(x[0], t[0]);
            F a[1] = {o[0]}, b[1] = {o[0]};
            fp_chunk_handover(a);
            fp_chunk_handover<false>(b);
            o[1] = a[0];
            o[2] = b[0];
        } else {
            return 5;
        }
        Out out;
        for (int i = 0; i < 6; i++) memcpy(out.v[i], o[i].l, 32);
        if (fwrite(&out, sizeof out, 1, g) != 1) return 6;
    }
    return fclose(g) == 0 ? 0 : 7;
}
