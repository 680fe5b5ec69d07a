// Host harness of tests/test_ntt_lazy_bounds_host.py: the portable fp_lazy_first_pair of csrc/field.hpp (the first stage pair of
// the fixed NTT pass), compiled by g++.  Input file: records of (red u32, pad u32, x0 .. x3 32 bytes each, w in Montgomery
// form 32 bytes); output file: per record the four rows it leaves, 32 bytes each.
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

struct Rec {
    uint32_t red, pad;
    uint32_t x[4][8], w[8];
};
struct Out {
    uint32_t x[4][8];
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
        Fp<FrParams> x[4], w;
        for (int i = 0; i < 4; i++) memcpy(x[i].l, in.x[i], 32);
        memcpy(w.l, in.w, 32);
        FpChunk<2> t;
        fp_chunk_table<2>(w, t);
        fp_lazy_first_pair(x[0], x[1], x[2], x[3], t, in.red != 0);
        Out out;
        for (int i = 0; i < 4; i++) memcpy(out.x[i], x[i].l, 32);
        if (fwrite(&out, sizeof out, 1, g) != 1) return 6;
    }
    return fclose(g) == 0 ? 0 : 7;
}
