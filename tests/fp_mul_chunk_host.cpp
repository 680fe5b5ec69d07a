// Host harness of tests/test_fp_mul_chunk_schedule.py: the portable fp_mul_chunk and fp_chunk_table of csrc/field.hpp, compiled
// by g++.  Input file: records of (field u32, chunk limbs u32, x 32 bytes, w in Montgomery form 32 bytes); output file: per
// record the table entry fp_chunk_table built (64 / chunk limbs words, padded to 256 bytes) and the product (32 bytes).
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
    uint32_t field, chunk_limbs;
    uint32_t x[8], w[8];
};
struct Out {
    uint32_t table[64];
    uint32_t r[8];
};

template <class P, int CL>
static void one(const Rec& in, Out& out) {
    Fp<P> x, w;
    memcpy(x.l, in.x, 32);
    memcpy(w.l, in.w, 32);
    FpChunk<CL> t;
    fp_chunk_table<CL>(w, t);
    memset(out.table, 0, sizeof out.table);
    memcpy(out.table, t.w, sizeof t.w);
    const Fp<P> r = fp_mul_chunk<CL>(x, t);
    memcpy(out.r, r.l, 32);
}

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
        Out out;
        if (in.field == 0 && in.chunk_limbs == 2) one<FrParams, 2>(in, out);
        else if (in.field == 0 && in.chunk_limbs == 1) one<FrParams, 1>(in, out);
        else if (in.field == 1 && in.chunk_limbs == 2) one<FqParams, 2>(in, out);
        else if (in.field == 1 && in.chunk_limbs == 1) one<FqParams, 1>(in, out);
        else return 5;
        if (fwrite(&out, sizeof out, 1, g) != 1) return 6;
    }
    return fclose(g) == 0 ? 0 : 7;
}
