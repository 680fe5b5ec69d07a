// Host harness of tests/test_fp_mul_chunk32_host.py: the portable fp_mul_chunk_planes, fp_mul_chunk<1> and fp_chunk_table<1> of
// csrc/field.hpp (Fr), compiled by g++.  Input file: records of (kind u32, 32 bytes, 256 bytes).  kind 0: x and an
// eight-chunk entry -> the product through fp_mul_chunk_planes (a plane fetch from the entry, 32 bytes), the product through
// fp_mul_chunk<1> (32 bytes), zero padding to 256 bytes.  kind 1: w in Montgomery form -> the entry fp_chunk_table<1> builds,
// written as tw_store's fourth form writes it (16-byte words in order, 256 bytes).
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

#pragma pack(push, 1)
struct Rec {
    uint32_t kind;
    uint32_t x[8];
    uint32_t entry[64];
};
#pragma pack(pop)

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
        uint32_t out[64];
        memset(out, 0, sizeof out);
        Fp<FrParams> x;
        memcpy(x.l, in.x, 32);
        if (in.kind == 0) {
            const uint32_t* const e = in.entry;
            const Fp<FrParams> r = fp_mul_chunk_planes<1>(x, [e](uint32_t (&w)[8], const uint32_t c) {
                for (int k = 0; k < 8; k++) w[k] = e[8 * c + k];
            });
            FpChunk<1> t;
            memcpy(t.w, in.entry, sizeof t.w);
            const Fp<FrParams> r2 = fp_mul_chunk<1>(x, t);
            memcpy(out, r.l, 32);
            memcpy(out + 8, r2.l, 32);
        } else if (in.kind == 1) {
            FpChunk<1> t;
            fp_chunk_table<1>(x, t);
            uint4 q[16];
            for (uint32_t k = 0; k < 16; k++) q[k] = make_uint4(t.w[4 * k], t.w[4 * k + 1], t.w[4 * k + 2], t.w[4 * k + 3]);
            memcpy(out, q, sizeof out);
        } else {
            return 5;
        }
        if (fwrite(out, sizeof out, 1, g) != 1) return 6;
    }
    return fclose(g) == 0 ? 0 : 7;
}
