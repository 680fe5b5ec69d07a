// tools/fp_mul_isa_probe.hip -- the constant-operand products of csrc/field.hpp and the radix-4 unit of k_ntt_pass8 as stand-alone
// kernels, for counting instructions (profiles/ntt_chunk_product_isa.txt).  Never run: compile for the device only,
//   hipcc -O3 -std=c++17 --offload-arch=gfx950 --cuda-device-only -S -I halo2-gpu-specific_amd/csrc tools/fp_mul_isa_probe.hip -o probe.s
// and count with tools/isa_classes.py probe.s.  The unit is the non-unit branch of ntt.hip's unit4 (4 elements, 2 stages, 4
// products), once with fp_mul_const and once with fp_mul_chunk; operands come from memory so that nothing folds away.
#include "field.hpp"

using namespace h2;

extern "C" __global__ void probe_mul_const(Fr* x, const Fr* t) {
    const uint32_t i = threadIdx.x;
    fp_store(x + i, fp_mul_const(fp_load(x + i), fp_load(t + 2 * i), fp_load(t + 2 * i + 1)));
}

extern "C" __global__ void probe_mul_chunk(Fr* x, const FpChunk<2>* t) {
    const uint32_t i = threadIdx.x;
    fp_store(x + i, fp_mul_chunk(fp_load(x + i), t[i]));
}

template <class Tw, class Mul>
__device__ __forceinline__ void unit4(Fr* x, const Tw* t, Mul mul) {
    const uint32_t i = threadIdx.x;
    Fr x0 = fp_load(x + 4 * i), x1 = fp_load(x + 4 * i + 1), x2 = fp_load(x + 4 * i + 2), x3 = fp_load(x + 4 * i + 3);
    x0 = fp_lazy_red2p(x0);
    x2 = fp_lazy_red2p(x2);
    const Tw wa = t[3 * i];
    x1 = mul(x1, wa);
    x3 = mul(x3, wa);
    const Fr y0 = fp_lazy_add_red(x0, x1), y1 = fp_lazy_sub_red(x0, x1);
    Fr y2 = fp_lazy_add(x2, x3), y3 = fp_lazy_sub(x2, x3);
    y2 = mul(y2, t[3 * i + 1]);
    y3 = mul(y3, t[3 * i + 2]);
    fp_store(x + 4 * i, fp_lazy_add(y0, y2));
    fp_store(x + 4 * i + 1, fp_lazy_add(y1, y3));
    fp_store(x + 4 * i + 2, fp_lazy_sub(y0, y2));
    fp_store(x + 4 * i + 3, fp_lazy_sub(y1, y3));
}

struct TwPair {
    Fr w, q;
};

extern "C" __global__ void probe_unit4_const(Fr* x, const TwPair* t) {
    unit4(x, t, [](const Fr& v, const TwPair& w) { return fp_mul_const(v, w.w, w.q); });
}

extern "C" __global__ void probe_unit4_chunk(Fr* x, const FpChunk<2>* t) {
    unit4(x, t, [](const Fr& v, const FpChunk<2>& w) { return fp_mul_chunk(v, w); });
}
