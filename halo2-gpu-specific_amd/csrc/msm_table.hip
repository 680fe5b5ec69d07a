// msm_table.hip -- shifted-base tables: the process-wide registry, the kernels that build and check a table, and
// h2_dev_bases_precompute / _forget.  How a table changes the pipeline's shape is msm_plan.cpp's msm_shape_table.
//
// A base table that is committed against again and again (the SRS: `params.g`, `params.g_lagrange`,
// poly/commitment.rs:148-170) can be expanded ONCE into T[j][i] = [2^(o_j)] P_i, o_j = the bit offset of digit j
// (h2_dev_bases_precompute; D x n x 64 B -- 12 GiB for 2^24 points, which is what 288 GB of HBM are for).  Digit j of
// scalar i then adds T[j][i] into bucket |d| - 1 of a bucket set SHARED by all digits:
//     sum_i s_i P_i = sum_i sum_j d_ij [2^(o_j)] P_i = sum_b (b + 1) * (sum of the +-T[j][i] with |d_ij| = b + 1),
// so the number of buckets no longer grows with the number of windows and the windows can be much wider than 17 bits:
// 12 digits of 22 / 21 bits instead of 15 of 17 at 2^24 (a fifth of the additions gone), one k_reduce window instead
// of 15-20 (the latency-bound tail of small MSMs), no Horner on the host.  Semantics unchanged (arithmetic.rs:20-108).
#include <map>
#include <mutex>

#include "msm.hpp"
#include "msm_kernels.hpp"
#include "msm_table.hpp"

namespace h2 {

namespace {
std::mutex g_tab_mu;
std::map<const uint64_t*, ShiftTable> g_tables;  // device base pointer -> its table
}  // namespace

bool table_find(const uint64_t* d_bases, size_t n, const MsmKnobs& k, ShiftTable* out) {
    if (k.no_table) return false;
    std::lock_guard<std::mutex> g(g_tab_mu);
    auto it = g_tables.upper_bound(d_bases);
    if (it == g_tables.begin()) return false;
    --it;
    if (d_bases + 8 * n > it->first + 8 * it->second.desc.n) return false;
    ShiftTable t = it->second;
    const size_t off = (size_t)(d_bases - it->first) / 8;
    t.table += off;
    t.blocks = (t.blocks && off % BLOCK_ROWS == 0) ? t.blocks + off / BLOCK_ROWS : nullptr;
    *out = t;
    return true;
}

void table_drop_containing(const uint64_t* d_bases) {
    const uint64_t* key = nullptr;
    {
        std::lock_guard<std::mutex> g(g_tab_mu);
        auto it = g_tables.upper_bound(d_bases);
        if (it == g_tables.begin()) return;
        --it;
        if (d_bases >= it->first + 8 * it->second.desc.n) return;
        key = it->first;
    }
    bases_forget(key);
}

std::vector<TableDesc> tables_covering(size_t n) {
    std::vector<TableDesc> out;
    std::lock_guard<std::mutex> g(g_tab_mu);
    for (const auto& kv : g_tables)
        if (kv.second.desc.n >= n) out.push_back(kv.second.desc);
    return out;
}

size_t table_library_bytes() {
    size_t bytes = 0;
    std::lock_guard<std::mutex> g(g_tab_mu);
    for (const auto& kv : g_tables) {
        const TableDesc& d = kv.second.desc;
        bytes += (size_t)d.D * d.n * sizeof(Affine) + (kv.second.blocks ? d.n / BLOCK_ROWS * sizeof(Affine) : 0);
    }
    return bytes;
}

// ---------------------------------------------------------------- shifted-base table build (h2_dev_bases_precompute)
// One lane per base point: level j = [2^(width of digit j - 1)] level j - 1 by Jacobian doublings (a = 0, 2M + 5S
// [dbl-2009-l]; BN254 G1 has prime order, so a doubling never meets the identity), X and Y parked in the table slot and
// Z kept per level; then ONE inversion for all levels of the point (Montgomery's trick) and x = X / Z^2, y = Y / Z^3.
// ~2300 field products per point: 0.3 s for 2^24 points, paid once per SRS.
__global__ void __launch_bounds__(256) k_table_build(const Affine* bases, size_t n, size_t stride, uint32_t D, uint32_t c,
                                                     uint32_t wfull, Affine* table) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const Affine p = affine_load(bases + i);
    fp_store(&table[i].x, p.x);
    fp_store(&table[i].y, p.y);
    if (affine_is_identity(p)) {
        const Fq zero = fp_zero<FqParams>();
        for (uint32_t j = 1; j < D; j++) {
            fp_store(&table[j * stride + i].x, zero);
            fp_store(&table[j * stride + i].y, zero);
        }
        return;
    }
    Fq z[TABLE_MAX_D], pre[TABLE_MAX_D];
    Fq X = p.x, Y = p.y, Z = fp_one<FqParams>();
#pragma unroll 1
    for (uint32_t j = 1; j < D; j++) {
        const uint32_t cw = c - ((j - 1) >= wfull ? 1u : 0u);
#pragma unroll 1
        for (uint32_t k = 0; k < cw; k++) {
            const Fq A = fp_sqr(X), B = fp_sqr(Y), C = fp_sqr(B);
            Fq Dd = fp_sub(fp_sub(fp_sqr(fp_add(X, B)), A), C);
            Dd = fp_dbl(Dd);
            const Fq E = fp_add(fp_dbl(A), A);
            const Fq F = fp_sqr(E);
            const Fq Z3 = fp_dbl(fp_mul(Y, Z));
            X = fp_sub(F, fp_dbl(Dd));
            const Fq C8 = fp_dbl(fp_dbl(fp_dbl(C)));
            Y = fp_sub(fp_mul(E, fp_sub(Dd, X)), C8);
            Z = Z3;
        }
        fp_store(&table[j * stride + i].x, X);
        fp_store(&table[j * stride + i].y, Y);
        z[j] = Z;
        pre[j] = j == 1 ? Z : fp_mul(pre[j - 1], Z);
    }
    if (D < 2) return;
    Fq inv = fq_inv_device(pre[D - 1]);
#pragma unroll 1
    for (uint32_t j = D - 1; j >= 1; j--) {
        const Fq zinv = j == 1 ? inv : fp_mul(inv, pre[j - 1]);
        inv = fp_mul(inv, z[j]);
        const Fq zi2 = fp_sqr(zinv);
        Affine* slot = table + (j * stride + i);
        fp_store(&slot->x, fp_mul(fp_load(&slot->x), zi2));
        fp_store(&slot->y, fp_mul(fp_load(&slot->y), fp_mul(zi2, zinv)));
    }
}

// A table is keyed by the ADDRESS of its bases: freed and re-allocated device memory can come back at the same address
// with other points in it.  Every MSM that is about to use a table therefore compares 64 sampled base rows with level 0
// of the table (a copy of the bases as they were) next to the scalar sampling -- same stream, same synchronisation -- and
// a table that no longer matches is dropped instead of producing a wrong commitment.
__global__ void __launch_bounds__(HOT_SAMPLES) k_table_check(const Affine* bases, const Affine* level0, size_t n, uint32_t* stale) {
    const size_t idx = ((size_t)threadIdx.x * 0x9E3779B1ull + 0x7F4A7C15ull) % n;
    const uint4* a = (const uint4*)(bases + idx);
    const uint4* b = (const uint4*)(level0 + idx);
    bool differ = false;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const uint4 x = a[k], y = b[k];
        differ |= x.x != y.x || x.y != y.y || x.z != y.z || x.w != y.w;
    }
    if (differ) *stale = 1u;
}

void table_check_launch(const Affine* bases, const Affine* level0, size_t n, uint32_t* stale, hipStream_t stream) {
    hipLaunchKernelGGL(k_table_check, dim3(1), dim3(HOT_SAMPLES), 0, stream, bases, level0, n, stale);
}

size_t bases_precompute_bytes(size_t n, uint32_t digits) {
    if (digits == 0) digits = table_default_digits(n, msm_knobs());
    return (size_t)digits * n * sizeof(Affine);
}

int bases_forget(const uint64_t* d_bases) {
    Affine *old = nullptr, *old_blocks = nullptr;
    {
        std::lock_guard<std::mutex> g(g_tab_mu);
        auto it = g_tables.find(d_bases);
        if (it == g_tables.end()) return H2_OK;
        old = const_cast<Affine*>(it->second.table);
        old_blocks = const_cast<Affine*>(it->second.blocks);
        g_tables.erase(it);
    }
    H2_HIP(hipDeviceSynchronize());  // nothing in flight reads the table
    H2_HIP(hipFree(old));
    if (old_blocks) H2_HIP(hipFree(old_blocks));
    return H2_OK;
}

int bases_precompute(const uint64_t* d_bases, size_t n, uint32_t digits, hipStream_t stream) {
    const MsmKnobs knobs = msm_knobs();
    if (n == 0) return H2_OK;
    if (digits == 0) digits = table_default_digits(n, knobs);
    if (digits < TABLE_MIN_D || digits > TABLE_MAX_D || (size_t)digits * n >= ((size_t)1 << 31)) {
        set_last_error("h2 bases_precompute: digits must be 11..32 and digits * n < 2^31 (table rows are indexed with 31 bits)");
        return H2_ERR_INVALID;
    }
    bases_forget(d_bases);
    ShiftTable t{};
    t.desc = table_desc(n, digits);
    Affine *table = nullptr, *blocks = nullptr;
    const size_t nblocks = n / BLOCK_ROWS;
    H2_HIP(hipMalloc(&table, (size_t)digits * n * sizeof(Affine)));
    if (nblocks && hipMalloc(&blocks, nblocks * sizeof(Affine)) != hipSuccess) blocks = nullptr;  // optional
    hipLaunchKernelGGL(k_table_build, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, (const Affine*)d_bases, n, n,
                       t.desc.D, t.desc.c, t.desc.wfull, table);
    if (blocks) block_sums_launch((const Affine*)d_bases, nblocks, blocks, stream);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    if (e != hipSuccess) {
        (void)hipFree(table);
        if (blocks) (void)hipFree(blocks);
        H2_HIP(e);
    }
    t.table = table;
    t.blocks = blocks;
    std::lock_guard<std::mutex> g(g_tab_mu);
    g_tables[d_bases] = t;
    return H2_OK;
}

}  // namespace h2
