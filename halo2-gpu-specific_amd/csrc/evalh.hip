// evalh.hip -- the drivers of the quotient numerator h(X) on the extended coset, Evaluator::evaluate_h.
//
// Reference: CPU twin plonk/evaluation.rs:778-1226; cuda driver plonk/evaluation.rs:1229-1985, which walks ProveExpression
// trees launching one elementwise kernel per AST node (evaluation_gpu.rs:594-803) and re-derives extended cosets on demand
// through a 5-entry cache.  Here the whole gate program runs in ONE pass over the domain it is given: as kernels generated
// for it (evalh_plan.hip), or on the interpreter kernels (evalh_interp.hip).  This file holds what calls them: the device
// driver, the host-buffer driver, and the coset-by-coset driver for columns in coefficient form with its multi-device
// dealer.  The drivers read the descriptor's columns through evalh_desc.hpp only.
#include <algorithm>
#include <map>
#include <set>
#include <string>
#include <thread>
#include <vector>

#include "common.hpp"
#include "evalh.hpp"
#include "evalh_desc.hpp"
#include "ntt.hpp"
#include "poly.hpp"
#include "resident.hpp"

namespace h2 {

int evalh_device(DeviceCtx* ctx, const h2_evalh_desc* d, Fr* d_values, hipStream_t stream) {
    if (const char* bad = d_values ? evalh_validate(d, "h2_evaluate_h", EVALH_DEVICE) : "h2_evaluate_h: null argument") {
        set_last_error(bad);
        return H2_ERR_INVALID;
    }
    const size_t size = (size_t)1 << d->extended_k;
    const size_t row_begin = d->row_count ? d->row_begin : 0, row_end = d->row_count ? (size_t)d->row_begin + d->row_count : size;
    // the program as generated straight-line kernels, unless switched off or unavailable
    if (!(d->flags & H2_EVALH_INTERPRET)) {
        if (EvalhPlanRef held = evalh_plan_get(d, nullptr)) {
            evalh_plan_launch(ctx, held.get(), d, d_values, row_begin, row_end, stream);
            return H2_OK;
        }
    }
    return evalh_interpret(ctx, d, d_values, row_begin, row_end, stream);
}

namespace {
// The device memory of one host-driver call: pieces of a block the slot keeps, when one was given and while it lasts, and
// allocations of the call's own, which are freed when the call ends -- however it ends -- after its stream has drained.
class CallMemory {
    hipStream_t stream_;
    char* block_ = nullptr;
    size_t block_bytes_ = 0, block_used_ = 0;
    std::vector<void*> owned_;

public:
    explicit CallMemory(hipStream_t stream) : stream_(stream) {}
    CallMemory(const CallMemory&) = delete;
    CallMemory& operator=(const CallMemory&) = delete;
    ~CallMemory() {
        (void)hipStreamSynchronize(stream_);
        for (void* q : owned_) (void)hipFree(q);
    }
    void cut_from(void* block, size_t bytes) {
        block_ = (char*)block;
        block_bytes_ = bytes;
    }
    void* get(size_t bytes) {
        const size_t take = (bytes + 255) & ~(size_t)255;
        if (block_ && block_used_ + take <= block_bytes_) {
            void* q = block_ + block_used_;
            block_used_ += take;
            return q;
        }
        void* q = nullptr;
        H2_HIP(hipMalloc(&q, bytes));
        owned_.push_back(q);
        return q;
    }
};
}  // namespace

// Host-buffer variant: upload every coset the descriptor references (each distinct pointer once),
// run, read the values back.
int evalh_host(DeviceCtx* ctx, const h2_evalh_desc* d, uint64_t* values) {
    const size_t bytes = sizeof(Fr) << d->extended_k;
    CallMemory mem(ctx->stream);
    std::map<const uint64_t*, const uint64_t*> up;  // host -> device
    const EvalhRemap on_device = evalh_remap(d, [&](evgen::Table, const uint64_t* h) {
        auto it = up.find(h);
        if (it != up.end()) return it->second;
        void* q = mem.get(bytes);
        host_upload(q, h, bytes, ctx->stream);
        return up[h] = (const uint64_t*)q;
    });
    void* d_values = mem.get(bytes);
    int rc = evalh_device(ctx, &on_device.desc, (Fr*)d_values, ctx->stream);
    if (rc == H2_OK) {
        host_download(values, d_values, bytes, ctx->stream);
        H2_HIP(hipStreamSynchronize(ctx->stream));
    }
    return rc;
}

// ---------------------------------------------------------------- coefficient forms in, extended values out
// out[i] = in[c * i + j]  /  out[c * i + j] = in[i]: one coset of the n-th roots of unity inside the extended domain
__global__ void __launch_bounds__(256) k_coset_gather(const Fr* in, Fr* out, size_t n, uint32_t log_c, uint32_t j) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) fp_store(out + i, fp_load(in + ((i << log_c) | j)));
}
__global__ void __launch_bounds__(256) k_coset_scatter(const Fr* in, Fr* out, size_t n, uint32_t log_c, uint32_t j) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) fp_store(out + ((i << log_c) | j), fp_load(in + i));
}

// The shape of the reference's cuda `Evaluator::evaluate_h` (plonk/evaluation.rs:1229-1985): every column arrives as a
// COEFFICIENT vector of 2^k elements in host memory (the `cuda` proving key keeps no extended cosets, plonk.rs:226-240),
// `l_active_row` as extended values (2^extended_k, host), and the numerator comes back as 2^extended_k host values.
// The reference re-derives extended cosets through a 5-entry cache while it walks its expression trees; here the
// extended domain is visited one coset g_j H of the n-th roots of unity at a time (g_j = zeta * extended_omega^j,
// extended index c i + j = point i of coset j, c = 2^(extended_k - k)): every distinct column is uploaded ONCE, taken to
// coset j by a[t] *= g_j^t and an n-point NTT, and the fused evaluator runs with extended_k := k, zeta := g_j,
// extended_omega := omega -- on one coset a rotation is an index shift and nothing else changes.  Device memory is
// (distinct columns) x 2 x 2^k x 32 B + two extended vectors: bounded by the circuit's width, not by width x 2^extended_k.
//
// One worker = one leased device running the cosets first, first + step, ...  With `whole` (the only worker) the values
// are scattered to their stride-c positions on the device and come back in one transfer; otherwise each coset's n values
// come back through the slot's pinned buffer and this thread writes them to values[c i + j] (the workers of the other
// devices do the same for their cosets at the same time: disjoint 32-byte cells of the caller's vector).
static int evalh_coeffs_worker(DeviceCtx* ctx, const h2_evalh_desc* d, uint64_t* values, uint32_t first, uint32_t step, bool whole,
                               const EvalhFinish* finish = nullptr) {
    const uint32_t log_c = d->extended_k - d->k, c = 1u << log_c;
    const size_t n = (size_t)1 << d->k, size = (size_t)1 << d->extended_k;
    const size_t nbytes = n * sizeof(Fr), ebytes = size * sizeof(Fr);
    hipStream_t stream = ctx->stream;
    CallMemory mem(stream);
    // the distinct coefficient vectors, in the descriptor's order (l_active_row is extended values: it goes its own way below)
    std::vector<const uint64_t*> distinct;
    {
        std::set<const uint64_t*> seen;
        evalh_for_each_column(d, [&](evgen::Table t, size_t, const uint64_t* h) {
            if (h && t != evgen::T_L_ACTIVE && seen.insert(h).second) distinct.push_back(h);
        });
    }
    // scratch of a batch of transforms: up to 16 vectors per launch, fewer when that would pass 1 GiB
    const size_t batch_width = std::max<size_t>(1, std::min<size_t>(16, ((size_t)1 << 30) / nbytes));
    // ONE device block for the call, handed out piece by piece (a call used to make ~2 x columns + 5 hipMalloc / hipFree pairs,
    // every hipFree a device synchronisation); sized from the distinct vectors of the descriptor, individual allocations if the
    // block cannot be had or turns out short.  The block belongs to the slot (ctx->coeff_arena, grow-only, given back by
    // h2_release_plans): a hipMalloc of 6.4 GiB per call (k = 22, 16 columns) took 0.3 ms when the runtime still had the range
    // of the previous call and 160 ms when it did not -- one proof in three of the literal drop-in's measured sequence.
    try {
        const size_t arena_bytes = (2 * distinct.size() + 2 + batch_width) * (nbytes + 256) + (whole ? 2 * (ebytes + 256) : 0);
        mem.cut_from(ctx->coeff_arena.get(arena_bytes), arena_bytes);
    } catch (const HipError&) {
        (void)hipGetLastError();
    }
    // every distinct coefficient vector once: (device coefficients, device values on the current coset)
    std::map<const uint64_t*, std::pair<Fr*, Fr*>> cols;
    for (const uint64_t* h : distinct) {
        // a vector inside a range registered with h2_poly_register (the proving key's fixed / sigma / l_0 / l_last forms,
        // plonk.rs:226-240) already has its device copy: only read here, never written
        Fr* dc = const_cast<Fr*>(poly_resident(ctx, h, n));
        if (!dc) {
            dc = (Fr*)mem.get(nbytes);
            host_upload(dc, h, nbytes, stream);
        }
        Fr* dv = (Fr*)mem.get(nbytes);
        cols[h] = {dc, dv};
    }
    Fr* d_active = nullptr;
    Fr* d_active_j = nullptr;
    Fr* d_values = nullptr;
    Fr* stage = nullptr;  // pinned, n elements: one coset of l_active_row on its way in, one coset of values on its way out
    if (d->l_active_row) d_active_j = (Fr*)mem.get(nbytes);
    if (whole) {
        if (d->l_active_row) {
            // (the proving key's l_active_row, extended values: registered with the key's other vectors, plonk.rs:224)
            d_active = const_cast<Fr*>(poly_resident(ctx, d->l_active_row, size));
            if (!d_active) {
                d_active = (Fr*)mem.get(ebytes);
                host_upload(d_active, d->l_active_row, ebytes, stream);
            }
        }
        d_values = (Fr*)mem.get(ebytes);
    } else {
        stage = (Fr*)ctx->pinned.get(nbytes);
    }
    Fr* d_values_j = (Fr*)mem.get(nbytes);
    Fr* d_tmp = (Fr*)mem.get(batch_width * nbytes);
    // omega = extended_omega^c generates the n-th roots of unity
    const Fr w_ext = fr_from_u64x4(d->extended_omega), zeta = fr_from_u64x4(d->zeta);
    Fr omega = w_ext;
    for (uint32_t t = 0; t < log_c; t++) omega = fp_sqr(omega);
    // the descriptor of one coset: every column's values on it, extended_k := k, extended_omega := omega; zeta := g_j below
    EvalhRemap on_coset = evalh_remap(d, [&](evgen::Table t, const uint64_t* h) {
        return (const uint64_t*)(t == evgen::T_L_ACTIVE ? d_active_j : cols[h].second);
    });
    on_coset.desc.extended_k = d->k;
    fr_to_u64x4(omega, on_coset.desc.extended_omega);
    PlanRef pl = ntt_get_plan(ctx, d->k, on_coset.desc.extended_omega, stream);
    const unsigned nblocks = (unsigned)((n + 255) / 256);
    const Fr w_step = fp_pow_u32(w_ext, step);
    Fr g = fp_mul(zeta, fp_pow_u32(w_ext, first));  // g_first
    const Fr* active_host = (const Fr*)d->l_active_row;
    for (uint32_t j = first; j < c; j += step) {
        {
            // every column to coset j in batched, fused coset transforms (ntt.hip: g_j^t applied in the first pass's load,
            // sixteen vectors per launch): no copy, no separate scaling pass
            std::vector<const Fr*> srcs;
            std::vector<Fr*> dsts, tmps;
            for (auto& kv : cols) {
                srcs.push_back(kv.second.first);
                dsts.push_back(kv.second.second);
                tmps.push_back(d_tmp + (tmps.size() % batch_width) * n);
            }
            NttTablePin tab = ntt_scale_table(pl.get(), g, nullptr, stream);
            for (size_t at = 0; at < srcs.size(); at += batch_width)   // (a chunk's scratch slots are distinct)
                ntt_run_many(ctx, pl.get(), srcs.data() + at, dsts.data() + at, tmps.data() + at,
                             std::min(batch_width, srcs.size() - at), (uint32_t)n, nullptr, nullptr, stream, tab.get(), 1u);
        }
        if (d_active) {
            hipLaunchKernelGGL(k_coset_gather, dim3(nblocks), dim3(256), 0, stream, d_active, d_active_j, n, log_c, j);
        } else if (active_host) {
            for (size_t i = 0; i < n; i++) stage[i] = active_host[(i << log_c) | j];
            H2_HIP(hipMemcpyAsync(d_active_j, stage, nbytes, hipMemcpyHostToDevice, stream));
        }
        fr_to_u64x4(g, on_coset.desc.zeta);
        if (int rc = evalh_device(ctx, &on_coset.desc, d_values_j, stream)) return rc;
        if (whole) {
            hipLaunchKernelGGL(k_coset_scatter, dim3(nblocks), dim3(256), 0, stream, d_values_j, d_values, n, log_c, j);
        } else {
            H2_HIP(hipMemcpyAsync(stage, d_values_j, nbytes, hipMemcpyDeviceToHost, stream));
            H2_HIP(hipStreamSynchronize(stream));
            Fr* out = (Fr*)values;
            for (size_t i = 0; i < n; i++) out[(i << log_c) | j] = stage[i];
        }
        g = fp_mul(g, w_step);
    }
    H2_HIP(hipGetLastError());
    int frc = H2_OK;
    if (whole && finish)
        frc = (*finish)(ctx, d_values, stream);          // (what follows the evaluation, on the device: capi.hip)
    else if (whole)
        host_download(values, d_values, ebytes, stream);
    H2_HIP(hipStreamSynchronize(stream));
    return frc;
}

// The reference's cuda evaluate_h deals its gates / lookups / shuffles over the N_GPU devices of the process inside the one
// call (plonk/evaluation.rs:326-333,1262-1275,1513-1520,1830-1837: `group_expr_len`, one thread per GPU).  Here the unit is a
// coset of the extended domain -- the work per coset is the same and nothing is exchanged between cosets: P = min(pool
// size, cosets) threads lease a device each (acquire_gpu, arithmetic.rs:314-321), upload the coefficient vectors once per
// device and take the cosets p, p + P, ...; with one device (or one coset) the caller's thread does it all.
uint32_t evalh_host_workers(const h2_evalh_desc* d) {
    const uint32_t c = 1u << (d->extended_k - d->k);
    return (uint32_t)std::max(1, std::min<int>(device_count(), (int)c));
}

int evalh_host_coeffs(const h2_evalh_desc* d, uint64_t* values) { return evalh_host_coeffs(d, values, nullptr, nullptr); }

int evalh_host_coeffs(const h2_evalh_desc* d, uint64_t* values, const EvalhFinish* finish, bool* finished) {
    if (finished) *finished = false;
    const uint32_t workers = evalh_host_workers(d);
    if (!values && !(finish && workers <= 1)) {
        set_last_error("h2_evaluate_h_coeff: null argument");
        return H2_ERR_INVALID;
    }
    if (workers <= 1) {
        DeviceLease lease;
        if (finished) *finished = finish != nullptr;
        return evalh_coeffs_worker(lease.ctx, d, values, 0, 1, true, finish);
    }
    std::vector<int> rcs(workers, H2_OK);
    std::vector<std::string> errs(workers);
    std::vector<std::thread> th;
    for (uint32_t p = 0; p < workers; p++) {
        th.emplace_back([&, p] {
            rcs[p] = guarded([&] {
                DeviceLease lease;
                return evalh_coeffs_worker(lease.ctx, d, values, p, workers, false);
            });
            if (rcs[p] != H2_OK) errs[p] = get_last_error();
        });
    }
    for (auto& t : th) t.join();
    for (uint32_t p = 0; p < workers; p++)
        if (rcs[p] != H2_OK) {
            set_last_error(errs[p]);
            return rcs[p];
        }
    return H2_OK;
}

}  // namespace h2
