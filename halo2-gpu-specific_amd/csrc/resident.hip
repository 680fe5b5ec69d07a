// resident.hip -- the process-wide registry of host ranges the caller promised not to modify (SRS points, polynomials),
// their device copies, and the host-buffer MSM drivers on top of them.
#include <algorithm>
#include <array>
#include <cstdlib>
#include <thread>

#include "g1util.hpp"
#include "msm.hpp"
#include "resident.hpp"

namespace h2 {

// ---- resident SRS: host ranges the caller promised not to modify (h2_bases_register).  The reference
// re-uploads the bases on every MSM (arithmetic.rs:354-360); at 2^20 that is 64 MiB of PCIe per call,
// about as long as the MSM itself.
namespace {
struct Registration {
    size_t len;    // in units of `unit` bytes: points (64) for an SRS range, field elements (32) for a polynomial
    uint64_t gen;  // bumped by every register / unregister: a device copy made for another generation is stale
    uint32_t unit; // 64: G1Affine points (h2_bases_register); 32: Fr coefficients / values (h2_poly_register: no table)
};
std::mutex g_reg_mu;
std::map<const uint64_t*, Registration> g_registered;  // host pointer -> length, generation, element size
uint64_t g_reg_gen = 0;
}  // namespace

int bases_register(const uint64_t* bases, size_t n) {
    std::lock_guard<std::mutex> g(g_reg_mu);
    g_registered[bases] = Registration{n, ++g_reg_gen, 64u};
    return H2_OK;
}

// h2_poly_register: a host vector of n field elements the caller promises not to modify -- the proving key's fixed / sigma / l_0 /
// l_last coefficient forms (plonk.rs:226-240), read by every proof (plonk/evaluation.rs:1229-1241, prover.rs:731-737) -- so that
// the host-slice entry points that READ vectors find a device copy uploaded once per device instead of crossing PCIe per call.
// Same registry, generations and unregister path as the SRS ranges; no shifted-base table, of course.
int poly_register(const uint64_t* values, size_t n) {
    std::lock_guard<std::mutex> g(g_reg_mu);
    g_registered[values] = Registration{n, ++g_reg_gen, 32u};
    return H2_OK;
}

int bases_unregister(const uint64_t* bases) {
    {
        std::lock_guard<std::mutex> g(g_reg_mu);
        g_registered.erase(bases);
        ++g_reg_gen;
    }
    // free the device copies now, on every device (under the locks of ALL its host-API slots: a host-buffer MSM holds its
    // slot's lock until its result is back, so nothing in flight reads the copy; then the shared map's own lock); a device
    // that never runs another MSM would keep them otherwise
    std::map<DeviceShared*, std::vector<DeviceCtx*>> by_device;
    for (DeviceCtx* ctx : existing_contexts()) by_device[ctx->shared].push_back(ctx);
    for (auto& dv : by_device) {
        std::sort(dv.second.begin(), dv.second.end(), [](DeviceCtx* a, DeviceCtx* b) { return a->slot < b->slot; });
        for (DeviceCtx* ctx : dv.second) ctx->mu.lock();
        {
            std::lock_guard<std::mutex> g(dv.first->mu);
            auto it = dv.first->resident.find((const void*)bases);
            if (it != dv.first->resident.end()) {
                bases_forget((const uint64_t*)it->second.ptr);
                (void)hipFree(it->second.ptr);
                dv.first->resident.erase(it);
            }
            for (ResidentCopy& c : dv.first->retired) {
                bases_forget((const uint64_t*)c.ptr);
                (void)hipFree(c.ptr);
            }
            dv.first->retired.clear();
        }
        for (DeviceCtx* ctx : dv.second) ctx->mu.unlock();
    }
    return H2_OK;
}

// device copy of a registered range that contains [bases, bases + n) -- or nullptr.  A copy is reused only for the
// registration (generation, length) it was uploaded for: unregister + refill + register of the same address uploads
// the new points.
static const void* resident_lookup_unit(DeviceCtx* ctx, const uint64_t* bases, size_t n, uint32_t unit) {
    const uint64_t* key = nullptr;
    Registration reg{0, 0, 0};
    const size_t words = unit / 8;
    // the device copies are shared by the host-API slots of the device: one slot uploads (and tabulates) an SRS, the other
    // waits here and finds it complete
    std::lock_guard<std::mutex> shared_lock(ctx->shared->mu);
    {
        std::lock_guard<std::mutex> g(g_reg_mu);
        // Device copies whose registration is gone or was replaced are never FREED here: this caller holds its own slot's
        // lock only, and the other host-API slot of the device may be in the middle of an MSM over such a copy.
        // A copy whose registration is gone is about to be freed by the h2_bases_unregister that removed it (under every
        // slot's lock); one whose registration was REPLACED (register again without unregister) steps aside into `retired`,
        // which the next unregister empties the same way.
        for (auto it = ctx->resident.begin(); it != ctx->resident.end();) {
            auto r = g_registered.find((const uint64_t*)it->first);
            if (r != g_registered.end() && (r->second.gen != it->second.gen || r->second.len != it->second.len)) {
                ctx->shared->retired.push_back(it->second);
                it = ctx->resident.erase(it);
            } else {
                ++it;
            }
        }
        auto it = g_registered.upper_bound(bases);
        if (it == g_registered.begin()) return nullptr;
        --it;
        if (it->second.unit != unit) return nullptr;      // points asked of a polynomial's range or the reverse
        if (bases + words * n > it->first + words * it->second.len) return nullptr;
        if ((size_t)(bases - it->first) % words) return nullptr;   // (not on an element boundary of the registered range)
        key = it->first;
        reg = it->second;
    }
    auto rit = ctx->resident.find((const void*)key);
    if (rit != ctx->resident.end() && (rit->second.gen != reg.gen || rit->second.len != reg.len)) return nullptr;  // (cannot happen: swept above)
    if (rit == ctx->resident.end()) {
        ResidentCopy c;
        c.len = reg.len;
        c.gen = reg.gen;
        H2_HIP(hipMalloc(&c.ptr, reg.len * (size_t)unit));
        host_upload(c.ptr, key, reg.len * (size_t)unit, ctx->stream);
        rit = ctx->resident.emplace((const void*)key, c).first;
        // a registered SRS is committed against for the life of the process: give its device copy a shifted-base table
        // when that takes less than half of the free memory (H2_MSM_TABLES=0: never)
        // -- an OPTIONAL optimisation: a failed build (allocation, launch) must not fail the MSM that triggered it; the
        // windowed pipeline answers with the same point
        const char* env = getenv("H2_MSM_TABLES");
        size_t free_b = 0, total_b = 0;
        if (unit == 64u && !(env && env[0] == '0') && reg.len >= ((size_t)1 << 15) && hipMemGetInfo(&free_b, &total_b) == hipSuccess &&
            bases_precompute_bytes(reg.len, 0) < free_b / 2) {
            try {
                if (bases_precompute((const uint64_t*)c.ptr, reg.len, 0, ctx->stream) != H2_OK) (void)hipGetLastError();
            } catch (const HipError&) {
                (void)hipGetLastError();  // clear the sticky error; no table for this copy
            }
        }
        H2_HIP(hipStreamSynchronize(ctx->stream));  // complete before another slot (another stream) can find it
    }
    return (const char*)rit->second.ptr + (size_t)(bases - key) * 8;
}
static const Affine* resident_lookup(DeviceCtx* ctx, const uint64_t* bases, size_t n) {
    return (const Affine*)resident_lookup_unit(ctx, bases, n, 64u);
}
// the device copy of host Fr values [values, values + n) when they lie inside a range registered with h2_poly_register (uploaded
// on this device's first use, complete when this returns) -- or nullptr: the caller uploads as before.  Call with the slot's lock.
const Fr* poly_resident(DeviceCtx* ctx, const uint64_t* values, size_t n) {
    {
        std::lock_guard<std::mutex> g(g_reg_mu);
        if (g_registered.empty()) return nullptr;     // (the common case of a caller that registers nothing: no device lock taken)
    }
    return (const Fr*)resident_lookup_unit(ctx, values, n, 32u);
}

int msm_host_resident_scalars(DeviceCtx* ctx, const Fr* d_scalars, const uint64_t* bases, size_t n, uint32_t max_bits,
                              uint64_t out_xyz[12]) {
    const Affine* d_bases = resident_lookup(ctx, bases, n);
    if (!d_bases) {
        Affine* up = (Affine*)ctx->buf_c.get(n * sizeof(Affine));
        host_upload(up, bases, n * sizeof(Affine), ctx->stream);
        d_bases = up;
    }
    size_t sb = msm_scratch_bytes(n, max_bits);
    void* scratch = ctx->msm_scratch.get(sb);
    return msm_device(ctx, d_scalars, (const uint64_t*)d_bases, n, max_bits, scratch, sb, out_xyz, ctx->stream);
}

int msm_host(DeviceCtx* ctx, const uint64_t* scalars, const uint64_t* bases, size_t n, uint32_t max_bits,
             uint64_t out_xyz[12]) {
    Fr* d_s = (Fr*)ctx->buf_d.get(n * sizeof(Fr));
    host_upload(d_s, scalars, n * sizeof(Fr), ctx->stream);
    return msm_host_resident_scalars(ctx, d_s, bases, n, max_bits, out_xyz);
}

// gpu_multiexp_bound (arithmetic.rs:413-440): ceil(n / N_GPU) contiguous chunks, one leased
// device each (par_chunks), partial points folded on the host (`reduce(|acc, x| acc + x)`).
int msm_host_multi(const uint64_t* scalars, const uint64_t* bases, size_t n, uint32_t max_bits, uint64_t out_xyz[12]) {
    int n_gpu = device_count();
    if (n_gpu <= 0) throw HipError{hipErrorNoDevice, "no HIP device visible", __FILE__, __LINE__};
    size_t part_len = (n + n_gpu - 1) / n_gpu;
    size_t nparts = (n + part_len - 1) / part_len;
    std::vector<std::array<uint64_t, 12>> parts(nparts);
    std::vector<int> rcs(nparts, H2_OK);
    std::vector<std::string> errs(nparts);
    std::vector<std::thread> th;
    for (size_t p = 0; p < nparts; p++) {
        th.emplace_back([&, p] {
            size_t lo = p * part_len, len = std::min(part_len, n - lo);
            rcs[p] = guarded([&] {
                DeviceLease lease;
                return msm_host(lease.ctx, scalars + 4 * lo, bases + 8 * lo, len, max_bits, parts[p].data());
            });
            if (rcs[p] != H2_OK) errs[p] = get_last_error();
        });
    }
    for (auto& t : th) t.join();
    for (size_t p = 0; p < nparts; p++)
        if (rcs[p] != H2_OK) {
            set_last_error(errs[p]);
            return rcs[p];
        }
    g1_sum_host(parts[0].data(), nparts, out_xyz);
    return H2_OK;
}
}  // namespace h2
