// capi.hip -- the extern "C" boundary declared in include/halo2_hip.h.
// Host-buffer entry points = the reference's gpu_* functions (arithmetic.rs:134-534) with the
// per-call program creation removed: a pooled device context keeps streams, scratch and
// twiddle plans alive across calls.  h2_dev_* = the same ops on device-resident data.
#include <cstring>
#include <sys/mman.h>
#include <thread>

#include "assigned.hpp"
#include "check.hpp"
#include "common.hpp"
#include "evalh.hpp"
#include "evalh_desc.hpp"
#include "g1mul.hpp"
#include "g1ntt.hpp"
#include "g1util.hpp"
#include "msm.hpp"
#include "ntt.hpp"
#include "poly.hpp"
#include "logup.hpp"
#include "permmap.hpp"
#include "place.hpp"
#include "selectors.hpp"
#include "coverage.hpp"
#include "rangecheck.hpp"
#include "resident.hpp"
#include "scan.hpp"
#include "sort.hpp"
#include "srscheck.hpp"
#include "values.hpp"

using namespace h2;

namespace {

hipStream_t pick_stream(DeviceCtx* ctx, void* stream) { return stream ? (hipStream_t)stream : ctx->stream; }

DeviceCtx* current_ctx() {
    int dev = 0;
    H2_HIP(hipGetDevice(&dev));
    return ctx_for(dev);
}

int bad(const char* msg) {
    set_last_error(msg);
    return H2_ERR_INVALID;
}

// do the element ranges [a, a + na) and [b, b + nb) share a byte?  (ranges that only touch do not; an empty one never does)
static bool fr_ranges_overlap(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return na && nb && a0 < b0 + nb * sizeof(Fr) && b0 < a0 + na * sizeof(Fr);
}

int dev_ntt_impl(DeviceCtx* ctx, const Fr* src, Fr* dst, Fr* tmp, uint32_t in_len, const uint64_t omega[4],
                 uint32_t log_n, const Fr* pre3, const Fr* post3, hipStream_t s) {
    if (log_n > 28) return bad("log_n exceeds the 2-adicity of Fr (S = 28)");
    std::vector<uint32_t> bits;
    ntt_split(log_n, bits);
    if (bits.size() >= 2 && tmp == nullptr) return bad("NTT of this size needs a scratch buffer (d_tmp)");
    PlanRef pl = ntt_get_plan(ctx, log_n, omega, s);  // pinned until the passes are launched
    ntt_run(ctx, pl.get(), src, dst, tmp, in_len, pre3, post3, s);
    return H2_OK;
}

int dev_extended_to_coeff_impl(DeviceCtx* ctx, Fr* d_a, Fr* d_tmp, uint32_t extended_k, const uint64_t g_coset[4],
                               const uint64_t g_coset_inv[4], const uint64_t extended_omega_inv[4],
                               const uint64_t extended_ifft_divisor[4], hipStream_t s) {
    // into_coset = false: coset_powers = [g_coset_inv, g_coset] (domain.rs:385-387), fused with the
    // iFFT divisor: y[i] *= divisor * {1, g_coset_inv, g_coset}[i % 3].
    Fr d = fr_from_u64x4(extended_ifft_divisor);
    Fr gi = fr_from_u64x4(g_coset_inv), g = fr_from_u64x4(g_coset);
    Fr post3[3] = {d, fp_mul(d, gi), fp_mul(d, g)};  // host-side Montgomery products
    return dev_ntt_impl(ctx, d_a, d_a, d_tmp, 1u << extended_k, extended_omega_inv, extended_k, nullptr, post3, s);
}

// Elementwise host-slice operations over long vectors run as a pipeline of chunks on three streams of the slot: chunk c + 1
// crosses PCIe on the copy stream while the kernel of chunk c runs on the compute stream and the result of chunk c - 1 leaves
// on the third -- the two directions of the link at once, instead of upload-all -> compute -> download-all on one stream.
// Two staging slots; `up` / `run` / `down` enqueue on the stream they are handed.  From page-locked host memory the copies are
// asynchronous DMA and the overlap is real; from ordinary memory hipMemcpyAsync stages and returns when the source has been
// read, so the chunks follow one another as before (no worse: the same bytes in smaller pieces).
constexpr size_t PIPE_CHUNK = (size_t)1 << 19;      // elements per chunk: 16 MiB
constexpr size_t PIPE_MIN = (size_t)1 << 21;        // shorter vectors keep the single-shot form
template <class Up, class Run, class Down>
void pipeline_chunks(DeviceCtx* ctx, size_t total, Up up, Run run, Down down) {
    hipEvent_t in_done[2], k_done[2], out_done[2];
    for (int i = 0; i < 2; i++) {
        H2_HIP(hipEventCreateWithFlags(&in_done[i], hipEventDisableTiming));
        H2_HIP(hipEventCreateWithFlags(&k_done[i], hipEventDisableTiming));
        H2_HIP(hipEventCreateWithFlags(&out_done[i], hipEventDisableTiming));
    }
    struct Guard {
        hipEvent_t* a;
        hipEvent_t* b;
        hipEvent_t* c;
        DeviceCtx* ctx;
        ~Guard() {
            // (also on the way out of a throw: nothing may still be reading the staging slots when the caller's frame goes)
            (void)hipStreamSynchronize(ctx->copy_stream);
            (void)hipStreamSynchronize(ctx->stream);
            (void)hipStreamSynchronize(ctx->aux_stream[0]);
            for (int i = 0; i < 2; i++) {
                (void)hipEventDestroy(a[i]);
                (void)hipEventDestroy(b[i]);
                (void)hipEventDestroy(c[i]);
            }
        }
    } guard{in_done, k_done, out_done, ctx};
    size_t c = 0;
    for (size_t off = 0; off < total; off += PIPE_CHUNK, c++) {
        const size_t len = std::min(PIPE_CHUNK, total - off);
        const int slot = (int)(c & 1);
        if (c >= 2) H2_HIP(hipStreamWaitEvent(ctx->copy_stream, out_done[slot], 0));   // the slot's previous result has left
        up(off, len, slot, ctx->copy_stream);
        H2_HIP(hipEventRecord(in_done[slot], ctx->copy_stream));
        H2_HIP(hipStreamWaitEvent(ctx->stream, in_done[slot], 0));
        run(off, len, slot, ctx->stream);
        H2_HIP(hipEventRecord(k_done[slot], ctx->stream));
        H2_HIP(hipStreamWaitEvent(ctx->aux_stream[0], k_done[slot], 0));
        down(off, len, slot, ctx->aux_stream[0]);
        H2_HIP(hipEventRecord(out_done[slot], ctx->aux_stream[0]));
    }
    H2_HIP(hipStreamSynchronize(ctx->aux_stream[0]));
    H2_HIP(hipStreamSynchronize(ctx->stream));
}
bool pipeline_enabled() {
    static const bool on = !(getenv("H2_HOST_PIPELINE") && atoi(getenv("H2_HOST_PIPELINE")) == 0);
    return on;
}
// page-locked host memory (hipHostMalloc / h2_host_alloc_pinned / hipHostRegister)?  Only then are the chunk copies asynchronous
// DMA; from ordinary memory every hipMemcpyAsync stages and blocks, and sixteen small blocking copies are slower than one large
// one (measured: the k = 22 drop-in proof from ordinary memory 1.25 -> 1.52 s with the pipeline forced on): single shot there.
bool use_pipeline(size_t size, std::initializer_list<const void*> host) {
    if (!pipeline_enabled() || size < PIPE_MIN) return false;
    for (const void* p : host)
        if (!host_pinned(p)) return false;
    return true;
}
// One early exit for a failed launch (the *_launch functions have set h2_last_error).
#define H2_TRY(expr)                        \
    do {                                    \
        const int h2_rc_ = (expr);          \
        if (h2_rc_ != H2_OK) return h2_rc_; \
    } while (0)

// A result vector in ORDINARY host memory that nobody has touched yet -- what every operation of the reference's data flow
// returns: a fresh `Vec` -- faults its pages in one by one under the device-to-host copy, on the runtime's single staging thread:
// 21 ms for the 128 MiB of a k = 22 vector against 2.5 ms on the link (tools/experiments/hostreg_probe.py).  The pages of the
// destination are populated HERE instead, by a few threads at once -- huge pages advised, then one read-write touch per 4 KiB
// page of the slice -- started when the call begins, under its uploads and kernels, and joined before the copy back is issued.
// Touching beats MADV_POPULATE_WRITE on the same advised range (a 128 MiB result: 5.6 ms per call against 8.4, 5.3 ms when the
// pages already exist; four calls at once 19.6-20 ms against 27-31: tools/experiments/prefault_mode_ab.sh);
// H2_HOST_PREFAULT_POPULATE=1 selects the madvise form.  Page-locked destinations and short ones are left alone;
// H2_HOST_PREFAULT=<threads> (default 4; 0 switches it off).
#ifndef MADV_POPULATE_WRITE
#define MADV_POPULATE_WRITE 23
#endif
// The RESULT of one host-slice call: `n` elements that the call writes to the caller's vector `host`.  `inputs`: every host
// vector the call reads.  A result that is one of them (an in-place call; h2_permutation_terms' num / den when they are
// multiplied into) has its pages already and is left alone; any other is prefaulted from here on.  Every way from device
// memory to `host` joins the touch threads first -- their `*q = *q` is a non-atomic read-then-write of a byte, and one that ran
// after a copy would put a stale byte over downloaded data -- and a result that is never written joins when it goes.
class HostResult {
    struct Prefault {
        std::vector<std::thread> workers;
        void start(void* dst, size_t bytes) {
            static const int threads = [] {
                const char* e = getenv("H2_HOST_PREFAULT");
                const int v = e ? atoi(e) : 4;
                return v < 0 ? 0 : (v > 32 ? 32 : v);
            }();
            if (!threads || !dst || bytes < ((size_t)4 << 20) || host_pinned(dst)) return;
            const uintptr_t page = 4096, lo = ((uintptr_t)dst + page - 1) & ~(page - 1), hi = ((uintptr_t)dst + bytes) & ~(page - 1);
            if (hi <= lo) return;
            // huge pages where the kernel grants them (transparent_hugepage = madvise or always): 512 times fewer faults to take
            (void)madvise((void*)lo, hi - lo, MADV_HUGEPAGE);
            const size_t pages = (hi - lo) / page, per = (((pages + threads - 1) / threads) + 511) & ~(size_t)511;   // slices of whole 2 MiB
            for (int t = 0; t < threads; t++) {
                const size_t first = (size_t)t * per, count = first < pages ? std::min(per, pages - first) : 0;
                if (!count) break;
                char* at = (char*)lo + first * page;
                workers.emplace_back([at, count] {
                    static const bool populate = getenv("H2_HOST_PREFAULT_POPULATE") && atoi(getenv("H2_HOST_PREFAULT_POPULATE")) != 0;
                    if (populate && madvise(at, count * page, MADV_POPULATE_WRITE) == 0) return;
                    for (size_t i = 0; i < count; i++) {   // (the value written is the one read)
                        volatile char* q = at + i * page;
                        *q = *q;
                    }
                });
            }
        }
        void join() {
            for (std::thread& w : workers) w.join();
            workers.clear();
        }
        ~Prefault() { join(); }
    };

    uint64_t* host_;
    size_t n_;
    Prefault pf_;
    friend class ChunkSink;
    void put(size_t off, size_t len, const Fr* d_src, hipStream_t s) {
        pf_.join();
        host_download(host_ + 4 * off, d_src, len * sizeof(Fr), s);
    }

public:
    HostResult(uint64_t* host, size_t n, const void* const* inputs, size_t n_inputs) : host_(host), n_(n) {
        for (size_t i = 0; i < n_inputs; i++)
            if (inputs[i] == (const void*)host) return;
        pf_.start(host, n * sizeof(Fr));
    }
    HostResult(uint64_t* host, size_t n, std::initializer_list<const void*> inputs = {}) : HostResult(host, n, inputs.begin(), inputs.size()) {}
    // the whole result from device memory; the stream has drained when this returns: the call may return its status
    int write(const Fr* d_src, hipStream_t s) {
        put(0, n_, d_src, s);
        H2_HIP(hipStreamSynchronize(s));
        return H2_OK;
    }
    // for a callee that copies into the vector itself (evalh_host, evalh_host_coeffs): joined here, just before that call
    uint64_t* handed_over() {
        pf_.join();
        return host_;
    }
};

// What `down` of HostCall::chunked is handed instead of a stream: rows [off, off + len) of a result, from device memory.
// Only chunked makes one, and chunked drains the stream behind it.
class ChunkSink {
    hipStream_t s_;
    friend class HostCall;
    explicit ChunkSink(hipStream_t s) : s_(s) {}

public:
    void operator()(HostResult& r, size_t off, size_t len, const Fr* d_src) const { r.put(off, len, d_src, s_); }
};

// The scope of one host-slice call: a slot of the device pool is leased for as long as it lives (one in-flight call per slot;
// the calling thread is on the slot's device), and the call's operands reach the device through it.
class HostCall {
    DeviceLease lease_;

public:
    DeviceCtx* const ctx;
    const hipStream_t stream;      // the slot's compute stream
    HostCall() : ctx(lease_.ctx), stream(lease_.ctx->stream) {}

    // A host vector that a call only READS: the device copy of a range registered with h2_poly_register (uploaded once per
    // device: the proving key's coefficient forms, a proof's final polynomials), or nullptr -- the caller then uploads as the
    // reference does.
    const Fr* resident(const uint64_t* host, size_t n) const { return host ? poly_resident(ctx, host, n) : nullptr; }
    // `bytes` of any host data into the staging buffer
    void* upload(DevBuf& buf, const void* host, size_t bytes) {
        void* d = buf.get(bytes);
        host_upload(d, host, bytes, stream);
        return d;
    }
    // a read-only operand of n elements: where it lies on the device when registered, else uploaded into the staging buffer
    const Fr* in(DevBuf& buf, const uint64_t* host, size_t n) {
        const Fr* d = resident(host, n);
        return d ? d : (const Fr*)upload(buf, host, n * sizeof(Fr));
    }
    // `count` read-only operands of n elements each: the registered ones where they lie, the others side by side in ONE staging
    // buffer (`extra` bytes longer), a host vector that is named several times once
    std::vector<const Fr*> in_packed(DevBuf& buf, const uint64_t* const* hosts, size_t count, size_t n, size_t extra = 0) {
        std::vector<const Fr*> d(count);
        std::map<const uint64_t*, size_t> staged;        // host vector -> its slot in the upload block
        for (size_t j = 0; j < count; j++) {
            d[j] = resident(hosts[j], n);
            if (!d[j]) staged.emplace(hosts[j], staged.size());
        }
        if (staged.empty() && !extra) return d;
        Fr* up = (Fr*)buf.get(staged.size() * n * sizeof(Fr) + extra);
        for (auto& kv : staged) host_upload(up + kv.second * n, kv.first, n * sizeof(Fr), stream);
        for (size_t j = 0; j < count; j++)
            if (!d[j]) d[j] = up + staged[hosts[j]] * n;
        return d;
    }

    // An elementwise operation over `total` elements, stated once as `up` / `run` / `down` (each enqueues rows [off, off + len)
    // in staging slot `slot`; `run` returns the launch's status): chunk by chunk through pipeline_chunks, or in one piece on the
    // compute stream.  The caller sizes its staging for the form it chose: chunk = pipelined ? PIPE_CHUNK : total.
    template <class Up, class Run, class Down>
    int chunked(size_t total, bool pipelined, Up up, Run run, Down down) {
        if (pipelined) {
            int rc = H2_OK;
            pipeline_chunks(ctx, total, up,
                [&](size_t off, size_t len, int slot, hipStream_t st) {
                    int r = run(off, len, slot, st);
                    if (r != H2_OK) rc = r;
                },
                [&](size_t off, size_t len, int slot, hipStream_t st) { down(off, len, slot, ChunkSink(st)); });
            return rc;
        }
        up(0, total, 0, stream);
        H2_TRY(run(0, total, 0, stream));
        down(0, total, 0, ChunkSink(stream));
        H2_HIP(hipStreamSynchronize(stream));
        return H2_OK;
    }
};

// h2_ntt / h2_intt / h2_intt_to / h2_msm_intt: the 2^log_n elements at `src` transformed into `d_a` (buf_a; scratch: buf_b),
// every output times `divisor` when there is one, and written to the result
int host_ntt(HostCall& call, HostResult& res, const Fr* src, Fr* d_a, const uint64_t omega[4], const uint64_t* divisor, uint32_t log_n) {
    Fr* d_t = (Fr*)call.ctx->buf_b.get(sizeof(Fr) << log_n);
    Fr post3[3];
    if (divisor) post3[0] = post3[1] = post3[2] = fr_from_u64x4(divisor);
    H2_TRY(dev_ntt_impl(call.ctx, src, d_a, d_t, 1u << log_n, omega, log_n, nullptr, divisor ? post3 : nullptr, call.stream));
    return res.write(d_a, call.stream);
}
const char* const BAD_LOG_N = "log_n exceeds the 2-adicity of Fr (S = 28)";

}  // namespace

extern "C" {

int h2_version(void) { return 1; }

int h2_device_count(void) { return device_count(); }

const char* h2_last_error(void) { return get_last_error(); }

int h2_synchronize(void) {
    return guarded([&] {
        int n = 0;
        if (hipGetDeviceCount(&n) != hipSuccess) n = 0;
        for (int d = 0; d < n; d++) {
            H2_HIP(hipSetDevice(d));
            H2_HIP(hipDeviceSynchronize());
        }
        return (int)H2_OK;
    });
}

// ------------------------------------------------------------------ device memory / streams for hosts without a HIP binding
int h2_set_device(int device) {
    return guarded([&] {
        H2_HIP(hipSetDevice(device));
        return (int)H2_OK;
    });
}

int h2_dev_alloc(size_t bytes, void** d_out) {
    if (!d_out) return bad("h2_dev_alloc: null argument");
    return guarded([&] {
        *d_out = nullptr;
        if (bytes) H2_HIP(hipMalloc(d_out, bytes));
        return (int)H2_OK;
    });
}

int h2_dev_free(void* d_ptr) {
    return guarded([&] {
        if (d_ptr) H2_HIP(hipFree(d_ptr));
        return (int)H2_OK;
    });
}

int h2_host_alloc_pinned(size_t bytes, void** out) {
    if (!out) return bad("h2_host_alloc_pinned: null argument");
    return guarded([&] {
        *out = nullptr;
        if (bytes) H2_HIP(hipHostMalloc(out, bytes, hipHostMallocDefault));
        return (int)H2_OK;
    });
}

int h2_host_free_pinned(void* ptr) {
    return guarded([&] {
        if (ptr) H2_HIP(hipHostFree(ptr));
        return (int)H2_OK;
    });
}

int h2_stream_create(void** stream_out) {
    if (!stream_out) return bad("h2_stream_create: null argument");
    return guarded([&] {
        hipStream_t s = nullptr;
        H2_HIP(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
        *stream_out = (void*)s;
        return (int)H2_OK;
    });
}

int h2_stream_destroy(void* stream) {
    return guarded([&] {
        if (stream) H2_HIP(hipStreamDestroy((hipStream_t)stream));
        return (int)H2_OK;
    });
}

int h2_stream_synchronize(void* stream) {
    return guarded([&] {
        H2_HIP(hipStreamSynchronize(pick_stream(current_ctx(), stream)));
        return (int)H2_OK;
    });
}

int h2_dev_upload(void* d_dst, const void* src, size_t bytes, void* stream) {
    if (bytes && (!d_dst || !src)) return bad("h2_dev_upload: null argument");
    return guarded([&] {
        if (bytes) host_upload(d_dst, src, bytes, pick_stream(current_ctx(), stream));
        return (int)H2_OK;
    });
}

int h2_dev_download(void* dst, const void* d_src, size_t bytes, void* stream) {
    if (bytes && (!dst || !d_src)) return bad("h2_dev_download: null argument");
    return guarded([&] {
        hipStream_t s = pick_stream(current_ctx(), stream);
        if (bytes) host_download(dst, d_src, bytes, s);
        H2_HIP(hipStreamSynchronize(s));
        return (int)H2_OK;
    });
}

// ------------------------------------------------------------------ library-held device memory
int h2_release_plans(void) {
    return guarded([&] {
        // the calling thread's current device is restored on every way out (a throw from H2_HIP included): later h2_dev_*
        // calls of this thread must not find themselves on another device
        struct RestoreDevice {
            int prev = 0;
            RestoreDevice() { (void)hipGetDevice(&prev); }
            ~RestoreDevice() { (void)hipSetDevice(prev); }
        } restore;
        for (DeviceCtx* ctx : existing_contexts()) {
            H2_HIP(hipSetDevice(ctx->device));
            {
                std::lock_guard<std::mutex> g(ctx->mu);      // coeff_arena is the slot's: no host-slice call of it is running
                ctx->coeff_arena.release();
            }
            ntt_release_idle_plans(ctx);                      // synchronises and frees with no lock held
        }
        return (int)H2_OK;
    });
}

int h2_set_table_budget(size_t bytes) {
    ntt_set_table_budget(bytes);
    return H2_OK;
}

size_t h2_library_memory_bytes(void) {
    size_t total = 0;
    int rc = guarded([&] {
        DeviceCtx* ctx = current_ctx();
        {
            std::lock_guard<std::mutex> g(ctx->mu);
            total = ntt_plan_bytes(ctx) + msm_library_bytes(ctx);          // shared by the host-API slots of the device
        }
        for (DeviceCtx* c : existing_contexts()) {                        // ... plus every slot's own buffers
            if (c->device != ctx->device) continue;
            std::lock_guard<std::mutex> g(c->mu);
            total += c->buf_a.cap + c->buf_b.cap + c->buf_c.cap + c->buf_d.cap + c->msm_scratch.cap + c->evalh_scratch.cap + c->coeff_arena.cap;
        }
        return (int)H2_OK;
    });
    return rc == H2_OK ? total : 0;
}

// ------------------------------------------------------------------ NTT, host buffers
int h2_ntt(uint64_t* a, const uint64_t omega[4], uint32_t log_n) {
    if (!a || !omega) return bad("h2_ntt: null argument");
    if (log_n > 28) return bad(BAD_LOG_N);
    return guarded([&] {
        HostCall call;
        HostResult res(a, (size_t)1 << log_n, {a});
        Fr* d_a = (Fr*)call.upload(call.ctx->buf_a, a, sizeof(Fr) << log_n);
        return host_ntt(call, res, d_a, d_a, omega, nullptr, log_n);
    });
}

int h2_intt(uint64_t* a, const uint64_t omega_inv[4], const uint64_t divisor[4], uint32_t log_n) {
    if (!a || !omega_inv || !divisor) return bad("h2_intt: null argument");
    if (log_n > 28) return bad(BAD_LOG_N);
    return guarded([&] {
        HostCall call;
        HostResult res(a, (size_t)1 << log_n, {a});
        Fr* d_a = (Fr*)call.upload(call.ctx->buf_a, a, sizeof(Fr) << log_n);
        return host_ntt(call, res, d_a, d_a, omega_inv, divisor, log_n);
    });
}

// lagrange_to_coeff of a vector the caller KEEPS (plonk/prover.rs:643-646: `domain.lagrange_to_coeff(advice_values.clone())` per
// column): the values are read where they are, the coefficients written to `out` -- no host copy of the column first
int h2_intt_to(const uint64_t* a, uint64_t* out, const uint64_t omega_inv[4], const uint64_t divisor[4], uint32_t log_n) {
    if (!a || !out || !omega_inv || !divisor) return bad("h2_intt_to: null argument");
    if (log_n > 28) return bad(BAD_LOG_N);
    return guarded([&] {
        HostCall call;
        HostResult res(out, (size_t)1 << log_n, {a});
        Fr* d_a = (Fr*)call.ctx->buf_a.get(sizeof(Fr) << log_n);
        return host_ntt(call, res, call.in(call.ctx->buf_a, a, (size_t)1 << log_n), d_a, omega_inv, divisor, log_n);
    });
}

int h2_coeff_to_extended(const uint64_t* coeffs, uint64_t* out, uint32_t k, uint32_t extended_k,
                         const uint64_t g_coset[4], const uint64_t g_coset_inv[4], const uint64_t extended_omega[4]) {
    if (!coeffs || !out || !g_coset || !g_coset_inv || !extended_omega) return bad("h2_coeff_to_extended: null argument");
    if (extended_k < k) return bad("h2_coeff_to_extended: extended_k < k");
    if (extended_k > 28) return bad(BAD_LOG_N);
    return guarded([&] {
        HostCall call;
        DeviceCtx* ctx = call.ctx;
        HostResult res(out, (size_t)1 << extended_k, {coeffs});
        size_t ext_bytes = sizeof(Fr) << extended_k;
        Fr* d_in = (Fr*)ctx->buf_a.get(ext_bytes);      // (the coefficients are staged at its start)
        Fr* d_t = (Fr*)ctx->buf_b.get(ext_bytes);
        // into_coset = true: coset_powers = [g_coset, g_coset_inv] (domain.rs:383-385)
        Fr pre3[3] = {fr_from_u64x4(g_coset), fr_from_u64x4(g_coset), fr_from_u64x4(g_coset_inv)};
        const Fr* src = call.in(ctx->buf_a, coeffs, (size_t)1 << k);
        H2_TRY(dev_ntt_impl(ctx, src, d_in, d_t, 1u << k, extended_omega, extended_k, pre3, nullptr, call.stream));
        return res.write(d_in, call.stream);
    });
}

int h2_extended_to_coeff(const uint64_t* a, uint64_t* out, size_t out_len, uint32_t extended_k,
                         const uint64_t g_coset[4], const uint64_t g_coset_inv[4],
                         const uint64_t extended_omega_inv[4], const uint64_t extended_ifft_divisor[4]) {
    if (!a || !out || !g_coset || !g_coset_inv || !extended_omega_inv || !extended_ifft_divisor)
        return bad("h2_extended_to_coeff: null argument");
    if (extended_k > 28) return bad(BAD_LOG_N);
    if (out_len > ((size_t)1 << extended_k)) return bad("h2_extended_to_coeff: out_len exceeds the extended domain");
    return guarded([&] {
        HostCall call;
        DeviceCtx* ctx = call.ctx;
        HostResult res(out, out_len, {a});
        size_t ext_bytes = sizeof(Fr) << extended_k;
        Fr* d_a = (Fr*)call.upload(ctx->buf_a, a, ext_bytes);
        Fr* d_t = (Fr*)ctx->buf_b.get(ext_bytes);
        H2_TRY(dev_extended_to_coeff_impl(ctx, d_a, d_t, extended_k, g_coset, g_coset_inv, extended_omega_inv,
                                          extended_ifft_divisor, call.stream));
        return res.write(d_a, call.stream);
    });
}

// ------------------------------------------------------------------ Montgomery conversion
static int host_batch_mont(uint64_t* a, size_t n, bool to_mont) {
    if (!a && n) return bad("h2_batch_mont: null argument");
    return guarded([&] {
        if (n == 0) return (int)H2_OK;
        HostCall call;
        HostResult res(a, n, {a});
        const bool pipe = use_pipeline(n, {a});
        const size_t chunk = pipe ? PIPE_CHUNK : n;
        Fr* slots = (Fr*)call.ctx->buf_a.get((pipe ? 2 * PIPE_CHUNK : n) * sizeof(Fr));
        return call.chunked(n, pipe,
            [&](size_t off, size_t len, int slot, hipStream_t st) { host_upload(slots + slot * chunk, a + 4 * off, len * sizeof(Fr), st); },
            [&](size_t, size_t len, int slot, hipStream_t st) { return batch_mont_launch(slots + slot * chunk, len, to_mont, st); },
            [&](size_t off, size_t len, int slot, const ChunkSink& to) { to(res, off, len, slots + slot * chunk); });
    });
}
int h2_batch_mont(uint64_t* a, size_t n) { return host_batch_mont(a, n, true); }
int h2_batch_unmont(uint64_t* a, size_t n) { return host_batch_mont(a, n, false); }

// ------------------------------------------------------------------ elementwise, host buffers
int h2_eval_op(int op, uint64_t* res, const uint64_t* l, const uint64_t* r, int32_t l_rot, int32_t r_rot, size_t size,
               const uint64_t c[4]) {
    if (!res) return bad("h2_eval_op: null result");
    return guarded([&] {
        if (size == 0) return (int)H2_OK;
        HostCall call;
        DeviceCtx* ctx = call.ctx;
        HostResult out(res, size, {l, r});
        const Fr* res_l = call.resident(l, size);
        const Fr* res_r = call.resident(r, size);
        // no rotation: element i depends on element i of the operands only -- chunk by chunk, both directions of PCIe at once
        const bool pipe = l_rot == 0 && r_rot == 0 &&
                          use_pipeline(size, {res, res_l ? nullptr : (const void*)l, res_r ? nullptr : (const void*)r});
        const size_t chunk = pipe ? PIPE_CHUNK : size, stage_bytes = (pipe ? 2 * PIPE_CHUNK : size) * sizeof(Fr);
        Fr* so = (Fr*)ctx->buf_a.get(stage_bytes);
        Fr* sl = (l && !res_l) ? (Fr*)ctx->buf_b.get(stage_bytes) : nullptr;
        Fr* sr = (r && !res_r) ? (Fr*)ctx->buf_c.get(stage_bytes) : nullptr;
        return call.chunked(size, pipe,
            [&](size_t off, size_t len, int slot, hipStream_t st) {
                if (sl) host_upload(sl + slot * chunk, l + 4 * off, len * sizeof(Fr), st);
                if (sr) host_upload(sr + slot * chunk, r + 4 * off, len * sizeof(Fr), st);
            },
            [&](size_t off, size_t len, int slot, hipStream_t st) {
                const Fr* pl = !l ? nullptr : (res_l ? res_l + off : sl + slot * chunk);
                const Fr* pr = !r ? nullptr : (res_r ? res_r + off : sr + slot * chunk);
                return eval_op_launch(op, so + slot * chunk, pl, pr, l_rot, r_rot, len, c, st);
            },
            [&](size_t off, size_t len, int slot, const ChunkSink& to) { to(out, off, len, so + slot * chunk); });
    });
}

int h2_divide_by_vanishing_poly(uint64_t* a, size_t size, const uint64_t* t_evaluations, size_t t_len) {
    if (!a || !t_evaluations) return bad("h2_divide_by_vanishing_poly: null argument");
    return guarded([&] {
        if (size == 0) return (int)H2_OK;
        HostCall call;
        HostResult res(a, size, {a});
        // a[i] *= t[i % t_len]: a chunk that starts at a multiple of t_len sees the table from its first entry
        const bool pipe = t_len && PIPE_CHUNK % t_len == 0 && use_pipeline(size, {a});
        const size_t chunk = pipe ? PIPE_CHUNK : size;
        Fr* slots = (Fr*)call.ctx->buf_a.get((pipe ? 2 * PIPE_CHUNK : size) * sizeof(Fr));
        const Fr* d_t = (const Fr*)call.upload(call.ctx->buf_b, t_evaluations, t_len * sizeof(Fr));   // (on the stream of every `run`)
        return call.chunked(size, pipe,
            [&](size_t off, size_t len, int slot, hipStream_t st) { host_upload(slots + slot * chunk, a + 4 * off, len * sizeof(Fr), st); },
            [&](size_t, size_t len, int slot, hipStream_t st) { return divide_by_vanishing_launch(slots + slot * chunk, len, d_t, t_len, st); },
            [&](size_t off, size_t len, int slot, const ChunkSink& to) { to(res, off, len, slots + slot * chunk); });
    });
}

// ------------------------------------------------------------------ MSM, host buffers
int h2_msm(const uint64_t* scalars, const uint64_t* bases, size_t n, uint32_t max_bits, uint64_t out_xyz[12]) {
    if (!out_xyz || (n && (!scalars || !bases))) return bad("h2_msm: null argument");
    return guarded([&] {
        if (max_bits == 0 || n == 0) {  // arithmetic.rs:346, :421
            msm_identity(out_xyz);
            return (int)H2_OK;
        }
        HostCall call;
        return msm_host(call.ctx, scalars, bases, n, max_bits, out_xyz);
    });
}

int h2_poly_register(const uint64_t* values, size_t n) {
    if (!values || n == 0) return bad("h2_poly_register: null / empty range");
    return poly_register(values, n);
}

int h2_poly_unregister(const uint64_t* values) {
    if (!values) return bad("h2_poly_unregister: null argument");
    return guarded([&] { return bases_unregister(values); });   // one registry: the device copies are freed the same way
}

int h2_bases_register(const uint64_t* bases, size_t n) {
    if (!bases || n == 0) return bad("h2_bases_register: null / empty range");
    return bases_register(bases, n);
}
int h2_bases_unregister(const uint64_t* bases) {
    if (!bases) return bad("h2_bases_unregister: null");
    return bases_unregister(bases);
}

int h2_g1_sum(const uint64_t* points_xyz, size_t count, uint64_t out_xyz[12]) {
    if (!out_xyz || (count && !points_xyz)) return bad("h2_g1_sum: null argument");
    g1_sum_host(points_xyz, count, out_xyz);
    return H2_OK;
}

int h2_dev_g1_fold(const void* d_points_xyz, uint32_t world, uint32_t count, void* d_out_xyz, void* stream) {
    if (count && (!d_points_xyz || !d_out_xyz)) return bad("h2_dev_g1_fold: null argument");
    return guarded([&] {
        DeviceCtx* ctx = current_ctx();
        return g1_fold_launch((const uint64_t*)d_points_xyz, world, count, (uint64_t*)d_out_xyz, pick_stream(ctx, stream));
    });
}

int h2_msm_multi(const uint64_t* scalars, const uint64_t* bases, size_t n, uint32_t max_bits, uint64_t out_xyz[12]) {
    if (!out_xyz || (n && (!scalars || !bases))) return bad("h2_msm_multi: null argument");
    return guarded([&] {
        if (max_bits == 0 || n == 0) {
            msm_identity(out_xyz);
            return (int)H2_OK;
        }
        return msm_host_multi(scalars, bases, n, max_bits, out_xyz);
    });
}

int h2_msm_intt(uint64_t* scalars, const uint64_t* bases, size_t n, uint32_t max_bits, const uint64_t omega_inv[4],
                const uint64_t divisor[4], uint32_t log_n, uint64_t out_xyz[12]) {
    if (!out_xyz || !scalars || !bases || !omega_inv || !divisor) return bad("h2_msm_intt: null argument");
    if (log_n > 28) return bad(BAD_LOG_N);
    if (n != ((size_t)1 << log_n)) return bad("h2_msm_intt: n != 2^log_n");
    return guarded([&] {
        HostCall call;
        HostResult res(scalars, n, {scalars});
        // one upload of the scalars feeds both the MSM and the iNTT (arithmetic.rs:402-404)
        Fr* d_s = (Fr*)call.upload(call.ctx->buf_a, scalars, n * sizeof(Fr));
        if (max_bits == 0)
            msm_identity(out_xyz);
        else
            H2_TRY(msm_host_resident_scalars(call.ctx, d_s, bases, n, max_bits, out_xyz));
        return host_ntt(call, res, d_s, d_s, omega_inv, divisor, log_n);
    });
}

// ------------------------------------------------------------------ device-resident entry points
int h2_dev_ntt(void* d_a, void* d_tmp, const uint64_t omega[4], uint32_t log_n, void* stream) {
    if (!d_a || !omega) return bad("h2_dev_ntt: null argument");
    return guarded([&] {
        DeviceCtx* ctx = current_ctx();
        return dev_ntt_impl(ctx, (Fr*)d_a, (Fr*)d_a, (Fr*)d_tmp, 1u << log_n, omega, log_n, nullptr, nullptr,
                            pick_stream(ctx, stream));
    });
}

int h2_dev_intt(void* d_a, void* d_tmp, const uint64_t omega_inv[4], const uint64_t divisor[4], uint32_t log_n,
                void* stream) {
    if (!d_a || !omega_inv || !divisor) return bad("h2_dev_intt: null argument");
    return guarded([&] {
        DeviceCtx* ctx = current_ctx();
        Fr d = fr_from_u64x4(divisor);
        Fr post3[3] = {d, d, d};
        return dev_ntt_impl(ctx, (Fr*)d_a, (Fr*)d_a, (Fr*)d_tmp, 1u << log_n, omega_inv, log_n, nullptr, post3,
                            pick_stream(ctx, stream));
    });
}

int h2_dev_coeff_to_extended(const void* d_coeffs, void* d_out, void* d_tmp, uint32_t k, uint32_t extended_k,
                             const uint64_t g_coset[4], const uint64_t g_coset_inv[4],
                             const uint64_t extended_omega[4], void* stream) {
    if (!d_coeffs || !d_out || !g_coset || !g_coset_inv || !extended_omega)
        return bad("h2_dev_coeff_to_extended: null argument");
    if (extended_k < k) return bad("h2_dev_coeff_to_extended: extended_k < k");
    return guarded([&] {
        DeviceCtx* ctx = current_ctx();
        Fr pre3[3] = {fr_from_u64x4(g_coset), fr_from_u64x4(g_coset), fr_from_u64x4(g_coset_inv)};
        if (d_coeffs == d_out && extended_k > 8 && d_tmp == nullptr) return bad("in-place extension needs d_tmp");
        return dev_ntt_impl(ctx, (const Fr*)d_coeffs, (Fr*)d_out, (Fr*)d_tmp, 1u << k, extended_omega, extended_k,
                            pre3, nullptr, pick_stream(ctx, stream));
    });
}

int h2_dev_coset_ntt(const void* d_coeffs, void* d_out, void* d_tmp, uint32_t log_n, const uint64_t g[4],
                     const uint64_t omega[4], void* stream) {
    if (!d_coeffs || !d_out || !g || !omega) return bad("h2_dev_coset_ntt: null argument");
    if (log_n > 28) return bad("log_n exceeds the 2-adicity of Fr (S = 28)");
    return guarded([&] {
        DeviceCtx* ctx = current_ctx();
        hipStream_t s = pick_stream(ctx, stream);
        std::vector<uint32_t> bits;
        ntt_split(log_n, bits);
        if (bits.size() >= 2 && d_tmp == nullptr) return bad("NTT of this size needs a scratch buffer (d_tmp)");
        PlanRef pl = ntt_get_plan(ctx, log_n, omega, s);
        NttTablePin tab = ntt_scale_table(pl.get(), fr_from_u64x4(g), nullptr, s);
        ntt_run(ctx, pl.get(), (const Fr*)d_coeffs, (Fr*)d_out, (Fr*)d_tmp, 1u << log_n, nullptr, nullptr, s, tab.get(), 1u);
        return (int)H2_OK;
    });
}

// Several vectors through one plan, up to 16 per launch: d_tmp = min(count, 16) x 2^log_n Fr, shared by the chunks.
static int dev_ntt_batch_impl(const void* const* srcs, void* const* dsts, size_t count, void* d_tmp, uint32_t log_n,
                              const uint64_t omega[4], const uint64_t* g, const uint64_t* divisor, uint32_t scale_mode,
                              void* stream, const char* what, uint32_t in_log = 0xffffffffu, const Fr* pre3 = nullptr) {
    if (count == 0) return H2_OK;
    if (!srcs || !dsts || !omega) return bad(what);
    if (log_n > 28) return bad("log_n exceeds the 2-adicity of Fr (S = 28)");
    for (size_t i = 0; i < count; i++)
        if (!srcs[i] || !dsts[i]) return bad(what);
    return guarded([&] {
        DeviceCtx* ctx = current_ctx();
        hipStream_t s = pick_stream(ctx, stream);
        std::vector<uint32_t> bits;
        ntt_split(log_n, bits);
        if (bits.size() >= 2 && d_tmp == nullptr) return bad("NTT of this size needs a scratch buffer (d_tmp)");
        PlanRef pl = ntt_get_plan(ctx, log_n, omega, s);
        NttTablePin tab_ref;
        Fr d{};
        Fr post3[3];
        const Fr* post = nullptr;
        if (divisor) d = fr_from_u64x4(divisor);
        if (g) {
            tab_ref = ntt_scale_table(pl.get(), fr_from_u64x4(g), divisor ? &d : nullptr, s);
        } else if (divisor) {
            post3[0] = post3[1] = post3[2] = d;
            post = post3;
        }
        const size_t n = (size_t)1 << log_n;
        std::vector<const Fr*> in(count);
        std::vector<Fr*> out(count), tmp(count);
        for (size_t i = 0; i < count; i++) {
            in[i] = (const Fr*)srcs[i];
            out[i] = (Fr*)dsts[i];
            tmp[i] = d_tmp ? (Fr*)d_tmp + (i % 16) * n : nullptr;
        }
        const uint32_t in_len = in_log == 0xffffffffu ? (uint32_t)n : (1u << in_log);   // shorter: zero-extended (coeff_to_extended)
        const Fr* tab = tab_ref.get();
        ntt_run_many(ctx, pl.get(), in.data(), out.data(), tmp.data(), count, in_len, pre3, post, s, tab,
                     tab ? scale_mode : 0u);
        return (int)H2_OK;
    });
}

int h2_dev_ntt_batch(void* const* d_a, size_t count, void* d_tmp, const uint64_t omega[4], uint32_t log_n, void* stream) {
    return dev_ntt_batch_impl((const void* const*)d_a, d_a, count, d_tmp, log_n, omega, nullptr, nullptr, 0, stream,
                              "h2_dev_ntt_batch: null argument");
}

int h2_dev_intt_batch(void* const* d_a, size_t count, void* d_tmp, const uint64_t omega_inv[4], const uint64_t divisor[4],
                      uint32_t log_n, void* stream) {
    if (!divisor) return bad("h2_dev_intt_batch: null argument");
    return dev_ntt_batch_impl((const void* const*)d_a, d_a, count, d_tmp, log_n, omega_inv, nullptr, divisor, 0, stream,
                              "h2_dev_intt_batch: null argument");
}

int h2_dev_coeff_to_extended_batch(const void* const* d_coeffs, void* const* d_out, size_t count, void* d_tmp, uint32_t k,
                                   uint32_t extended_k, const uint64_t g_coset[4], const uint64_t g_coset_inv[4],
                                   const uint64_t extended_omega[4], void* stream) {
    if (!g_coset || !g_coset_inv) return bad("h2_dev_coeff_to_extended_batch: null argument");
    if (extended_k < k) return bad("h2_dev_coeff_to_extended_batch: extended_k < k");
    const Fr pre3[3] = {fr_from_u64x4(g_coset), fr_from_u64x4(g_coset), fr_from_u64x4(g_coset_inv)};
    return dev_ntt_batch_impl(d_coeffs, d_out, count, d_tmp, extended_k, extended_omega, nullptr, nullptr, 0, stream,
                              "h2_dev_coeff_to_extended_batch: null argument", k, pre3);
}

int h2_dev_coset_ntt_batch(const void* const* d_coeffs, void* const* d_out, size_t count, void* d_tmp, uint32_t log_n,
                           const uint64_t g[4], const uint64_t omega[4], void* stream) {
    if (!g) return bad("h2_dev_coset_ntt_batch: null argument");
    return dev_ntt_batch_impl(d_coeffs, d_out, count, d_tmp, log_n, omega, g, nullptr, 1u, stream,
                              "h2_dev_coset_ntt_batch: null argument");
}

int h2_dev_coset_intt(void* d_a, void* d_tmp, uint32_t log_n, const uint64_t g_inv[4], const uint64_t omega_inv[4],
                      const uint64_t divisor[4], void* stream) {
    if (!d_a || !g_inv || !omega_inv || !divisor) return bad("h2_dev_coset_intt: null argument");
    if (log_n > 28) return bad("log_n exceeds the 2-adicity of Fr (S = 28)");
    return guarded([&] {
        DeviceCtx* ctx = current_ctx();
        hipStream_t s = pick_stream(ctx, stream);
        std::vector<uint32_t> bits;
        ntt_split(log_n, bits);
        if (bits.size() >= 2 && d_tmp == nullptr) return bad("NTT of this size needs a scratch buffer (d_tmp)");
        PlanRef pl = ntt_get_plan(ctx, log_n, omega_inv, s);
        const Fr d = fr_from_u64x4(divisor);
        NttTablePin tab = ntt_scale_table(pl.get(), fr_from_u64x4(g_inv), &d, s);
        ntt_run(ctx, pl.get(), (const Fr*)d_a, (Fr*)d_a, (Fr*)d_tmp, 1u << log_n, nullptr, nullptr, s, tab.get(), 2u);
        return (int)H2_OK;
    });
}

int h2_dev_extended_to_coeff(void* d_a, void* d_tmp, uint32_t extended_k, const uint64_t g_coset[4],
                             const uint64_t g_coset_inv[4], const uint64_t extended_omega_inv[4],
                             const uint64_t extended_ifft_divisor[4], void* stream) {
    if (!d_a || !g_coset || !g_coset_inv || !extended_omega_inv || !extended_ifft_divisor)
        return bad("h2_dev_extended_to_coeff: null argument");
    return guarded([&] {
        DeviceCtx* ctx = current_ctx();
        return dev_extended_to_coeff_impl(ctx, (Fr*)d_a, (Fr*)d_tmp, extended_k, g_coset, g_coset_inv,
                                          extended_omega_inv, extended_ifft_divisor, pick_stream(ctx, stream));
    });
}

size_t h2_msm_scratch_bytes(size_t n, uint32_t max_bits) { return msm_scratch_bytes(n, max_bits); }
size_t h2_msm_batch_scratch_bytes(size_t n, uint32_t max_bits, size_t count) { return msm_batch_scratch_bytes(n, max_bits, count); }
int h2_msm_shape(size_t n, uint32_t max_bits, uint32_t* c, uint32_t* windows, uint32_t* buckets_per_window) {
    msm_shape_query(n, max_bits, c, windows, buckets_per_window);
    return H2_OK;
}

size_t h2_msm_last_launches(h2_msm_launch_info* out, size_t cap) { return msm_last_launches(cap ? out : nullptr, out ? cap : 0); }

int h2_ntt_shape(uint32_t log_n, uint32_t in_log, h2_ntt_pass_shape* out, size_t cap, size_t* count) {
    static_assert(sizeof(h2_ntt_pass_shape) == 7 * sizeof(uint32_t), "h2_ntt_pass_shape is seven words");
    if (!count || (cap && !out)) return bad("h2_ntt_shape: null argument");
    if (log_n > 28 || in_log > log_n) return bad("h2_ntt_shape: log_n <= 28 and in_log <= log_n");
    *count = ntt_shape_query(log_n, in_log, (uint32_t*)out, cap);
    if (*count > cap) return bad("h2_ntt_shape: `cap` is below the number of passes (see *count)");
    return H2_OK;
}

int h2_dev_msm(const void* d_scalars, const void* d_bases, size_t n, uint32_t max_bits, void* d_scratch,
               size_t scratch_bytes, uint64_t out_xyz[12], void* stream) {
    if (!out_xyz || (n && (!d_scalars || !d_bases))) return bad("h2_dev_msm: null argument");
    return guarded([&] {
        DeviceCtx* ctx = current_ctx();
        return msm_device(ctx, (const Fr*)d_scalars, (const uint64_t*)d_bases, n, max_bits, d_scratch, scratch_bytes,
                          out_xyz, pick_stream(ctx, stream));
    });
}

int h2_dev_msm_batch(const void* const* d_scalars, size_t count, const void* d_bases, size_t n, uint32_t max_bits,
                     void* d_scratch, size_t scratch_bytes, uint64_t* out_xyz, void* stream) {
    if (count && (!d_scalars || !out_xyz || (n && !d_bases))) return bad("h2_dev_msm_batch: null argument");
    return guarded([&] {
        DeviceCtx* ctx = current_ctx();
        std::lock_guard<std::mutex> g(ctx->mu);  // uses the context's two internal streams and pinned staging
        return msm_device_batch(ctx, (const Fr* const*)d_scalars, count, (const uint64_t*)d_bases, n, max_bits, d_scratch,
                                scratch_bytes, out_xyz, pick_stream(ctx, stream));
    });
}

int h2_dev_bases_precompute(const void* d_bases, size_t n, uint32_t digits, void* stream) {
    if (n && !d_bases) return bad("h2_dev_bases_precompute: null argument");
    return guarded([&] {
        DeviceCtx* ctx = current_ctx();
        return bases_precompute((const uint64_t*)d_bases, n, digits, pick_stream(ctx, stream));
    });
}
int h2_dev_bases_forget(const void* d_bases) {
    return guarded([&] { return bases_forget((const uint64_t*)d_bases); });
}
size_t h2_dev_bases_precompute_bytes(size_t n, uint32_t digits) { return bases_precompute_bytes(n, digits); }

int h2_dev_random_points(uint64_t seed, size_t n, void* d_out, void* stream) {
    if (!d_out && n) return bad("h2_dev_random_points: null argument");
    return guarded([&] {
        DeviceCtx* ctx = current_ctx();
        return random_points_launch(seed, n, (uint64_t*)d_out, pick_stream(ctx, stream));
    });
}

int h2_dev_msm_batch_ex(const void* const* d_scalars, const void* const* d_bases_each, const uint32_t* max_bits_each,
                        size_t count, size_t n, void* d_scratch, size_t scratch_bytes, uint64_t* out_xyz, void* stream) {
    if (count && (!d_scalars || !d_bases_each || !max_bits_each || !out_xyz)) return bad("h2_dev_msm_batch_ex: null argument");
    return guarded([&] {
        DeviceCtx* ctx = current_ctx();
        std::lock_guard<std::mutex> g(ctx->mu);  // uses the context's two internal streams and pinned staging
        return msm_device_batch_ex(ctx, (const Fr* const*)d_scalars, (const uint64_t* const*)d_bases_each, max_bits_each,
                                   count, nullptr, n, 0, d_scratch, scratch_bytes, out_xyz, pick_stream(ctx, stream));
    });
}

int h2_dev_fixed_base_mul(const void* d_scalars, const void* d_table, size_t n, void* d_points, void* stream) {
    if (n && (!d_scalars || !d_table || !d_points)) return bad("h2_dev_fixed_base_mul: null argument");
    return guarded([&] {
        DeviceCtx* ctx = current_ctx();
        return fixed_base_mul_launch((const Fr*)d_scalars, (const uint64_t*)d_table, n, (uint64_t*)d_points,
                                     pick_stream(ctx, stream));
    });
}

size_t h2_g1_ntt_scratch_bytes(uint32_t log_n) { return g1_ntt_scratch_bytes(log_n); }

int h2_dev_g1_ntt(const void* d_in, void* d_out, uint32_t log_n, int inverse, void* d_scratch, size_t scratch_bytes,
                  void* stream) {
    if (int rc = g1_ntt_args(d_in, d_out, log_n, inverse, d_scratch, scratch_bytes)) return rc;
    return guarded([&] {
        DeviceCtx* ctx = current_ctx();
        return g1_ntt_launch(ctx, (const uint64_t*)d_in, (uint64_t*)d_out, log_n, inverse == 1, d_scratch,
                             pick_stream(ctx, stream));
    });
}

int h2_dev_g1_mul_each(const void* d_points, const void* d_scalars, size_t n, void* d_out, void* stream) {
    if (int rc = g1_mul_each_args(d_points, d_scalars, n, d_out)) return rc;
    if (n == 0) return H2_OK;
    return guarded([&] {
        DeviceCtx* ctx = current_ctx();
        return g1_mul_each_launch((const uint64_t*)d_points, (const Fr*)d_scalars, n, (uint64_t*)d_out,
                                  pick_stream(ctx, stream));
    });
}

int h2_dev_points_decompress(const void* d_bytes, size_t n, void* d_points, void* stream) {
    if (n && (!d_bytes || !d_points)) return bad("h2_dev_points_decompress: null argument");
    return guarded([&] {
        DeviceCtx* ctx = current_ctx();
        std::lock_guard<std::mutex> g(ctx->mu);
        hipStream_t s = pick_stream(ctx, stream);
        uint32_t* d_bad = (uint32_t*)ctx->buf_d.lend(256, s);
        return points_decompress_launch(d_bytes, n, (uint64_t*)d_points, d_bad, s);  // (has waited for `s`: nothing lent is left)
    });
}

int h2_dev_points_compress(const void* d_points, size_t n, void* d_bytes, void* stream) {
    if (n && (!d_bytes || !d_points)) return bad("h2_dev_points_compress: null argument");
    return guarded([&] {
        DeviceCtx* ctx = current_ctx();
        return points_compress_launch((const uint64_t*)d_points, n, d_bytes, pick_stream(ctx, stream));
    });
}

int h2_dev_random_fr(const uint8_t key[32], size_t n, void* d_out, void* stream) {
    if ((!d_out && n) || !key) return bad("h2_dev_random_fr: null argument");
    return guarded([&] {
        DeviceCtx* ctx = current_ctx();
        return random_fr_launch(key, n, (uint64_t*)d_out, pick_stream(ctx, stream));
    });
}

// the same into a host vector (the reference fills its `random_poly` on the host, plonk/vanishing/prover.rs:47-61: a host that
// wants the device's keyed stream in a `Vec` gets it with one copy down)
int h2_random_fr(const uint8_t key[32], size_t n, uint64_t* out) {
    if ((!out && n) || !key) return bad("h2_random_fr: null argument");
    return guarded([&] {
        if (n == 0) return (int)H2_OK;
        HostCall call;
        HostResult res(out, n);
        uint64_t* d = (uint64_t*)call.ctx->buf_a.get(n * sizeof(Fr));
        H2_TRY(random_fr_launch(key, n, d, call.stream));
        return res.write((const Fr*)d, call.stream);
    });
}

int h2_dev_eval_op(int op, void* d_res, const void* d_l, const void* d_r, int32_t l_rot, int32_t r_rot, size_t size,
                   const uint64_t c[4], void* stream) {
    return guarded([&] {
        DeviceCtx* ctx = current_ctx();
        return eval_op_launch(op, (Fr*)d_res, (const Fr*)d_l, (const Fr*)d_r, l_rot, r_rot, size, c,
                              pick_stream(ctx, stream));
    });
}

int h2_dev_divide_by_vanishing_poly(void* d_a, size_t size, const void* d_t, size_t t_len, void* stream) {
    return guarded([&] {
        DeviceCtx* ctx = current_ctx();
        return divide_by_vanishing_launch((Fr*)d_a, size, (const Fr*)d_t, t_len, pick_stream(ctx, stream));
    });
}

int h2_dev_batch_mont(void* d_a, size_t n, void* stream) {
    return guarded([&] {
        DeviceCtx* ctx = current_ctx();
        return batch_mont_launch((Fr*)d_a, n, true, pick_stream(ctx, stream));
    });
}
int h2_dev_max_scalar_bits(const void* const* d_cols, size_t count, size_t n, void* d_words, uint32_t* out_bits,
                           void* stream) {
    return guarded([&] {
        DeviceCtx* ctx = current_ctx();
        if (count && (!d_cols || !d_words || !out_bits)) {
            set_last_error("h2_dev_max_scalar_bits: null argument");
            return (int)H2_ERR_INVALID;
        }
        return max_scalar_bits_launch((const Fr* const*)d_cols, count, n, (uint32_t*)d_words, out_bits,
                                      pick_stream(ctx, stream));
    });
}
int h2_dev_batch_unmont(void* d_a, size_t n, void* stream) {
    return guarded([&] {
        DeviceCtx* ctx = current_ctx();
        return batch_mont_launch((Fr*)d_a, n, false, pick_stream(ctx, stream));
    });
}
int h2_dev_widen_u64(const void* d_src, size_t n, void* d_dst, void* stream) {
    if (n && (!d_src || !d_dst)) return bad("h2_dev_widen_u64: null argument");
    return guarded([&] {
        DeviceCtx* ctx = current_ctx();
        return widen_u64_launch((const uint64_t*)d_src, n, (Fr*)d_dst, pick_stream(ctx, stream));
    });
}

// ------------------------------------------------------------------ adjacent numerics (a24)
int h2_dev_eval_polynomial(const void* d_poly, size_t n, const uint64_t point[4], uint64_t out[4], void* stream) {
    if (!point || !out || (n && !d_poly)) return bad("h2_dev_eval_polynomial: null argument");
    return guarded([&] {
        DeviceCtx* ctx = current_ctx();
        std::lock_guard<std::mutex> g(ctx->mu);
        hipStream_t s = pick_stream(ctx, stream);
        Fr* tmp = (Fr*)ctx->buf_d.lend(eval_polynomial_tmp_elems(n) * sizeof(Fr), s);
        return eval_polynomial_launch((const Fr*)d_poly, n, point, tmp, out, s);  // (has waited for `s`)
    });
}

int h2_dev_eval_polynomial_batch(const void* const* d_polys, size_t count, size_t n, const uint64_t* points, uint64_t* out,
                                 void* stream) {
    if (count && (!d_polys || !points || !out)) return bad("h2_dev_eval_polynomial_batch: null argument");
    return guarded([&] {
        DeviceCtx* ctx = current_ctx();
        std::lock_guard<std::mutex> g(ctx->mu);
        hipStream_t s = pick_stream(ctx, stream);
        Fr* tmp = (Fr*)ctx->buf_d.lend(eval_polynomial_batch_tmp_bytes(count, n), s);
        return eval_polynomial_batch_launch((const Fr* const*)d_polys, count, n, points, tmp, out, s);  // (has waited for `s`)
    });
}

int h2_eval_polynomial(const uint64_t* poly, size_t n, const uint64_t point[4], uint64_t out[4]) {
    if (!point || !out || (n && !poly)) return bad("h2_eval_polynomial: null argument");
    return guarded([&] {
        HostCall call;
        Fr* tmp = (Fr*)call.ctx->buf_d.get(eval_polynomial_tmp_elems(n) * sizeof(Fr));
        const Fr* d = n ? call.in(call.ctx->buf_a, poly, n) : (const Fr*)call.ctx->buf_a.get(sizeof(Fr));
        return eval_polynomial_launch(d, n, point, tmp, out, call.stream);
    });
}

// `count` evaluations, polynomial j at point j, in one call (plonk/prover.rs:700-790 evaluates every committed polynomial at x,
// omega x, ... in a rayon par_iter over eval_polynomial_st): every level of the folds is ONE launch over all of them and the
// values come back in one copy, instead of `count` latency-bound calls.  A polynomial inside a registered range is read on
// the device; one that is not goes up once however many points it is evaluated at.
int h2_eval_polynomial_batch(const uint64_t* const* polys, size_t count, size_t n, const uint64_t* points, uint64_t* out) {
    if (count && (!polys || !points || !out)) return bad("h2_eval_polynomial_batch: null argument");
    for (size_t j = 0; n && j < count; j++)
        if (!polys[j]) return bad("h2_eval_polynomial_batch: null polynomial");
    return guarded([&] {
        if (count == 0) return (int)H2_OK;
        if (n == 0) {
            memset(out, 0, 32 * count);
            return (int)H2_OK;
        }
        HostCall call;
        std::vector<const Fr*> d = call.in_packed(call.ctx->buf_a, polys, count, n);
        Fr* tmp = (Fr*)call.ctx->buf_d.get(eval_polynomial_batch_tmp_bytes(count, n));
        return eval_polynomial_batch_launch(d.data(), count, n, points, tmp, out, call.stream);
    });
}

int h2_dev_batch_invert(void* d_a, void* d_tmp, size_t n, void* stream) {
    if (n && (!d_a || !d_tmp)) return bad("h2_dev_batch_invert: null argument");
    return guarded([&] {
        DeviceCtx* ctx = current_ctx();
        return batch_invert_launch((Fr*)d_a, (Fr*)d_tmp, n, pick_stream(ctx, stream));
    });
}

int h2_batch_invert(uint64_t* a, size_t n) {
    if (n && !a) return bad("h2_batch_invert: null argument");
    return guarded([&] {
        if (n == 0) return (int)H2_OK;
        HostCall call;
        HostResult res(a, n, {a});
        Fr* d = (Fr*)call.upload(call.ctx->buf_a, a, n * sizeof(Fr));
        Fr* t = (Fr*)call.ctx->buf_b.get(n * sizeof(Fr));
        H2_TRY(batch_invert_launch(d, t, n, call.stream));
        return res.write(d, call.stream);
    });
}

int h2_dev_kate_division(const void* d_a, size_t n, const uint64_t b[4], void* d_q, void* stream) {
    if (!b || (n >= 2 && (!d_a || !d_q))) return bad("h2_dev_kate_division: null argument");
    // workgroup B writes q[n-2-j] while workgroup B+1 still reads a[n-1-j']: they meet at one element per block boundary
    if (n >= 2 && fr_ranges_overlap(d_a, n, d_q, n - 1)) return bad("h2_dev_kate_division: a and q must not overlap");
    return guarded([&] {
        DeviceCtx* ctx = current_ctx();
        std::lock_guard<std::mutex> g(ctx->mu);
        // the one borrower of buf_d that returns with its kernels still queued: the next one -- any stream -- waits for them
        hipStream_t s = pick_stream(ctx, stream);
        Fr* tmp = (Fr*)ctx->buf_d.lend(scan_tmp_elems(n) * sizeof(Fr), s);
        H2_TRY(kate_division_launch((const Fr*)d_a, n, b, (Fr*)d_q, tmp, s));
        ctx->buf_d.lent(s);
        return (int)H2_OK;
    });
}

int h2_kate_division(const uint64_t* a, size_t n, const uint64_t b[4], uint64_t* q) {
    if (!b || (n >= 2 && (!a || !q))) return bad("h2_kate_division: null argument");
    return guarded([&] {
        if (n < 2) return (int)H2_OK;
        HostCall call;
        DeviceCtx* ctx = call.ctx;
        HostResult res(q, n - 1, {a});
        Fr* d_q = (Fr*)ctx->buf_b.get(n * sizeof(Fr));
        Fr* tmp = (Fr*)ctx->buf_d.get(scan_tmp_elems(n) * sizeof(Fr));
        H2_TRY(kate_division_launch(call.in(ctx->buf_a, a, n), n, b, d_q, tmp, call.stream));
        return res.write(d_q, call.stream);
    });
}

int h2_dev_prefix_product(const void* d_f, size_t n, const uint64_t init[4], void* d_z, void* stream) {
    if (!init || (n && !d_z) || (n > 1 && !d_f)) return bad("h2_dev_prefix_product: null argument");
    if (n > 1 && fr_ranges_overlap(d_f, n - 1, d_z, n)) return bad("h2_dev_prefix_product: f and z must not overlap");
    return guarded([&] {
        DeviceCtx* ctx = current_ctx();
        std::lock_guard<std::mutex> g(ctx->mu);
        hipStream_t s = pick_stream(ctx, stream);
        Fr* tmp = (Fr*)ctx->buf_d.lend(scan_tmp_elems(n) * sizeof(Fr), s);
        return prefix_product_launch((const Fr*)d_f, n, init, (Fr*)d_z, tmp, s);  // (has waited for `s`)
    });
}

// h2_prefix_product / h2_prefix_sum: z[0] = init, z[i + 1] = z[i] (*|+) f[i] -- n - 1 elements up, one scan, n down
typedef int (*ScanLaunch)(const Fr*, size_t, const uint64_t*, Fr*, Fr*, hipStream_t);
static int host_prefix_scan(ScanLaunch scan, const char* null_msg, const uint64_t* f, size_t n, const uint64_t init[4], uint64_t* z) {
    if (!init || (n && !z) || (n > 1 && !f)) return bad(null_msg);
    return guarded([&] {
        if (n == 0) return (int)H2_OK;
        HostCall call;
        DeviceCtx* ctx = call.ctx;
        HostResult res(z, n, {f});
        Fr* d_f = (Fr*)ctx->buf_a.get(n * sizeof(Fr));
        Fr* d_z = (Fr*)ctx->buf_b.get(n * sizeof(Fr));
        Fr* tmp = (Fr*)ctx->buf_d.get(scan_tmp_elems(n) * sizeof(Fr));
        if (n > 1) host_upload(d_f, f, (n - 1) * sizeof(Fr), call.stream);
        H2_TRY(scan(d_f, n, init, d_z, tmp, call.stream));
        return res.write(d_z, call.stream);
    });
}
int h2_prefix_product(const uint64_t* f, size_t n, const uint64_t init[4], uint64_t* z) {
    return host_prefix_scan(prefix_product_launch, "h2_prefix_product: null argument", f, n, init, z);
}

int h2_dev_lincomb(void* d_res, const void* const* d_polys, const uint64_t* coeffs, size_t count, size_t size,
                   void* stream) {
    if (!d_res || (count && (!d_polys || !coeffs))) return bad("h2_dev_lincomb: null argument");
    return guarded([&] {
        DeviceCtx* ctx = current_ctx();
        return lincomb_launch((Fr*)d_res, (const Fr* const*)d_polys, coeffs, count, size, pick_stream(ctx, stream));
    });
}

// host buffers: every operand crosses PCIe once (count x size x 32 B in, size x 32 B out)
int h2_lincomb(uint64_t* res, const uint64_t* const* polys, const uint64_t* coeffs, size_t count, size_t size) {
    if (!res || (count && (!polys || !coeffs))) return bad("h2_lincomb: null argument");
    for (size_t i = 0; i < count; i++)
        if (!polys[i]) return bad("h2_lincomb: null operand");
    return guarded([&] {
        if (count == 0 || size == 0) {
            memset(res, 0, size * sizeof(Fr));
            return (int)H2_OK;
        }
        HostCall call;
        DeviceCtx* ctx = call.ctx;
        HostResult out(res, size, (const void* const*)polys, count);
        // operands inside a range registered with h2_poly_register are read where they lie on the device; the others cross PCIe
        std::vector<const Fr*> ptrs(count);
        std::vector<size_t> staged;                     // operands that have to be uploaded
        for (size_t i = 0; i < count; i++) {
            ptrs[i] = call.resident(polys[i], size);
            if (!ptrs[i]) staged.push_back(i);
        }
        bool pinned_all = host_pinned(res);
        for (size_t j : staged) pinned_all = pinned_all && host_pinned(polys[j]);
        // chunk by chunk: the operands' chunk c + 1 goes up while chunk c is combined and the result of chunk c - 1 comes down
        const bool pipe = pinned_all && use_pipeline(size, {});
        const size_t chunk = pipe ? PIPE_CHUNK : size, slots = pipe ? 2 : 1, ns = staged.size();
        Fr* sin = ns ? (Fr*)ctx->buf_a.get(slots * ns * chunk * sizeof(Fr)) : nullptr;
        Fr* sout = (Fr*)ctx->buf_b.get(slots * chunk * sizeof(Fr));
        return call.chunked(size, pipe,
            [&](size_t off, size_t len, int slot, hipStream_t st) {
                for (size_t j = 0; j < ns; j++) host_upload(sin + (slot * ns + j) * chunk, polys[staged[j]] + 4 * off, len * sizeof(Fr), st);
            },
            [&](size_t off, size_t len, int slot, hipStream_t st) {
                std::vector<const Fr*> at(count);
                for (size_t i = 0; i < count; i++) at[i] = ptrs[i] ? ptrs[i] + off : nullptr;
                for (size_t j = 0; j < ns; j++) at[staged[j]] = sin + (slot * ns + j) * chunk;
                return lincomb_launch(sout + slot * chunk, at.data(), coeffs, count, len, st);
            },
            [&](size_t off, size_t len, int slot, const ChunkSink& to) { to(out, off, len, sout + slot * chunk); });
    });
}

// The quotient contributions of a multi-point opening in ONE call (poly/multiopen/shplonk/prover.rs:95-153: every rotation set's
// linear combination, minus its low-degree remainder polynomial, divided by the set's vanishing polynomial, the sets folded by
// powers of v; and :205-219 with n_sets = 1: the final quotient l(X) / (X - u)):
//   out = sum_s  (sum_i coeffs[s][i] * polys[s][i](X)  -  low_s(X)) / prod_j (X - points[s][j])
// The caller multiplies v^(R-1-s) into set s's coeffs and low (division is linear: the same field elements).  Operands inside
// a range registered with h2_poly_register are read where they lie on the device, the others go up once; every combination,
// subtraction and synthetic division stays on the device; `out` (n coefficients) comes down once.  `remainders` (optional):
// what each division left, in order -- the value of its dividend at the point (the reference's must_be_zero check, :213-214).
int h2_quotient_sum(uint64_t* out, size_t n, size_t n_sets, const size_t* counts, const uint64_t* const* polys, const uint64_t* coeffs,
                    const size_t* low_counts, const uint64_t* low, const size_t* point_counts, const uint64_t* points,
                    uint64_t* remainders) {
    if (!out || (n_sets && (!counts || !polys || !coeffs || !low_counts || !point_counts))) return bad("h2_quotient_sum: null argument");
    size_t total = 0, total_low = 0, total_points = 0;
    for (size_t s = 0; s < n_sets; s++) {
        total += counts[s];
        total_low += low_counts[s];
        total_points += point_counts[s];
        if (low_counts[s] > n) return bad("h2_quotient_sum: more low coefficients than coefficients");
    }
    if ((total_low && !low) || (total_points && !points)) return bad("h2_quotient_sum: null argument");
    for (size_t i = 0; i < total; i++)
        if (!polys[i]) return bad("h2_quotient_sum: null operand");
    return guarded([&] {
        const size_t bytes = n * sizeof(Fr);
        if (n == 0) return (int)H2_OK;
        if (n_sets == 0) {
            memset(out, 0, bytes);
            return (int)H2_OK;
        }
        HostCall call;
        DeviceCtx* ctx = call.ctx;
        hipStream_t s = call.stream;
        HostResult res(out, n, (const void* const*)polys, total);
        size_t max_staged = 0, max_low = 0;
        {
            size_t at = 0;
            for (size_t set = 0; set < n_sets; set++) {
                size_t st = 0;
                for (size_t i = 0; i < counts[set]; i++)
                    if (!call.resident(polys[at + i], n)) st++;
                max_staged = std::max(max_staged, st);
                max_low = std::max(max_low, low_counts[set]);
                at += counts[set];
            }
        }
        if (max_staged) ctx->buf_a.get(bytes * max_staged);        // (every set's staged operands fit: no set moves the block)
        Fr* cur = (Fr*)ctx->buf_b.get(bytes);
        Fr* nxt = (Fr*)ctx->buf_c.get(bytes);
        // one block: the running sum, the synthetic divisions' scratch, a set's low coefficients
        const size_t tmp_elems = std::max(scan_tmp_elems(n), eval_polynomial_tmp_elems(n));
        Fr* acc = (Fr*)ctx->buf_d.get((n + tmp_elems + max_low) * sizeof(Fr));
        Fr* tmp = acc + n;
        Fr* d_low = tmp + tmp_elems;
        H2_HIP(hipMemsetAsync(acc, 0, bytes, s));
        size_t at = 0, at_low = 0, at_pt = 0;
        for (size_t set = 0; set < n_sets; set++) {
            const size_t count = counts[set];
            if (count) {
                std::vector<const Fr*> ptrs = call.in_packed(ctx->buf_a, polys + at, count, n);
                H2_TRY(lincomb_launch(cur, ptrs.data(), coeffs + 4 * at, count, n, s));
            } else {
                H2_HIP(hipMemsetAsync(cur, 0, bytes, s));
            }
            if (low_counts[set]) {
                host_upload(d_low, low + 4 * at_low, low_counts[set] * sizeof(Fr), s);
                H2_TRY(eval_op_launch(H2_OP_SUB, cur, cur, d_low, 0, 0, low_counts[set], nullptr, s));
            }
            for (size_t j = 0; j < point_counts[set]; j++) {
                const uint64_t* pt = points + 4 * (at_pt + j);
                if (remainders) H2_TRY(eval_polynomial_launch(cur, n, pt, tmp, remainders + 4 * (at_pt + j), s));
                if (n >= 2) H2_TRY(kate_division_launch(cur, n, pt, nxt, tmp, s));      // n - 1 coefficients
                H2_HIP(hipMemsetAsync(nxt + (n - 1), 0, sizeof(Fr), s));    // (resized as shplonk/prover.rs:118)
                std::swap(cur, nxt);
            }
            H2_TRY(eval_op_launch(H2_OP_SUM, acc, acc, cur, 0, 0, n, nullptr, s));
            at += count;
            at_low += low_counts[set];
            at_pt += point_counts[set];
        }
        return res.write(acc, s);
    });
}

int h2_dev_permutation_sigma(void* d_out, const void* d_map_col, const void* d_map_row, size_t n,
                             const uint64_t delta[4], const uint64_t omega[4], void* stream) {
    if (n && (!d_out || !d_map_col || !d_map_row || !delta || !omega)) return bad("h2_dev_permutation_sigma: null argument");
    return guarded([&] {
        DeviceCtx* ctx = current_ctx();
        return perm_sigma_launch((Fr*)d_out, (const uint32_t*)d_map_col, (const uint32_t*)d_map_row, n, delta, omega,
                                 pick_stream(ctx, stream));
    });
}

// host buffers: the reference computes these products in a rayon loop between its GPU calls (permutation/prover.rs:89-128); a
// host that wants them on the device calls this -- value / sigma (sigma: a proving-key column, found on the device when
// registered with h2_poly_register) in, num / den out (first == 0: read, multiplied into, written back), chunk-pipelined
int h2_permutation_terms(uint64_t* num, uint64_t* den, const uint64_t* value, const uint64_t* sigma, size_t n,
                         const uint64_t beta[4], const uint64_t gamma[4], const uint64_t delta_pow[4], const uint64_t omega[4], int first) {
    if (n && (!num || !den || !value || !sigma || !beta || !gamma || !delta_pow || !omega)) return bad("h2_permutation_terms: null argument");
    return guarded([&] {
        if (n == 0) return (int)H2_OK;
        HostCall call;
        DeviceCtx* ctx = call.ctx;
        const Fr* res_sigma = call.resident(sigma, n);
        const Fr* res_value = call.resident(value, n);
        // first == 0: num / den are read, multiplied into and written back -- inputs as well as results
        HostResult r_num(num, n, {first ? nullptr : num}), r_den(den, n, {first ? nullptr : den});
        const bool pipe = use_pipeline(n, {num, den, res_value ? nullptr : (const void*)value, res_sigma ? nullptr : (const void*)sigma});
        const size_t chunk = pipe ? PIPE_CHUNK : n;
        Fr* s_num = (Fr*)ctx->buf_a.get(2 * chunk * sizeof(Fr));
        Fr* s_den = (Fr*)ctx->buf_b.get(2 * chunk * sizeof(Fr));
        Fr* s_val = res_value ? nullptr : (Fr*)ctx->buf_c.get(2 * chunk * sizeof(Fr));
        Fr* s_sig = res_sigma ? nullptr : (Fr*)ctx->buf_d.get(2 * chunk * sizeof(Fr));
        return call.chunked(n, pipe,
            [&](size_t off, size_t len, int slot, hipStream_t st) {
                if (s_val) host_upload(s_val + slot * chunk, value + 4 * off, len * sizeof(Fr), st);
                if (s_sig) host_upload(s_sig + slot * chunk, sigma + 4 * off, len * sizeof(Fr), st);
                if (!first) {
                    host_upload(s_num + slot * chunk, num + 4 * off, len * sizeof(Fr), st);
                    host_upload(s_den + slot * chunk, den + 4 * off, len * sizeof(Fr), st);
                }
            },
            [&](size_t off, size_t len, int slot, hipStream_t st) {
                // rows [off, off + len): the numerator's delta^c omega^i starts at delta_pow * omega^off
                uint64_t dp[4];
                fr_to_u64x4(fp_mul(fr_from_u64x4(delta_pow), fp_pow_u32(fr_from_u64x4(omega), (uint32_t)off)), dp);
                return perm_terms_launch(s_num + slot * chunk, s_den + slot * chunk, res_value ? res_value + off : s_val + slot * chunk,
                                         res_sigma ? res_sigma + off : s_sig + slot * chunk, len, beta, gamma, dp, omega, first, st);
            },
            [&](size_t off, size_t len, int slot, const ChunkSink& to) {
                to(r_num, off, len, s_num + slot * chunk);
                to(r_den, off, len, s_den + slot * chunk);
            });
    });
}

// One grand-product column of the permutation argument in ONE call (permutation/prover.rs:72-165, for one set of columns):
//   z[0] = init;   z[i + 1] = z[i] * prod_j (value_j[i] + beta * delta_pow * delta^j * omega^i + gamma)
//                                   / prod_j (value_j[i] + beta * sigma_j[i] + gamma)
// -- the per-column products, the batch inversion of the denominators, the product with the numerators and the prefix scan
// stay on the device: the columns go up once (those registered with h2_poly_register not at all), z comes down once, instead
// of num / den crossing PCIe in both directions around every step.  The caller writes its blinding rows into z and reads
// z[n - (blinding_factors + 1)] as the next set's init, as the reference does on its vectors.
int h2_permutation_product(uint64_t* z, const uint64_t* const* values, const uint64_t* const* sigmas, size_t count, size_t n,
                           const uint64_t beta[4], const uint64_t gamma[4], const uint64_t delta_pow[4], const uint64_t delta[4],
                           const uint64_t omega[4], const uint64_t init[4]) {
    if (n && (!z || !count || !values || !sigmas || !beta || !gamma || !delta_pow || !delta || !omega || !init))
        return bad("h2_permutation_product: null argument");
    for (size_t j = 0; n && j < count; j++)
        if (!values[j] || !sigmas[j]) return bad("h2_permutation_product: null column");
    return guarded([&] {
        if (n == 0) return (int)H2_OK;
        HostCall call;
        DeviceCtx* ctx = call.ctx;
        hipStream_t s = call.stream;
        std::vector<const void*> inputs(values, values + count);
        inputs.insert(inputs.end(), sigmas, sigmas + count);
        HostResult res(z, n, inputs.data(), inputs.size());
        const size_t bytes = n * sizeof(Fr);
        Fr* num = (Fr*)ctx->buf_a.get(bytes);
        Fr* den = (Fr*)ctx->buf_b.get(bytes);
        // (buf_c / buf_d: a column's staging first, then the scans' scratch)
        Fr* tmp_c = (Fr*)ctx->buf_c.get(std::max(bytes, scan_tmp_elems(n) * sizeof(Fr)));
        Fr* tmp_d = (Fr*)ctx->buf_d.get(std::max(bytes, scan_tmp_elems(n) * sizeof(Fr)));
        Fr dp = fr_from_u64x4(delta_pow);
        const Fr d = fr_from_u64x4(delta);
        for (size_t j = 0; j < count; j++) {
            const Fr* value = call.in(ctx->buf_c, values[j], n);
            const Fr* sigma = call.in(ctx->buf_d, sigmas[j], n);
            uint64_t dpj[4];
            fr_to_u64x4(dp, dpj);
            H2_TRY(perm_terms_launch(num, den, value, sigma, n, beta, gamma, dpj, omega, j == 0, s));
            dp = fp_mul(dp, d);
        }
        H2_TRY(batch_invert_launch(den, tmp_c, n, s));
        H2_TRY(eval_op_launch(H2_OP_MUL, num, num, den, 0, 0, n, nullptr, s));
        H2_TRY(prefix_product_launch(num, n, init, den, tmp_d, s));      // z over the inverted denominators' block
        return res.write(den, s);
    });
}

int h2_dev_permutation_terms(void* d_num, void* d_den, const void* d_value, const void* d_sigma, size_t n,
                             const uint64_t beta[4], const uint64_t gamma[4], const uint64_t delta_pow[4],
                             const uint64_t omega[4], int first, void* stream) {
    if (n && (!d_num || !d_den || !d_value || !d_sigma || !beta || !gamma || !delta_pow || !omega))
        return bad("h2_dev_permutation_terms: null argument");
    return guarded([&] {
        DeviceCtx* ctx = current_ctx();
        return perm_terms_launch((Fr*)d_num, (Fr*)d_den, (const Fr*)d_value, (const Fr*)d_sigma, n, beta, gamma,
                                 delta_pow, omega, first, pick_stream(ctx, stream));
    });
}

int h2_dev_distribute_powers(void* d_a, size_t n, const uint64_t g[4], void* stream) {
    if ((n && !d_a) || !g) return bad("h2_dev_distribute_powers: null argument");
    return guarded([&] {
        DeviceCtx* ctx = current_ctx();
        return distribute_powers_launch((Fr*)d_a, n, g, pick_stream(ctx, stream));
    });
}

int h2_dev_prefix_sum(const void* d_f, size_t n, const uint64_t init[4], void* d_z, void* stream) {
    if (!init || (n && !d_z) || (n > 1 && !d_f)) return bad("h2_dev_prefix_sum: null argument");
    if (n > 1 && fr_ranges_overlap(d_f, n - 1, d_z, n)) return bad("h2_dev_prefix_sum: f and z must not overlap");
    return guarded([&] {
        DeviceCtx* ctx = current_ctx();
        std::lock_guard<std::mutex> g(ctx->mu);
        hipStream_t s = pick_stream(ctx, stream);
        Fr* tmp = (Fr*)ctx->buf_d.lend(scan_tmp_elems(n) * sizeof(Fr), s);
        return prefix_sum_launch((const Fr*)d_f, n, init, (Fr*)d_z, tmp, s);  // (has waited for `s`)
    });
}

size_t h2_logup_scratch_bytes(size_t n) { return logup_scratch_bytes(n); }

// ---- host-vector twins of the remaining steps of a proof with lookups (the reference runs them as host loops: scan
// plonk/logup/prover.rs:353-367, multiplicities :104-180, sigma columns plonk/permutation/keygen.rs:197-238,
// distribute_powers_zeta poly/domain.rs:382-398): a host that keeps its vectors in memory needs no device pointer for any of them
int h2_prefix_sum(const uint64_t* f, size_t n, const uint64_t init[4], uint64_t* z) {
    return host_prefix_scan(prefix_sum_launch, "h2_prefix_sum: null argument", f, n, init, z);
}

// One grand-sum column of a logup lookup in ONE call (plonk/logup/prover.rs:243-347, `commit_z`, for one set of inputs):
//   z[0] = init;   z[i + 1] = z[i] + sum_j 1 / (beta + inputs[j][i])  -  m[i] / (beta + table[i])
// the last term only for the set that carries the table (table != NULL: the first set, :283-290).  The reference makes a
// vector of beta + f per input, batch-inverts it, adds it in, and scans on the host; here every one of those vectors lives on the
// device: the inputs (and table, m) go up once -- registered ones not at all -- and z comes down once.
int h2_logup_grand_sum(uint64_t* z, const uint64_t* const* inputs, size_t count, const uint64_t* table, const uint64_t* m, size_t n,
                       const uint64_t beta[4], const uint64_t init[4]) {
    if (n && (!z || !beta || !init || (count && !inputs) || ((table == nullptr) != (m == nullptr))))
        return bad("h2_logup_grand_sum: null argument");
    for (size_t j = 0; n && j < count; j++)
        if (!inputs[j]) return bad("h2_logup_grand_sum: null input");
    return guarded([&] {
        if (n == 0) return (int)H2_OK;
        HostCall call;
        DeviceCtx* ctx = call.ctx;
        hipStream_t s = call.stream;
        std::vector<const void*> read(inputs, inputs + count);
        read.push_back(table);
        read.push_back(m);
        HostResult res(z, n, read.data(), read.size());
        const size_t bytes = n * sizeof(Fr);
        DevBuf& up = ctx->buf_a;                                   // one operand at a time is staged here
        Fr* term = (Fr*)ctx->buf_b.get(bytes);
        Fr* tmp = (Fr*)ctx->buf_c.get(bytes);
        Fr* acc = (Fr*)ctx->buf_d.get((2 * n + scan_tmp_elems(n)) * sizeof(Fr));
        Fr* d_z = acc + n;
        Fr* scan_tmp = d_z + n;
        H2_HIP(hipMemsetAsync(acc, 0, bytes, s));
        for (size_t j = 0; j < count; j++) {
            H2_TRY(eval_op_launch(H2_OP_SUM_C, term, call.in(up, inputs[j], n), nullptr, 0, 0, n, beta, s));     // beta + f_j
            H2_TRY(batch_invert_launch(term, tmp, n, s));
            H2_TRY(eval_op_launch(H2_OP_SUM, acc, acc, term, 0, 0, n, nullptr, s));
        }
        if (table) {
            H2_TRY(eval_op_launch(H2_OP_SUM_C, term, call.in(up, table, n), nullptr, 0, 0, n, beta, s));         // beta + t
            H2_TRY(batch_invert_launch(term, tmp, n, s));
            H2_TRY(eval_op_launch(H2_OP_MUL, term, term, call.in(up, m, n), 0, 0, n, nullptr, s));               // m / (beta + t)
            H2_TRY(eval_op_launch(H2_OP_SUB, acc, acc, term, 0, 0, n, nullptr, s));
        }
        H2_TRY(prefix_sum_launch(acc, n, init, d_z, scan_tmp, s));
        return res.write(d_z, s);
    });
}

int h2_distribute_powers(uint64_t* a, size_t n, const uint64_t g[4]) {
    if ((n && !a) || !g) return bad("h2_distribute_powers: null argument");
    return guarded([&] {
        if (n == 0) return (int)H2_OK;
        HostCall call;
        HostResult res(a, n, {a});
        Fr* d = (Fr*)call.upload(call.ctx->buf_a, a, n * sizeof(Fr));
        H2_TRY(distribute_powers_launch(d, n, g, call.stream));
        return res.write(d, call.stream);
    });
}

int h2_permutation_sigma(uint64_t* out, const uint32_t* map_col, const uint32_t* map_row, size_t n, const uint64_t delta[4],
                         const uint64_t omega[4]) {
    if (n && (!out || !map_col || !map_row || !delta || !omega)) return bad("h2_permutation_sigma: null argument");
    return guarded([&] {
        if (n == 0) return (int)H2_OK;
        HostCall call;
        HostResult res(out, n, {map_col, map_row});
        Fr* d_out = (Fr*)call.ctx->buf_a.get(n * sizeof(Fr));
        uint32_t* d_col = (uint32_t*)call.ctx->buf_b.get(2 * n * sizeof(uint32_t));
        uint32_t* d_row = d_col + n;
        host_upload(d_col, map_col, n * sizeof(uint32_t), call.stream);
        host_upload(d_row, map_row, n * sizeof(uint32_t), call.stream);
        H2_TRY(perm_sigma_launch(d_out, d_col, d_row, n, delta, omega, call.stream));
        return res.write(d_out, call.stream);
    });
}

// table and inputs: host vectors of n elements (registered ones are read on the device); m: n elements out; *max_bits_out
// (optional): the bit length of the largest multiplicity
int h2_logup_multiplicity(const uint64_t* table, const uint64_t* const* inputs, size_t n_inputs, size_t usable_rows, size_t n,
                          uint64_t* m, uint32_t* max_bits_out) {
    if (n && (!table || !m || (n_inputs && !inputs))) return bad("h2_logup_multiplicity: null argument");
    for (size_t i = 0; n && i < n_inputs; i++)
        if (!inputs[i]) return bad("h2_logup_multiplicity: null input");
    if (usable_rows > n) return bad("h2_logup_multiplicity: usable_rows > n");
    return guarded([&] {
        if (max_bits_out) *max_bits_out = 0;
        if (n == 0) return (int)H2_OK;
        HostCall call;
        DeviceCtx* ctx = call.ctx;
        std::vector<const uint64_t*> hosts(inputs, inputs + n_inputs);   // the inputs, then the table
        hosts.push_back(table);
        HostResult res(m, n, (const void* const*)hosts.data(), hosts.size());
        const size_t sbytes = logup_scratch_bytes(n);
        std::vector<const Fr*> d_in = call.in_packed(ctx->buf_a, hosts.data(), hosts.size(), n, 256);
        Fr* d_m = (Fr*)ctx->buf_b.get(n * sizeof(Fr));
        void* d_scratch = ctx->buf_c.get(sbytes);
        uint32_t max_count = 0;
        H2_TRY(logup_multiplicity_launch(d_in[n_inputs], d_in.data(), n_inputs, usable_rows, n, d_m, d_scratch, sbytes, call.stream, &max_count));
        if (max_bits_out) {
            uint32_t bits = 0;
            while (bits < 32 && (max_count >> bits)) bits++;
            *max_bits_out = bits;
        }
        return res.write(d_m, call.stream);
    });
}


int h2_dev_logup_counts(const void* d_table, const void* const* d_inputs, size_t n_inputs, size_t usable_rows, size_t n,
                        size_t row_begin, size_t row_end, void* d_counts, void* d_scratch, size_t scratch_bytes, void* stream) {
    if (!d_table || !d_counts || !d_scratch || (n_inputs && !d_inputs)) return bad("h2_dev_logup_counts: null argument");
    return guarded([&] {
        DeviceCtx* ctx = current_ctx();
        return logup_counts_launch((const Fr*)d_table, (const Fr* const*)d_inputs, n_inputs, usable_rows, n, row_begin, row_end,
                                   (uint32_t*)d_counts, d_scratch, scratch_bytes, pick_stream(ctx, stream));
    });
}

int h2_dev_logup_emit(const void* d_counts, size_t usable_rows, size_t n, void* d_m, void* stream) {
    if (!d_counts || !d_m) return bad("h2_dev_logup_emit: null argument");
    return guarded([&] {
        DeviceCtx* ctx = current_ctx();
        return logup_emit_launch((const uint32_t*)d_counts, usable_rows, n, (Fr*)d_m, pick_stream(ctx, stream));
    });
}

int h2_dev_logup_multiplicity(const void* d_table, const void* const* d_inputs, size_t n_inputs, size_t usable_rows,
                              size_t n, void* d_m, void* d_scratch, size_t scratch_bytes, void* stream) {
    if (!d_table || !d_m || !d_scratch || (n_inputs && !d_inputs)) return bad("h2_dev_logup_multiplicity: null argument");
    return guarded([&] {
        DeviceCtx* ctx = current_ctx();
        return logup_multiplicity_launch((const Fr*)d_table, (const Fr* const*)d_inputs, n_inputs, usable_rows, n, (Fr*)d_m,
                                         d_scratch, scratch_bytes, pick_stream(ctx, stream));
    });
}

int h2_dev_logup_multiplicity_bits(const void* d_table, const void* const* d_inputs, size_t n_inputs, size_t usable_rows,
                                   size_t n, void* d_m, void* d_scratch, size_t scratch_bytes, uint32_t* max_bits_out,
                                   void* stream) {
    if (!d_table || !d_m || !d_scratch || !max_bits_out || (n_inputs && !d_inputs)) return bad("h2_dev_logup_multiplicity_bits: null argument");
    return guarded([&] {
        DeviceCtx* ctx = current_ctx();
        uint32_t max_count = 0;
        const int rc = logup_multiplicity_launch((const Fr*)d_table, (const Fr* const*)d_inputs, n_inputs, usable_rows, n, (Fr*)d_m,
                                                 d_scratch, scratch_bytes, pick_stream(ctx, stream), &max_count);
        uint32_t bits = 0;
        while (bits < 32 && (max_count >> bits)) bits++;
        *max_bits_out = bits;
        return rc;
    });
}

// ------------------------------------------------------------------ range-check witness completion
size_t h2_range_check_scratch_bytes(const uint64_t* vmin, const uint64_t* vmax, size_t pairs) {
    return range_check_scratch_bytes(vmin, vmax, pairs);
}

int h2_dev_range_check_complete(void* const* d_origins, void* const* d_companions, const uint32_t* origin_forms,
                                const uint32_t* companion_forms, const uint64_t* vmin, const uint64_t* vmax, const uint64_t* step,
                                const uint64_t* first_unassigned, size_t pairs, size_t usable_rows, size_t n, void* d_status,
                                void* d_scratch, size_t scratch_bytes, void* stream) {
    if (const char* what = range_check_validate(d_origins, d_companions, origin_forms, companion_forms, vmin, vmax, step, pairs,
                                                usable_rows, n, d_status, d_scratch, scratch_bytes))
        return bad((std::string("h2_dev_range_check_complete: ") + what).c_str());
    return guarded([&] {
        DeviceCtx* ctx = current_ctx();
        return range_check_complete_launch(d_origins, d_companions, origin_forms, companion_forms, vmin, vmax, step,
                                           first_unassigned, pairs, usable_rows, n, (uint32_t*)d_status, d_scratch,
                                           pick_stream(ctx, stream));
    });
}

// ------------------------------------------------------------------ the circuit front end's device assembly
size_t h2_cells_place_scratch_bytes(size_t count) { return cells_place_scratch_bytes(count); }

int h2_dev_cells_place(const h2_place_segment* segments, size_t count, size_t n, uint32_t out_form, void* d_scratch,
                       size_t scratch_bytes, void* stream) {
    if (const char* what = cells_place_validate(segments, count, n, out_form, d_scratch, scratch_bytes))
        return bad((std::string("h2_dev_cells_place: ") + what).c_str());
    return guarded([&] {
        DeviceCtx* ctx = current_ctx();
        return cells_place_launch(segments, count, n, out_form, d_scratch, pick_stream(ctx, stream));
    });
}

// ------------------------------------------------------------------ selectors: bitmaps and combination columns
size_t h2_selectors_mark_scratch_bytes(size_t count) { return selectors_mark_scratch_bytes(count); }

int h2_dev_selectors_mark(const h2_selector_segment* segments, size_t count, size_t n, size_t num_selectors, void* d_bitmaps,
                          void* d_scratch, size_t scratch_bytes, void* stream) {
    if (const char* what = selectors_mark_validate(segments, count, n, num_selectors, d_bitmaps, d_scratch, scratch_bytes))
        return bad((std::string("h2_dev_selectors_mark: ") + what).c_str());
    return guarded([&] {
        DeviceCtx* ctx = current_ctx();
        return selectors_mark_launch(segments, count, n, (uint32_t*)d_bitmaps, d_scratch, pick_stream(ctx, stream));
    });
}

int h2_dev_selectors_conflicts(const void* d_bitmaps, size_t num_selectors, size_t n, void* d_matrix, void* stream) {
    if (const char* what = selectors_conflicts_validate(d_bitmaps, num_selectors, n, d_matrix))
        return bad((std::string("h2_dev_selectors_conflicts: ") + what).c_str());
    return guarded([&] {
        DeviceCtx* ctx = current_ctx();
        return selectors_conflicts_launch((const uint32_t*)d_bitmaps, num_selectors, n, (uint8_t*)d_matrix,
                                          pick_stream(ctx, stream));
    });
}

int h2_dev_selectors_combine(const h2_selector_column* plan, size_t columns, const h2_selector_member* members,
                             size_t num_members, size_t n, size_t num_selectors, const void* d_bitmaps, uint32_t out_form,
                             void* stream) {
    if (const char* what = selectors_combine_validate(plan, columns, members, num_members, n, num_selectors, d_bitmaps, out_form))
        return bad((std::string("h2_dev_selectors_combine: ") + what).c_str());
    return guarded([&] {
        DeviceCtx* ctx = current_ctx();
        return selectors_combine_launch(plan, columns, members, n, (const uint32_t*)d_bitmaps, pick_stream(ctx, stream));
    });
}

int h2_selectors_combine(const h2_selector_column* plan, size_t columns, const h2_selector_member* members, size_t num_members,
                         size_t n, size_t num_selectors, const void* bitmaps, uint32_t out_form) {
    if (const char* what = selectors_combine_validate(plan, columns, members, num_members, n, num_selectors, bitmaps, out_form))
        return bad((std::string("h2_selectors_combine: ") + what).c_str());
    selectors_combine_host(plan, columns, members, n, (const uint32_t*)bitmaps);
    return H2_OK;
}

// ------------------------------------------------------------------ coverage: the cells each region assigned (coverage.hip)
size_t h2_coverage_scratch_bytes(size_t segments, size_t planes, size_t queries, size_t uses, size_t earlier) {
    return coverage_scratch_bytes(segments, planes, queries, uses, earlier);
}

int h2_dev_coverage_mark(const h2_coverage_plane* planes, size_t num_planes, const h2_coverage_segment* segments, size_t count,
                         void* d_bits, size_t words, void* d_scratch, size_t scratch_bytes, void* stream) {
    if (const char* what = coverage_mark_validate(planes, num_planes, segments, count, d_bits, words, true, d_scratch, scratch_bytes))
        return bad((std::string("h2_dev_coverage_mark: ") + what).c_str());
    return guarded([&] {
        DeviceCtx* ctx = current_ctx();
        return coverage_mark_launch(planes, segments, count, (uint32_t*)d_bits, d_scratch, pick_stream(ctx, stream));
    });
}

int h2_dev_coverage_check(const h2_coverage_plane* planes, size_t num_planes, const h2_coverage_query* queries,
                          size_t num_queries, const h2_coverage_use* uses, size_t num_uses, const uint32_t* earlier,
                          size_t num_earlier, size_t n, const void* d_bits, size_t words, void* d_scratch, size_t scratch_bytes,
                          uint64_t* d_count, h2_check_record* d_records, size_t cap, void* stream) {
    if (const char* what = coverage_check_validate(planes, num_planes, queries, num_queries, uses, num_uses, earlier, num_earlier, n,
                                                   d_bits, words, true, d_scratch, scratch_bytes, d_count, d_records, cap))
        return bad((std::string("h2_dev_coverage_check: ") + what).c_str());
    return guarded([&] {
        DeviceCtx* ctx = current_ctx();
        return coverage_check_launch(planes, num_planes, queries, num_queries, uses, num_uses, earlier, num_earlier, n,
                                     (const uint32_t*)d_bits, d_scratch, d_count, d_records, cap, pick_stream(ctx, stream));
    });
}

int h2_coverage_mark(const h2_coverage_plane* planes, size_t num_planes, const h2_coverage_segment* segments, size_t count,
                     void* bits, size_t words) {
    if (const char* what = coverage_mark_validate(planes, num_planes, segments, count, bits, words, false, nullptr, 0))
        return bad((std::string("h2_coverage_mark: ") + what).c_str());
    coverage_mark_host(planes, segments, count, (uint32_t*)bits);
    return H2_OK;
}

int h2_coverage_check(const h2_coverage_plane* planes, size_t num_planes, const h2_coverage_query* queries, size_t num_queries,
                      const h2_coverage_use* uses, size_t num_uses, const uint32_t* earlier, size_t num_earlier, size_t n,
                      const void* bits, size_t words, uint64_t* count, h2_check_record* records, size_t cap) {
    if (const char* what = coverage_check_validate(planes, num_planes, queries, num_queries, uses, num_uses, earlier, num_earlier, n,
                                                   bits, words, false, nullptr, 0, count, records, cap))
        return bad((std::string("h2_coverage_check: ") + what).c_str());
    coverage_check_host(planes, queries, uses, num_uses, earlier, n, (const uint32_t*)bits, count, records, cap);
    return H2_OK;
}

// ------------------------------------------------------------------ values: witness arithmetic, one fused launch (values.hip)
int h2_values_limits(h2_values_caps* out) {
    if (!out) return bad("h2_values_limits: null argument");
    values_caps(out);
    return H2_OK;
}

int h2_dev_values_eval(const h2_values_leaf* leaves, size_t num_leaves, const uint64_t* constants, size_t num_constants,
                       const h2_values_op* ops, size_t num_ops, const h2_values_output* outputs, size_t num_outputs, size_t m,
                       void* stream) {
    if (m == 0) return H2_OK;
    ValProgram P;
    if (const char* what = values_lower(leaves, num_leaves, constants, num_constants, ops, num_ops, outputs, num_outputs, m, true, &P))
        return bad((std::string("h2_dev_values_eval: ") + what).c_str());
    return guarded([&] {
        DeviceCtx* ctx = current_ctx();
        return values_eval_launch(P, m, pick_stream(ctx, stream));
    });
}

int h2_values_eval(const h2_values_leaf* leaves, size_t num_leaves, const uint64_t* constants, size_t num_constants,
                   const h2_values_op* ops, size_t num_ops, const h2_values_output* outputs, size_t num_outputs, size_t m) {
    if (m == 0) return H2_OK;
    ValProgram P;
    if (const char* what = values_lower(leaves, num_leaves, constants, num_constants, ops, num_ops, outputs, num_outputs, m, false, &P))
        return bad((std::string("h2_values_eval: ") + what).c_str());
    values_eval_host(P, m);
    return H2_OK;
}

// ------------------------------------------------------------------ sorting field elements (sort.hip)
int h2_sort_limits(h2_sort_caps* out) {
    if (!out) return bad("h2_sort_limits: null argument");
    *out = h2_sort_caps{SORT_TILE, SORT_MAX_KEYS, H2_SORT_STATUS_WORDS, 0};
    return H2_OK;
}

size_t h2_sort_scratch_bytes(size_t n, size_t num_keys) {
    const uint32_t forms[SORT_MAX_KEYS] = {}, bits[SORT_MAX_KEYS] = {};
    SortPlan plan;
    return sort_plan(forms, bits, num_keys, n, &plan) ? 0 : plan.total;
}

int h2_dev_sort_permutation(const void* const* d_keys, const uint32_t* forms, const uint32_t* bits, size_t num_keys, size_t n,
                            void* d_perm, uint32_t perm_width, uint32_t* d_status, void* d_scratch, size_t scratch_bytes,
                            void* stream) {
    SortPlan plan;
    if (const char* what = sort_validate(d_keys, forms, bits, num_keys, n, d_perm, perm_width, d_status, true, d_scratch,
                                         scratch_bytes, &plan))
        return bad((std::string("h2_dev_sort_permutation: ") + what).c_str());
    return guarded([&] {
        return sort_permutation_launch(plan, d_keys, d_perm, perm_width, d_status, d_scratch, pick_stream(current_ctx(), stream));
    });
}

int h2_sort_permutation(const void* const* keys, const uint32_t* forms, const uint32_t* bits, size_t num_keys, size_t n,
                        void* perm, uint32_t perm_width, uint32_t* status) {
    SortPlan plan;
    if (const char* what = sort_validate(keys, forms, bits, num_keys, n, perm, perm_width, status, false, nullptr, 0, &plan))
        return bad((std::string("h2_sort_permutation: ") + what).c_str());
    return guarded([&] {
        sort_permutation_host(plan, keys, perm, perm_width, status);
        return (int)H2_OK;
    });
}

// the reference's gpu_sort (arithmetic.rs:167-216): Montgomery residues, in place, ascending by canonical integer
int h2_sort(uint64_t* values, size_t n) {
    if (n && !values) return bad("h2_sort: null argument");
    if (n >> 32) return bad("h2_sort: n is 2^32 or more");
    return guarded([&] {
        if (n < 2) return (int)H2_OK;
        const uint32_t form = H2_ASSIGNED_FORM_MONTGOMERY, bits = 0;
        SortPlan plan;
        if (const char* what = sort_plan(&form, &bits, 1, n, &plan)) return bad((std::string("h2_sort: ") + what).c_str());
        HostCall call;
        HostResult res(values, n, {values});
        const void* d = call.upload(call.ctx->buf_a, values, n * sizeof(Fr));
        // the scratch, then the permutation and the status words behind it
        const size_t perm_at = plan.total, status_at = perm_at + ((n * 4 + 255) & ~(size_t)255);
        char* work = (char*)call.ctx->buf_b.get(status_at + 256);
        Fr* out = (Fr*)call.ctx->buf_c.get(n * sizeof(Fr));
        H2_TRY(sort_permutation_launch(plan, &d, work + perm_at, 4, (uint32_t*)(work + status_at), work, call.stream));
        H2_TRY(sort_gather_launch(d, (const uint32_t*)(work + perm_at), out, n, call.stream));
        return res.write(out, call.stream);
    });
}

// ------------------------------------------------------------------ rational (Assigned) cells
int h2_dev_assigned_resolve(const void* const* d_num, const uint32_t* num_forms, const void* const* d_den,
                            const uint32_t* den_forms, const uint32_t* const* d_rows, const uint64_t* counts,
                            void* const* d_out, size_t cols, size_t n, uint32_t out_form, void* d_status, void* stream) {
    if (const char* what = assigned_validate(d_num, num_forms, d_den, den_forms, d_rows, counts, d_out, cols, n, out_form,
                                             d_status, true))
        return bad((std::string("h2_dev_assigned_resolve: ") + what).c_str());
    return guarded([&] {
        if (cols == 0) return (int)H2_OK;
        hipStream_t s = pick_stream(current_ctx(), stream);
        std::vector<AssignedColumn> c(cols);
        for (size_t i = 0; i < cols; i++) {
            const uint32_t* rows = d_rows ? d_rows[i] : nullptr;
            c[i] = AssignedColumn{d_num[i], d_den[i], rows, d_out[i], (uint32_t*)d_status + i * H2_ASSIGNED_STATUS_WORDS,
                                  rows ? counts[i] : (uint64_t)n, num_forms[i], den_forms[i], 0};
        }
        H2_TRY(assigned_status_init((uint32_t*)d_status, cols, s));
        return assigned_resolve_launch(c.data(), cols, n, out_form, s);
    });
}

// What keygen.rs:276 (`batch_invert_assigned` of the fixed columns) and assign_advice would call: the columns go through the
// staging buffers one after the other, a dense one of page-locked memory chunk by chunk (a chunk of rows is a batch
// inversion of its own); a sparse one in one piece (its rows index the whole column).
int h2_assigned_resolve(const void* const* num, const uint32_t* num_forms, const void* const* den, const uint32_t* den_forms,
                        const uint32_t* const* rows, const uint64_t* counts, void* const* out, size_t cols, size_t n,
                        uint32_t out_form, uint32_t* status) {
    if (const char* what = assigned_validate(num, num_forms, den, den_forms, rows, counts, out, cols, n, out_form, status, false))
        return bad((std::string("h2_assigned_resolve: ") + what).c_str());
    return guarded([&] {
        if (cols == 0) return (int)H2_OK;
        HostCall call;
        DeviceCtx* ctx = call.ctx;
        const size_t status_bytes = cols * H2_ASSIGNED_STATUS_WORDS * sizeof(uint32_t);
        uint32_t* d_status = (uint32_t*)ctx->buf_d.get(status_bytes);
        H2_TRY(assigned_status_init(d_status, cols, call.stream));
        for (size_t i = 0; i < cols; i++) {
            const uint32_t* r = rows ? rows[i] : nullptr;
            const size_t m = r ? (size_t)counts[i] : n;
            const size_t ncell = num_forms[i] == H2_ASSIGNED_FORM_COMPACT ? 8 : 32, dcell = den_forms[i] == H2_ASSIGNED_FORM_COMPACT ? 8 : 32;
            HostResult res((uint64_t*)out[i], n, {num[i], den[i]});
            const bool pipe = !r && use_pipeline(n, {num[i], den[i], out[i]});
            const size_t chunk = pipe ? PIPE_CHUNK : n, slots = pipe ? 2 : 1;
            const size_t den_bytes = (std::min(chunk, m) * dcell + 15) & ~(size_t)15;        // (the rows follow the denominators)
            char* d_num = (char*)ctx->buf_a.get(slots * chunk * ncell);
            char* d_den = (char*)ctx->buf_b.get(slots * den_bytes + (r ? m * sizeof(uint32_t) : 0) + 16);
            Fr* d_out = (Fr*)ctx->buf_c.get(slots * chunk * sizeof(Fr));
            uint32_t* d_rows = r ? (uint32_t*)(d_den + den_bytes) : nullptr;
            H2_TRY(call.chunked(n, pipe,
                [&](size_t off, size_t len, int slot, hipStream_t st) {
                    host_upload(d_num + slot * chunk * ncell, (const char*)num[i] + off * ncell, len * ncell, st);
                    if (r) {
                        if (m) host_upload(d_den, den[i], m * dcell, st);
                        if (m) host_upload(d_rows, r, m * sizeof(uint32_t), st);
                    } else {
                        host_upload(d_den + slot * den_bytes, (const char*)den[i] + off * dcell, len * dcell, st);
                    }
                },
                [&](size_t off, size_t len, int slot, hipStream_t st) {
                    const AssignedColumn c{d_num + slot * chunk * ncell, d_den + slot * den_bytes, d_rows, d_out + slot * chunk,
                                           d_status + i * H2_ASSIGNED_STATUS_WORDS, (uint64_t)(r ? m : len), num_forms[i], den_forms[i],
                                           (uint32_t)off};
                    return assigned_resolve_launch(&c, 1, len, out_form, st);
                },
                [&](size_t off, size_t len, int slot, const ChunkSink& to) { to(res, off, len, d_out + slot * chunk); }));
        }
        host_download(status, d_status, status_bytes, call.stream);
        H2_HIP(hipStreamSynchronize(call.stream));
        return (int)H2_OK;
    });
}

// ------------------------------------------------------------------ the copy constraints' cycle mapping
size_t h2_permutation_mapping_scratch_bytes(size_t n_columns, size_t n, size_t copies) {
    return permutation_mapping_scratch_bytes(n_columns, n, copies);
}

int h2_dev_permutation_mapping_phases(const uint32_t* d_copies, size_t copies, size_t n_columns, size_t n, uint32_t* d_map_col,
                                      uint32_t* d_map_row, uint32_t* d_status, void* d_scratch, size_t scratch_bytes,
                                      float* phase_ms, void* stream) {
    if (const char* what = permutation_mapping_validate(d_copies, copies, n_columns, n, d_map_col, d_map_row, d_status, d_scratch,
                                                        scratch_bytes))
        return bad((std::string("h2_dev_permutation_mapping: ") + what).c_str());
    return guarded([&] {
        DeviceCtx* ctx = current_ctx();
        return permutation_mapping_launch(d_copies, copies, n_columns, n, d_map_col, d_map_row, d_status, d_scratch, phase_ms,
                                          pick_stream(ctx, stream));
    });
}

int h2_dev_permutation_mapping(const uint32_t* d_copies, size_t copies, size_t n_columns, size_t n, uint32_t* d_map_col,
                               uint32_t* d_map_row, uint32_t* d_status, void* d_scratch, size_t scratch_bytes, void* stream) {
    return h2_dev_permutation_mapping_phases(d_copies, copies, n_columns, n, d_map_col, d_map_row, d_status, d_scratch,
                                             scratch_bytes, nullptr, stream);
}

// ------------------------------------------------------------------ evaluate_h: the generated form
int h2_evalh_prepare(const h2_evalh_desc* desc, h2_evalh_info* info) {
    if (!desc) return bad("h2_evalh_prepare: null argument");
    return guarded([&] {
        current_ctx();  // the device of this thread is initialised
        int cached = 0;
        std::string why;
        EvalhPlanRef held = evalh_plan_get(desc, &cached, &why);
        const EvalhPlan* plan = held.get();
        // (an error, not an info without stages: a caller that prepares at keygen time wants to hear that this circuit will run on the
        //  interpreter kernels, and why -- evaluate_h itself goes on, with one warning)
        if (!plan && !why.empty()) return bad(("h2_evalh_prepare: no generated kernels for this program: " + why).c_str());
        if (!plan) return bad("h2_evalh_prepare: no generated kernels for this program (H2_EVALH_JIT=0)");
        if (info) {
            evalh_plan_info(plan, info);
            info->from_cache = (uint32_t)cached;
        }
        return (int)H2_OK;
    });
}

int h2_evalh_compile(const h2_evalh_desc* desc, h2_evalh_info* info) {
    if (!desc) return bad("h2_evalh_compile: null argument");
    return guarded([&] {
        evgen::Generated g = evgen::compile(desc, evgen::Options::from_env());
        if (info) evalh_gen_info(g, info);
        return (int)H2_OK;
    });
}

int h2_evalh_source(const h2_evalh_desc* desc, uint32_t stage, char* buf, size_t cap, size_t* len) {
    if (!desc || !len || (cap && !buf)) return bad("h2_evalh_source: null argument");
    return guarded([&] {
        evgen::Generated g = evgen::generate(desc, evgen::Options::from_env());
        if (stage >= g.stages.size()) return bad("h2_evalh_source: no such stage");
        const std::string& src = g.stages[stage].source;
        *len = src.size();
        if (cap) {
            const size_t n = std::min(cap - 1, src.size());
            memcpy(buf, src.data(), n);
            buf[n] = 0;
        }
        return (int)H2_OK;
    });
}

int h2_evalh_stage_args(const h2_evalh_desc* desc, uint32_t stage, uint64_t* values, const uint64_t* tw_lo, const uint64_t* tw_hi,
                        uint64_t row_begin, uint64_t row_end, void* buf, size_t cap, size_t* len) {
    if (!desc || !len || (cap && !buf)) return bad("h2_evalh_stage_args: null argument");
    return guarded([&] {
        if (desc->extended_k < desc->k || desc->extended_k > 28) return bad("h2_evalh_stage_args: bad k / extended_k");
        evgen::Generated g = evgen::generate(desc, evgen::Options::from_env());
        if (stage >= g.stages.size()) return bad("h2_evalh_stage_args: no such stage");
        alignas(16) unsigned char tmp[4096];  // (pointers, u64 and Fr values are stored into it)
        *len = evalh_fill_stage_args(g.stages[stage], desc, (Fr*)values, (const Fr*)tw_lo, (const Fr*)tw_hi, (size_t)row_begin,
                                     (size_t)row_end, tmp, sizeof tmp);
        if (cap) {
            if (cap < *len) return bad("h2_evalh_stage_args: buffer too small");
            memcpy(buf, tmp, *len);
        }
        return (int)H2_OK;
    });
}

uint64_t h2_evalh_generated_launches(void) { return evalh_generated_launches(); }

// ------------------------------------------------------------------ evaluate_h
// (the copy back is inside evalh_host / evalh_host_coeffs: the prefault of `values` starts once the descriptor is known to be
// sound, runs under the wait for a slot, and is joined just before that call)
int h2_evaluate_h(const h2_evalh_desc* desc, uint64_t* values) {
    if (!desc || !values) return bad("h2_evaluate_h: null argument");
    if (const char* msg = evalh_validate(desc, "h2_evaluate_h", EVALH_HOST_EXTENDED)) return bad(msg);
    return guarded([&] {
        HostResult res(values, (size_t)1 << desc->extended_k);
        HostCall call;
        return evalh_host(call.ctx, desc, res.handed_over());
    });
}

int h2_evaluate_h_coeff(const h2_evalh_desc* desc, uint64_t* values) {
    if (!desc || !values) return bad("h2_evaluate_h_coeff: null argument");
    if (const char* msg = evalh_validate(desc, "h2_evaluate_h_coeff", EVALH_HOST_COEFF)) return bad(msg);
    return guarded([&] {
        HostResult res(values, (size_t)1 << desc->extended_k);
        return evalh_host_coeffs(desc, res.handed_over());      // (leases its devices itself)
    });
}

// The vanishing argument's quotient, from coefficient forms to coefficient form, in ONE call: what the reference's cuda path does
// in three steps on host vectors of 2^extended_k elements -- Evaluator::evaluate_h (plonk/evaluation.rs:1229-1985), then
// divide_by_vanishing_poly (poly/domain.rs:354-373) and extended_to_coeff (:328-350) in vanishing::Argument::construct
// (plonk/vanishing/prover.rs:69-112).  The 2^extended_k values of the numerator stay on the device: divided there, taken back
// to coefficients there, and only the out_len = n * quotient_poly_degree coefficients of h(X) cross PCIe (k = 22, degree 4:
// 384 MiB down instead of 512 MiB down + up + down + up + 384 MiB down, and two 512 MiB host vectors that never exist).
// With several devices in the pool the cosets are dealt over them as h2_evaluate_h_coeff does and the two other steps follow
// through a host vector of the call's own.
int h2_quotient_poly_coeff(const h2_evalh_desc* desc, const uint64_t* t_evaluations, size_t t_len, const uint64_t g_coset[4],
                           const uint64_t g_coset_inv[4], const uint64_t extended_omega_inv[4],
                           const uint64_t extended_ifft_divisor[4], uint64_t* out, size_t out_len) {
    if (!desc || !t_evaluations || !t_len || !g_coset || !g_coset_inv || !extended_omega_inv || !extended_ifft_divisor || !out)
        return bad("h2_quotient_poly_coeff: null argument");
    if (const char* msg = evalh_validate(desc, "h2_quotient_poly_coeff", EVALH_HOST_COEFF)) return bad(msg);
    const size_t size = (size_t)1 << desc->extended_k;
    if (out_len > size) return bad("h2_quotient_poly_coeff: out_len exceeds the extended domain");
    if (size % t_len) return bad("h2_quotient_poly_coeff: t_len does not divide the extended domain");
    return guarded([&] {
        const uint32_t ek = desc->extended_k;
        if (evalh_host_workers(desc) <= 1) {
            // under the evaluation's own lease, on its stream
            HostResult res(out, out_len);
            EvalhFinish finish = [&](DeviceCtx* ctx, Fr* d_values, hipStream_t s) -> int {
                Fr* d_t = (Fr*)ctx->buf_c.get(t_len * sizeof(Fr));
                host_upload(d_t, t_evaluations, t_len * sizeof(Fr), s);
                H2_TRY(divide_by_vanishing_launch(d_values, size, d_t, t_len, s));
                Fr* d_tmp = (Fr*)ctx->buf_b.get(size * sizeof(Fr));
                H2_TRY(dev_extended_to_coeff_impl(ctx, d_values, d_tmp, ek, g_coset, g_coset_inv, extended_omega_inv, extended_ifft_divisor, s));
                return res.write(d_values, s);
            };
            bool finished = false;
            int rc = evalh_host_coeffs(desc, nullptr, &finish, &finished);
            if (rc == H2_OK && !finished) return bad("h2_quotient_poly_coeff: the evaluation did not hand its values over");
            return rc;
        }
        // (no result of this call's own here: h2_extended_to_coeff declares `out` as its result)
        std::vector<uint64_t> values(4 * size);
        H2_TRY(evalh_host_coeffs(desc, values.data()));
        H2_TRY(h2_divide_by_vanishing_poly(values.data(), size, t_evaluations, t_len));
        return h2_extended_to_coeff(values.data(), out, out_len, ek, g_coset, g_coset_inv, extended_omega_inv, extended_ifft_divisor);
    });
}

int h2_dev_evaluate_h(const h2_evalh_desc* desc, void* d_values, void* stream) {
    if (!desc || !d_values) return bad("h2_dev_evaluate_h: null argument");
    return guarded([&] {
        DeviceCtx* ctx = current_ctx();
        std::lock_guard<std::mutex> g(ctx->mu);  // the interpreter work space is per device
        return evalh_device(ctx, desc, (Fr*)d_values, pick_stream(ctx, stream));
    });
}

// ------------------------------------------------------------------ witness checks (check.hip)
size_t h2_check_scratch_bytes(size_t n) { return check_scratch_bytes(n); }

static bool check_out_ok(const uint64_t* d_count, const h2_check_record* d_records, size_t cap, uint32_t circuit) {
    return d_count && (d_records || cap == 0) && circuit < (1u << 24);
}

int h2_dev_check_nonzero_rows(const void* d_values, size_t usable_rows, uint32_t* d_rows, uint64_t* d_row_count, void* stream) {
    if (!d_values || !d_rows || !d_row_count) return bad("h2_dev_check_nonzero_rows: null argument");
    if (usable_rows >= 0x7fffffffu) return bad("h2_dev_check_nonzero_rows: bad sizes");
    return guarded([&] {
        DeviceCtx* ctx = current_ctx();
        return check_nonzero_rows_launch((const Fr*)d_values, usable_rows, d_rows, d_row_count, pick_stream(ctx, stream));
    });
}

int h2_dev_check_gates(const h2_evalh_desc* desc, const uint32_t* d_rows, const uint64_t* d_row_count, uint32_t circuit,
                       uint64_t* d_count, h2_check_record* d_records, size_t cap, void* stream) {
    if (!desc || !d_rows || !d_row_count || !check_out_ok(d_count, d_records, cap, circuit))
        return bad("h2_dev_check_gates: null argument");
    if (int rc = check_gates_args(desc)) return rc;
    return guarded([&] {
        DeviceCtx* ctx = current_ctx();
        return check_gates_launch(ctx, desc, d_rows, d_row_count, circuit, d_count, d_records, cap, pick_stream(ctx, stream));
    });
}

int h2_dev_check_lookup(const void* d_table, const void* const* d_inputs, const uint32_t* tags, size_t n_inputs,
                        size_t usable_rows, size_t n, uint32_t lookup_index, uint32_t circuit, void* d_scratch,
                        size_t scratch_bytes, uint64_t* d_count, h2_check_record* d_records, size_t cap, void* stream) {
    if (!d_table || !d_scratch || (n_inputs && (!d_inputs || !tags)) || !check_out_ok(d_count, d_records, cap, circuit))
        return bad("h2_dev_check_lookup: null argument");
    for (size_t j = 0; j < n_inputs; j++)
        if (!d_inputs[j]) return bad("h2_dev_check_lookup: null input");
    if (int rc = check_columns_args("h2_dev_check_lookup", usable_rows, n, scratch_bytes)) return rc;
    return guarded([&] {
        DeviceCtx* ctx = current_ctx();
        return check_lookup_launch((const Fr*)d_table, (const Fr* const*)d_inputs, tags, n_inputs, usable_rows, n, lookup_index,
                                   circuit, d_scratch, scratch_bytes, d_count, d_records, cap, pick_stream(ctx, stream));
    });
}

int h2_dev_check_shuffle(const void* d_input, const void* d_shuffle, size_t usable_rows, size_t n, uint32_t group, uint32_t unit,
                         uint32_t circuit, void* d_scratch, size_t scratch_bytes, uint64_t* d_count, h2_check_record* d_records,
                         size_t cap, void* stream) {
    if (!d_input || !d_shuffle || !d_scratch || !check_out_ok(d_count, d_records, cap, circuit))
        return bad("h2_dev_check_shuffle: null argument");
    if (int rc = check_columns_args("h2_dev_check_shuffle", usable_rows, n, scratch_bytes)) return rc;
    return guarded([&] {
        DeviceCtx* ctx = current_ctx();
        return check_shuffle_launch((const Fr*)d_input, (const Fr*)d_shuffle, usable_rows, n, group, unit, circuit, d_scratch,
                                    scratch_bytes, d_count, d_records, cap, pick_stream(ctx, stream));
    });
}

int h2_dev_check_copies(const void* const* d_columns, size_t n_columns, const uint32_t* d_map_col, const uint32_t* d_map_row,
                        size_t n, uint32_t circuit, uint64_t* d_count, h2_check_record* d_records, size_t cap, void* stream) {
    if ((n_columns && (!d_columns || !d_map_col || !d_map_row)) || !check_out_ok(d_count, d_records, cap, circuit))
        return bad("h2_dev_check_copies: null argument");
    if (int rc = check_copies_args(n_columns, n)) return rc;
    return guarded([&] {
        DeviceCtx* ctx = current_ctx();
        return check_copies_launch((const Fr* const*)d_columns, n_columns, d_map_col, d_map_row, n, circuit, d_count, d_records, cap,
                                   pick_stream(ctx, stream));
    });
}

// ------------------------------------------------------------------ SRS point screening (srscheck.hip)
int h2_dev_g1_check_points(const void* d_points, size_t n, uint32_t table, uint32_t flags, uint64_t* d_count,
                           h2_check_record* d_records, size_t cap, void* stream) {
    if (int rc = g1_check_points_args(d_points, n, flags, d_count, d_records, cap)) return rc;
    return guarded([&] {
        DeviceCtx* ctx = current_ctx();
        return g1_check_points_launch(d_points, n, table, flags, d_count, d_records, cap, pick_stream(ctx, stream));
    });
}

// ------------------------------------------------------------------ HIP-event timer for bench.py
namespace {
std::mutex g_timer_mu;
std::map<void*, std::pair<hipEvent_t, hipEvent_t>> g_timers;
}  // namespace

int h2_timer_start(void* stream) {
    return guarded([&] {
        DeviceCtx* ctx = current_ctx();
        hipStream_t s = pick_stream(ctx, stream);
        std::lock_guard<std::mutex> g(g_timer_mu);
        auto& t = g_timers[(void*)s];
        if (!t.first) {
            H2_HIP(hipEventCreate(&t.first));
            H2_HIP(hipEventCreate(&t.second));
        }
        H2_HIP(hipEventRecord(t.first, s));
        return (int)H2_OK;
    });
}

int h2_timer_stop(void* stream, float* ms_out) {
    if (!ms_out) return bad("h2_timer_stop: null argument");
    return guarded([&] {
        DeviceCtx* ctx = current_ctx();
        hipStream_t s = pick_stream(ctx, stream);
        std::lock_guard<std::mutex> g(g_timer_mu);
        auto it = g_timers.find((void*)s);
        if (it == g_timers.end()) return bad("h2_timer_stop without h2_timer_start");
        H2_HIP(hipEventRecord(it->second.second, s));
        H2_HIP(hipEventSynchronize(it->second.second));
        H2_HIP(hipEventElapsedTime(ms_out, it->second.first, it->second.second));
        return (int)H2_OK;
    });
}

}  // extern "C"
