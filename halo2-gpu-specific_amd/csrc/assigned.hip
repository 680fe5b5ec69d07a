// assigned.hip -- the rational cells of a witness or of a fixed column (`Assigned<F>`, plonk/assigned.rs) resolved to field
// elements: out[r] = num[r] * den[r]^-1, and 0 where den[r] = 0 (`Assigned::evaluate`; poly::batch_invert_assigned,
// poly.rs:148-173, keeps zeros as they are, so the cell is num * 0).  ONE launch resolves every column of a call
// (blockIdx.y = column) by Montgomery's trick: one strided chain per lane and one field inversion per workgroup, exactly
// as k_batch_invert (the workgroup step is shared: batchinv.hpp).
// No scratch: the forward pass leaves the running prefix of a lane's chain in `out`, the backward pass replaces it by
// inv * prefix * num -- so `out` overlaps neither `num` nor `den` (refused on the host).
// Forms.  num and den are canonical 32-byte, Montgomery 32-byte or compact 8-byte cells, out canonical or Montgomery, and
// nothing is converted cell by cell: the Montgomery product of RAW words x y / R is exact algebra whatever the words stand
// for.  With den = d R^a, num = u R^b (a, b = 1 for Montgomery cells, else 0) the chain and the shared inversion give
// R^(2-a) / d per cell, the product with num gives (u / d) R^(1-a+b), and the result is wanted as (u / d) R^c: the missing
// R^(c+a-b-1) -- between R^-2 and R -- is multiplied into each LANE's inverse once, before its backward pass.  4 products
// per cell in every combination of forms.  (As everywhere in the library, 32-byte cells hold reduced values.)
// Sparse columns (`rows`): only the listed rows have a denominator -- the reference's `Option<F>` -- and only they cross
// PCIe; the other rows are num in the output form, written first by the widen / copy / conversion kernels on the same
// stream.  The chain then runs over the listed rows; an index that is not below n or not above its predecessor is
// reported (BAD_ROWS, the first such index) and never written through.
#include <cstring>

#include "assigned.hpp"
#include "batchinv.hpp"
#include "poly.hpp"

namespace h2 {

namespace {

constexpr uint32_t ASG_MONTGOMERY = H2_ASSIGNED_FORM_MONTGOMERY, ASG_COMPACT = H2_ASSIGNED_FORM_COMPACT;
constexpr uint32_t ASG_NONE = 0xffffffffu;
constexpr int ASG_COLS_PER_LAUNCH = 32;      // 56 bytes of kernel arguments each
// status words
constexpr int ST_CODE = 0, ST_ZEROS = 1, ST_FIRST_ZERO = 2, ST_FIRST_BAD = 3;

struct AsgCol {
    const void* num;
    const void* den;
    const uint32_t* rows;
    void* out;
    uint32_t* status;
    uint32_t count, nform, dform, row_base;
};
struct AsgArgs {
    AsgCol c[ASG_COLS_PER_LAUNCH];
    uint32_t n, oform;
};

// the raw words of cell i
__device__ __forceinline__ Fr asg_load(const void* col, uint32_t form, size_t i) {
    if (form == ASG_COMPACT) {
        const uint64_t x = ((const uint64_t*)col)[i];
        Fr v = fp_zero<FrParams>();
        v.l[0] = (uint32_t)x;
        v.l[1] = (uint32_t)(x >> 32);
        return v;
    }
    return fp_load((const Fr*)col + i);
}

// the row of element j of a column's chain; false: rows[j] is not a row of the column, or does not ascend
__device__ __forceinline__ bool asg_row(const AsgCol& c, uint32_t n, size_t j, uint32_t& r) {
    if (!c.rows) {
        r = (uint32_t)j;
        return true;
    }
    r = c.rows[j];
    return r < n && (j == 0 || r > c.rows[j - 1]);
}

__global__ void __launch_bounds__(256) k_assigned_status_init(uint32_t* status, uint32_t words) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i < words) status[i] = (i % H2_ASSIGNED_STATUS_WORDS) < ST_FIRST_ZERO ? 0u : ASG_NONE;
}

__global__ void __launch_bounds__(256) k_assigned_resolve(AsgArgs a) {
    __shared__ uint4 sh_lo[256], sh_hi[256];
    const AsgCol& c = a.c[blockIdx.y];
    const size_t count = c.count;
    const size_t nthreads = batch_invert_threads(count);
    // (the grid is sized for the longest chain set of the launch; the same for every lane of the workgroup)
    if ((size_t)blockIdx.x * 256 >= nthreads) return;
    const uint32_t tid = threadIdx.x, n = a.n;
    const size_t t = (size_t)blockIdx.x * 256 + tid;
    const bool active = t < nthreads;      // nthreads <= count: an active lane has at least one element
    Fr* out = (Fr*)c.out;
    Fr acc = fp_one<FrParams>();
    size_t last = t;
    uint32_t zeros = 0, first_zero = ASG_NONE, first_bad = ASG_NONE;
    if (active) {
        for (size_t j = t; j < count; j += nthreads) {
            last = j;
            uint32_t r;
            if (!asg_row(c, n, j, r)) {
                if (first_bad == ASG_NONE) first_bad = (uint32_t)j;
                continue;
            }
            const Fr v = asg_load(c.den, c.dform, j);
            fp_store(out + r, acc);
            if (fp_is_zero(v)) {          // never enters the product
                zeros++;
                if (first_zero == ASG_NONE) first_zero = r;
            } else {
                acc = fp_mul(acc, v);
            }
        }
    }
    // what the lanes found, one atomic of each kind per wave (whole waves are here: nobody has left yet)
#pragma unroll
    for (int off = 32; off; off >>= 1) {
        zeros += (uint32_t)__shfl_xor((int)zeros, off, 64);
        const uint32_t z = (uint32_t)__shfl_xor((int)first_zero, off, 64), b = (uint32_t)__shfl_xor((int)first_bad, off, 64);
        first_zero = z < first_zero ? z : first_zero;
        first_bad = b < first_bad ? b : first_bad;
    }
    if ((tid & 63) == 0) {
        if (zeros) atomicAdd(&c.status[ST_ZEROS], zeros);
        if (first_zero != ASG_NONE) atomicMin(&c.status[ST_FIRST_ZERO], c.row_base + first_zero);
        if (first_bad != ASG_NONE) {
            atomicMin(&c.status[ST_FIRST_BAD], first_bad);
            atomicMax(&c.status[ST_CODE], (uint32_t)H2_ASSIGNED_BAD_ROWS);
        }
    }
    Fr inv = block_invert_products(acc, sh_lo, sh_hi);
    if (!active) return;
    // the power of R the forms leave open (see the head of the file), once per lane
    const int e = (int)(a.oform == ASG_MONTGOMERY) + (int)(c.dform == ASG_MONTGOMERY) - (int)(c.nform == ASG_MONTGOMERY) - 1;
    if (e == 1) inv = fp_to_mont(inv);
    if (e <= -1) inv = fp_from_mont(inv);
    if (e == -2) inv = fp_from_mont(inv);
    for (size_t j = last;; j -= nthreads) {
        uint32_t r;
        if (asg_row(c, n, j, r)) {
            const Fr v = asg_load(c.den, c.dform, j);
            Fr o = fp_zero<FrParams>();
            if (!fp_is_zero(v)) {
                o = fp_mul(fp_mul(inv, fp_load(out + r)), asg_load(c.num, c.nform, r));
                inv = fp_mul(inv, v);
            }
            fp_store(out + r, o);
        }
        if (j < nthreads) break;
    }
}

size_t cell_bytes(uint32_t form) { return form == ASG_COMPACT ? 8 : 32; }

bool overlap(const void* a, size_t a_bytes, const void* b, size_t b_bytes) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return a_bytes && b_bytes && x < y + b_bytes && y < x + a_bytes;
}

}  // namespace

const char* assigned_validate(const void* const* num, const uint32_t* num_forms, const void* const* den,
                              const uint32_t* den_forms, const uint32_t* const* rows, const uint64_t* counts,
                              void* const* out, size_t cols, size_t n, uint32_t out_form, const void* status, bool device) {
    if (cols == 0) return nullptr;
    if (!num) return device ? "d_num is null" : "num is null";
    if (!num_forms) return "num_forms is null";
    if (!den) return device ? "d_den is null" : "den is null";
    if (!den_forms) return "den_forms is null";
    if (!out) return device ? "d_out is null" : "out is null";
    if (!status) return device ? "d_status is null" : "status is null";
    if (rows && !counts) return "counts is null";
    if (n == 0) return "n is zero";
    if (n > 0xffffffffull) return "n exceeds 2^32 - 1";
    if (out_form > ASG_MONTGOMERY) return "out_form is an unknown form code (canonical or Montgomery)";
    if ((uintptr_t)status % 4) return device ? "d_status is misaligned" : "status is misaligned";
    const size_t wide = device ? 16 : 8;
    for (size_t i = 0; i < cols; i++) {
        const bool sparse = rows && rows[i];
        if (num_forms[i] > ASG_COMPACT) return "num_forms holds an unknown form code";
        if (den_forms[i] > ASG_COMPACT) return "den_forms holds an unknown form code";
        if (sparse && counts[i] > n) return "counts holds more rows than n";
        if (!num[i]) return device ? "d_num holds a null pointer" : "num holds a null pointer";
        if (!den[i] && !(sparse && counts[i] == 0)) return device ? "d_den holds a null pointer" : "den holds a null pointer";
        if (!out[i]) return device ? "d_out holds a null pointer" : "out holds a null pointer";
        if ((uintptr_t)num[i] % (num_forms[i] == ASG_COMPACT ? 8 : wide) || (uintptr_t)den[i] % (den_forms[i] == ASG_COMPACT ? 8 : wide) ||
            (uintptr_t)out[i] % wide)
            return "a column is misaligned for its form";
        if (sparse && (uintptr_t)rows[i] % 4) return "a rows array is misaligned";
    }
    // the prefix lives in `out` between the two passes: a column read after another one's `out` was written would be wrong too
    for (size_t i = 0; i < cols; i++) {
        for (size_t j = 0; j < cols; j++) {
            const size_t m = rows && rows[j] ? (size_t)counts[j] : n;
            if (overlap(out[i], n * 32, num[j], n * cell_bytes(num_forms[j]))) return "an out column overlaps a num column";
            if (overlap(out[i], n * 32, den[j], m * cell_bytes(den_forms[j]))) return "an out column overlaps a den column";
            if (rows && rows[j] && overlap(out[i], n * 32, rows[j], m * 4)) return "an out column overlaps a rows array";
            if (i != j && overlap(out[i], n * 32, out[j], n * 32)) return "two out columns overlap";
        }
    }
    return nullptr;
}

int assigned_status_init(uint32_t* d_status, size_t cols, hipStream_t stream) {
    if (cols == 0) return H2_OK;
    const uint32_t words = (uint32_t)(cols * H2_ASSIGNED_STATUS_WORDS);
    hipLaunchKernelGGL(k_assigned_status_init, dim3((words + 255) / 256), dim3(256), 0, stream, d_status, words);
    H2_HIP(hipGetLastError());
    return H2_OK;
}

int assigned_resolve_launch(const AssignedColumn* cols, size_t count, size_t n, uint32_t out_form, hipStream_t stream) {
    // the rows of a sparse column that have no denominator: num, in the output form
    for (size_t i = 0; i < count; i++) {
        const AssignedColumn& c = cols[i];
        if (!c.rows) continue;
        if (c.num_form == ASG_COMPACT) {
            const int rc = widen_u64_launch((const uint64_t*)c.num, n, (Fr*)c.out, stream);
            if (rc != H2_OK) return rc;
        } else {
            H2_HIP(hipMemcpyAsync(c.out, c.num, n * sizeof(Fr), hipMemcpyDeviceToDevice, stream));
        }
        if ((c.num_form == ASG_MONTGOMERY) != (out_form == ASG_MONTGOMERY)) {
            const int rc = batch_mont_launch((Fr*)c.out, n, out_form == ASG_MONTGOMERY, stream);
            if (rc != H2_OK) return rc;
        }
    }
    // the kernel arguments are passed by value: more columns than fit go in slices
    for (size_t first = 0; first < count; first += ASG_COLS_PER_LAUNCH) {
        AsgArgs a;
        memset(&a, 0, sizeof a);
        a.n = (uint32_t)n;
        a.oform = out_form;
        const size_t slice = count - first < (size_t)ASG_COLS_PER_LAUNCH ? count - first : (size_t)ASG_COLS_PER_LAUNCH;
        size_t blocks = 0;
        for (size_t j = 0; j < slice; j++) {
            const AssignedColumn& c = cols[first + j];
            AsgCol& k = a.c[j];
            k.num = c.num, k.den = c.den, k.rows = c.rows, k.out = c.out, k.status = c.status;
            k.count = (uint32_t)(c.rows ? c.count : n);
            k.nform = c.num_form, k.dform = c.den_form, k.row_base = c.row_base;
            const size_t b = (batch_invert_threads(k.count) + 255) / 256;
            if (b > blocks) blocks = b;
        }
        if (blocks == 0) continue;             // nothing but sparse columns without a listed row
        hipLaunchKernelGGL(k_assigned_resolve, dim3((unsigned)blocks, (unsigned)slice), dim3(256), 0, stream, a);
        H2_HIP(hipGetLastError());
    }
    return H2_OK;
}

}  // namespace h2
