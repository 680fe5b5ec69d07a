// srscheck.hpp -- screening the points of an SRS on the device (srscheck.hip): every coordinate a canonical residue, every
// point on y^2 = x^3 + 3 and, where the caller forbids it, none the identity.  The reference takes its points as they come:
// Params::read unwraps `from_bytes` per point (poly/commitment.rs:262-275) and nothing looks at a table built in memory.
//
// One lane takes one point.  A point fails in exactly one way, tested in the order NONCANONICAL, IDENTITY, OFF_CURVE
// (include/halo2_hip.h: H2_SRS_*), and appends one h2_check_record {kind, index = table, sub = 0, row = point index} by the
// scheme of check.hpp (append.hpp): the count accumulates over calls and stays exact after the buffer fills.
#pragma once
#include "common.hpp"

namespace h2 {
constexpr size_t G1_CHECK_MAX_POINTS = (size_t)1 << 28;
// argument checks of the entry point, host-only (the C ABI runs them before it touches a device); H2_OK or H2_ERR_INVALID
int g1_check_points_args(const void* d_points, size_t n, uint32_t flags, const uint64_t* d_count,
                         const h2_check_record* d_records, size_t cap);
int g1_check_points_launch(const void* d_points, size_t n, uint32_t table, uint32_t flags, uint64_t* d_count,
                           h2_check_record* d_records, size_t cap, hipStream_t stream);
}  // namespace h2
