// check.hpp -- MockProver-style constraint checking of a witness on the device (check.hip).
//
// Every failure is one h2_check_record (include/halo2_hip.h) appended to a caller-owned buffer of `cap` records with a
// caller-zeroed 64-bit count: each wave ballots its failing lanes and makes ONE agent-scope atomicAdd for all of them; a lane
// writes its record only when its slot is < cap, so the count stays exact after the buffer is full (which records are kept
// then is not specified).  record.kind = H2_CHECK_* | circuit << 8.
//
// Shuffles differ on purpose from the reference (dev.rs:1209-1262, which sorts both sides' tuples and reports the rows where
// the sorted lists part): compression by theta destroys the order of the tuples, so here both sides' compressed values are
// counted in one hash table and every INPUT row whose value is counted differently on the two sides is reported.
#pragma once
#include "common.hpp"

namespace h2 {
size_t check_scratch_bytes(size_t n);
// argument checks of the entry points, host-only (the C ABI runs them before it touches a device); H2_OK or H2_ERR_INVALID
int check_gates_args(const h2_evalh_desc* d);
int check_columns_args(const char* what, size_t usable, size_t n, size_t scratch_bytes);
int check_copies_args(size_t n_columns, size_t n);
int check_nonzero_rows_launch(const Fr* d_values, size_t usable, uint32_t* d_rows, uint64_t* d_row_count, hipStream_t stream);
int check_gates_launch(DeviceCtx* ctx, const h2_evalh_desc* d, const uint32_t* d_rows, const uint64_t* d_row_count,
                       uint32_t circuit, uint64_t* d_count, h2_check_record* d_records, size_t cap, hipStream_t stream);
int check_lookup_launch(const Fr* d_table, const Fr* const* d_inputs, const uint32_t* tags, size_t n_inputs, size_t usable,
                        size_t n, uint32_t lookup_index, uint32_t circuit, void* d_scratch, size_t scratch_bytes, uint64_t* d_count,
                        h2_check_record* d_records, size_t cap, hipStream_t stream);
int check_shuffle_launch(const Fr* d_input, const Fr* d_shuffle, size_t usable, size_t n, uint32_t group, uint32_t unit,
                         uint32_t circuit, void* d_scratch, size_t scratch_bytes, uint64_t* d_count, h2_check_record* d_records,
                         size_t cap, hipStream_t stream);
int check_copies_launch(const Fr* const* d_columns, size_t n_columns, const uint32_t* d_map_col, const uint32_t* d_map_row,
                        size_t n, uint32_t circuit, uint64_t* d_count, h2_check_record* d_records, size_t cap, hipStream_t stream);
}  // namespace h2
