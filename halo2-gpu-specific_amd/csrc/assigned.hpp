// assigned.hpp -- rational (`Assigned`) cells resolved on the device: out = num / den, zero for a zero denominator
// (assigned.hip)
#pragma once
#include "common.hpp"

namespace h2 {
// one column of a call; every pointer is device memory
struct AssignedColumn {
    const void* num;        // n cells in num_form
    const void* den;        // count cells in den_form
    const uint32_t* rows;   // count strictly increasing row indices, or nullptr: den is dense (count = n)
    void* out;              // n cells of 32 bytes
    uint32_t* status;       // H2_ASSIGNED_STATUS_WORDS words, initialised by assigned_status_init
    uint64_t count;
    uint32_t num_form, den_form;
    uint32_t row_base;      // added to the rows this column reports (a chunk of a longer column)
};

// the argument checks of h2_dev_assigned_resolve / h2_assigned_resolve: nullptr when the arguments are usable, else what
// is wrong with them.  `device`: the addresses are device memory (32-byte cells then need 16-byte alignment; host arrays
// are staged, 8 bytes do).  Host only -- nothing here touches a device.
const char* assigned_validate(const void* const* num, const uint32_t* num_forms, const void* const* den,
                              const uint32_t* den_forms, const uint32_t* const* rows, const uint64_t* counts,
                              void* const* out, size_t cols, size_t n, uint32_t out_form, const void* status, bool device);
// {OK, 0, none, none} for every column; asynchronous on `stream`
int assigned_status_init(uint32_t* d_status, size_t cols, hipStream_t stream);
// validated arguments only; asynchronous on `stream`.  The statuses ACCUMULATE (a column resolved chunk by chunk).
int assigned_resolve_launch(const AssignedColumn* cols, size_t count, size_t n, uint32_t out_form, hipStream_t stream);
}  // namespace h2
