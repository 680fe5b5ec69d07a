// sort.hpp -- the stable radix sort of field elements behind Value.argsort (values.py; DESIGN.md 3b, "Sorting a witness"):
// up to H2_SORT_MAX_KEYS key columns, each read as the integer in [0, r), ordered lexicographically; the output is the
// permutation.  Least significant digit first, 8 bits a pass, over INDICES: a pass reads the permutation so far, gathers one
// byte of each key through it, ranks the tile (sort.hip) and scatters the indices; the keys never move.
//   sort_plan.cpp   what a call decides before anything is enqueued: the candidate (key, byte) positions given forms and
//                   bits, the tiles, the scratch layout.  Host only, no HIP: tests/sort_host_main.cpp checks it alone.
//   sort_host.cpp   the argument checks and the host twin (h2_sort_permutation): the same passes, the same skips, the same
//                   status words, one row after another
//   sort.hip        the kernels and the driver
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/halo2_hip.h"

namespace h2 {

constexpr uint32_t SORT_TILE = H2_SORT_TILE;             // rows a workgroup of a pass ranks: 256 lanes x 8 rounds
constexpr uint32_t SORT_SCAN_TILE = 2 * SORT_TILE;       // words a workgroup of the histogram's scan takes: 16 a lane
constexpr uint32_t SORT_MAX_KEYS = H2_SORT_MAX_KEYS;
constexpr uint32_t SORT_MAX_POS = 32 * SORT_MAX_KEYS;    // digit positions a call can have
constexpr uint32_t SORT_SURVEY_BLOCKS = 1024;            // most workgroups of the survey (each walks several tiles)
// the misc block of the scratch, in u32 words
constexpr uint32_t SORT_MISC_BAD = 0;                    // u64: min over broken promises of row << 32 | key
constexpr uint32_t SORT_MISC_FINAL = 2;                  // where the finished permutation lies: buffer 0 / 1, or SORT_IDENTITY
constexpr uint32_t SORT_MISC_ACTIVE = 16;                // [SORT_MAX_POS]: does position p move data
constexpr uint32_t SORT_MISC_SRC = SORT_MISC_ACTIVE + SORT_MAX_POS;   // [SORT_MAX_POS]: the buffer position p reads
constexpr uint32_t SORT_MISC_WORDS = 512;
constexpr uint32_t SORT_IDENTITY = 2;                    // "buffer" of the permutation nobody has written yet: perm[i] = i

struct SortPos {
    uint8_t key, byte;
};

struct SortPlan {
    uint32_t num_keys, num_pos;
    uint32_t form[SORT_MAX_KEYS], bits[SORT_MAX_KEYS];   // bits: the promise in force (never 0)
    uint32_t first_pos[SORT_MAX_KEYS];                   // the key's byte b is position first_pos[key] + b
    SortPos pos[SORT_MAX_POS];                           // in the order the passes run: last key first, low byte first
    size_t n, tiles, hist_words, scan_words;
    // byte offsets into the scratch, each a multiple of 256
    size_t off_misc, off_ghist, off_perm[2], off_digits, off_hist, off_scan, off_canon[SORT_MAX_KEYS], total;
};

inline size_t sort_ceil_div(size_t a, size_t b) { return (a + b - 1) / b; }

// bits in force for a key: the promise, or all a cell of that form can hold
uint32_t sort_effective_bits(uint32_t form, uint32_t bits);
// byte positions of a key that can differ under its promise
uint32_t sort_candidate_bytes(uint32_t form, uint32_t bits);
// tiles of SORT_TILE rows
size_t sort_tiles(size_t n);
// u32 words of the partial sums of every level of the scan over `words` words
size_t sort_scan_tmp_words(size_t words);
// levels of that scan: 1 while one workgroup takes it all
uint32_t sort_scan_levels(size_t words);
// nullptr and *out filled, or what is wrong with forms / bits / num_keys / n
const char* sort_plan(const uint32_t* forms, const uint32_t* bits, size_t num_keys, size_t n, SortPlan* out);

// the argument checks of h2_dev_sort_permutation (device: 16-byte aligned cells and scratch) and h2_sort_permutation
const char* sort_validate(const void* const* keys, const uint32_t* forms, const uint32_t* bits, size_t num_keys, size_t n,
                          const void* perm, uint32_t perm_width, const uint32_t* status, bool device, const void* scratch,
                          size_t scratch_bytes, SortPlan* plan);
// the host twin; arguments validated
void sort_permutation_host(const SortPlan& plan, const void* const* keys, void* perm, uint32_t perm_width, uint32_t* status);

#ifdef __HIPCC__
// asynchronous on `stream`; arguments validated
int sort_permutation_launch(const SortPlan& plan, const void* const* d_keys, void* d_perm, uint32_t perm_width,
                            uint32_t* d_status, void* d_scratch, hipStream_t stream);
// out[i] = in[perm[i]], 32-byte cells
int sort_gather_launch(const void* d_in, const uint32_t* d_perm, void* d_out, size_t n, hipStream_t stream);
#endif

}  // namespace h2
