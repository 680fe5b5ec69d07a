// coverage_host.cpp -- the coverage check's argument checks, the mark launch's plan and the host twins of the two kernels
// (coverage.hpp): plain host C++, no HIP (tests/coverage_host_main.cpp builds it with g++ alone, under the sanitizers).
#include "coverage.hpp"

namespace h2 {

static size_t round16(size_t bytes) { return (bytes + 15) / 16 * 16; }

size_t coverage_scratch_bytes(size_t segments, size_t planes, size_t queries, size_t uses, size_t earlier) {
    // a mark: the segment table and its two prefix sums; a check: planes, queries, uses, earlier, the uses' prefix sums
    size_t bytes = 0;
    if (segments) bytes += segments * sizeof(CovSeg) + 2 * round16((segments + 1) * sizeof(uint64_t));
    if (uses)
        bytes += planes * sizeof(h2_coverage_plane) + queries * sizeof(h2_coverage_query) + uses * sizeof(h2_coverage_use) +
                 round16(earlier * sizeof(uint32_t)) + round16((uses + 1) * sizeof(uint64_t));
    return bytes;
}

static const char* coverage_shape(const h2_coverage_plane* planes, size_t num_planes, const void* bits, size_t words) {
    if (num_planes && !planes) return "null plane table";
    if (num_planes >= H2_COVERAGE_NO_PLANE) return "2^32 - 1 planes or more";
    if (!bits || ((uintptr_t)bits & 3)) return "the bit array must be a 4-byte aligned pointer";
    if (words == 0 || words > COV_MAX_WORDS) return "the bit array must have between 1 and 2^30 words";
    for (size_t p = 0; p < num_planes; p++) {
        const size_t need = ((size_t)planes[p].rows + 31) / 32;
        if (planes[p].first_word > words || need > words - planes[p].first_word) return "a plane lies outside the bit array";
        if ((uint64_t)planes[p].row_lo + planes[p].rows > ((uint64_t)1 << 31)) return "a plane reaches beyond row 2^31 - 1";
    }
    return nullptr;
}

static const char* coverage_scratch(const void* d_scratch, size_t scratch_bytes, size_t need) {
    if (!d_scratch || ((uintptr_t)d_scratch & 15)) return "the scratch must be a 16-byte aligned device pointer";
    if (scratch_bytes < need) return "the scratch is smaller than h2_coverage_scratch_bytes";
    return nullptr;
}

const char* coverage_mark_validate(const h2_coverage_plane* planes, size_t num_planes, const h2_coverage_segment* segs, size_t count,
                                   const void* bits, size_t words, bool device, const void* d_scratch, size_t scratch_bytes) {
    if (count == 0) return nullptr;
    if (!segs) return "null segment table";
    if (const char* what = coverage_shape(planes, num_planes, bits, words)) return what;
    if (count >= ((size_t)1 << 31)) return "2^31 segments or more";
    if (device)
        if (const char* what = coverage_scratch(d_scratch, scratch_bytes, coverage_scratch_bytes(count, 0, 0, 0, 0))) return what;
    uint64_t units = 0;
    for (size_t s = 0; s < count; s++) {
        const h2_coverage_segment& g = segs[s];
        if (g.plane >= num_planes) return "a segment names a plane that does not exist";
        if (g.count == 0) continue;
        const h2_coverage_plane& p = planes[g.plane];
        if (g.stride == 0 || g.stride > ((uint64_t)1 << 31)) return "a segment's stride must be between 1 and 2^31";
        // the last cell, first + (count - 1) stride, inside [row_lo, row_lo + rows): no product overflows, all are <= 2^62
        if (g.first_row < p.row_lo || g.first_row - p.row_lo >= p.rows || g.count > p.rows ||
            (g.count - 1) * g.stride >= p.rows - (g.first_row - p.row_lo))
            return "a segment reaches outside its plane";
        units += g.count;  // an upper bound of the words too
    }
    if ((units + COV_CHUNK - 1) / COV_CHUNK >= ((uint64_t)1 << 30)) return "too many cells for one launch";
    return nullptr;
}

const char* coverage_check_validate(const h2_coverage_plane* planes, size_t num_planes, const h2_coverage_query* queries,
                                    size_t num_queries, const h2_coverage_use* uses, size_t num_uses, const uint32_t* earlier,
                                    size_t num_earlier, size_t n, const void* bits, size_t words, bool device, const void* d_scratch,
                                    size_t scratch_bytes, const uint64_t* count, const h2_check_record* records, size_t cap) {
    if (!count || ((uintptr_t)count & 7)) return "the count must be an 8-byte aligned pointer";
    if (cap && (!records || ((uintptr_t)records & (device ? 15 : 3))))
        return "the records must be a 16-byte aligned pointer (4 on the host)";
    if (num_uses == 0) return nullptr;
    if (!uses) return "null use table";
    if (n == 0 || n > ((size_t)1 << 31)) return "n must be between 1 and 2^31";
    if (const char* what = coverage_shape(planes, num_planes, bits, words)) return what;
    if (num_queries && !queries) return "null query table";
    if (num_earlier && !earlier) return "null table of earlier uses";
    if (num_uses >= ((size_t)1 << 31) || num_queries >= ((size_t)1 << 32) || num_earlier >= ((size_t)1 << 32))
        return "too long a table";
    if (device)
        if (const char* what = coverage_scratch(d_scratch, scratch_bytes,
                                                coverage_scratch_bytes(0, num_planes, num_queries, num_uses, num_earlier)))
            return what;
    for (size_t q = 0; q < num_queries; q++) {
        if (queries[q].plane != H2_COVERAGE_NO_PLANE && queries[q].plane >= num_planes)
            return "a query names a plane that does not exist";
        if (queries[q].rotation >= (int64_t)n || -(int64_t)queries[q].rotation >= (int64_t)n) return "a rotation of n rows or more";
    }
    uint64_t rows = 0;
    for (size_t i = 0; i < num_uses; i++) {
        const h2_coverage_use& u = uses[i];
        if (u.gate >= (1u << 16) || u.num_queries >= (1u << 16)) return "a gate index or a gate's number of queries is 2^16 or more";
        if (u.first_query > num_queries || u.num_queries > num_queries - u.first_query)
            return "a use's queries lie outside the query table";
        if (u.first_earlier > num_earlier || u.num_earlier > num_earlier - u.first_earlier)
            return "a use's earlier uses lie outside their table";
        for (uint32_t e = 0; e < u.num_earlier; e++)
            if (earlier[u.first_earlier + e] >= i) return "an earlier use that is not earlier";
        if (u.count == 0) continue;
        if (u.stride == 0 || u.stride > n) return "a use's stride must be between 1 and n";
        if (u.first_row >= n || u.count > n || (u.count - 1) * u.stride >= n - u.first_row) return "a use reaches beyond row n - 1";
        rows += u.count;
    }
    if ((rows + COV_CHUNK - 1) / COV_CHUNK >= ((uint64_t)1 << 30)) return "too many rows for one launch";
    return nullptr;
}

CovMarkPlan coverage_mark_plan(const h2_coverage_plane* planes, const h2_coverage_segment* segs, size_t count) {
    CovMarkPlan plan;
    std::vector<CovSeg> strided;
    uint64_t words = 0, cells = 0;
    for (size_t s = 0; s < count; s++) {
        const h2_coverage_segment& g = segs[s];
        if (g.count == 0) continue;  // the kernel relies on it: every segment of its tables has a unit
        const h2_coverage_plane& p = planes[g.plane];
        const CovSeg seg{p.first_word * 32 + (g.first_row - p.row_lo), (uint32_t)g.count, (uint32_t)g.stride};
        if (g.stride == 1 || g.count == 1) {
            plan.segs.push_back(CovSeg{seg.first_bit, seg.count, 1});
            plan.word_prefix.push_back(words);
            words += ((seg.first_bit + seg.count - 1) >> 5) - (seg.first_bit >> 5) + 1;
        } else {
            strided.push_back(seg);
            plan.cell_prefix.push_back(cells);
            cells += g.count;
        }
    }
    if (!plan.word_prefix.empty()) plan.word_prefix.push_back(words);
    if (!plan.cell_prefix.empty()) plan.cell_prefix.push_back(cells);
    plan.segs.insert(plan.segs.end(), strided.begin(), strided.end());
    return plan;
}

void coverage_mark_host(const h2_coverage_plane* planes, const h2_coverage_segment* segs, size_t count, uint32_t* bits) {
    // the plan's two splits, unit by unit, as the kernel's lanes take them
    const CovMarkPlan plan = coverage_mark_plan(planes, segs, count);
    for (size_t s = 0; s < plan.by_word(); s++) {
        const CovSeg& g = plan.segs[s];
        for (uint64_t w = g.first_bit >> 5; w <= (g.first_bit + g.count - 1) >> 5; w++)
            bits[w] |= coverage_word_mask(g.first_bit, g.count, w);
    }
    for (size_t s = 0; s < plan.by_cell(); s++) {
        const CovSeg& g = plan.segs[plan.by_word() + s];
        for (uint64_t c = 0; c < g.count; c++) {
            const uint64_t bit = g.first_bit + c * g.stride;
            bits[bit >> 5] |= 1u << (bit & 31);
        }
    }
}

void coverage_check_host(const h2_coverage_plane* planes, const h2_coverage_query* queries, const h2_coverage_use* uses,
                         size_t num_uses, const uint32_t* earlier, size_t n, const uint32_t* bits, uint64_t* count,
                         h2_check_record* records, size_t cap) {
    for (size_t i = 0; i < num_uses; i++) {
        const h2_coverage_use& u = uses[i];
        for (uint64_t c = 0; c < u.count; c++) {
            const uint64_t row = u.first_row + c * u.stride;
            if (coverage_row_repeated(uses, earlier, u, row)) continue;
            for (uint32_t q = 0; q < u.num_queries; q++) {
                uint32_t cell_row;
                if (coverage_assigned(planes, bits, queries[u.first_query + q], row, n, cell_row)) continue;
                const uint64_t slot = (*count)++;
                if (slot < cap) records[slot] = h2_check_record{H2_CHECK_CELL, u.gate << 16 | q, u.region, cell_row};
            }
        }
    }
}

}  // namespace h2
