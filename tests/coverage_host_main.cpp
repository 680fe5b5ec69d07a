// coverage_host_main.cpp -- csrc/coverage_host.cpp on its own, for the sanitizers (tests/test_coverage_host.py builds this with
// g++ -fsanitize=address,undefined; no HIP, no Python).  A few hundred random tables: the argument checks accept them, the mark
// gives exactly the bits a vector<bool> per plane says (the bit array is sized to the word, so a stray write is an ASan error),
// the check gives exactly the records a plain loop says, with the exact count under a short record buffer; and every table
// spoilt in one field is refused.  usage: coverage_host_main TRIALS
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <tuple>
#include <vector>

#include "coverage.hpp"

using namespace h2;

static uint64_t state = 0x9E3779B97F4A7C15ull;
static uint64_t draw(uint64_t below) {  // xorshift64*
    state ^= state >> 12;
    state ^= state << 25;
    state ^= state >> 27;
    return (state * 0x2545F4914F6CDD1Dull >> 16) % below;
}

#define REQUIRE(cond)                                                          \
    do {                                                                       \
        if (!(cond)) {                                                         \
            fprintf(stderr, "trial %d, line %d: %s\n", trial, __LINE__, #cond); \
            return 1;                                                          \
        }                                                                      \
    } while (0)

int main(int argc, char** argv) {
    const int trials = argc > 1 ? atoi(argv[1]) : 300;
    static const uint64_t strides[] = {1, 1, 2, 3, 31, 32, 33, 37};
    for (int trial = 0; trial < trials; trial++) {
        const size_t n = (size_t)1 << (4 + draw(7));
        std::vector<h2_coverage_plane> planes(1 + draw(6));
        size_t words = 0;
        for (auto& p : planes) {
            words += draw(3);  // a gap
            p.rows = (uint32_t)(1 + draw(std::min<size_t>(n, 100)));
            p.row_lo = (uint32_t)draw(n - p.rows + 1);
            p.first_word = words;
            words += (p.rows + 31) / 32;
        }
        std::vector<std::vector<bool>> model;
        for (auto& p : planes) model.emplace_back(p.rows, false);
        std::vector<h2_coverage_segment> segs(draw(13));
        for (auto& g : segs) {
            g.plane = (uint32_t)draw(planes.size());
            g.reserved = 0;
            const h2_coverage_plane& p = planes[g.plane];
            g.stride = strides[draw(8)];
            const uint64_t off = draw(p.rows);
            g.first_row = p.row_lo + off;
            g.count = draw((p.rows - 1 - off) / g.stride + 2);  // 0 now and then
            for (uint64_t c = 0; c < g.count; c++) model[g.plane][off + c * g.stride] = true;
        }
        std::vector<uint32_t> bits(words, 0);
        REQUIRE(!coverage_mark_validate(planes.data(), planes.size(), segs.data(), segs.size(), bits.data(), words, false, nullptr, 0));
        coverage_mark_host(planes.data(), segs.data(), segs.size(), bits.data());
        std::vector<uint32_t> want(words, 0);
        for (size_t p = 0; p < planes.size(); p++)
            for (uint32_t r = 0; r < planes[p].rows; r++)
                if (model[p][r]) want[planes[p].first_word + r / 32] |= 1u << (r % 32);
        REQUIRE(bits == want);

        std::vector<h2_coverage_query> queries(1 + draw(12));
        for (auto& q : queries) {
            q.plane = draw(4) ? (uint32_t)draw(planes.size()) : H2_COVERAGE_NO_PLANE;
            q.column = 0;
            q.rotation = (int32_t)draw(7) - 3;
            q.reserved = 0;
        }
        std::vector<h2_coverage_use> uses(draw(10));
        std::vector<uint32_t> earlier;
        for (size_t i = 0; i < uses.size(); i++) {
            h2_coverage_use& u = uses[i];
            if (i && draw(3) == 0) {  // an earlier use once more, which it names
                const uint32_t e = (uint32_t)draw(i);
                u = uses[e];
                u.first_earlier = (uint32_t)earlier.size();
                u.num_earlier = 1;
                earlier.push_back(e);
                continue;
            }
            u.region = (uint32_t)draw(5);
            u.gate = (uint32_t)draw(3);
            u.first_query = (uint32_t)draw(queries.size());
            u.num_queries = (uint32_t)draw(queries.size() - u.first_query + 1);
            u.first_earlier = (uint32_t)earlier.size();
            u.num_earlier = 0;
            u.stride = std::min<uint64_t>(strides[draw(8)], n);
            u.first_row = draw(n);
            u.count = draw((n - 1 - u.first_row) / u.stride + 2);
        }
        std::vector<std::tuple<uint32_t, uint32_t, uint32_t>> expect;
        for (const auto& u : uses)
            for (uint64_t c = 0; c < u.count; c++) {
                const uint64_t row = u.first_row + c * u.stride;
                bool repeated = false;
                for (uint32_t e = 0; e < u.num_earlier; e++) {
                    const auto& v = uses[earlier[u.first_earlier + e]];
                    for (uint64_t d = 0; d < v.count; d++) repeated |= v.first_row + d * v.stride == row;
                }
                if (repeated) continue;
                for (uint32_t q = 0; q < u.num_queries; q++) {
                    const auto& qu = queries[u.first_query + q];
                    const int64_t cell = ((int64_t)row + (int64_t)n + qu.rotation) % (int64_t)n;
                    bool ok = false;
                    if (qu.plane != H2_COVERAGE_NO_PLANE) {
                        const auto& p = planes[qu.plane];
                        if (cell >= p.row_lo && cell < (int64_t)p.row_lo + p.rows) ok = model[qu.plane][cell - p.row_lo];
                    }
                    if (!ok) expect.emplace_back(u.gate << 16 | q, u.region, (uint32_t)cell);
                }
            }
        for (size_t cap : {expect.size() + 3, expect.size() / 2, (size_t)0}) {
            std::vector<h2_check_record> records(cap);
            uint64_t count = 0;
            REQUIRE(!coverage_check_validate(planes.data(), planes.size(), queries.data(), queries.size(), uses.data(), uses.size(),
                                             earlier.data(), earlier.size(), n, bits.data(), words, false, nullptr, 0, &count,
                                             records.data(), cap));
            coverage_check_host(planes.data(), queries.data(), uses.data(), uses.size(), earlier.data(), n, bits.data(), &count,
                                records.data(), cap);
            REQUIRE(count == expect.size());
            std::vector<std::tuple<uint32_t, uint32_t, uint32_t>> got;
            for (size_t i = 0; i < std::min<size_t>(cap, count); i++) {
                REQUIRE(records[i].kind == H2_CHECK_CELL);
                got.emplace_back(records[i].index, records[i].sub, records[i].row);
            }
            auto sorted = expect;
            std::sort(sorted.begin(), sorted.end());
            std::sort(got.begin(), got.end());
            if (cap >= count) REQUIRE(got == sorted);
            REQUIRE(std::includes(sorted.begin(), sorted.end(), got.begin(), got.end()));
        }

        // one field spoilt: refused, and nothing is read past a table
        uint64_t count = 0;
        auto mark_refuses = [&](std::vector<h2_coverage_plane> ps, std::vector<h2_coverage_segment> ss) {
            return coverage_mark_validate(ps.data(), ps.size(), ss.data(), ss.size(), bits.data(), words, false, nullptr, 0) != nullptr;
        };
        auto check_refuses = [&](std::vector<h2_coverage_query> qs, std::vector<h2_coverage_use> us, std::vector<uint32_t> es, size_t rows) {
            return coverage_check_validate(planes.data(), planes.size(), qs.data(), qs.size(), us.data(), us.size(), es.data(),
                                           es.size(), rows, bits.data(), words, false, nullptr, 0, &count, nullptr, 0) != nullptr;
        };
        const h2_coverage_plane& p0 = planes[0];
        REQUIRE(mark_refuses(planes, {{(uint32_t)planes.size(), 0, p0.row_lo, 1, 1}}));
        REQUIRE(mark_refuses(planes, {{0, 0, p0.row_lo, 0, 2}}));
        REQUIRE(mark_refuses(planes, {{0, 0, (uint64_t)p0.row_lo + p0.rows, 1, 1}}));
        REQUIRE(mark_refuses(planes, {{0, 0, p0.row_lo, 1, (uint64_t)p0.rows + 1}}));
        REQUIRE(mark_refuses(planes, {{0, 0, p0.row_lo, p0.rows, 2}}));
        if (p0.row_lo) REQUIRE(mark_refuses(planes, {{0, 0, (uint64_t)p0.row_lo - 1, 1, 1}}));
        auto spoilt = planes;
        spoilt.back().first_word = words - (spoilt.back().rows + 31) / 32 + 1;
        REQUIRE(mark_refuses(spoilt, {{0, 0, p0.row_lo, 1, 1}}));
        const h2_coverage_use good{0, 0, 0, 1, 0, 0, 0, 1, 1};
        REQUIRE(!check_refuses(queries, {good}, {}, n));
        auto use = [&](auto change) {
            h2_coverage_use u = good;
            change(u);
            return std::vector<h2_coverage_use>{good, u};
        };
        REQUIRE(check_refuses(queries, use([&](h2_coverage_use& u) { u.first_row = n; }), {}, n));
        REQUIRE(check_refuses(queries, use([&](h2_coverage_use& u) { u.first_row = n - 1, u.count = 2; }), {}, n));
        REQUIRE(check_refuses(queries, use([&](h2_coverage_use& u) { u.stride = 0; }), {}, n));
        REQUIRE(check_refuses(queries, use([&](h2_coverage_use& u) { u.gate = 1u << 16; }), {}, n));
        REQUIRE(check_refuses(queries, use([&](h2_coverage_use& u) { u.num_queries = (uint32_t)queries.size() + 1; }), {}, n));
        REQUIRE(check_refuses(queries, use([&](h2_coverage_use& u) { u.num_earlier = 1; }), {}, n));
        REQUIRE(check_refuses(queries, use([&](h2_coverage_use& u) { u.num_earlier = 1; }), {1}, n));
        REQUIRE(!check_refuses(queries, use([&](h2_coverage_use& u) { u.num_earlier = 1; }), {0}, n));
        auto bad_queries = queries;
        bad_queries[0].plane = (uint32_t)planes.size();
        REQUIRE(check_refuses(bad_queries, {good}, {}, n));
        bad_queries = queries;
        bad_queries[0].rotation = -(int32_t)n;
        REQUIRE(check_refuses(bad_queries, {good}, {}, n));
        REQUIRE(check_refuses(queries, {good}, {}, 0));
    }
    printf("ok %d\n", trials);
    return 0;
}
