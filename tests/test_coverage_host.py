"""check_assignments without a GPU: MockProver's CellNotAssigned (dev.rs:959-1000) as the host assembly (synthesis.HostCoverage)
and the library's host twins (h2_coverage_mark + h2_coverage_check through ctypes) compute it, against the brute-force model of
tests/coverage_cases.py -- random front-end circuits under both planners, pairs with a known answer (every required cell
assigned; the same with chosen cells left out), every consequence DESIGN.md 3b "Checking assignments" lists as a hand case,
the reference's examples, the argument checks of the five entry points, the header against SYMBOLS and the numpy dtypes, the
decoding of the records, and csrc/coverage_host.cpp under the address and undefined-behaviour sanitizers as a stand-alone
program."""
import os
import re
import subprocess

import numpy as np
import pytest

import coverage_cases as cc
import halo2_gpu_specific_amd as h2
from halo2_gpu_specific_amd import check, circuits_frontend as fe, prover, synthesis as syn
from halo2_gpu_specific_amd._lib import SYMBOLS
from halo2_gpu_specific_amd.check import CellNotAssigned

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "halo2-gpu-specific_amd", "csrc")
SIZES = [16, 32, 64, 1 << 10]
PLANNERS = [syn.FlatFloorPlanner, syn.V1]
ALL = 1 << 20


def host_result(circuit, n, planner=None):
    failures, total = check.check_assignments(None, circuit, n.bit_length() - 1, planner, max_failures=ALL, resident=False)
    return sorted(failures), total


def library_result(circuit, n, cap=ALL):
    """h2_coverage_mark + h2_coverage_check over a host bit array -> (failures, total, the bit array)"""
    L = h2.lib()
    cov = syn.synthesize_coverage(None, circuit, n.bit_length() - 1, resident=False)
    planes, segments, queries, uses, earlier, words = cov.build()
    bits = np.zeros(words, dtype="<u4")
    rc = L.h2_coverage_mark(planes.ctypes.data, len(planes), segments.ctypes.data, len(segments), bits.ctypes.data, words)
    assert rc == 0, L.h2_last_error()
    count, records = np.zeros(1, dtype=np.uint64), np.zeros((max(cap, 1), 4), dtype=np.uint32)
    rc = L.h2_coverage_check(planes.ctypes.data, len(planes), queries.ctypes.data, len(queries), uses.ctypes.data, len(uses),
                             earlier.ctypes.data, len(earlier), n, bits.ctypes.data, words, count.ctypes.data, records.ctypes.data, cap)
    assert rc == 0, L.h2_last_error()
    total = int(count[0])
    return check.check_failures(None, records[:min(total, cap)], cov), total, (bits, cov)


# -- random front-end circuits ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("planner", PLANNERS, ids=lambda p: p.__name__)
@pytest.mark.parametrize("seed", range(24))
def test_random_circuits_match_the_model(seed, planner):
    n = SIZES[seed % 4]
    spec = cc.random_spec(seed, planner, n)
    circuit = cc.SpecCircuit(spec, planner)
    want = cc.model(spec, planner, n)
    assert host_result(circuit, n) == want
    failures, total, (bits, cov) = library_result(circuit, n)
    assert (sorted(failures), total) == want
    assert np.array_equal(bits, cov.bitmap())
    assert len(cov.regions) == len(spec["regions"])


def test_the_random_circuits_cover_the_ground():
    """the generator does produce what the test above claims to cover"""
    seen = set()
    for seed in range(24):
        for planner in PLANNERS:
            spec = cc.random_spec(seed, planner, SIZES[seed % 4])
            _, total = cc.model(spec, planner, SIZES[seed % 4])
            ops = [op for _, _, _, region in spec["regions"] for op in region]
            seen |= {"failures" if total else "clean", "regions %d" % min(len(spec["regions"]), 30)}
            seen |= {"stride %d" % op[3] for op in ops if op[0] in ("advice", "fixed") and op[4] > 1}
            seen |= {op[0] for op in ops} | {kind for _, kind, _, _ in spec["regions"]}
            seen |= {"instance query" for _, polys in spec["gates"] for _, cells in polys for c, _ in cells if c[0] == "instance"}
            seen |= {"complex" for simple in spec["selectors"] if not simple}
    for what in ["failures", "regions 1", "regions 30", "table", "constant", "instance", "instance query", "complex",
                 "enable"] + ["stride %d" % s for s in cc.STRIDES]:
        assert what in seen, what


# -- pairs with a known answer ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("planner", PLANNERS, ids=lambda p: p.__name__)
@pytest.mark.parametrize("seed", range(24))
def test_complete_circuits_are_silent_and_holes_are_named(seed, planner):
    n = SIZES[seed % 4]
    complete, holed, expected = cc.paired_specs(seed, planner, n)
    assert expected[1] > 0                                               # both variants occur for every seed
    assert host_result(cc.SpecCircuit(complete, planner), n) == ([], 0)
    assert library_result(cc.SpecCircuit(complete, planner), n)[:2] == ([], 0)
    assert host_result(cc.SpecCircuit(holed, planner), n) == expected
    failures, total, _ = library_result(cc.SpecCircuit(holed, planner), n)
    assert (sorted(failures), total) == expected
    assert cc.model(holed, planner, n) == expected and cc.model(complete, planner, n) == ([], 0)


# -- hand cases ----------------------------------------------------------------------------------------------------------------
class Hand(syn.Circuit):
    """a, b, c advice, f fixed, i instance; selector s gates `polys(cs, columns)`; `regions`: [(name, body(region, columns, s))]"""

    def __init__(self, regions, polys=None, planner=syn.FlatFloorPlanner):
        self.regions, self.polys, self.planner = regions, polys, planner

    def without_witnesses(self):
        return self

    def configure(self, cs):
        columns = {"a": cs.advice_column(), "b": cs.advice_column(), "c": cs.advice_column(), "f": cs.fixed_column(),
                   "i": cs.instance_column()}
        s = cs.selector()
        polys = self.polys or (lambda cs, col: [cs.query_advice(col["a"]) * cs.query_advice(col["b"]) - cs.query_advice(col["c"])])
        cs.create_gate("mul", [cs.query_selector(s) * p for p in polys(cs, columns)])
        return columns, s

    def synthesize(self, config, layouter):
        for name, body in self.regions:
            layouter.assign_region(name, lambda region, body=body: body(region, *config))


def abc(rows, skip=()):
    def body(region, col, s):
        for name in "abc":
            if name not in skip:
                region.assign_advice(col[name], rows[0], None, count=len(rows))
        region.enable_selector(s, rows[0], count=len(rows))
    return body


def test_a_cell_another_region_assigned_does_not_count():
    """under FlatFloorPlanner both regions sit on rows 0 and 1: the second one's c is the first one's, not its own"""
    circuit = Hand([("first", abc([0, 1])), ("second", abc([0, 1], skip="c"))])
    assert host_result(circuit, 16) == ([CellNotAssigned(0, "mul", 1, "second", ("advice", 2), 0, 0),
                                         CellNotAssigned(0, "mul", 1, "second", ("advice", 2), 1, 1)], 2)


def test_a_column_the_region_never_touched_fails_on_every_enabled_row():
    failures, total = host_result(Hand([("r", abc(list(range(3, 8)), skip="b"))]), 32)
    assert total == 5 and failures == [CellNotAssigned(0, "mul", 0, "r", ("advice", 1), row - 3, row) for row in range(3, 8)]


def test_an_instance_column_a_gate_queries_fails_on_every_enabled_row():
    """the reference's regions never track instance cells; kept"""
    polys = lambda cs, col: [cs.query_advice(col["a"]) - cs.query_instance(col["i"])]   # noqa: E731
    failures, total = host_result(Hand([("r", abc([0, 1, 2]))], polys), 16)
    assert total == 3 and failures == [CellNotAssigned(0, "mul", 0, "r", ("instance", 0), row, row) for row in range(3)]


def test_a_rotation_that_wraps_past_row_0_or_leaves_the_usable_rows_fails():
    polys = lambda cs, col: [cs.query_advice(col["a"], -1) + cs.query_advice(col["a"], 1)]   # noqa: E731
    n = 16
    usable = n - 6

    def body(region, col, s):
        region.assign_advice(col["a"], 0, None, count=usable)
        region.enable_selector(s, 0)
        region.enable_selector(s, usable - 1)
        region.enable_selector(s, 4)

    failures, total = host_result(Hand([("r", body)], polys), n)
    assert (failures, total) == ([CellNotAssigned(0, "mul", 0, "r", ("advice", 0), usable, usable),
                                  CellNotAssigned(0, "mul", 0, "r", ("advice", 0), n - 1, n - 1)], 2)


def test_offset_counts_from_the_first_assigned_row_not_the_planners_start():
    """V1 starts the region at row 0; its first assigned cell is at offset 2, and that is where offsets count from"""
    def body(region, col, s):
        region.assign_advice(col["a"], 2, None, count=3)
        region.assign_advice(col["b"], 3, None, count=2)
        region.enable_selector(s, 3)

    circuit = Hand([("r", body)], planner=syn.V1)
    assert syn.region_starts(circuit) == [0]
    assert host_result(circuit, 16) == ([CellNotAssigned(0, "mul", 0, "r", ("advice", 2), 1, 3)], 1)


def test_offset_of_a_region_without_cells_counts_from_the_planners_start():
    """the reference panics there; here the planner's start row stands in.  V1 puts the second region below the first."""
    only = lambda region, col, s: region.enable_selector(s, 1)                           # noqa: E731
    circuit = Hand([("full", abc([0, 1, 2])), ("empty", only)], planner=syn.V1)
    starts = syn.region_starts(circuit)
    assert starts[1] != starts[0]
    failures, total = host_result(circuit, 16)
    assert total == 3 and failures == [CellNotAssigned(0, "mul", 1, "empty", ("advice", c), 1, starts[1] + 1) for c in range(3)]


def test_each_failure_is_reported_once_and_in_order():
    """a selector row enabled twice, by a single row and by two overlapping ranges, and a cell queried twice: one failure per
    (region, gate, queried cell, row), sorted by region, gate, the cell's first appearance in the polynomials, then row"""
    polys = lambda cs, col: [cs.query_advice(col["c"]) * cs.query_advice(col["a"], 1),                    # noqa: E731
                             cs.query_advice(col["c"]) + cs.query_fixed(col["f"]) * cs.query_advice(col["a"], 1)]

    def body(region, col, s):
        region.enable_selector(s, 2, count=3)
        region.enable_selector(s, 3)
        region.enable_selector(s, 2, stride=2, count=2)
        region.enable_selector(s, 3)

    circuit = Hand([("r", body)], polys)
    failures, total = check.check_assignments(None, circuit, 4, resident=False)
    queried = [(("advice", 2), 0), (("advice", 0), 1), (("fixed", 0), 0)]
    assert syn.synthesize_coverage(None, circuit, 4, resident=False).gates == [("mul", [0], queried)]
    assert total == 9 and failures == [CellNotAssigned(0, "mul", 0, "r", column, row + rotation, row + rotation)
                                       for column, rotation in queried for row in (2, 3, 4)]
    assert library_result(circuit, 16)[:2] == (failures, 9)
    assert library_result(circuit, 16, cap=4)[1] == 9


def test_tables_take_a_region_index_and_what_lies_outside_regions_belongs_to_none():
    """the table is region 1; its fill_from_row and the constant's fixed cell are nobody's -- and nobody enables a gate there"""
    class WithTable(Hand):
        def configure(self, cs):
            columns, s = Hand.configure(self, cs)
            columns["t"], columns["k"] = cs.lookup_table_column(), cs.fixed_column()
            cs.enable_constant(columns["k"])
            cs.enable_equality(columns["a"])
            return columns, s

        def synthesize(self, config, layouter):
            columns, s = config
            layouter.assign_region("before", lambda region: region.assign_advice_from_constant(columns["a"], 0, 7))
            layouter.assign_table("table", lambda table: table.assign_cell(columns["t"], 0, 1, count=3))
            layouter.assign_region("after", lambda region: abc([0], skip="a")(region, columns, s))

    cov = syn.synthesize_coverage(None, WithTable([]), 4, resident=False)
    assert cov.regions == [("before", 0), ("table", 0), ("after", 0)]
    assert sorted(cov.segments) == sorted([(0, ("advice", 0), 0, 1, 1), (1, ("fixed", 1), 0, 1, 3), (2, ("advice", 1), 0, 1, 1),
                                           (2, ("advice", 2), 0, 1, 1)])
    assert host_result(WithTable([]), 16) == ([CellNotAssigned(0, "mul", 2, "after", ("advice", 0), 0, 0)], 1)


def test_the_coverage_assembly_keeps_the_bounds_checks_and_takes_missing_advice():
    usable = 16 - 6
    with pytest.raises(syn.NotEnoughRowsAvailable):
        host_result(Hand([("r", abc([usable]))]), 16)
    with pytest.raises(syn.NotEnoughRowsAvailable):
        host_result(Hand([("r", lambda region, col, s: region.enable_selector(s, usable))]), 16)
    with pytest.raises(syn.BoundsFailure):
        host_result(Hand([("r", lambda region, col, s: region.assign_advice(("advice", 3), 0, None))]), 16)
    with pytest.raises(syn.SynthesisError):
        host_result(Hand([("r", lambda region, col, s: region.assign_fixed(col["f"], 0, None))]), 16)
    assert host_result(Hand([("r", abc([usable - 1]))]), 16) == ([], 0)


def test_the_total_of_planes_that_does_not_fit_is_a_value_error(monkeypatch):
    monkeypatch.setattr(syn, "COVERAGE_MAX_WORDS", 1)
    with pytest.raises(ValueError, match="2\\^35 bits"):
        host_result(Hand([("r", abc([0, 1]))]), 16)


# -- the reference's examples ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("circuit,k", [(fe.LookupApi(), 8), (fe.LookupApiSet(), 8), (fe.RangeCheck(8, vmax=63, count=100), 8), (fe.ShuffleGates(8), 8),
                                       (fe.ShuffleApi(), 8), (fe.ShuffleApiGroup(), 8), (fe.MiniPlonk(5), 5), (fe.Wide(6, 2), 6),
                                       (fe.SimpleExample(), 4), (fe.TwoChip(), 4), (fe.SelectorGates(6), 6)],
                         ids=lambda v: type(v).__name__)
def test_the_examples_assign_every_cell_their_gates_read(circuit, k):
    assert check.check_assignments(None, circuit, k, resident=False) == ([], 0)
    assert library_result(circuit, 1 << k)[:2] == ([], 0)


# -- the library's side ------------------------------------------------------------------------------------------------------------
def test_entry_points_check_their_arguments_before_any_launch():
    L = h2.lib()
    fake = np.zeros(64, dtype=np.uint64)                                 # an aligned address nothing is launched on
    ptr = fake.ctypes.data
    assert ptr % 16 == 0
    n, words = 64, 4
    planes = np.array([(0, 5, 40), (2, 0, 64)], dtype=syn.COVERAGE_PLANE)

    def mark(segment, planes=planes, bits=ptr, words=words, scratch=ptr, nbytes=1 << 12, host=False):
        segs = np.array([segment], dtype=syn.COVERAGE_SEGMENT)
        args = (planes.ctypes.data, len(planes), segs.ctypes.data, 1, bits, words)
        return L.h2_coverage_mark(*args) if host else L.h2_dev_coverage_mark(*(args + (scratch, nbytes, None)))

    for host, name in ((False, b"h2_dev_coverage_mark: "), (True, b"h2_coverage_mark: ")):
        for segment in ((2, 0, 5, 1, 1), (0, 0, 5, 0, 2), (0, 0, 4, 1, 1), (0, 0, 45, 1, 1), (0, 0, 5, 1, 41), (0, 0, 44, 2, 2),
                        (0, 0, 5, 40, 2)):
            assert mark(segment, host=host) == 1 and L.h2_last_error().startswith(name), segment
        assert mark((0, 0, 5, 1, 1), bits=None, host=host) == 1 and mark((0, 0, 5, 1, 1), bits=ptr + 2, host=host) == 1
        assert mark((0, 0, 5, 1, 1), words=3, host=host) == 1            # plane 1 ends at word 4
        assert mark((0, 0, 5, 1, 1), words=0, host=host) == 1 and mark((0, 0, 5, 1, 1), words=(1 << 30) + 1, host=host) == 1
        assert mark((0, 0, 5, 1, 1), planes=np.array([(4, 0, 1)], dtype=syn.COVERAGE_PLANE), host=host) == 1
    assert mark((0, 0, 5, 1, 1), scratch=None) == 1 and mark((0, 0, 5, 1, 1), scratch=ptr + 8) == 1
    assert mark((0, 0, 5, 1, 1), nbytes=8) == 1 and b"scratch" in L.h2_last_error()
    assert L.h2_dev_coverage_mark(planes.ctypes.data, 2, None, 1, ptr, words, ptr, 1 << 12, None) == 1
    assert L.h2_coverage_mark(planes.ctypes.data, 2, None, 1, ptr, words) == 1
    assert L.h2_dev_coverage_mark(None, 2, fake.ctypes.data, 1, ptr, words, ptr, 1 << 12, None) == 1
    assert L.h2_coverage_scratch_bytes(5, 0, 0, 0, 0) >= 5 * 16 + 2 * 6 * 8
    assert L.h2_coverage_scratch_bytes(0, 2, 3, 5, 1) >= 2 * 16 + 3 * 16 + 5 * 48 + 4 + 6 * 8
    assert mark((0, 0, 44, 1, 1), host=True) == 0 and fake[0] == 1 << 39 and not fake[1:].any()     # the last cell of plane 0
    fake[0] = 0

    good_use, good_query = (0, 0, 0, 1, 0, 0, 0, 1, 1), (0, 0, 0, 0)

    def run(use=good_use, query=good_query, earlier=(), n=n, bits=ptr, words=words, scratch=ptr, nbytes=1 << 12, count=ptr,
            records=ptr + 64, cap=4, host=False, uses=None):
        uses = np.array(uses or [use], dtype=syn.COVERAGE_USE)
        queries = np.array([query], dtype=syn.COVERAGE_QUERY)
        earlier = np.array(earlier, dtype=np.uint32)
        args = (planes.ctypes.data, len(planes), queries.ctypes.data, 1, uses.ctypes.data, len(uses), earlier.ctypes.data, len(earlier),
                n, bits, words)
        out = (count, records, cap)
        return L.h2_coverage_check(*(args + out)) if host else L.h2_dev_coverage_check(*(args + (scratch, nbytes) + out + (None,)))

    for host, name in ((False, b"h2_dev_coverage_check: "), (True, b"h2_coverage_check: ")):
        for bad in (dict(use=(0, 0, 0, 1, 0, 0, 64, 1, 1)), dict(use=(0, 0, 0, 1, 0, 0, 63, 1, 2)), dict(use=(0, 0, 0, 1, 0, 0, 0, 0, 2)),
                    dict(use=(0, 0, 0, 1, 0, 0, 1, 63, 2)), dict(use=(0, 1 << 16, 0, 1, 0, 0, 0, 1, 1)), dict(use=(0, 0, 0, 2, 0, 0, 0, 1, 1)),
                    dict(use=(0, 0, 1, 1, 0, 0, 0, 1, 1)), dict(use=(0, 0, 0, 1, 0, 1, 0, 1, 1)), dict(use=(0, 0, 0, 1, 0, 1, 0, 1, 1), earlier=[0]),
                    dict(query=(2, 0, 0, 0)), dict(query=(0, 0, 64, 0)), dict(query=(0, 0, -64, 0)), dict(n=0), dict(n=(1 << 31) + 1),
                    dict(bits=None), dict(bits=ptr + 1), dict(words=3), dict(count=None), dict(count=ptr + 4), dict(records=None)):
            assert run(host=host, **bad) == 1 and L.h2_last_error().startswith(name), bad
        assert run(uses=[good_use, (0, 0, 0, 1, 0, 1, 0, 1, 1)], earlier=[1], host=host) == 1       # an earlier use must be earlier
    assert run(scratch=None) == 1 and run(scratch=ptr + 8) == 1 and run(nbytes=16) == 1 and run(records=ptr + 8) == 1
    assert not fake.any()
    # and what is in order runs on the host: row 0 reads plane 0, whose rows begin at 5 -> one record; NO_PLANE: the same
    assert run(host=True) == 0 and run(query=(syn.COVERAGE_NO_PLANE, 0, 0, 0), host=True) == 0
    assert fake[0] == 2 and fake[8:12].view(np.uint32).tolist() == [4, 0, 0, 0, 4, 0, 0, 0]


def test_header_symbols_and_dtypes_agree():
    text = open(os.path.join(ROOT, "include", "halo2_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    L = h2.lib()
    names = ("h2_coverage_scratch_bytes", "h2_dev_coverage_mark", "h2_dev_coverage_check", "h2_coverage_mark", "h2_coverage_check")
    for name in names:
        declared = re.search(r"\b%s\s*\(([^)]*)\)" % name, text)
        assert declared and name in SYMBOLS and hasattr(L, name), name
        assert len(declared.group(1).split(",")) == len(SYMBOLS[name][1]), name
    assert sorted(n for n in SYMBOLS if "coverage" in n) == sorted(names)
    sizes = {"uint64_t": 8, "uint32_t": 4, "int32_t": 4}
    for struct, dtype, size in (("h2_coverage_plane", syn.COVERAGE_PLANE, 16), ("h2_coverage_segment", syn.COVERAGE_SEGMENT, 32),
                                ("h2_coverage_query", syn.COVERAGE_QUERY, 16), ("h2_coverage_use", syn.COVERAGE_USE, 48)):
        body = re.search(r"typedef struct \{([^}]*)\} %s;" % struct, text).group(1)
        fields = re.findall(r"(\w+)\s+(\w+);", body)
        assert [name for _, name in fields] == list(dtype.names), struct
        assert [sizes[kind] for kind, _ in fields] == [dtype[name].itemsize for name in dtype.names], struct
        assert dtype.itemsize == size == sum(sizes[kind] for kind, _ in fields), struct        # no padding on either side
    assert re.search(r"H2_CHECK_CELL = %d\b" % check.CHECK_CELL, text)
    assert re.search(r"#define H2_COVERAGE_NO_PLANE 0x%xu" % syn.COVERAGE_NO_PLANE, text)
    srcs = open(os.path.join(CSRC, "Makefile")).read()
    assert " coverage.hip " in srcs and " coverage.hpp " in srcs and "coverage_host.o" in srcs
    assert "hip/" not in open(os.path.join(CSRC, "coverage_host.cpp")).read() + open(os.path.join(CSRC, "coverage.hpp")).read()


def test_records_decode_to_named_failures_and_text():
    circuit = Hand([("first", abc([0, 1])), ("second", abc([4, 5], skip="c"))])
    cov = syn.synthesize_coverage(None, circuit, 4, resident=False)
    records = np.array([[4, 0 << 16 | 2, 1, 5], [4, 2, 1, 4], [4, 2, 1, 5], [0, 0, 0, 3]], dtype=np.uint32)
    cs = prover.synthesize_keygen(None, circuit, 4)[0]
    failures = check.check_failures(cs, records, cov)
    assert failures == [CellNotAssigned(0, "mul", 1, "second", ("advice", 2), 0, 4), CellNotAssigned(0, "mul", 1, "second", ("advice", 2), 1, 5),
                        check.ConstraintNotSatisfied(0, "mul", 0, 3, 0)]
    assert check._describe_failure(failures[1]) == \
        "region 1 'second' enables gate 0 'mul' over advice column 2 at offset 1 (row 5), a cell it never assigned"
    with pytest.raises(ValueError):
        check.check_failures(cs, records)
    words = np.concatenate([np.array([3, 0, 0, 0], dtype=np.uint32), records[:3].reshape(-1)])
    assert check.check_result(None, words, 3, cov) == (failures[:2], 3)
    assert prover.CellNotAssigned is CellNotAssigned and prover.check_assignments is check.check_assignments
    assert prover.check_circuit is check.check_circuit and prover.assert_circuit_satisfied is check.assert_circuit_satisfied
    assert prover.CHECK_CELL == 4 and prover.synthesize_coverage is syn.synthesize_coverage
    assert "CellNotAssigned" not in check.check_witness.__doc__ and "ConstraintPoisoned" in check.check_witness.__doc__


# -- the host code under the sanitizers ----------------------------------------------------------------------------------------
def test_coverage_host_under_the_sanitizers(tmp_path):
    """a stand-alone program: nothing is preloaded into Python"""
    exe = tmp_path / "coverage_host_main"
    cmd = ["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I", CSRC, os.path.join(ROOT, "tests", "coverage_host_main.cpp"), os.path.join(CSRC, "coverage_host.cpp"), "-o", str(exe)]
    built = subprocess.run(cmd, capture_output=True, text=True, timeout=240)
    assert built.returncode == 0, built.stderr[-4000:]
    ran = subprocess.run([str(exe), "400"], capture_output=True, text=True, timeout=120)
    assert ran.returncode == 0 and not ran.stderr and ran.stdout.split() == ["ok", "400"], (ran.returncode, ran.stderr[-3000:])
