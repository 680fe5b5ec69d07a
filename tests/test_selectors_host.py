"""Selectors on the host: the constraint system's selector objects and rules, compress_selectors against plans worked by hand
and against the property the reference's own proptest states (plonk/circuit/compress_selectors.rs:282-), the front end's
`enable_selector` under both planners, the binary form's selector_map, the two reference examples that need selectors, and the
argument checks of the device entry points -- none of which needs a GPU."""
import os
import re

import numpy as np
import pytest

import ref_plonk as rp
import halo2_gpu_specific_amd as h2
from halo2_gpu_specific_amd import circuit as hc, circuits, circuits_frontend as fe, cs_format, synthesis as syn
from halo2_gpu_specific_amd._lib import SYMBOLS
from halo2_gpu_specific_amd.circuit import ConstraintSystem
from halo2_gpu_specific_amd.transcript import R_MOD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def evaluate(e, cell):
    """an expression over big integers; cell(kind name, column, rotation) -> value"""
    if isinstance(e, hc.Constant):
        return e.v % R_MOD
    if isinstance(e, hc.Query):
        return cell(e.name, e.column, e.rotation)
    if isinstance(e, hc.Negated):
        return -evaluate(e.e, cell) % R_MOD
    if isinstance(e, hc.Scaled):
        return evaluate(e.e, cell) * e.c % R_MOD
    a, b = evaluate(e.a, cell), evaluate(e.b, cell)
    return (a + b if isinstance(e, hc.Sum) else a * b) % R_MOD


def ints(column):
    return [sum(int(x) << (64 * j) for j, x in enumerate(row)) for row in column]


def failing_rows(cs, k, advice, fixed, instances):
    """[(gate, polynomial, row)] of the gate polynomials that are non-zero on a usable row"""
    n = 1 << k
    cols = {"advice": [ints(c) for c in advice], "fixed": [ints(c) for c in fixed],
            "instance": [list(c) + [0] * (n - len(c)) for c in instances]}
    bad = []
    for g, (_, polys) in enumerate(cs.gates):
        for p, poly in enumerate(polys):
            for row in range(n - (cs.blinding_factors() + 1)):
                if evaluate(poly, lambda kind, column, rotation: cols[kind][column][(row + rotation) % n]):
                    bad.append((g, p, row))
    return bad


def selector_system(degrees, max_degree, complex_ones=()):
    """one advice column; selector i gates a^(degrees[i] - 1) (no gate for degree 0); the minimum degree pins cs.degree()"""
    cs = ConstraintSystem()
    a = cs.advice_column()
    selectors = [cs.complex_selector() if i in complex_ones else cs.selector() for i in range(len(degrees))]
    for sel, d in zip(selectors, degrees):
        if d:
            poly = cs.query_selector(sel)
            for _ in range(d - 1):
                poly = poly * cs.query_advice(a)
            cs.create_gate("g%d" % sel.index, [poly])
    cs.set_minimum_degree(max_degree)
    return cs, selectors


def no_conflicts(count):
    return [[0] * count for _ in range(count)]


# -- plans worked by hand ---------------------------------------------------------------------------------------------------------
def test_three_disjoint_selectors_share_two_columns():
    """degrees 2, 2, 2 and max_degree 3: selector 0 opens {0} with d = 1; selector 1 joins (1 + 1 + 1 <= 3), after which
    d + len = 3 closes the combination; selector 2 gets its own.  Substitutes q (2 - q), q (1 - q) and q."""
    cs, _ = selector_system([2, 2, 2], 3)
    assert cs.num_selectors == 3 and cs.degree() == 3
    combinations = cs.compress_selectors(no_conflicts(3))
    assert combinations == [[0, 1], [2]]
    assert cs.selector_map == [("fixed", 0), ("fixed", 0), ("fixed", 1)] and cs.num_fixed == 2 and cs.num_selectors == 3
    assert cs.fixed_queries == [(0, 0), (1, 0)]
    two, one = "0x%064x" % 2, "0x%064x" % 1
    assert [p.identifier() for _, polys in cs.gates for p in polys] == [
        "((fixed[0][0]*(%s+(-fixed[0][0])))*advice[0][0])" % two,
        "((fixed[0][0]*(%s+(-fixed[0][0])))*advice[0][0])" % one,
        "(fixed[1][0]*advice[0][0])"]
    # column 0 holds 1 on selector 0's rows and 2 on selector 1's
    host = syn.HostSelectors(3, 8)
    host.enable(0, 0, 2, 2)
    host.enable(1, 1, 1, 1)
    host.enable(2, 0, 1, 8)
    columns = host.combine(combinations)
    assert [int(v) for v in columns[0][:, 0]] == [1, 2, 1, 0, 0, 0, 0, 0] and not columns[0][:, 1:].any()
    assert [int(v) for v in columns[1][:, 0]] == [1] * 8
    with pytest.raises(ValueError):
        cs.compress_selectors(no_conflicts(3))                        # twice


def test_selectors_that_share_a_row_are_kept_apart():
    cs, _ = selector_system([2, 2, 2], 3)
    conflicts = no_conflicts(3)
    conflicts[0][1] = conflicts[1][0] = 1
    # selector 0 opens {0}; 1 conflicts; 2 joins (1 + 1 + 1 <= 3) -> {0, 2}, {1}: two columns.  With max_degree 2 nothing can
    # join anything (d + len = 1 + 1 = 2 closes every combination at once): three columns
    assert cs.compress_selectors(conflicts) == [[0, 2], [1]]
    cs, _ = selector_system([2, 2, 2], 2)
    assert cs.degree() == 3                                             # the permutation argument's floor
    plan, assignment = hc.compress_selectors_plan([(0, 2, {1}), (1, 2, {0}), (2, 2, set())], 2)
    assert plan == [[0], [1], [2]] and assignment == {0: (0, 1, 1), 1: (1, 1, 1), 2: (2, 1, 1)}
    host = syn.HostSelectors(3, 8)
    host.enable(0, 3, 1, 1)
    host.enable(1, 3, 1, 2)
    host.enable(2, 5, 1, 1)
    assert host.conflicts().tolist() == [[0, 1, 0], [1, 0, 0], [0, 0, 0]]


def test_complex_and_unused_selectors_get_columns_of_their_own_first():
    cs, selectors = selector_system([2, 2, 0, 0], 3, complex_ones=(2,))
    q = cs.query_advice(("advice", 0))
    cs.create_gate("complex", [cs.query_selector(selectors[2]) * q + q])           # a complex selector may be added
    assert cs.selector_degrees() == [2, 2, 0, 0]
    assert cs.compress_selectors(no_conflicts(4)) == [[2], [3], [0, 1]]
    assert cs.selector_map == [("fixed", 2), ("fixed", 2), ("fixed", 0), ("fixed", 1)]
    assert cs.gates[-1][1][0].identifier() == "((fixed[0][0]*advice[0][0])+advice[0][0])"


# -- the reference's proptest property -------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(40))
def test_compression_keeps_the_property_of_the_reference_proptest(seed):
    rng = np.random.Generator(np.random.PCG64(0xC0FFEE + seed))
    max_degree = int(rng.integers(3, 11))
    count, n = int(rng.integers(1, 13)), int(rng.integers(1, 25))
    degrees = [int(rng.integers(0, max_degree + 1)) for _ in range(count)]
    host = syn.HostSelectors(count, n)
    host.bits[:] = rng.random((count, n)) < rng.choice([0.05, 0.2, 0.6])
    cs, _ = selector_system(degrees, max_degree)
    assert cs.degree() == max_degree
    before = [p.degree() for _, polys in cs.gates for p in polys]
    combinations = cs.compress_selectors(host.conflicts())
    assert sorted(s for group in combinations for s in group) == list(range(count))
    columns = host.combine(combinations)
    assert len(columns) == cs.num_fixed
    for group in combinations:
        for i in group:                                                 # members are pairwise disjoint
            for j in group:
                assert i == j or not (host.bits[i] & host.bits[j]).any()
        if len(group) > 1 or degrees[group[0]]:
            assert max(degrees[s] for s in group) - 1 + len(group) <= max_degree
    # a selector's substitute, on its column's value, is non-zero exactly on its activations
    for s in range(count):
        column = [int(v) for v in columns[cs.selector_map[s][1]][:, 0]]
        root = combinations[cs.selector_map[s][1]].index(s) + 1
        substitute = hc.substitute_expression(hc.Fixed(0, 0), root, len(combinations[cs.selector_map[s][1]]))
        for row in range(n):
            assert (evaluate(substitute, lambda *_: column[row]) != 0) == bool(host.bits[s, row])
    after = [p.degree() for _, polys in cs.gates for p in polys]
    assert len(after) == len(before) and all(d <= max_degree for d in after) and cs.degree() == max_degree
    assert not any(hc.contains_selector(p) for _, polys in cs.gates for p in polys)


# -- the rules ---------------------------------------------------------------------------------------------------------------
def test_simple_selector_rules_are_typed_errors():
    cs = ConstraintSystem()
    a = cs.query_advice(cs.advice_column())
    s, t, c = cs.query_selector(cs.selector()), cs.query_selector(cs.selector()), cs.query_selector(cs.complex_selector())
    assert s.degree() == 1 and s.identifier() == "selector[0]" and c.identifier() == "selector[2]"
    for bad in (lambda: s + a, lambda: a + s, lambda: a - s, lambda: s - a, lambda: (s * a) + 1, lambda: 1 + s * a):
        with pytest.raises(hc.SelectorInSum):
            bad()
    for bad in (lambda: s * t, lambda: (s * a) * (a * t), lambda: s * s):
        with pytest.raises(hc.SelectorProduct):
            bad()
    assert issubclass(hc.SelectorInSum, ValueError) and issubclass(hc.SelectorProduct, ValueError)
    assert issubclass(hc.SelectorInArgument, ValueError)
    table = cs.query_fixed(cs.fixed_column())
    for bad in (lambda: cs.lookup("l", [(s * a, table)]), lambda: cs.lookup("l", [(a, s * table)]),
                lambda: cs.lookup_any("l", [table], [[[s * a]]]), lambda: cs.shuffle("s", [(s * a, a)]),
                lambda: cs.shuffle("s", [(a, s * a)]), lambda: cs.shuffle_group([("s", [s * a], [a])])):
        with pytest.raises(hc.SelectorInArgument):
            bad()
    cs.lookup("l", [(c * a, table)])                                   # complex selectors may go anywhere
    assert (c * a + a).degree() == 2 and (c * c).degree() == 2 and (s * 3).degree() == 1
    assert hc.extract_simple_selector(s * (a * a)) == hc.Selector(0, True)
    assert hc.extract_simple_selector(c * a) is None and hc.extract_simple_selector(a * a) is None
    assert hc.extract_simple_selector(c * (a * t)) == hc.Selector(1, True)
    with pytest.raises(hc.SelectorProduct):
        hc.extract_simple_selector(hc.Product(s, t))                   # built past the operators
    with pytest.raises(TypeError):
        cs.query_selector(hc.Selector(9, True))


def test_evaluators_refuse_a_selector_that_was_not_compiled_away():
    from halo2_gpu_specific_amd import verifier

    cs = ConstraintSystem()
    a = cs.query_advice(cs.advice_column())
    poly = cs.query_selector(cs.selector()) * a
    cs.create_gate("g", [poly])
    for compile_ in (lambda: hc.compile_gates(cs), lambda: hc.compile_evaluator(cs), lambda: hc.compile_compress([poly]),
                     lambda: verifier._evaluate(poly, None, None, None), lambda: cs_format.cs_store(cs)):
        with pytest.raises(hc.SelectorNotCompiled):
            compile_()
    cs.compress_selectors([[0]])
    hc.compile_gates(cs)
    cs_format.cs_store(cs)


# -- the front end --------------------------------------------------------------------------------------------------------------
class _SharedSelector(syn.Circuit):
    """two regions of two rows that use different advice columns and, with `shared`, the same selector"""
    planner = syn.V1

    def __init__(self, shared):
        self.shared = shared

    def without_witnesses(self):
        return self

    def configure(self, cs):
        a, b = cs.advice_column(), cs.advice_column()
        s = cs.selector()
        cs.create_gate("g", [cs.query_selector(s) * cs.query_advice(a) * cs.query_advice(b)])
        return a, b, s

    def synthesize(self, config, layouter):
        a, b, s = config

        def region(column):
            def body(region):
                region.assign_advice(column, 0, 0, count=2)
                if self.shared:
                    s.enable(region, 0)
            return body

        layouter.assign_region("first", region(a))
        layouter.assign_region("second", region(b))


def test_v1_keeps_regions_that_share_only_a_selector_apart():
    """equal areas: the region declared last is placed first, at row 0; the other one's advice column is free from row 0, its
    selector only from row 2 (v1/strategy.rs:107-161 over the columns in RegionColumn's order)"""
    assert syn.region_starts(_SharedSelector(False)) == [0, 0]
    assert syn.region_starts(_SharedSelector(True)) == [2, 0]
    cs, fixed, _ = syn.synthesize_keygen(None, _SharedSelector(True), 4)
    assert [int(v) for v in fixed[0][:, 0]] == [1, 0, 1] + [0] * 13
    assert sorted([("selector", 1), ("fixed", 7), ("advice", 3), ("selector", 0), ("instance", 9)], key=syn._column_key) == [
        ("instance", 9), ("advice", 3), ("fixed", 7), ("selector", 0), ("selector", 1)]


def test_enable_selector_rows_and_the_witness_pass():
    class Late(_SharedSelector):
        def synthesize(self, config, layouter):
            layouter.assign_region("r", lambda region: region.enable_selector(config[2], self.shared))

    k = 4
    usable = 16 - 6
    cs, fixed, _ = syn.synthesize_keygen(None, Late(usable - 1), k)
    assert np.flatnonzero(fixed[0][:, 0]).tolist() == [usable - 1]
    with pytest.raises(syn.NotEnoughRowsAvailable):
        syn.synthesize_keygen(None, Late(usable), k)
    with pytest.raises(syn.NotEnoughRowsAvailable):
        syn.synthesize_keygen(None, Late(usable), k, planner=syn.FlatFloorPlanner)
    # the witness pass ignores the call (and its row), and accepts the compressed constraint system as the circuit's own
    advice, _ = syn.synthesize_witness(None, Late(usable), cs, k, planner=syn.FlatFloorPlanner, resident=False)
    assert len(advice) == 2 and cs.num_fixed == 1
    with pytest.raises(ValueError):
        syn.synthesize_witness(None, fe.TwoChip(), cs, k, resident=False)


def test_bulk_enable_is_strided_and_idempotent():
    host = syn.HostSelectors(2, 40)
    host.enable(0, 30, 3, 3)
    host.enable(0, 33, 1, 1)
    host.enable(1, 0, 1, 0)
    assert np.flatnonzero(host.bits[0]).tolist() == [30, 33, 36] and not host.bits[1].any()
    words = host.bitmaps()
    assert words.shape == (2, 2) and words.dtype == np.dtype("<u4")
    assert [int(w) for w in words[0]] == [1 << 30, (1 << 1) | (1 << 4)]


# -- the binary form ----------------------------------------------------------------------------------------------------------------
def test_cs_store_carries_the_selector_map():
    cs, fixed, _ = syn.synthesize_keygen(None, fe.SelectorGates(6), 6)
    blob = cs_format.cs_store(cs)
    words = np.frombuffer(blob[:20 + 4 * cs.num_advice + 4 + 4 * cs.num_selectors], dtype="<u4").tolist()
    assert words[:5] == [3, 0, 5, 5, 3]                                 # advice, instance, SELECTORS, fixed, advice again
    assert words[5 + cs.num_advice:] == [5, 3, 3, 4, 1, 2]              # selector_map: a count and the columns
    back = cs_format.cs_fetch(cs_format._Reader(blob))
    assert back.num_selectors == 5 and back.selector_map == cs.selector_map and cs_format.cs_store(back) == blob
    syn.synthesize_witness(None, fe.SelectorGates(6), back, 6, resident=False)     # the probe knows the declared columns
    # a selector count without its map is refused still
    live = blob[:8] + (5).to_bytes(4, "little") + blob[12:20 + 4 * cs.num_advice] + (0).to_bytes(4, "little") + \
        blob[20 + 4 * cs.num_advice + 4 + 4 * cs.num_selectors:]
    with pytest.raises(IOError):
        cs_format.cs_fetch(cs_format._Reader(live))


def test_cs_store_of_a_circuit_without_selectors_is_unchanged():
    """against the independent writer of tests/ref_plonk.py, which knows nothing of selectors"""
    assert cs_format.cs_store(circuits.mini_plonk()) == rp.MiniPlonk.cs_bytes()
    assert cs_format.cs_store(circuits.lookup_api()) == rp.LookupApi.cs_bytes()
    cs, _, _ = syn.synthesize_keygen(None, fe.ShuffleApi(), 6)
    assert cs.num_selectors == 0 and cs.selector_map == [] and cs_format.cs_store(cs) == rp.ShuffleApi.cs_bytes()


# -- the two examples ---------------------------------------------------------------------------------------------------------------
def test_simple_example_on_the_host_assembly():
    k, circuit = 4, fe.SimpleExample()
    cs, fixed, copies = syn.synthesize_keygen(None, circuit, k)
    assert syn.region_starts(circuit) == [8, 7, 6, 4, 2, 0]            # equal areas: the last region declared comes first
    assert (cs.num_advice, cs.num_fixed, cs.num_instance, cs.num_selectors) == (2, 2, 1, 1)
    assert cs.selector_map == [("fixed", 1)] and cs.constants == [("fixed", 0)]
    assert [int(v) for v in fixed[1][:, 0]] == [1, 0, 1, 0, 1] + [0] * 11          # the three mul regions
    assert ints(fixed[0]) == [7] + [0] * 15                             # no region uses the constants column: its row 0 is free
    assert len(copies) == 2 * 3 + 1 + 1                                 # two copy_advice per mul, the constant, the instance
    instances = circuit.public_inputs()
    assert instances == [[7 * 4 * 9]]
    advice, _ = syn.synthesize_witness(None, circuit, cs, k, resident=False, instances=instances)
    assert failing_rows(cs, k, advice, fixed, instances) == []
    assert int(advice[0][1, 0]) == 252                                  # c, next to the last multiplication
    advice[0][1, 0] += np.uint64(1)
    assert failing_rows(cs, k, advice, fixed, instances) == [(0, 0, 0)]
    advice[0][1, 0] -= np.uint64(1)
    advice[1][1, 0] = np.uint64(99)                                     # a cell no enabled row reads
    assert failing_rows(cs, k, advice, fixed, instances) == []


def test_two_chip_on_the_host_assembly():
    k, circuit = 4, fe.TwoChip(5, 6, 7)
    cs, fixed, copies = syn.synthesize_keygen(None, circuit, k)
    assert syn.region_starts(circuit) == [6, 5, 4, 2, 0]
    assert (cs.num_advice, cs.num_fixed, cs.num_instance, cs.num_selectors) == (2, 2, 1, 2)
    assert cs.selector_map == [("fixed", 0), ("fixed", 1)]              # degree 3 gates under max_degree 3: nothing combines
    assert np.flatnonzero(fixed[0][:, 0]).tolist() == [2] and np.flatnonzero(fixed[1][:, 0]).tolist() == [0]
    assert len(copies) == 2 * 2 + 1
    instances = circuit.public_inputs()
    assert instances == [[77]]
    advice, _ = syn.synthesize_witness(None, circuit, cs, k, resident=False, instances=instances)
    assert failing_rows(cs, k, advice, fixed, instances) == []
    assert [int(v) for v in advice[0][:4, 0]] == [11, 77, 5, 11] and [int(v) for v in advice[1][:3, 0]] == [7, 0, 6]
    advice[0][3, 0] = np.uint64(12)                                     # a + b, under the add selector of row 2
    assert failing_rows(cs, k, advice, fixed, instances) == [(0, 0, 2)]


def test_selector_gates_circuit_is_satisfied_and_combines_as_its_docstring_says():
    k, circuit = 6, fe.SelectorGates(6)
    cs, fixed, copies = syn.synthesize_keygen(None, circuit, k)
    assert cs.degree() == 5 and cs.selector_map == [("fixed", 3), ("fixed", 3), ("fixed", 4), ("fixed", 1), ("fixed", 2)]
    rows = np.arange(56)
    want = [(rows % 8 == 0).astype(int), np.where(rows % 4 == 0, 1, np.where(rows % 4 == 3, 1, 0)),     # s_idle, then s_tab
            np.where(rows % 4 == 0, 1, np.where((rows % 4 == 1) | (rows % 4 == 2), 2, 0)), (rows % 4 == 2).astype(int)]
    for column, values in zip(fixed[1:], want):
        assert [int(v) for v in column[:56, 0]] == values.tolist() and not column[56:].any() and not column[:, 1:].any()
    advice, _ = syn.synthesize_witness(None, circuit, cs, k, resident=False)
    assert failing_rows(cs, k, advice, fixed, []) == []
    assert all(int(advice[0][r, 0]) < 16 for r in range(56) if r % 4 in (0, 3))
    assert len(copies) == 1


# -- the library's side, without a GPU ----------------------------------------------------------------------------------------
def _tables(combinations, columns, montgomery=False):
    return syn.selector_plan_tables(combinations, [c.ctypes.data for c in columns], montgomery)


@pytest.mark.parametrize("montgomery", [False, True])
def test_host_twin_of_combine_matches_numpy(montgomery):
    L = h2.lib()
    rng = np.random.Generator(np.random.PCG64(7))
    n, count = 77, 40
    host = syn.HostSelectors(count, n)
    owner = rng.integers(0, 60, size=n)                                  # at most one selector per row: anything may combine
    for s in range(count):
        host.bits[s] = owner == s
    combinations = [[3], list(range(4, 23)) + [0, 1, 2], [], list(range(23, 40))]        # 22 members: two slices of 16
    want = host.combine(combinations)
    if montgomery:
        want = [np.array([syn._limbs((int(v) << 256) % R_MOD) for v in column[:, 0]], dtype=np.uint64) for column in want]
    columns = [np.full((n, 4), 0xDEAD, dtype=np.uint64) for _ in combinations]
    plan, members = _tables(combinations, columns, montgomery)
    words = host.bitmaps()
    rc = L.h2_selectors_combine(plan.ctypes.data, len(plan), members.ctypes.data, len(members), n, count, words.ctypes.data,
                                int(montgomery))
    assert rc == 0, L.h2_last_error()
    for got, expect in zip(columns, want):
        assert np.array_equal(got, expect)


def test_entry_points_check_their_arguments_before_any_launch():
    L = h2.lib()
    n, count = 64, 3
    fake = np.zeros(64, dtype=np.uint64)                                 # an aligned address nothing is launched on
    ptr = fake.ctypes.data
    assert ptr % 16 == 0

    def mark(selector, first, stride, rows, n=n, count=count, bitmaps=ptr, scratch=ptr, nbytes=1 << 12):
        segs = np.array([(selector, 0, first, stride, rows)], dtype=syn.SELECTOR_SEGMENT)
        return L.h2_dev_selectors_mark(segs.ctypes.data, 1, n, count, bitmaps, scratch, nbytes, None)

    place = np.array([(ptr, ptr, 60, 1, 5, 0, 0)], dtype=syn.PLACE_SEGMENT)
    bad_segment = L.h2_dev_cells_place(place.ctypes.data, 1, n, 0, ptr, 1 << 12, None)
    assert bad_segment == 1                                              # H2_ERR_INVALID: what a bad segment gives there
    for args in ((0, 60, 1, 5), (0, 64, 1, 1), (0, 0, 0, 2), (3, 0, 1, 1), (0, 1, 63, 3), (0, 0, 65, 2)):
        assert mark(*args) == bad_segment and b"h2_dev_selectors_mark" in L.h2_last_error(), args
    assert mark(0, 0, 1, 1, n=0) == 1 and mark(0, 0, 1, 1, count=0) == 1 and mark(0, 0, 1, 1, count=1 << 16) == 1
    assert mark(0, 0, 1, 1, bitmaps=None) == 1 and mark(0, 0, 1, 1, scratch=None) == 1 and mark(0, 0, 1, 1, scratch=ptr + 8) == 1
    assert mark(0, 0, 1, 1, nbytes=8) == 1
    assert L.h2_selectors_mark_scratch_bytes(5) >= 5 * 16 + 6 * 8
    assert L.h2_dev_selectors_mark(None, 1, n, count, ptr, ptr, 1 << 12, None) == 1

    assert L.h2_dev_selectors_conflicts(None, count, n, ptr, None) == 1
    assert L.h2_dev_selectors_conflicts(ptr, count, n, None, None) == 1
    assert L.h2_dev_selectors_conflicts(ptr, 0, n, ptr, None) == 1
    assert L.h2_dev_selectors_conflicts(ptr, 1 << 16, n, ptr, None) == 1
    assert L.h2_dev_selectors_conflicts(ptr, count, (1 << 31) + 1, ptr, None) == 1
    assert b"h2_dev_selectors_conflicts" in L.h2_last_error()

    column = np.zeros((n, 4), dtype=np.uint64)

    def combine(plan, members, form=0, count=count, bitmaps=ptr, host=False):
        plan = np.array(plan, dtype=syn.SELECTOR_COLUMN)
        members = np.array(members, dtype=syn.SELECTOR_MEMBER)
        args = (plan.ctypes.data, len(plan), members.ctypes.data if len(members) else None, len(members), n, count, bitmaps, form)
        return L.h2_selectors_combine(*args) if host else L.h2_dev_selectors_combine(*(args + (None,)))

    one = ([1, 0, 0, 0], 0, 0)
    modulus = ([(R_MOD >> (64 * j)) & (2 ** 64 - 1) for j in range(4)], 0, 0)
    for host in (False, True):
        assert combine([(column.ctypes.data, 0, 1)], [([1, 0, 0, 0], 3, 0)], host=host) == 1           # selector 3 of 3
        assert combine([(column.ctypes.data, 0, 2)], [one], host=host) == 1                            # members past the table
        assert combine([(column.ctypes.data, 1, 1)], [one], host=host) == 1
        assert combine([(column.ctypes.data + 8, 0, 1)], [one], host=host) == 1                        # misaligned column
        assert combine([(0, 0, 1)], [one], host=host) == 1
        assert combine([(column.ctypes.data, 0, 1)], [one], form=2, host=host) == 1
        assert combine([(column.ctypes.data, 0, 1)], [modulus], host=host) == 1                        # not below the modulus
        assert combine([(column.ctypes.data, 0, 1)], [one], bitmaps=None, host=host) == 1
        assert combine([(column.ctypes.data, 0, 1)], [one], count=0, host=host) == 1
    assert b"h2_selectors_combine" in L.h2_last_error() and not column.any()


def test_header_declares_the_selector_entry_points():
    text = open(os.path.join(ROOT, "include", "halo2_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    L = h2.lib()
    names = ("h2_selectors_mark_scratch_bytes", "h2_dev_selectors_mark", "h2_dev_selectors_conflicts",
             "h2_dev_selectors_combine", "h2_selectors_combine")
    for name in names:
        assert re.search(r"\b%s\s*\(" % name, text) and name in SYMBOLS and hasattr(L, name), name
    assert sorted(n for n in SYMBOLS if "selectors" in n) == sorted(names)
    for struct, dtype in (("h2_selector_segment", syn.SELECTOR_SEGMENT), ("h2_selector_column", syn.SELECTOR_COLUMN),
                          ("h2_selector_member", syn.SELECTOR_MEMBER)):
        body = re.search(r"typedef struct \{([^}]*)\} %s;" % struct, text).group(1)
        fields = re.findall(r"(\w+)(?:\[\d+\])?;", body)
        assert fields == list(dtype.names), struct
    assert syn.SELECTOR_SEGMENT.itemsize == 32 and syn.SELECTOR_COLUMN.itemsize == 16 and syn.SELECTOR_MEMBER.itemsize == 40
