"""The circuit front end on the host assembly (synthesis.py, circuits_frontend.py): every front-end circuit lays out exactly
what its hand-laid twin of circuits.py does; V1 and FlatFloorPlanner place regions and constants where a hand computation of
v1/strategy.rs and flat.rs puts them; every typed error has its smallest trigger; constants columns reach the verifying
key's digest preimage and leave the digest of a circuit without them alone."""
import json
import os
import struct

import numpy as np
import pytest

import ref_plonk as rp
from halo2_gpu_specific_amd import circuits, circuits_frontend as fe, cs_format, synthesis as syn
from halo2_gpu_specific_amd.circuit import ConstraintSystem
from halo2_gpu_specific_amd.domain import Domain
from halo2_gpu_specific_amd.keygen import permutation_mapping
from halo2_gpu_specific_amd.transcript import Q_MOD, R_MOD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = 8

TWINS = {
    "mini_plonk": lambda: (fe.MiniPlonk(K), circuits.mini_plonk(), circuits.mini_plonk_synthesize(K)),
    "lookup_api": lambda: (fe.LookupApi(), circuits.lookup_api(), circuits.lookup_api_synthesize(K)),
    "lookup_api_set": lambda: (fe.LookupApiSet(), circuits.lookup_api_set(), circuits.lookup_api_set_synthesize(K)),
    "range_check": lambda: (fe.RangeCheck(K, vmax=63, count=100), circuits.range_check(0, 63, 2),
                            circuits.range_check_synthesize(K, vmax=63, count=100)),
    "shuffle_gates": lambda: (fe.ShuffleGates(K), circuits.shuffle_gates(), circuits.shuffle_gates_synthesize(K)),
    "shuffle_api": lambda: (fe.ShuffleApi(), circuits.shuffle_api(), circuits.shuffle_api_synthesize(K)),
    "shuffle_api_group": lambda: (fe.ShuffleApiGroup(), circuits.shuffle_api_group(), circuits.shuffle_api_group_synthesize(K)),
    "wide": lambda: (fe.Wide(K, 2), circuits.wide(2), circuits.wide_synthesize(K, 2)),
}


def columns_equal(mine, theirs):
    return len(mine) == len(theirs) and all(np.array_equal(a, b) for a, b in zip(mine, theirs))


@pytest.mark.parametrize("name", sorted(TWINS))
def test_front_end_circuit_reproduces_its_hand_laid_twin(name):
    circuit, twin_cs, (twin_advice, twin_fixed, twin_copies) = TWINS[name]()
    cs, fixed, copies = syn.synthesize_keygen(None, circuit, K)
    assert cs_format.cs_store(cs) == cs_format.cs_store(twin_cs)
    assert columns_equal(fixed, twin_fixed)                              # the table's default fill included
    ncols, n = len(cs.perm_columns), 1 << K
    if ncols:
        assert columns_equal(permutation_mapping(ncols, n, copies), permutation_mapping(ncols, n, twin_copies))
    else:
        assert len(copies) == 0 and len(twin_copies) == 0
    advice, first_unassigned = syn.synthesize_witness(None, circuit, cs, K, resident=False)
    assert columns_equal(advice, twin_advice)
    # first_unassigned = 1 + the last assigned row, per column: for these circuits, 1 + the last non-zero row of the twin
    for index, column in enumerate(twin_advice):
        used = np.flatnonzero(column.any(axis=1))
        if index in first_unassigned:
            assert len(used) == 0 or first_unassigned[index] >= used[-1] + 1
        else:
            assert len(used) == 0


def test_lookup_table_default_fill_is_the_columns_first_value():
    class Offset(fe.LookupApi):
        def without_witnesses(self):
            return self

        def synthesize(self, config, layouter):
            layouter.assign_table("t", lambda t: t.assign_cell(config.table, 0, np.arange(5, 9, dtype=np.uint64)))

    _, fixed, _ = syn.synthesize_keygen(None, Offset(), K)
    usable = (1 << K) - 6
    assert fixed[2][:usable, 0].tolist() == [5, 6, 7, 8] + [5] * (usable - 4) and not fixed[2][usable:].any()


def test_first_unassigned_is_one_past_the_last_assigned_row():
    circuit = fe.RangeCheck(K, vmax=63, count=100)
    cs, _, _ = syn.synthesize_keygen(None, circuit, K)
    _, first_unassigned = syn.synthesize_witness(None, circuit, cs, K, resident=False)
    assert first_unassigned == {0: 100}                                  # the companion column is never assigned
    circuit = fe.MiniPlonk(K)
    cs, _, _ = syn.synthesize_keygen(None, circuit, K)
    _, first_unassigned = syn.synthesize_witness(None, circuit, cs, K, resident=False)
    assert first_unassigned == {0: 32, 1: 32, 2: 32}                     # 2^(K-4) pairs: rows 0 .. 31


def test_assigned_cells_slice_like_ranges():
    cells = syn.AssignedCells(("advice", 0), 10, 8, 2)
    assert cells.rows().tolist() == list(range(10, 26, 2))
    assert cells[1:4].rows().tolist() == [12, 14, 16] and cells[::3].rows().tolist() == [10, 16, 22]
    assert cells[-1].rows().tolist() == [24] and len(cells[2:]) == 6


# ---- planners on hand-computed cases --------------------------------------------------------------------------------------
class Plan(syn.Circuit):
    """`regions`: [(columns, rows)]; every column of a region is assigned on all its rows.  Two advice and two fixed columns
    more than the regions name exist; advice 0 and the constants column fixed 0 are in the permutation."""
    planner = syn.V1

    def __init__(self, regions, constants=(), planner=syn.V1, constant_columns=1):
        self.regions, self.constants, self.planner, self.constant_columns = regions, constants, planner, constant_columns

    def without_witnesses(self):
        return self

    def configure(self, cs):
        advice = [cs.advice_column() for _ in range(3)]
        fixed = [cs.fixed_column() for _ in range(2)]
        cs.enable_equality(advice[0])
        cs.enable_equality(advice[1])
        for column in fixed[:self.constant_columns]:
            cs.enable_constant(column)
        return advice, fixed

    def synthesize(self, config, layouter):
        for index, (columns, rows) in enumerate(self.regions):
            def body(region, columns=columns, rows=rows, index=index):
                for column in columns:
                    if column[0] == "advice":
                        region.assign_advice(column, 0, np.full(rows, 100 + index, dtype=np.uint64))
                    else:
                        region.assign_fixed(column, 0, np.full(rows, 200 + index, dtype=np.uint64))
                for at, column, offset, value in self.constants:
                    if at == index:
                        region.assign_advice_from_constant(column, offset, value)
            layouter.assign_region("region %d" % index, body)


A0, A1, A2, F0, F1 = ("advice", 0), ("advice", 1), ("advice", 2), ("fixed", 0), ("fixed", 1)


@pytest.mark.parametrize("regions,starts", [
    ([([A0], 3), ([A0], 2)], [0, 3]),                                     # two regions sharing a column stack
    ([([A0], 3), ([A1], 2)], [0, 0]),                                     # disjoint columns share rows
    # areas 30, 10, 20: region 0 first (rows 0 .. 14 of a0, a1), then region 2 (a0 is free from 15: rows 15 .. 24 of a0, a2),
    # then region 1 drops into the gap rows 0 .. 14 of a2 left above region 2
    ([([A0, A1], 15), ([A2], 10), ([A2, A0], 10)], [0, 0, 15]),
    ([([A0], 2), ([A0], 2)], [2, 0]),                                     # equal areas: the region declared last goes first
    ([([A0], 2), ([A0], 2), ([A0], 3)], [5, 3, 0]),
    ([([F0], 4), ([A0], 1)], [0, 0]),                                     # a region without advice has area 0, and still a place
])
def test_v1_places_regions_as_computed_by_hand(regions, starts):
    assert syn.region_starts(Plan(regions)) == starts
    cs, fixed, _ = syn.synthesize_keygen(None, Plan(regions), 6)
    advice, _ = syn.synthesize_witness(None, Plan(regions), cs, 6, resident=False)
    for index, ((columns, rows), start) in enumerate(zip(regions, starts)):
        for kind, column in columns:
            got = (advice if kind == "advice" else fixed)[column][start:start + rows, 0]
            assert got.tolist() == [(100 if kind == "advice" else 200) + index] * rows


def test_free_intervals_and_first_fit_follow_the_strategy():
    allocations = {2: 3, 8: 2}                                           # rows 2 .. 4 and 8 .. 9 are taken
    assert list(syn.free_intervals(allocations, 0, None)) == [(0, 2), (5, 8), (10, None)]
    assert list(syn.free_intervals(allocations, 3, 9)) == [(5, 8)]
    assert list(syn.free_intervals(allocations, 0, 12)) == [(0, 2), (5, 8), (10, 12)]
    assert list(syn.free_intervals({}, 4, None)) == [(4, None)]
    columns = {A0: dict(allocations), A1: {0: 6}}
    assert syn.first_fit_region(columns, [A0, A1], 2, 0, None) == 6     # rows 0 .. 1 of a0 are free, a1 only from 6 on
    assert columns[A0][6] == 2 and columns[A1][6] == 2


def test_v1_puts_constants_into_the_free_rows_of_the_constants_column():
    # areas: region 0 = 1 x 2, region 1 = 1 x 3 -> region 1 at rows 0 .. 2 of a0; region 0 (a0, f0) at rows 3 .. 4.  The
    # first unassigned row is 5 and f0 is free on rows 0 .. 2: the constants of (a0, row 0) and (a0, row 2) take rows 0 and 1.
    circuit = Plan([([A0, F0], 2), ([A0], 3)], constants=[(1, A0, 2, 77), (1, A0, 0, 55)])
    assert syn.region_starts(circuit) == [3, 0]
    cs, fixed, copies = syn.synthesize_keygen(None, circuit, 6)
    assert fixed[0][:6, 0].tolist() == [55, 77, 0, 200, 200, 0]
    f0, a0 = cs.perm_columns.index(F0), cs.perm_columns.index(A0)
    assert sorted(copies.tolist()) == [[f0, 0, a0, 0], [f0, 1, a0, 2]]
    advice, _ = syn.synthesize_witness(None, circuit, cs, 6, resident=False)
    assert advice[0][:5, 0].tolist() == [55, 101, 77, 100, 100]          # the later assignment of a cell wins
    # one constant too many for the three free cells
    crowded = Plan([([A0, F0], 2), ([A0], 3)], constants=[(1, A0, i % 3, 9) for i in range(4)])
    with pytest.raises(syn.NotEnoughColumnsForConstants):
        syn.synthesize_keygen(None, crowded, 6)


def test_flat_puts_constants_at_the_top_of_the_first_constants_column():
    circuit = Plan([([A2], 1)], constants=[(0, A1, 5, 31), (0, A0, 7, 32), (0, A0, 2, 33)], planner=syn.FlatFloorPlanner,
                   constant_columns=2)
    cs, fixed, copies = syn.synthesize_keygen(None, circuit, 6)
    assert fixed[0][:4, 0].tolist() == [33, 32, 31, 0] and not fixed[1].any()      # by (column, row) of the advice cell
    f0, a0, a1 = (cs.perm_columns.index(c) for c in (F0, A0, A1))
    assert copies.tolist() == [[f0, 0, a0, 2], [f0, 1, a0, 7], [f0, 2, a1, 5]]
    # proving ignores fixed cells and copies; the advice cells carry the constants
    advice, _ = syn.synthesize_witness(None, circuit, cs, 6, resident=False)
    assert (advice[0][2, 0], advice[0][7, 0], advice[1][5, 0]) == (33, 32, 31)


def test_instance_cells_are_copied_and_tied():
    class Public(syn.Circuit):
        planner = syn.V1

        def without_witnesses(self):
            return self

        def configure(self, cs):
            a, inst = cs.advice_column(), cs.instance_column()
            cs.enable_equality(a)
            cs.enable_equality(inst)
            return a, inst

        def synthesize(self, config, layouter):
            a, inst = config

            def body(region):
                cell, value = region.assign_advice_from_instance(inst, 2, a, 1)
                return cell, value, region.assign_advice(a, 3, np.array([8, 9], dtype=np.uint64))

            self.cell, self.value, tail = layouter.assign_region("public", body)
            layouter.constrain_instance(tail, inst, 0)

    circuit = Public()
    cs, _, copies = syn.synthesize_keygen(None, circuit, 6)
    a, inst = cs.perm_columns.index(("advice", 0)), cs.perm_columns.index(("instance", 0))
    assert copies.tolist() == [[a, 1, inst, 2], [a, 3, inst, 0], [a, 4, inst, 1]] and circuit.value is None
    advice, first_unassigned = syn.synthesize_witness(None, circuit, cs, 6, resident=False, instances=[[8, 9, 77]])
    assert advice[0][:5, 0].tolist() == [0, 77, 0, 8, 9] and circuit.value == 77 and first_unassigned == {0: 5}
    assert circuit.cell.rows().tolist() == [1]
    with pytest.raises(syn.SynthesisError):
        syn.synthesize_witness(None, circuit, cs, 6, resident=False)          # no instance values to take the cell from


# ---- typed errors, each by its smallest trigger -----------------------------------------------------------------------------
def usable_rows(k):
    return (1 << k) - 6                                                  # blinding_factors() = 5 for these circuits


@pytest.mark.parametrize("planner", [syn.FlatFloorPlanner, syn.V1])
def test_a_cell_at_the_first_unusable_row_is_not_enough_rows(planner):
    k = 4
    last_ok = Plan([([A0], 1)], constants=[(0, A0, usable_rows(k) - 1, 1)], planner=planner)
    syn.synthesize_keygen(None, last_ok, k)
    beyond = Plan([([A0], 1)], constants=[(0, A0, usable_rows(k), 1)], planner=planner)
    with pytest.raises(syn.NotEnoughRowsAvailable) as err:
        syn.synthesize_keygen(None, beyond, k)
    assert err.value.current_k == k
    cs, _, _ = syn.synthesize_keygen(None, last_ok, k)
    with pytest.raises(syn.NotEnoughRowsAvailable):
        syn.synthesize_witness(None, Plan([([A0], usable_rows(k) + 1)], planner=planner), cs, k, resident=False)


def test_a_constant_without_a_constants_column():
    with pytest.raises(syn.NotEnoughColumnsForConstants):
        syn.synthesize_keygen(None, Plan([([A0], 1)], constants=[(0, A0, 0, 1)], planner=syn.FlatFloorPlanner, constant_columns=0), 6)
    with pytest.raises(syn.NotEnoughColumnsForConstants):
        syn.synthesize_keygen(None, Plan([([A0], 1)], constants=[(0, A0, 0, 1)], constant_columns=0), 6)


def test_a_copy_on_a_column_outside_the_permutation():
    class Copy(Plan):
        def synthesize(self, config, layouter):
            def body(region):
                left = region.assign_advice(A0, 0, 1)
                right = region.assign_advice(A2, 0, 1)                   # a2 was never given to enable_equality
                region.constrain_equal(left, right)
            layouter.assign_region("copy", body)

    with pytest.raises(syn.ColumnNotInPermutation) as err:
        syn.synthesize_keygen(None, Copy([]), 6)
    assert err.value.column == A2


def test_a_column_the_constraint_system_does_not_have():
    class Stray(Plan):
        def synthesize(self, config, layouter):
            layouter.assign_region("stray", lambda region: region.assign_fixed(("fixed", 2), 0, 1))

    with pytest.raises(syn.BoundsFailure):
        syn.synthesize_keygen(None, Stray([], planner=syn.FlatFloorPlanner), 6)


@pytest.mark.parametrize("misuse", ["hole", "no row 0", "row 0 twice", "lengths", "two tables", "empty"])
def test_table_misuse_is_a_synthesis_error(misuse):
    u = lambda *v: np.array(v, dtype=np.uint64)                          # noqa: E731

    class Tables(Plan):
        def synthesize(self, config, layouter):
            def first(table):
                if misuse == "hole":
                    table.assign_cell(F0, 0, u(1, 2))
                    table.assign_cell(F0, 3, u(4))
                elif misuse == "no row 0":
                    table.assign_cell(F0, 1, u(1, 2))
                elif misuse == "row 0 twice":
                    table.assign_cell(F0, 0, u(1, 2))
                    table.assign_cell(F0, 0, u(1))
                elif misuse == "lengths":
                    table.assign_cell(F0, 0, u(1, 2))
                    table.assign_cell(F1, 0, u(1, 2, 3))
                elif misuse == "two tables":
                    table.assign_cell(F0, 0, u(1, 2))
            layouter.assign_table("first", first)
            if misuse == "two tables":
                layouter.assign_table("second", lambda table: table.assign_cell(F0, 0, u(5)))

    with pytest.raises(syn.SynthesisError) as err:
        syn.synthesize_keygen(None, Tables([], constant_columns=0), 6)
    assert type(err.value) is syn.SynthesisError
    # ... and the well-formed two-column table passes, in pieces and out of order
    class Good(Plan):
        def synthesize(self, config, layouter):
            def body(table):
                table.assign_cell(F0, 2, u(7, 8))
                table.assign_cell(F0, 0, u(5, 6))
                table.assign_cell(F1, 0, u(1, 2, 3, 4))
            layouter.assign_table("good", body)

    _, fixed, _ = syn.synthesize_keygen(None, Good([], constant_columns=0), 6)
    assert fixed[0][:6, 0].tolist() == [5, 6, 7, 8, 5, 5] and fixed[1][:6, 0].tolist() == [1, 2, 3, 4, 1, 1]


# ---- constants columns in the serialised constraint system and the digest ------------------------------------------------
def tiny_constants_cs():
    cs = ConstraintSystem("tiny")
    a = cs.advice_column()
    f = cs.fixed_column()
    cs.enable_equality(a)
    cs.enable_constant(f)
    cs.enable_constant(f)                                                # idempotent, as the reference's
    return cs


def test_digest_preimage_of_a_circuit_with_a_constants_column_written_out_by_hand():
    cs = tiny_constants_cs()
    assert cs.constants == [("fixed", 0)] and cs.perm_columns == [("advice", 0), ("fixed", 0)]
    u32 = lambda *v: b"".join(struct.pack("<I", x) for x in v)           # noqa: E731
    by_hand = (u32(1, 0, 0, 1)            # advice columns, instance columns, selectors, fixed columns
               + u32(1, 1)                # num_advice_queries: one column, one query
               + u32(0)                   # selector_map: empty
               + u32(1, 0)                # constants: one column, fixed 0            <- the list this change carries
               + u32(1, 0, 0)             # advice queries: (column 0, rotation 0)
               + u32(0)                   # instance queries
               + u32(1, 0, 0)             # fixed queries: (column 0, rotation 0), from enable_equality
               + u32(2, 0, 0, 0, 1)       # permutation columns: (index 0, advice), (index 0, fixed)
               + u32(0, 0, 0, 0, 0))      # lookups, shuffles, range checks, named advices, gates
    assert cs_format.cs_store(cs) == by_hand
    dom = Domain(4, cs.degree())
    body = (b"halo2-hip-vk-v2" + u32(4, dom.extended_k) + dom.omega.to_bytes(32, "little") + R_MOD.to_bytes(32, "little")
            + Q_MOD.to_bytes(32, "little") + u32(len(by_hand)) + by_hand + u32(0) + u32(0))
    assert cs_format.vk_digest_preimage(cs, dom, [], []) == struct.pack("<Q", len(body)) + body
    # the list survives the round trip, and a second constants column changes the digest
    back = cs_format.cs_fetch(cs_format._Reader(by_hand))
    assert back.constants == [("fixed", 0)] and cs_format.cs_store(back) == by_hand
    other = tiny_constants_cs()
    other.enable_constant(other.fixed_column())
    assert cs_format.vk_digest(other, dom, [], []) != cs_format.vk_digest(cs, dom, [], [])


def test_a_circuit_without_constants_keeps_its_committed_digest():
    with open(os.path.join(ROOT, "tests", "golden", "proof_hash_kat.json")) as f:
        case = next(c for c in json.load(f) if c["circuit"] == "mini-plonk" and c["k"] == 12)
    k = case["k"]
    cs, fixed, copies = syn.synthesize_keygen(None, fe.MiniPlonk(k), k)
    assert cs.constants == []
    rpk = rp.keygen(rp.MiniPlonk, k, int(case["trapdoor"], 16), [[int(v) for v in f[:, 0]] for f in fixed],
                    [((int(c[0]), int(c[1])), (int(c[2]), int(c[3]))) for c in copies])
    digest = cs_format.vk_digest(cs, Domain(k, cs.degree()), rpk.fixed_commitments, rpk.perm_commitments)
    assert digest == int(case["vk_digest"], 16)
