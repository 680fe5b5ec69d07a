"""Circuits for the tests of check_assignments (tests/test_coverage_host.py, tests/test_gpu_coverage.py): a generator of random
front-end circuits from a plain description (`spec`), the circuit class that plays a description through the front end, and
the brute-force model of MockProver's CellNotAssigned -- dev.rs:959-1000 taken literally: a set of cells and a set of
enabled (selector, row) pairs per region, filled one Python step per cell, and one membership test per enabled row, gate and
queried cell.  The model reads the description and never the library's tables.

A description:
  advice / fixed / instance   numbers of columns; the LAST fixed column takes constants, the one before it is a lookup table's
  selectors                   [simple?]
  gates                       [(name, [(selector, [((kind, column), rotation), ...]), ...])]: one polynomial per entry,
                              selector x an expression that holds every listed cell (repeats included)
  regions                     [(name, "region" | "table", base, [op])] with op one of
                                ("advice" | "fixed", column, offset, stride, count)     offsets relative to the region
                                ("enable", selector, offset, stride, count)
                                ("constant", advice column, offset) / ("instance", advice column, offset, instance row)
                                ("cell", offset, count)                                  a table's assign_cell
                              `base` is added to every offset under FlatFloorPlanner (whose offsets are absolute) and is 0
                              under V1, which places the regions itself
"""
import numpy as np

from halo2_gpu_specific_amd import synthesis as syn
from halo2_gpu_specific_amd.check import CellNotAssigned
from halo2_gpu_specific_amd.circuit import ConstraintSystem

STRIDES = [1, 2, 3, 31, 32, 33, 37]


class SpecCircuit(syn.Circuit):
    def __init__(self, spec, planner):
        self.spec, self.planner = spec, planner

    def without_witnesses(self):
        return self

    def configure(self, cs):
        spec = self.spec
        advice = [cs.advice_column() for _ in range(spec["advice"])]
        fixed = [cs.fixed_column() for _ in range(spec["fixed"])]
        instance = [cs.instance_column() for _ in range(spec["instance"])]
        for column in advice + instance:
            cs.enable_equality(column)
        cs.enable_constant(fixed[-1])
        selectors = [cs.selector() if simple else cs.complex_selector() for simple in spec["selectors"]]
        query = {"advice": cs.query_advice, "fixed": cs.query_fixed, "instance": cs.query_instance}
        for name, polys in spec["gates"]:
            built = []
            for selector, cells in polys:
                leaves = [query[column[0]](column, rotation) for column, rotation in cells]
                expr = leaves[0]
                for i, leaf in enumerate(leaves[1:]):                 # sums, products, negations and scalings, left to right
                    expr = (expr * leaf, expr + leaf, expr - leaf * 3, -expr + leaf)[i % 4]
                built.append(cs.query_selector(selectors[selector]) * expr)
            cs.create_gate(name, built)
        return advice, fixed, instance, selectors

    def synthesize(self, config, layouter):
        advice, fixed, instance, selectors = config
        flat = self.planner is syn.FlatFloorPlanner

        def play(base, ops):
            def body(region):
                for op in ops:
                    if op[0] == "advice":
                        region.assign_advice(advice[op[1]], base + op[2], None, stride=op[3], count=op[4])
                    elif op[0] == "fixed":
                        region.assign_fixed(fixed[op[1]], base + op[2], 5, stride=op[3], count=op[4])
                    elif op[0] == "enable":
                        region.enable_selector(selectors[op[1]], base + op[2], stride=op[3], count=op[4])
                    elif op[0] == "constant":
                        region.assign_advice_from_constant(advice[op[1]], base + op[2], 9)
                    else:
                        region.assign_advice_from_instance(instance[0], op[3], advice[op[1]], base + op[2])
            return body

        for name, kind, base, ops in self.spec["regions"]:
            if kind == "table":
                layouter.assign_table(name, lambda table, ops=ops: [table.assign_cell(fixed[-2], op[1], 1, count=op[2]) for op in ops])
            else:
                layouter.assign_region(name, play(base if flat else 0, ops))


def usable_rows(spec, n):
    cs = ConstraintSystem()
    SpecCircuit(spec, syn.V1).configure(cs)
    assert n >= cs.minimum_rows()
    return n - (cs.blinding_factors() + 1)


def gate_sets(spec):
    """S(g) and Q(g) as sets, from the description"""
    return [({selector for selector, _ in polys}, {cell for _, cells in polys for cell in cells}) for _, polys in spec["gates"]]


def model(spec, planner, n):
    """-> the sorted CellNotAssigned tuples and the number of failures (g, r, q, cell_row): one Python step per cell"""
    circuit = SpecCircuit(spec, planner)
    flat = planner is syn.FlatFloorPlanner
    planned = iter(syn.region_starts(circuit, planner))       # of the assign_region calls; a table starts at row 0
    regions = []
    for name, kind, base, ops in spec["regions"]:
        start = 0 if kind == "table" else next(planned)
        origin = base if flat else start
        cells, enabled = set(), set()
        for op in ops:
            if op[0] in ("advice", "fixed"):
                for i in range(op[4]):
                    cells.add(((op[0], op[1]), origin + op[2] + i * op[3]))
            elif op[0] == "enable":
                for i in range(op[4]):
                    enabled.add((op[1], origin + op[2] + i * op[3]))
            elif op[0] == "cell":
                for i in range(op[2]):
                    cells.add((("fixed", spec["fixed"] - 2), op[1] + i))
            else:
                cells.add((("advice", op[1]), origin + op[2]))
        regions.append((name, min([row for _, row in cells], default=start), cells, enabled))
    failures = set()
    for r, (_, _, cells, enabled) in enumerate(regions):
        for selector, row in enabled:
            for g, (selectors, queried) in enumerate(gate_sets(spec)):
                if selector in selectors:
                    for column, rotation in queried:
                        cell_row = (row + n + rotation) % n
                        if (column, cell_row) not in cells:
                            failures.add((g, r, (column, rotation), cell_row))
    named = sorted(CellNotAssigned(g, spec["gates"][g][0], r, regions[r][0], column, cell_row - regions[r][1], cell_row)
                   for g, r, (column, _), cell_row in failures)
    return named, len(failures)


def _constraint_side(rng, n, instance_queries):
    reach = 1 if n == 16 else 3                               # seven rotations of one column leave no usable row at n = 16
    spec = {"advice": int(rng.integers(2, 5)), "fixed": int(rng.integers(3, 5)), "instance": 1,
            "selectors": [bool(rng.integers(0, 4)) for _ in range(int(rng.integers(1, 7)))], "gates": [], "regions": []}
    columns = [("advice", i) for i in range(spec["advice"])] + [("fixed", i) for i in range(spec["fixed"] - 2)]
    if instance_queries:
        columns.append(("instance", 0))
    for g in range(int(rng.integers(1, 5))):
        polys = []
        for _ in range(int(rng.integers(1, 3))):
            cells = [(columns[int(rng.integers(0, len(columns)))], int(rng.integers(-reach, reach + 1)))
                     for _ in range(int(rng.integers(1, 5)))]
            polys.append((int(rng.integers(0, len(spec["selectors"]))), cells + cells[:int(rng.integers(0, 2))]))
        spec["gates"].append(("gate %d" % g, polys))
    return spec, reach


def _heights(rng, planner, regions, usable, least):
    """(base, height) per region: anywhere, overlapping, under the flat planner; a share of the usable rows under V1"""
    if planner is syn.FlatFloorPlanner:
        heights = [int(rng.integers(least, max(least, min(usable, 80)) + 1)) for _ in range(regions)]
        return [(int(rng.choice([0, 5, 31, 33, int(rng.integers(0, usable - h + 1))])) if usable - h >= 33 else
                 int(rng.integers(0, usable - h + 1)), h) for h in heights]
    regions = max(1, min(regions, usable // least))
    return [(0, int(rng.integers(least, usable // regions + 1))) for _ in range(regions)]


def random_spec(seed, planner, n, regions=None):
    """anything: cells nobody needs, enabled rows whose cells nobody assigned, instance queries, rotations that wrap past row 0
    or leave the usable rows, selector rows enabled twice, a table, constants, cells taken from the instance"""
    rng = np.random.Generator(np.random.PCG64(seed))
    spec, _ = _constraint_side(rng, n, True)
    usable = usable_rows(spec, n)
    regions = int(rng.integers(1, 41)) if regions is None else regions
    for r, (base, height) in enumerate(_heights(rng, planner, regions, usable, 1)):
        if r == 1 and rng.integers(0, 2):
            spec["regions"].append(("table", "table", 0, [("cell", 0, 2), ("cell", 2, int(rng.integers(1, 4)))]))

        def segment():
            stride = int(rng.choice(STRIDES))
            offset = int(rng.integers(0, height))
            return offset, stride, int(rng.integers(1, (height - 1 - offset) // stride + 2))

        ops = []
        for _ in range(int(rng.integers(1, 7))):
            kind = ("advice", "advice", "fixed")[int(rng.integers(0, 3))]
            ops.append((kind, int(rng.integers(0, spec[kind] - (2 if kind == "fixed" else 0))),) + segment())
        for _ in range(int(rng.integers(0, 4))):
            ops.append(("enable", int(rng.integers(0, len(spec["selectors"]))),) + segment())
        if rng.integers(0, 3) == 0:
            ops.append(ops[-1])                                # the same cells, or the same selector rows, once more
        if r == 0 and rng.integers(0, 2):                     # one constant: the planners need a free cell for each
            ops.append(("constant", int(rng.integers(0, spec["advice"])), int(rng.integers(0, height))))
        if rng.integers(0, 4) == 0:
            ops.append(("instance", int(rng.integers(0, spec["advice"])), int(rng.integers(0, height)), int(rng.integers(0, 3))))
        order = rng.permutation(len(ops))
        spec["regions"].append(("region %d" % r, "region", base, [ops[i] for i in order]))
    return spec


def _cover(rng, cells):
    """segments that assign exactly `cells` (a set of (column, row)): runs, halves of runs two rows apart, single cells"""
    ops = []
    for column in sorted({column for column, _ in cells}):
        rows = sorted(row for c, row in cells if c == column)
        runs, first = [], rows[0]
        for a, b in zip(rows, rows[1:] + [None]):
            if b != a + 1:
                runs.append((first, a - first + 1))
                first = b
        for first, count in runs:
            how = int(rng.integers(0, 3))
            if how == 0 or count < 4:
                ops.append((column[0], column[1], first, 1, count))
            elif how == 1:
                ops.append((column[0], column[1], first, 2, (count + 1) // 2))
                ops.append((column[0], column[1], first + 1, 2, count // 2))
            else:
                ops.extend((column[0], column[1], first + i, 1, 1) for i in range(count))
    return ops


def paired_specs(seed, planner, n, regions=None):
    """-> (complete, holed, expected): the same circuit with every required cell assigned, and with `holes` of them -- single-cell
    assignments of the complete one -- left out; expected = the sorted CellNotAssigned tuples and the failure count of the
    holed one, computed from the removed cells alone"""
    rng = np.random.Generator(np.random.PCG64(seed))
    spec, reach = _constraint_side(rng, n, False)
    usable = usable_rows(spec, n)
    sets = gate_sets(spec)
    regions = int(rng.integers(1, 41)) if regions is None else regions
    complete, holed, failures, names = [], [], set(), []
    for r, (base, height) in enumerate(_heights(rng, planner, regions, usable, 2 * reach + 1)):
        enables = []
        for e in range(int(rng.integers(1, 4))):
            stride = int(rng.choice(STRIDES[:4]))
            offset = int(rng.integers(reach, height - reach))
            # the first region's first selector is one a gate uses: every seed has a required cell to leave out
            selector = spec["gates"][0][1][0][0] if r == 0 and e == 0 else int(rng.integers(0, len(spec["selectors"])))
            enables.append(("enable", selector, offset, stride,
                            int(rng.integers(1, (height - reach - 1 - offset) // stride + 2))))
        required = {}                                          # (column, offset) -> the failures its absence causes
        for _, selector, offset, stride, count in enables:
            for i in range(count):
                for g, (selectors, queried) in enumerate(sets):
                    if selector in selectors:
                        for column, rotation in queried:
                            cell = (column, offset + i * stride + rotation)
                            required.setdefault(cell, set()).add((g, (column, rotation)))
        holes = set()
        if required and (r == 0 or rng.integers(0, 2)):
            cells = sorted(required)
            holes = {cells[i] for i in rng.choice(len(cells), size=min(len(cells), int(rng.integers(1, 4))), replace=False)}
        kept = _cover(rng, set(required) - holes) if set(required) - holes else []
        extra = [("advice", int(rng.integers(0, spec["advice"])), int(rng.integers(0, height)), 1, 1) for _ in range(2)]
        extra = [op for op in extra if ((op[0], op[1]), op[2]) not in holes]       # cells nobody needs
        singles = [(column[0], column[1], offset, 1, 1) for column, offset in sorted(holes)]
        name = "region %d" % r
        names.append(name)
        complete.append((name, "region", base, enables + kept + extra + singles))
        holed.append((name, "region", base, enables + kept + extra))
        for cell in holes:
            for g, query in required[cell]:
                failures.add((g, r, query, cell))
    one, two = dict(spec, regions=complete), dict(spec, regions=holed)
    # offsets count from the holed region's smallest assigned row; absolute rows need the planner's starts
    circuit = SpecCircuit(two, planner)
    starts = syn.region_starts(circuit, planner)
    named = []
    for g, r, (column, _), (_, offset) in failures:
        origin = holed[r][2] if planner is syn.FlatFloorPlanner else starts[r]
        assigned = [origin + op[2] for op in holed[r][3] if op[0] != "enable"]
        start = min(assigned, default=starts[r])
        named.append(CellNotAssigned(g, spec["gates"][g][0], r, names[r], column, origin + offset - start, origin + offset))
    return one, two, (sorted(named), len(failures))
