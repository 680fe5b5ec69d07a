"""The reference's examples written the way the reference writes them -- `configure` + `synthesize` against a Layouter
(synthesis.py) -- next to the hand-laid twins of circuits.py, which they reproduce cell for cell:

  LookupApi          examples/lookup_api.rs:112-160           V1
  LookupApiSet       examples/lookup_api_set.rs:111-170       V1
  RangeCheck         examples/range-check.rs:30-97            V1
  ShuffleGates       examples/shuffle.rs:138-245              V1
  ShuffleApi         examples/shuffle_api.rs:115-166          V1
  ShuffleApiGroup    examples/shuffle_api_group.rs:127-176    V1
  MiniPlonk          examples/simple-example-2.rs:169-243     FlatFloorPlanner, strided bulk assignments
  Wide               circuits.wide, the benchmark's lookup-bearing circuit (no .rs text)
  SimpleExample      examples/simple-example.rs:257-312       V1, one simple selector, a constant, a public input
  TwoChip            examples/two-chip.rs:473-509             V1, two simple selectors (an add and a mul chip)
  SelectorGates      simple, complex and unused selectors enabled in bulk, strided (no .rs text)
  ShuffleGatesValues ShuffleGates with its witness computed on the device by Values (values.py), at any height
  LimbDecomposition  p = a b mod 2^(bits words) split into limbs that a range table is looked up for: integer Values
  SortedAccessLog    an access log and the same rows ordered by (address, time) by Value.sort_by: a memory-consistency table

Where an example assigns cell by cell in a loop, the class assigns the loop's range at once; the calls are otherwise the
example's, in its order."""
import numpy as np

from . import circuits
from .circuit import R_MOD, Constant
from .synthesis import V1, Circuit, FlatFloorPlanner
from .values import Value


class _Config:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def _u64(values):
    return np.array(values, dtype=np.uint64)


class LookupApi(Circuit):
    planner = V1

    def without_witnesses(self):
        return LookupApi()

    def configure(self, cs):
        i0, i1, i2 = cs.advice_column(), cs.advice_column(), cs.advice_column()
        s0, s1 = cs.fixed_column(), cs.fixed_column()
        table = cs.lookup_table_column()
        cs.create_gate("", [cs.query_fixed(s0) * (cs.query_advice(i0) * 1 - cs.query_advice(i1))])
        cs.lookup("table1", [(cs.query_advice(i0), cs.query_fixed(table))])
        cs.lookup("table2", [(cs.query_advice(i1) * 2, cs.query_fixed(table))])
        cs.lookup("table3", [(cs.query_advice(i2), cs.query_fixed(table))])
        q0, q1, q2 = cs.query_advice(i0), cs.query_advice(i1), cs.query_advice(i2)
        f0, f1 = cs.query_fixed(s0), cs.query_fixed(s1)
        cs.lookup("any", [(f0 * q0, f0 * q1), (f1 * q0, f1 * q2)])
        return _Config(input_0=i0, input_1=i1, input_2=i2, s_0=s0, s_1=s1, table=table)

    def synthesize(self, config, layouter):
        def inputs(region):
            region.assign_advice(config.input_0, 0, 1)
            region.assign_advice(config.input_1, 0, 1)
            region.assign_fixed(config.s_0, 0, 1)
            region.assign_advice(config.input_0, 1, 3)
            region.assign_advice(config.input_2, 1, 3)
            region.assign_fixed(config.s_1, 1, 1)

        layouter.assign_region("inputs", inputs)
        layouter.assign_table("common range table", lambda table: table.assign_cell(config.table, 0, np.arange(9, dtype=np.uint64)))


class LookupApiSet(Circuit):
    planner = V1

    def without_witnesses(self):
        return LookupApiSet()

    def configure(self, cs):
        ins = [cs.advice_column() for _ in range(6)]
        s0, s1 = cs.fixed_column(), cs.fixed_column()
        table = cs.lookup_table_column()
        cs.create_gate("", [cs.query_fixed(s0) * (cs.query_advice(ins[0]) * 1 - cs.query_advice(ins[1]))])
        for i, scale in enumerate((None, 2, None, 10, None, None)):
            q = cs.query_advice(ins[i])
            cs.lookup("table%d" % i, [(q * scale if scale else q, cs.query_fixed(table))])
        return _Config(inputs=ins, s_0=s0, s_1=s1, table=table)

    def synthesize(self, config, layouter):
        def inputs(region):
            for i in range(6):
                region.assign_advice(config.inputs[i], 0, 1)
            region.assign_fixed(config.s_0, 0, 1)
            for i in range(6):
                region.assign_advice(config.inputs[i], 1, 3)
            region.assign_fixed(config.s_1, 1, 1)

        layouter.assign_region("inputs", inputs)
        layouter.assign_table("common range table", lambda table: table.assign_cell(config.table, 0, np.arange(100, dtype=np.uint64)))


class RangeCheck(Circuit):
    """`count` seeded random values of [vmin, vmax] on the rows 0 .. count - 1 of the range-checked column; the example's
    sizes are the defaults"""
    planner = V1

    def __init__(self, k, seed=0x52414E4745, vmin=0, vmax=0xFFFF, step=2, count=0xFFFF, witness=True):
        self.k, self.seed, self.vmin, self.vmax, self.step, self.count, self.witness = k, seed, vmin, vmax, step, count, witness

    def without_witnesses(self):
        return RangeCheck(self.k, self.seed, self.vmin, self.vmax, self.step, self.count, witness=False)

    def configure(self, cs):
        l_0, l_active, l_last_active = cs.fixed_column(), cs.fixed_column(), cs.fixed_column()
        adv = cs.advice_column_range(l_0, l_active, l_last_active, self.vmin, self.vmax, self.step)
        return _Config(l_0=l_0, l_active=l_active, l_last_active=l_last_active, adv=adv,
                       l_last_offset=(1 << self.k) - (cs.blinding_factors() + 1))

    def synthesize(self, config, layouter):
        def body(region):
            region.assign_fixed(config.l_0, 0, 1)
            region.assign_fixed(config.l_last_active, config.l_last_offset - 1, 1)
            region.assign_fixed(config.l_active, 0, 1, count=config.l_last_offset)
            values = None
            if self.witness:
                rng = np.random.Generator(np.random.PCG64(self.seed))
                values = rng.integers(self.vmin, self.vmax + 1, size=self.count, dtype=np.uint64)
            region.assign_advice(config.adv, 0, values, count=self.count)

        layouter.assign_region("region", body)


class ShuffleGates(Circuit):
    planner = V1

    def __init__(self, k, width=4, height=32, theta=111, beta=222, seed=0x5348554646, witness=True):
        self.k, self.width, self.height, self.theta, self.beta, self.seed, self.witness = k, width, height, theta, beta, seed, witness

    def without_witnesses(self):
        return ShuffleGates(self.k, self.width, self.height, self.theta, self.beta, self.seed, witness=False)

    def configure(self, cs):
        q_shuffle, q_first, q_last = cs.fixed_column(), cs.fixed_column(), cs.fixed_column()
        original = [cs.advice_column() for _ in range(self.width)]
        shuffled = [cs.advice_column() for _ in range(self.width)]
        z = cs.advice_column()
        th, be = Constant(self.theta), Constant(self.beta)
        cs.create_gate("z should start with 1", [cs.query_fixed(q_first) * (Constant(1) - cs.query_advice(z))])
        cs.create_gate("z should end with 1", [cs.query_fixed(q_last) * (Constant(1) - cs.query_advice(z))])
        qs = cs.query_fixed(q_shuffle)
        orig = [cs.query_advice(c) for c in original]
        shuf = [cs.query_advice(c) for c in shuffled]
        z_cur, z_next = cs.query_advice(z), cs.query_advice(z, 1)

        def compress(cells):
            acc = cells[0]
            for cell in cells[1:]:
                acc = acc * th + cell
            return acc

        cs.create_gate("z should have valid transition", [qs * (z_cur * (compress(orig) + be) - z_next * (compress(shuf) + be))])
        return _Config(q_shuffle=q_shuffle, q_first=q_first, q_last=q_last, original=original, shuffled=shuffled, z=z)

    def synthesize(self, config, layouter):
        H, W = self.height, self.width
        columns = None
        if self.witness:
            adv, _ = circuits.shuffle_gates_witness(self.k, W, H, self.theta, self.beta, self.seed)
            limbs = lambda col: _u64([[(v >> (64 * j)) & 0xFFFFFFFFFFFFFFFF for j in range(4)] for v in col])   # noqa: E731
            columns = [limbs(col[:H + 1]) for col in adv]

        def body(region):
            region.assign_fixed(config.q_first, 0, 1)
            region.assign_fixed(config.q_last, H, 1)
            region.assign_fixed(config.q_shuffle, 0, 1, count=H)
            for i, column in enumerate(config.original + config.shuffled):
                region.assign_advice(column, 0, columns[i][:H] if columns else None, count=H)
            region.assign_advice(config.z, 0, columns[2 * W] if columns else None, count=H + 1)

        layouter.assign_region("Shuffle original into shuffled", body)


class ShuffleApi(Circuit):
    planner = V1

    def __init__(self, input0=(1, 2, 4, 1), shuffle0=(4, 1, 1, 2)):
        self.input0, self.shuffle0 = input0, shuffle0

    def without_witnesses(self):
        return ShuffleApi(self.input0, self.shuffle0)           # (the example's `Self::default()` keeps the lengths it needs)

    def configure(self, cs):
        in0, in1, sh0, sh1 = (cs.advice_column() for _ in range(4))
        s_in, s_sh = cs.fixed_column(), cs.fixed_column()
        cs.create_gate("", [cs.query_fixed(s_in) * (cs.query_advice(in0) * 10 - cs.query_advice(in1))])
        q_in0, q_sh0, q_in1, q_sh1 = cs.query_advice(in0), cs.query_advice(sh0), cs.query_advice(in1), cs.query_advice(sh1)
        f_in, f_sh = cs.query_fixed(s_in), cs.query_fixed(s_sh)
        cs.shuffle("shuffle", [(f_in * q_in0, f_sh * q_sh0), (f_in * q_in1, f_sh * q_sh1)])
        return _Config(input_0=in0, input_1=in1, shuffle_0=sh0, shuffle_1=sh1, s_input=s_in, s_shuffle=s_sh)

    def synthesize(self, config, layouter):
        m = len(self.input0)

        def inputs(region):
            region.assign_advice(config.input_0, 0, _u64(self.input0))
            region.assign_advice(config.input_1, 0, 10 * _u64(self.input0))
            region.assign_fixed(config.s_input, 0, 1, count=m)

        def shuffles(region):
            region.assign_advice(config.shuffle_0, 0, _u64(self.shuffle0))
            region.assign_advice(config.shuffle_1, 0, 10 * _u64(self.shuffle0))
            region.assign_fixed(config.s_shuffle, 0, 1, count=m)

        layouter.assign_region("inputs", inputs)
        layouter.assign_region("shuffles", shuffles)


class ShuffleApiGroup(Circuit):
    planner = V1

    def __init__(self, input0=(1, 2, 4, 1), input1=(4, 1, 1, 2)):
        self.input0, self.input1 = input0, input1

    def without_witnesses(self):
        return ShuffleApiGroup(self.input0, self.input1)

    def configure(self, cs):
        ins = [cs.advice_column() for _ in range(5)]
        shs = [cs.advice_column() for _ in range(5)]
        s_in = [cs.fixed_column() for _ in range(2)]
        s_sh = [cs.fixed_column() for _ in range(2)]
        cs.create_gate("", [cs.query_fixed(s_in[0]) * (cs.query_advice(ins[0]) - cs.query_advice(ins[1]))])
        cs.shuffle("shuffle1", [(cs.query_advice(ins[0]), cs.query_advice(shs[0])), (cs.query_advice(ins[1]), cs.query_advice(shs[1]))])
        cs.shuffle("shuffle2", [(cs.query_advice(ins[2]), cs.query_advice(shs[2]))])
        cs.shuffle("shuffle3", [(cs.query_advice(ins[3]) * cs.query_fixed(s_in[0]), cs.query_advice(shs[3]) * cs.query_fixed(s_sh[0]))])
        cs.shuffle("shuffle4", [(cs.query_advice(ins[4]) * cs.query_fixed(s_in[0]) * cs.query_fixed(s_in[1]),
                                 cs.query_advice(shs[4]) * cs.query_fixed(s_sh[0]) * cs.query_fixed(s_sh[1]))])
        return _Config(inputs=ins, shuffles=shs, s_inputs=s_in, s_shuffles=s_sh)

    def synthesize(self, config, layouter):
        m = len(self.input0)

        def inputs(region):
            for column in config.inputs:
                region.assign_advice(column, 0, _u64(self.input0))
            for column in config.shuffles:
                region.assign_advice(column, 0, _u64(self.input1))
            for column in (config.s_inputs[0], config.s_shuffles[0], config.s_inputs[1], config.s_shuffles[1]):
                region.assign_fixed(column, 0, 1, count=m)

        layouter.assign_region("inputs", inputs)


class MiniPlonk(Circuit):
    """2^(k - 4) times { raw_multiply(a, a, a^2); raw_add(a, a^2, a + a^2); copy a0 = a1; copy b1 = c0 }: under
    FlatFloorPlanner the multiplications are the even rows and the additions the odd ones, each one strided assignment"""
    planner = FlatFloorPlanner

    def __init__(self, k, a=5):
        self.k, self.a = k, a

    def without_witnesses(self):
        return MiniPlonk(self.k, None)

    def configure(self, cs):
        a, b, c = cs.advice_column(), cs.advice_column(), cs.advice_column()
        for col in (a, b, c):
            cs.enable_equality(col)
        sm, sa, sb, sc = cs.fixed_column(), cs.fixed_column(), cs.fixed_column(), cs.fixed_column()
        qa, qb, qc = cs.query_advice(a), cs.query_advice(b), cs.query_advice(c)
        qsa, qsb, qsc, qsm = cs.query_fixed(sa), cs.query_fixed(sb), cs.query_fixed(sc), cs.query_fixed(sm)
        cs.create_gate("mini plonk", [qa * qsa + qb * qsb + qa * qb * qsm + (qc * qsc) * (-1)])
        return _Config(a=a, b=b, c=c, sa=sa, sb=sb, sc=sc, sm=sm)

    def synthesize(self, config, layouter):
        pairs, a = 1 << (self.k - 4), self.a
        a2 = None if a is None else a * a
        fin = None if a is None else a + a2

        def raw(offset, values, selectors):
            def body(region):
                cells = [region.assign_advice(column, offset, value, stride=2, count=pairs)
                         for column, value in zip((config.a, config.b, config.c), values)]
                for column, value in zip((config.sa, config.sb, config.sc, config.sm), selectors):
                    region.assign_fixed(column, offset, value, stride=2, count=pairs)
                return cells
            return body

        a0, _, c0 = layouter.assign_region("mul", raw(0, (a, a, a2), (0, 0, 1, 1)))
        a1, b1, _ = layouter.assign_region("add", raw(1, (a, a2, fin), (1, 1, 1, 0)))
        layouter.assign_region("copy", lambda region: region.constrain_equal(a0, a1))
        layouter.assign_region("copy", lambda region: region.constrain_equal(b1, c0))


class Wide(Circuit):
    """circuits.wide / wide_synthesize through the front end: one region of compact bulk assignments"""
    planner = FlatFloorPlanner

    def __init__(self, k, quads=16, witness=True):
        self.k, self.quads, self.witness = k, quads, witness

    def without_witnesses(self):
        return Wide(self.k, self.quads, witness=False)

    def configure(self, cs):
        quads = self.quads
        adv = [cs.advice_column() for _ in range(4 * quads)]
        q, t = cs.fixed_column(), cs.fixed_column()
        cs.enable_equality(adv[0])
        cs.enable_equality(adv[1])
        qq = cs.query_fixed(q)
        cells = [cs.query_advice(col) for col in adv]
        cs.create_gate("mul3", [qq * (cells[4 * i] * cells[4 * i + 1] * cells[4 * i + 2] + cells[4 * i + 3] * (-1))
                                for i in range(quads)])
        tt = cs.query_fixed(t)
        for l in range(quads // 2):
            cs.lookup_any("range%d" % l, [tt], [[[cells[8 * l]], [cells[8 * l + 4]]]])
        cs.set_minimum_degree(5)
        return _Config(advice=adv, q=q, t=t, usable=(1 << self.k) - 6)

    def synthesize(self, config, layouter):
        usable = config.usable
        T = min(usable, 1 << 16)
        rows = np.arange(usable, dtype=np.uint64) if self.witness else None

        def body(region):
            region.assign_fixed(config.q, 0, 1, count=usable)
            region.assign_fixed(config.t, 0, np.arange(T, dtype=np.uint64))
            first = []
            for qd in range(self.quads):
                vals = [None] * 4
                if self.witness:
                    vals = [((rows * np.uint64(2654435761) + np.uint64(40503 * (4 * qd + j) + 7)) >> np.uint64(5)) % np.uint64(T)
                            for j in range(3)]
                    if qd == 0:
                        vals[1] = np.concatenate([np.array([3 % T], dtype=np.uint64), vals[0][:-1]])
                    vals.append(vals[0] * vals[1] * vals[2])
                cells = [region.assign_advice(config.advice[4 * qd + j], 0, vals[j], count=usable) for j in range(4)]
                if qd == 0:
                    first = cells
            m = min(usable - 1, 1 << 16)
            region.constrain_equal(first[0][:m], first[1][1:m + 1])

        layouter.assign_region("rows", body)


def _copy_advice(region, cell, value, column, offset):
    """AssignedCell::copy_advice (circuit.rs:131-147): a new cell with the value, constrained equal to the old one"""
    new = region.assign_advice(column, offset, value)
    region.constrain_equal(new, cell)
    return new


def _mul(a, b):
    return None if a is None or b is None else a * b % R_MOD


def _add(a, b):
    return None if a is None or b is None else (a + b) % R_MOD


class _Chip:
    """the instructions the two examples share: a number is (cell, value); value None at keygen"""

    def __init__(self, config):
        self.config = config

    def load_private(self, layouter, value):
        return layouter.assign_region("load private", lambda region: (region.assign_advice(self.config.advice[0], 0, value), value))

    def load_constant(self, layouter, constant):
        return layouter.assign_region(
            "load constant", lambda region: (region.assign_advice_from_constant(self.config.advice[0], 0, constant), constant))

    def _binary(self, layouter, name, selector, op, a, b):
        def body(region):
            selector.enable(region, 0)
            _copy_advice(region, a[0], a[1], self.config.advice[0], 0)
            _copy_advice(region, b[0], b[1], self.config.advice[1], 0)
            value = op(a[1], b[1])
            return region.assign_advice(self.config.advice[0], 1, value), value

        return layouter.assign_region(name, body)

    def mul(self, layouter, a, b):
        return self._binary(layouter, "mul", self.config.s_mul, _mul, a, b)

    def add(self, layouter, a, b):
        return self._binary(layouter, "add", self.config.s_add, _add, a, b)

    def expose_public(self, layouter, num, row):
        layouter.constrain_instance(num[0], self.config.instance, row)


class SimpleExample(Circuit):
    """c = constant * a^2 * b^2 by three multiplications under one simple selector; c is instance row 0 (the example: k = 4,
    constant 7, a 2, b 3)"""
    planner = V1

    def __init__(self, constant=7, a=2, b=3):
        self.constant, self.a, self.b = constant, a, b

    def without_witnesses(self):
        # the example's `Self::default()` also zeroes the constant, and hands keygen the full circuit; here keygen runs over
        # this one, and the constant is part of the circuit's fixed cells
        return SimpleExample(self.constant, None, None)

    def public_inputs(self):
        return [[self.constant * self.a ** 2 * self.b ** 2 % R_MOD]]

    def configure(self, cs):
        advice = [cs.advice_column(), cs.advice_column()]
        instance = cs.instance_column()
        constant = cs.fixed_column()
        cs.enable_equality(instance)
        cs.enable_constant(constant)
        for column in advice:
            cs.enable_equality(column)
        s_mul = cs.selector()
        lhs, rhs, out = cs.query_advice(advice[0]), cs.query_advice(advice[1]), cs.query_advice(advice[0], 1)
        cs.create_gate("mul", [cs.query_selector(s_mul) * (lhs * rhs - out)])
        return _Config(advice=advice, instance=instance, s_mul=s_mul)

    def synthesize(self, config, layouter):
        chip = _Chip(config)
        a = chip.load_private(layouter.namespace("load a"), self.a)
        b = chip.load_private(layouter.namespace("load b"), self.b)
        constant = chip.load_constant(layouter.namespace("load constant"), self.constant)
        ab = chip.mul(layouter.namespace("a * b"), a, b)
        absq = chip.mul(layouter.namespace("ab * ab"), ab, ab)
        c = chip.mul(layouter.namespace("constant * absq"), constant, absq)
        chip.expose_public(layouter.namespace("expose c"), c, 0)


class TwoChip(Circuit):
    """d = (a + b) * c by an add chip and a mul chip, each with a simple selector of its own; d is instance row 0 (the example
    draws a, b, c at random: here they are arguments)"""
    planner = V1

    def __init__(self, a=11, b=13, c=17):
        self.a, self.b, self.c = a, b, c

    def without_witnesses(self):
        return TwoChip(None, None, None)

    def public_inputs(self):
        return [[(self.a + self.b) * self.c % R_MOD]]

    def configure(self, cs):
        advice = [cs.advice_column(), cs.advice_column()]
        instance = cs.instance_column()
        lhs, rhs, out = (lambda: cs.query_advice(advice[0])), (lambda: cs.query_advice(advice[1])), (lambda: cs.query_advice(advice[0], 1))
        s_add = cs.selector()                                    # AddChip::configure
        cs.create_gate("add", [cs.query_selector(s_add) * (lhs() + rhs() - out())])
        for column in advice:                                    # MulChip::configure
            cs.enable_equality(column)
        s_mul = cs.selector()
        cs.create_gate("mul", [cs.query_selector(s_mul) * (lhs() * rhs() - out())])
        cs.enable_equality(instance)
        return _Config(advice=advice, instance=instance, s_add=s_add, s_mul=s_mul)

    def synthesize(self, config, layouter):
        chip = _Chip(config)
        a = chip.load_private(layouter.namespace("load a"), self.a)
        b = chip.load_private(layouter.namespace("load b"), self.b)
        c = chip.load_private(layouter.namespace("load c"), self.c)
        ab = chip.add(layouter.namespace("a + b"), a, b)
        d = chip.mul(layouter.namespace("(a + b) * c"), ab, c)
        chip.expose_public(layouter.namespace("expose d"), d, 0)


class SelectorGates(Circuit):
    """Every kind of selector, enabled in bulk over the usable rows: row r is of kind r % 4 --
      0  s_mul (a b = c) and the complex s_tab (s_tab a is in the table 0 .. 15)     1  s_add (a + b = c)
      2  s_add and s_bool (b (1 - b) = 0) together, so that the two conflict         3  s_tab alone
    and s_idle, in no gate, on every eighth row.  The cell a of row 4 is a copy of the cell a of row 0.  compress_selectors
    gives s_tab and s_idle a column each, combines s_mul with s_add and leaves s_bool alone (the degree is 5)."""
    planner = FlatFloorPlanner
    TABLE = 16

    def __init__(self, k, seed=0x53454C, witness=True):
        self.k, self.seed, self.witness = k, seed, witness

    def without_witnesses(self):
        return SelectorGates(self.k, self.seed, witness=False)

    def configure(self, cs):
        a, b, c = cs.advice_column(), cs.advice_column(), cs.advice_column()
        table = cs.lookup_table_column()
        cs.enable_equality(a)
        s_mul, s_add, s_bool, s_idle = cs.selector(), cs.selector(), cs.selector(), cs.selector()
        s_tab = cs.complex_selector()
        qa, qb, qc = cs.query_advice(a), cs.query_advice(b), cs.query_advice(c)
        cs.create_gate("mul", [cs.query_selector(s_mul) * (qa * qb - qc)])
        cs.create_gate("add", [cs.query_selector(s_add) * (qa + qb - qc)])
        cs.create_gate("bool", [cs.query_selector(s_bool) * (qb * (Constant(1) - qb))])
        cs.lookup("a in table", [(cs.query_selector(s_tab) * qa, cs.query_fixed(table))])
        return _Config(a=a, b=b, c=c, table=table, s_mul=s_mul, s_add=s_add, s_bool=s_bool, s_idle=s_idle, s_tab=s_tab,
                       rows=((1 << self.k) - 6) // 4 * 4)

    def witness_columns(self, rows):
        """-> a, b, c (u64 arrays of `rows` values)"""
        rng = np.random.Generator(np.random.PCG64(self.seed))
        kind = np.arange(rows) % 4
        a = rng.integers(0, self.TABLE, size=rows, dtype=np.uint64)
        b = rng.integers(0, self.TABLE, size=rows, dtype=np.uint64)
        b[kind == 2] &= np.uint64(1)
        a[4] = a[0]
        c = np.where(kind == 0, a * b, a + b)
        c[kind == 3] = rng.integers(0, 1 << 40, size=int((kind == 3).sum()), dtype=np.uint64)    # unconstrained
        return a, b, c

    def synthesize(self, config, layouter):
        rows = config.rows
        quarter = rows // 4
        values = self.witness_columns(rows) if self.witness else (None, None, None)

        def body(region):
            cells = [region.assign_advice(column, 0, v, count=rows) for column, v in zip((config.a, config.b, config.c), values)]
            region.enable_selector(config.s_mul, 0, stride=4, count=quarter)
            region.enable_selector(config.s_add, 1, stride=4, count=quarter)
            region.enable_selector(config.s_add, 2, stride=4, count=quarter)
            region.enable_selector(config.s_bool, 2, stride=4, count=quarter)
            region.enable_selector(config.s_tab, 0, stride=4, count=quarter)
            region.enable_selector(config.s_tab, 3, stride=4, count=quarter)
            region.enable_selector(config.s_tab, 3)                     # a row enabled twice
            region.enable_selector(config.s_idle, 0, stride=8, count=(rows + 7) // 8)
            region.constrain_equal(cells[0][0], cells[0][4])

        layouter.assign_region("rows", body)
        layouter.assign_table("range table", lambda table: table.assign_cell(config.table, 0, np.arange(self.TABLE, dtype=np.uint64)))


class ShuffleGatesValues(Circuit):
    """ShuffleGates with its witness computed by Values (values.py): the random originals come from the same seeded stream as
    circuits.shuffle_gates_witness, the shuffle is a `take`, and the running product is
    z = ((compress(original) + beta) / (compress(shuffled) + beta)).cumprod() -- one fused launch for the denominators, one
    batch inversion, one launch for the quotients and one scan, at any height up to usable - 1.  Keygen passes unknowns:
    there is no branch on a witness flag.  `device`: where the Values live (None: the host backend)."""
    planner = V1

    def __init__(self, k, width=4, height=32, theta=111, beta=222, seed=0x5348554646, device=None, originals=None):
        self.k, self.width, self.height, self.theta, self.beta, self.seed, self.device = k, width, height, theta, beta, seed, device
        self.originals = originals            # [Value] * width, unknown at keygen; drawn on first use otherwise
        self._columns = None

    def without_witnesses(self):
        return ShuffleGatesValues(self.k, self.width, self.height, self.theta, self.beta, self.seed, self.device,
                                  [Value.unknown(self.height)] * self.width)

    configure = ShuffleGates.configure

    def witness_inputs(self):
        """the originals and the shuffle's order, as circuits.shuffle_gates_witness draws them"""
        import random

        rnd = random.Random(self.seed)
        H = self.height
        original = [np.array([rnd.randrange(R_MOD).to_bytes(32, "little") for _ in range(H)], dtype="V32").view(np.uint64).reshape(H, 4)
                    for _ in range(self.width)]
        order = list(range(H))
        for row in range(H - 1, 0, -1):
            other = rnd.getrandbits(32) % row
            order[row], order[other] = order[other], order[row]
        return [Value.from_limbs(self.device, col) for col in original], np.array(order, dtype=np.int64)

    def columns(self):
        """[original] * W + [shuffled] * W + [z] as Values, built once"""
        if self._columns is None:
            order = None
            if self.originals is None:
                self.originals, order = self.witness_inputs()
            original = self.originals
            shuffled = [col.take(order) if col.known else col for col in original]

            def compress(cols):
                acc = cols[0]
                for col in cols[1:]:
                    acc = acc * self.theta + col
                return acc

            z = ((compress(original) + self.beta) / (compress(shuffled) + self.beta)).cumprod()
            self._columns = list(original) + shuffled + [z]
        return self._columns

    def synthesize(self, config, layouter):
        H, W = self.height, self.width
        columns = self.columns()

        def body(region):
            region.assign_fixed(config.q_first, 0, 1)
            region.assign_fixed(config.q_last, H, 1)
            region.assign_fixed(config.q_shuffle, 0, 1, count=H)
            for i, column in enumerate(config.original + config.shuffled):
                region.assign_advice(column, 0, columns[i], count=H)
            return region.assign_advice(config.z, 0, columns[2 * W], count=H + 1)

        return layouter.assign_region("Shuffle original into shuffled", body)


class LimbDecomposition(Circuit):
    """p = a * b mod 2^(bits * words) and the `words` limbs of `bits` bits of p, on `height` rows: every limb column is looked up
    in the range table 0 .. 2^bits - 1, and the gate  q (p - sum_j limb_j 2^(bits j)) = 0  ties them to p.  The whole witness
    exists only as Values (values.py): a and b are seeded u64 cells, p is `(a * b).low(bits * words)` and the limbs are
    `p.limbs(bits, words, strict=True)` -- the integer half of Value, computed where the Values live.  Keygen passes unknowns:
    there is no branch on a witness flag.  `columns`: [a, b, p] + limbs as Values instead of the seeded ones."""
    planner = V1

    def __init__(self, k, bits=8, words=4, height=None, seed=0x4C494D4253, device=None, columns=None):
        self.k, self.bits, self.words, self.seed, self.device = k, bits, words, seed, device
        self.height = (1 << k) - 6 if height is None else height
        if not (1 <= bits and bits * words <= 128 and (1 << bits) <= (1 << k) - 6 and 0 < self.height <= (1 << k) - 6):
            raise ValueError("LimbDecomposition: the table of 2^bits rows and the height must fit the usable rows, bits * words <= 128")
        self._columns = columns

    def without_witnesses(self):
        return LimbDecomposition(self.k, self.bits, self.words, self.height, self.seed, self.device,
                                 [Value.unknown(self.height)] * (3 + self.words))

    def configure(self, cs):
        a, b, p = cs.advice_column(), cs.advice_column(), cs.advice_column()
        limbs = [cs.advice_column() for _ in range(self.words)]
        q = cs.fixed_column()
        table = cs.lookup_table_column()
        total = cs.query_advice(limbs[0])
        for j in range(1, self.words):
            total = total + cs.query_advice(limbs[j]) * Constant(1 << (self.bits * j))
        cs.create_gate("p is the sum of its limbs", [cs.query_fixed(q) * (cs.query_advice(p) - total)])
        for j, limb in enumerate(limbs):
            cs.lookup("limb %d is in range" % j, [(cs.query_advice(limb), cs.query_fixed(table))])
        return _Config(a=a, b=b, p=p, limbs=limbs, q=q, table=table)

    def witness_inputs(self):
        """the seeded u64 cells of a and b"""
        rng = np.random.Generator(np.random.PCG64(self.seed))
        return rng.integers(0, 1 << 64, size=self.height, dtype=np.uint64), rng.integers(0, 1 << 64, size=self.height, dtype=np.uint64)

    def columns(self):
        """[a, b, p] + limbs as Values, built once"""
        if self._columns is None:
            a, b = (Value.from_u64(self.device, x) for x in self.witness_inputs())
            p = (a * b).low(self.bits * self.words)
            self._columns = [a, b, p] + p.limbs(self.bits, self.words, strict=True)
        return self._columns

    def synthesize(self, config, layouter):
        H = self.height
        columns = self.columns()

        def body(region):
            region.assign_fixed(config.q, 0, 1, count=H)
            for column, values in zip([config.a, config.b, config.p] + config.limbs, columns):
                region.assign_advice(column, 0, values, count=H)

        layouter.assign_region("limbs", body)
        layouter.assign_table("range table", lambda table: table.assign_cell(config.table, 0, np.arange(1 << self.bits, dtype=np.uint64)))


class SortedAccessLog(Circuit):
    """A memory-consistency table: a seeded log of `height` accesses in program order -- columns (a, t, v, w): an address below
    2^addr_bits, the time t = row + 1, the value, and w = 1 for a write; a read returns what a replay of the log finds at its
    address (0 before the first write) -- next to the same rows ordered by (address, time), (A, T, V, W), which exist only as
    `Value.sort_by([a, t], [a, t, v, w])` (values.py; csrc/sort.hip): the order is computed where the Values live.  With
    delta = A' - A on the rows 0 .. height - 2 of the sorted side the remaining advice is Values too:
        inv = delta.invert(),  s = 1 - delta inv  (1 where the address stays),  d = select(s, T' - T - 1, delta - 1).
    Relations (q on the `height` rows, q_adj on the first height - 1):
        shuffle   (q a, q t, q v, q w)  <->  (q A, q T, q V, q W)           the sorted side holds the log's rows (t >= 1 keeps
                                                                           an enabled row apart from the padding)
        gates     q_adj delta s = 0;  q_adj (s - 1 + delta inv) = 0         s = [delta = 0]
                  q_adj s (1 - W') (V' - V) = 0                             a read returns what the address held
                  q_adj (d - s (T' - T - 1) - (1 - s) (delta - 1)) = 0      d is the gap in time, or in address, less one
        lookup    d in 0 .. 2^b - 1, 2^b >= max(height, 2^addr_bits)        the gap is positive: the order is STRICT in
                                                                           (address, time)
    s has a column of its own, which keeps the gates at degree 4 (q_adj s (1 - W') (V' - V)); the shuffle is 2 + 2 and the
    lookup 2 + 1 + 1: the constraint system's degree is 4, below the wide circuit's 5.  Keygen passes unknowns: there is no
    branch on a witness flag.  `columns`: [a, t, v, w, A, T, V, W, inv, s, d] as Values instead of the seeded ones (the last
    three of height - 1 elements)."""
    planner = V1

    def __init__(self, k, addr_bits=4, height=None, seed=0x534F5254, device=None, columns=None):
        self.k, self.addr_bits, self.seed, self.device = k, addr_bits, seed, device
        self.height = 1 << (k - 1) if height is None else height
        self.table_bits = max(addr_bits, (self.height - 1).bit_length())
        if not (1 <= addr_bits <= 32 and 2 <= self.height and (1 << self.table_bits) <= (1 << k) - 6):
            raise ValueError("SortedAccessLog: height >= 2, and a table of max(height, 2^addr_bits) rows must fit the usable rows")
        self._columns = columns

    def without_witnesses(self):
        H = self.height
        return SortedAccessLog(self.k, self.addr_bits, H, self.seed, self.device,
                               [Value.unknown(H)] * 8 + [Value.unknown(H - 1)] * 3)

    def configure(self, cs):
        log = [cs.advice_column() for _ in range(4)]
        ordered = [cs.advice_column() for _ in range(4)]
        inv, s, d = cs.advice_column(), cs.advice_column(), cs.advice_column()
        q, q_adj = cs.fixed_column(), cs.fixed_column()
        table = cs.lookup_table_column()
        f_q, f_adj = cs.query_fixed(q), cs.query_fixed(q_adj)
        cs.shuffle("the sorted side holds the log's rows",
                   [(f_q * cs.query_advice(x), f_q * cs.query_advice(y)) for x, y in zip(log, ordered)])
        A, T, V = (cs.query_advice(c) for c in ordered[:3])
        A1, T1, V1_, W1 = (cs.query_advice(c, 1) for c in ordered)
        delta, one = A1 - A, Constant(1)
        q_inv, q_s, q_d = cs.query_advice(inv), cs.query_advice(s), cs.query_advice(d)
        cs.create_gate("the address stays or s is 0", [f_adj * delta * q_s])
        cs.create_gate("s is 1 where the address stays", [f_adj * (q_s - one + delta * q_inv)])
        cs.create_gate("a read returns the value before it", [f_adj * q_s * (one - W1) * (V1_ - V)])
        cs.create_gate("d is the gap less one", [f_adj * (q_d - q_s * (T1 - T - one) - (one - q_s) * (delta - one))])
        cs.lookup("the gap is positive", [(q_d, cs.query_fixed(table))])
        return _Config(log=log, ordered=ordered, inv=inv, s=s, d=d, q=q, q_adj=q_adj, table=table)

    def witness_inputs(self):
        """the seeded log as u64 cells: (a, t, v, w), the reads' values by a plain replay"""
        rng = np.random.Generator(np.random.PCG64(self.seed))
        H = self.height
        a = rng.integers(0, 1 << self.addr_bits, size=H, dtype=np.uint64)
        w = rng.integers(0, 2, size=H, dtype=np.uint64)
        v = rng.integers(0, 1 << 64, size=H, dtype=np.uint64)
        memory = {}
        for row in range(H):
            if w[row]:
                memory[int(a[row])] = v[row]
            else:
                v[row] = memory.get(int(a[row]), 0)
        return a, np.arange(1, H + 1, dtype=np.uint64), v, w

    def columns(self):
        """[a, t, v, w, A, T, V, W, inv, s, d] as Values, built once"""
        if self._columns is None:
            log = [Value.from_u64(self.device, x) for x in self.witness_inputs()]
            A, T, V, W = Value.sort_by(log[:2], log, bits=[self.addr_bits, self.height.bit_length()])
            delta = A[1:] - A[:-1]
            inv = delta.invert()
            s = 1 - delta * inv
            d = Value.select(s, T[1:] - T[:-1] - 1, delta - 1)
            self._columns = log + [A, T, V, W, inv, s, d]
        return self._columns

    def synthesize(self, config, layouter):
        H = self.height
        columns = self.columns()

        def body(region):
            region.assign_fixed(config.q, 0, 1, count=H)
            region.assign_fixed(config.q_adj, 0, 1, count=H - 1)
            for column, values in zip(config.log + config.ordered, columns[:8]):
                region.assign_advice(column, 0, values, count=H)
            for column, values in zip([config.inv, config.s, config.d], columns[8:]):
                region.assign_advice(column, 0, values, count=H - 1)

        layouter.assign_region("access log", body)
        layouter.assign_table("gap table", lambda table: table.assign_cell(config.table, 0, np.arange(1 << self.table_bits, dtype=np.uint64)))
