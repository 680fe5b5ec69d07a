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

Where an example assigns cell by cell in a loop, the class assigns the loop's range at once; the calls are otherwise the
example's, in its order."""
import numpy as np

from . import circuits
from .circuit import Constant
from .synthesis import V1, Circuit, FlatFloorPlanner


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
