"""Values without a GPU: the compiler of halo2_gpu_specific_amd/values.py (common subexpressions, Sethi-Ullman order, slots by
last use, splitting at every cap, staged inversions), unknown Values, the host twin h2_values_eval against Python integers
mod r (tests/values_cases.py), a seeded fuzz of random expressions, the argument checks of the entry points, the header
against SYMBOLS and the numpy dtypes, the front end's `Value` path through HostColumns, ShuffleGatesValues against
ShuffleGates, and csrc/values_host.cpp under the address and undefined-behaviour sanitizers as a stand-alone program."""
import os
import random
import re
import subprocess

import numpy as np
import pytest

import halo2_gpu_specific_amd as h2
import values_cases as vc
from halo2_gpu_specific_amd import circuits_frontend as fe, prover, synthesis as syn, values as V
from halo2_gpu_specific_amd._lib import SYMBOLS
from halo2_gpu_specific_amd.values import Value
from values_cases import R_MOD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "halo2-gpu-specific_amd", "csrc")
CAPS = V.limits()


def field(seed, count):
    rng = random.Random(seed)
    return [rng.randrange(R_MOD) for _ in range(count)]


def launches(fn):
    """(result of fn, evaluator launches, inversions, the programs launched) on the host backend"""
    before = (V.HOST.values_launches, V.HOST.values_inversions)
    del V.LAST_PROGRAMS[:]
    out = fn()
    return out, V.HOST.values_launches - before[0], V.HOST.values_inversions - before[1], list(V.LAST_PROGRAMS)


# -- the compiler ----------------------------------------------------------------------------------------------------------------
def test_shared_subexpressions_are_evaluated_once():
    A, B = field(1, 9), field(2, 9)
    a, b = Value.from_ints(None, A), Value.from_ints(None, B)
    shared = a * b + 5
    x, y = shared * a, (b * a + 5) * b                       # the same product and sum, written twice, operands swapped
    (xs, ys), n, _, progs = launches(lambda: Value.materialize([x, y]))
    assert n == 1 and len(progs[0].ops) == 4                 # a b, + 5, * a, * b -- not 6
    assert vc.ints(xs) == [(p * q + 5) * p % R_MOD for p, q in zip(A, B)] and vc.ints(ys) == [(p * q + 5) * q % R_MOD for p, q in zip(A, B)]
    # materialised together or not, and again from the cache: no further launch
    assert launches(lambda: x.to_ints())[1] == 0
    # a sliced view of a shared expression shares too: the view reaches the leaves
    u, v = shared[2:8:2] * 3, (a[2:8:2] * b[2:8:2] + 5) - 1
    (_, n, _, progs) = launches(lambda: Value.materialize([u, v]))
    assert n == 1 and len(progs[0].ops) == 4


def tree(leaves, op):
    while len(leaves) > 1:
        leaves = [op(leaves[i], leaves[i + 1]) for i in range(0, len(leaves), 2)]
    return leaves[0]


def test_a_balanced_tree_of_128_leaves_fits_the_slot_cap():
    A = field(3, 128 + 40)
    a = Value.from_ints(None, A)
    t = tree([a[i:i + 40] for i in range(128)], lambda p, q: p * q)
    dag = V._Dag()
    whole = V._schedule(dag, [dag.add(t)], dict(CAPS, leaves=1 << 20))       # with room for the leaves: the slots alone
    assert len(whole.ops) == 127 and whole.slots_used <= CAPS["slots"] and whole.slots_used == 6
    # and as it is launched, split at the leaf cap: every launch within every cap, the values right
    got, n, _, progs = launches(t.to_ints)
    assert n == len(progs) > 1 and all(len(p.leaves) <= CAPS["leaves"] and p.slots_used <= CAPS["slots"] for p in progs)
    want = [1] * 40
    for i in range(128):
        want = [w * A[i + j] % R_MOD for j, w in enumerate(want)]
    assert got == want


def test_one_live_value_more_than_the_cap_splits_into_two_launches():
    A, B = field(4, 33), field(5, 33)
    a, b = Value.from_ints(None, A), Value.from_ints(None, B)
    terms = [a * b + i for i in range(CAPS["slots"] + 1)]                     # all of them are read before AND after their product
    u = terms[0]
    for t in terms[1:]:
        u = u * t
    v = u * terms[0]
    for t in terms[1:]:
        v = v + u * t
    dag = V._Dag()
    with pytest.raises(V._Overflow, match="slots"):
        V._schedule(dag, [dag.add(v)], CAPS)
    got, n, _, progs = launches(v.to_ints)
    assert n == 2 and all(p.slots_used <= CAPS["slots"] for p in progs)
    want = []
    for p, q in zip(A, B):
        ts = [(p * q + i) % R_MOD for i in range(CAPS["slots"] + 1)]
        prod = 1
        for t in ts:
            prod = prod * t % R_MOD
        want.append(sum(prod * t for t in ts) % R_MOD)
    assert got == want


@pytest.mark.parametrize("over", [0, 1], ids=["at the cap", "one beyond"])
def test_programs_at_and_beyond_each_cap(over):
    A = field(6, 64)
    a = Value.from_ints(None, A)
    # leaves: a sum of cap (+ 1) different views
    count = CAPS["leaves"] + over
    s = a[0:8]
    for i in range(1, count):
        s = s + a[i:i + 8]
    got, n, _, progs = launches(s.to_ints)
    assert n == 1 + over and max(len(p.leaves) for p in progs) == CAPS["leaves"]
    assert got == [sum(A[i + j] for i in range(count)) % R_MOD for j in range(8)]
    # ops: a chain of cap (+ 1) squarings and additions
    c, want = a[:8], A[:8]
    for i in range(CAPS["ops"] + over):
        c, want = (c.square(), [w * w % R_MOD for w in want]) if i % 2 else (c + a[8:16], [(w + x) % R_MOD for w, x in zip(want, A[8:16])])
    got, n, _, progs = launches(c.to_ints)
    assert n == 1 + over and max(len(p.ops) for p in progs) == CAPS["ops"] and got == want
    # constants: cap (+ 1) different ones (the first launch of a split keeps to the cap too)
    count = CAPS["constants"] + over
    k, want = a[:8], A[:8]
    for i in range(count):
        k, want = k * (1000 + i), [w * (1000 + i) % R_MOD for w in want]
    got, n, _, progs = launches(k.to_ints)
    assert n == 1 + over and max(len(p.constants) for p in progs) == CAPS["constants"] and got == want
    # outputs: cap (+ 1) Values materialised together
    outs = [a[:8] * (i + 2) for i in range(CAPS["outputs"] + over)]
    got, n, _, progs = launches(lambda: Value.materialize(outs))
    assert n == 1 + over and [vc.ints(g) for g in got] == [[x * (i + 2) % R_MOD for x in A[:8]] for i in range(len(outs))]


def test_divisions_are_staged_by_depth():
    A, B, C = field(7, 20), field(8, 20), field(9, 20)
    a, b, c = (Value.from_ints(None, x) for x in (A, B, C))
    inv = lambda x: pow(x, -1, R_MOD)                                        # noqa: E731
    got, n, i, _ = launches((a / b + b / c + c / a).to_ints)
    assert (n, i) == (2, 1) and got == [(p * inv(q) + q * inv(s) + s * inv(p)) % R_MOD for p, q, s in zip(A, B, C)]
    got, n, i, _ = launches((a / (b + c / a)).to_ints)
    assert (n, i) == (3, 2) and got == [p * inv((q + s * inv(p)) % R_MOD) % R_MOD for p, q, s in zip(A, B, C)]


# -- unknown ---------------------------------------------------------------------------------------------------------------------
def test_unknown_propagates_through_every_operator():
    u, a = Value.unknown(12), Value.from_ints(None, field(10, 12))
    results = [u + a, a + u, u - a, a - u, u * a, a * u, -u, u.square(), u ** 3, u + 1, 2 * u, 3 - u, u / a, a / u, 1 / u, u.invert(),
               u.is_zero(), Value.select(u, a, a), Value.select(a, u, a), Value.select(a, a, u), u.take([0, 1, 2] * 4)]
    assert all(not r.known and len(r) == 12 for r in results)
    assert not u.cumprod().known and len(u.cumprod()) == 13 and len(u.cumsum(5)) == 13
    assert len(Value.concat([u, a])) == 24 and not Value.concat([a, u]).known
    assert len(u[2:11:3]) == 3 and not u[2:11:3].known and len(u[5]) == 1 and len(u) == 12
    with pytest.raises(ValueError):
        u.tensor()
    with pytest.raises(ValueError):
        (u * a).to_ints()
    with pytest.raises(ValueError, match="12 and 5"):
        a + Value.from_ints(None, [1] * 5)
    with pytest.raises(ValueError, match="12 and 5"):
        u * Value.unknown(5)


# -- the host twin against integers --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", vc.SIZES)
def test_host_twin_matches_the_integers(m):
    L = h2.lib()
    for program in vc.programs(max(vc.SIZES)):
        assert program.decode(vc.run_host(L, program, m)) == program.expected(m), program.name
    cap = vc.slot_cap_program(max(vc.SIZES), CAPS["slots"])
    assert cap.decode(vc.run_host(L, cap, m)) == cap.expected(m)


@pytest.mark.parametrize("m", vc.SIZES)
def test_values_on_the_host_backend(m):
    rng = random.Random(m)
    A, B = vc.edge_field(rng, m), vc.edge_compact(rng, m)
    a, b = Value.from_ints(None, A), Value.from_u64(None, B)
    inv = lambda x: pow(x, -1, R_MOD) if x else 0                             # noqa: E731
    assert (a / b).to_ints() == [p * inv(q) % R_MOD for p, q in zip(A, B)]   # x / 0 = 0
    assert (a * a.invert()).to_ints() == [int(p != 0) for p in A]
    nonzero = Value.select(a.is_zero(), 1, a)
    assert (nonzero * nonzero.invert(strict=True)).to_ints() == [1] * m
    with pytest.raises(ZeroDivisionError, match="element 0 of the %d" % m):  # edge_field puts 0 first
        a.invert(strict=True).to_ints()
    z, s = [7], [R_MOD - 2]
    for p in A:
        z.append(z[-1] * p % R_MOD)
        s.append((s[-1] + p) % R_MOD)
    nz, zs = [1], None
    for p in A:
        nz.append(nz[-1] * (p or 1) % R_MOD)
    assert a.cumprod(7).to_ints() == z and a.cumsum(R_MOD - 2).to_ints() == s and nonzero.cumprod().to_ints() == nz
    assert a.cumsum().to_ints()[-1] == sum(A) % R_MOD and len(a.cumprod()) == m + 1
    order = list(range(m))
    rng.shuffle(order)
    assert a.take(order).to_ints() == [A[i] for i in order] and (b.take(order) * 2).to_ints() == [2 * B[i] % R_MOD for i in order]
    assert Value.concat([a, b * 1, a[::2]]).to_ints() == A + [q % R_MOD for q in B] + A[::2]
    assert Value.full(None, m, -1).to_ints() == [R_MOD - 1] * m and (a ** 5).to_ints() == [pow(p, 5, R_MOD) for p in A]
    assert a.cumprod()[1:m + 1:2].to_ints() == a.cumprod().to_ints()[1::2]   # a scan is materialised, then sliced
    got = a.tensor(montgomery=True)
    assert vc.ints(got) == [p * vc.R % R_MOD for p in A] and a.tensor(montgomery=True) is got


FUZZ_SEEDS, FUZZ_ROWS = 300, 200


@pytest.mark.parametrize("chunk", range(6))
def test_fuzz_random_expressions(chunk):
    leaves = vc.fuzz_leaves(None, FUZZ_ROWS)
    leaf_ints = [x[4] for x in vc.fuzz_inputs(FUZZ_ROWS)]
    for seed in range(chunk * FUZZ_SEEDS // 6, (chunk + 1) * FUZZ_SEEDS // 6):
        value, want = vc.fuzz_expression(seed, leaves, leaf_ints)
        assert value.to_ints() == want, seed


# -- validation ------------------------------------------------------------------------------------------------------------------
def test_entry_points_refuse_malformed_programs_by_name():
    L = h2.lib()
    m = 8
    data = vc.limbs(field(11, 32))
    out = np.zeros((m, 4), dtype=np.uint64)
    good_leaf, good_op, good_out = (data.ctypes.data, 0, 1, len(data), 0, 0), (vc.ADD, 0, vc.LEAF | 0, vc.CONST | 0, 0), (out.ctypes.data, 0, 0, 0)

    def run(leaf=good_leaf, ops=(good_op,), output=good_out, m=m, device=False, leaves=None, outputs=None, constants=1):
        leaves = np.array(leaves if leaves is not None else [leaf], dtype=V.VALUES_LEAF)
        ops = np.array(list(ops), dtype=np.uint32).reshape(-1, 5)
        outputs = np.array(outputs if outputs is not None else [output], dtype=V.VALUES_OUTPUT)
        consts = np.zeros((max(constants, 1), 4), dtype=np.uint64)
        args = (leaves.ctypes.data, len(leaves), consts.ctypes.data, constants, ops.ctypes.data, len(ops), outputs.ctypes.data, len(outputs), m)
        return L.h2_dev_values_eval(*(args + (None,))) if device else L.h2_values_eval(*args)

    slots = CAPS["slots"]
    bad = [(dict(ops=[(vc.ADD, slots, vc.LEAF | 0, vc.CONST | 0, 0)]), b"writes slot %d, at or above the cap" % slots),
           (dict(ops=[(vc.ADD, 0, vc.SLOT | slots, vc.CONST | 0, 0)]), b"reads slot %d, at or above the cap" % slots),
           (dict(ops=[(vc.ADD, 0, vc.SLOT | 1, vc.CONST | 0, 0)]), b"slot 1, which was never written"),
           (dict(ops=[(vc.ADD, 0, vc.LAST, vc.CONST | 0, 0)]), b"reads the last result, and there is none"),
           (dict(output=(out.ctypes.data, 0, 1, 0)), b"output 0 reads slot 1, which was never written"),
           (dict(leaf=(data.ctypes.data, 25, 1, len(data), 0, 0)), b"leaf 0 reaches beyond its buffer of 32 elements"),
           (dict(leaf=(data.ctypes.data, 0, 5, len(data), 0, 0)), b"leaf 0 reaches beyond its buffer"),
           (dict(leaf=(data.ctypes.data, 0, 0, len(data), 0, 0)), b"stride"),
           (dict(leaf=(data.ctypes.data, 0, 1, len(data), 3, 0)), b"leaf 0 has an unknown form code 3"),
           (dict(leaf=(0, 0, 1, len(data), 0, 0)), b"leaf 0 has a null pointer"),
           (dict(leaf=(data.ctypes.data + 4, 0, 1, 16, 0, 0)), b"misaligned"),
           (dict(ops=[(7, 0, vc.LEAF | 0, vc.CONST | 0, 0)]), b"op 0 has an unknown op code 7"),
           (dict(ops=[(vc.ADD, 0, 4 << 24, vc.CONST | 0, 0)]), b"operand of unknown kind 4"),
           (dict(ops=[(vc.ADD, 0, vc.LEAF | 1, vc.CONST | 0, 0)]), b"reads leaf 1, which does not exist"),
           (dict(ops=[(vc.ADD, 0, vc.LEAF | 0, vc.CONST | 1, 0)]), b"reads constant 1, which does not exist"),
           (dict(output=(out.ctypes.data, 0, 0, 2)), b"output 0 has an unknown form code 2"),
           (dict(output=(data.ctypes.data + 32, 0, 0, 0)), b"output 0 overlaps leaf 0"),            # shifted by one element
           (dict(output=(data.ctypes.data, 0, 0, 0), leaf=(data.ctypes.data, 0, 2, len(data), 0, 0)), b"output 0 overlaps leaf 0"),
           (dict(outputs=[good_out, (out.ctypes.data, 0, 0, 1)]), b"output 1 overlaps output 0"),
           (dict(leaves=[good_leaf] * (CAPS["leaves"] + 1)), b"%d leaves, the cap is %d" % (CAPS["leaves"] + 1, CAPS["leaves"])),
           (dict(ops=[good_op] * (CAPS["ops"] + 1)), b"%d ops, the cap is %d" % (CAPS["ops"] + 1, CAPS["ops"])),
           (dict(constants=CAPS["constants"] + 1), b"constants, the cap is"),
           (dict(outputs=[good_out] * (CAPS["outputs"] + 1)), b"outputs, the cap is")]
    for device, name in ((False, b"h2_values_eval: "), (True, b"h2_dev_values_eval: ")):
        for kw, text in bad:
            if device and b"misaligned" in text:
                continue
            assert run(device=device, **kw) == 1, kw
            message = L.h2_last_error()
            assert message.startswith(name) and text in message, (kw, message)
        assert run(device=device, m=0, leaf=(0, 99, 0, 0, 9, 0)) == 0                                  # m = 0: nothing is looked at
    assert run(device=True, leaf=(data.ctypes.data + 8, 0, 1, 16, 0, 0)) == 1 and b"misaligned" in L.h2_last_error()
    assert not out.any()
    # the same element mapping is allowed: in place, and the stated rule's other side (a compact leaf) is not
    work = data.copy()
    assert run(leaf=(work.ctypes.data, 4, 1, len(work), 0, 0), output=(work.ctypes.data, 4, 0, 0),
               ops=[(vc.ADD, 0, vc.LEAF | 0, vc.LEAF | 0, 0)]) == 0
    assert vc.ints(work[4:4 + m]) == [2 * v % R_MOD for v in vc.ints(data[4:4 + m])] and np.array_equal(work[:4], data[:4])
    assert np.array_equal(work[4 + m:], data[4 + m:])
    assert run(leaf=(work.ctypes.data, 0, 1, 4 * len(work), 2, 0), output=(work.ctypes.data, 0, 0, 0)) == 1
    assert run() == 0 and vc.ints(out) == vc.ints(data[:m])


def test_header_symbols_and_dtypes_agree():
    text = open(os.path.join(ROOT, "include", "halo2_hip.h")).read()
    plain = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    L = h2.lib()
    names = ("h2_values_limits", "h2_dev_values_eval", "h2_values_eval")
    for name in names:
        declared = re.search(r"\b%s\s*\(([^)]*)\)" % name, plain)
        assert declared and name in SYMBOLS and hasattr(L, name), name
        assert len(declared.group(1).split(",")) == len(SYMBOLS[name][1]), name
    assert sorted(n for n in SYMBOLS if "values" in n) == sorted(names)
    sizes = {"uint64_t": 8, "uint32_t": 4}
    for struct, dtype, size in (("h2_values_leaf", V.VALUES_LEAF, 40), ("h2_values_op", V.VALUES_OP, 20),
                                ("h2_values_output", V.VALUES_OUTPUT, 24), ("h2_values_caps", V.VALUES_CAPS, 32)):
        body = re.search(r"typedef struct \{([^}]*)\} %s;" % struct, plain).group(1)
        fields = re.findall(r"(\w+)\s+(\w+);", body)
        assert [name for _, name in fields] == list(dtype.names), struct
        assert dtype.itemsize == size == sum(sizes[kind] for kind, _ in fields), struct
    for name, code in V.OP_CODES.items():
        assert re.search(r"H2_VALUES_%s = %d\b" % (name.upper(), code), plain), name
    assert re.search(r"H2_VALUES_LEAF = 0, H2_VALUES_CONST = 1, H2_VALUES_SLOT = 2, H2_VALUES_LAST = 3", plain)
    assert re.search(r"#define H2_VALUES_NO_SLOT 0x%xu" % V.NO_SLOT, plain)
    assert "a < 2^256" in text and "Overlap rule" in text               # the header says which inputs are reduced and which overlap is allowed
    srcs = open(os.path.join(CSRC, "Makefile")).read()
    assert " values.hip " in srcs and " values.hpp " in srcs and "values_host.o" in srcs
    assert prover.Value is Value
    assert set(CAPS) == {"leaves", "ops", "constants", "outputs", "slots", "blocks", "threads"} and CAPS["threads"] == 256


# -- the front end ---------------------------------------------------------------------------------------------------------------
class Products(syn.Circuit):
    """c = a * b over `count` rows, then d = c[::2] + 1 computed from the assigned cells' own values"""
    planner = syn.V1

    def __init__(self, a, b, count):
        self.a, self.b, self.count = a, b, count

    def without_witnesses(self):
        return Products(Value.unknown(self.count), Value.unknown(self.count), self.count)

    def configure(self, cs):
        return [cs.advice_column() for _ in range(4)]

    def synthesize(self, config, layouter):
        def body(region):
            a = region.assign_advice(config[0], 0, self.a, count=self.count)
            b = region.assign_advice(config[1], 0, self.b, count=self.count)
            c = region.assign_advice(config[2], 0, a.value() * b.value())
            d = region.assign_advice(config[3], 1, c[::2].value() + 1, stride=2)
            region.assign_advice(config[3], 3, 99)                      # a later overlapping assignment wins
            return a, c, d

        return layouter.assign_region("products", body)


def test_assigning_values_through_the_host_assembly():
    A, B = field(12, 10), field(13, 10)
    circuit = Products(Value.from_ints(None, A), Value.from_ints(None, B), 10)
    cs, fixed, copies = prover.synthesize_keygen(None, circuit, 5)
    # keygen with unknowns is keygen with None: cells assigned from None have an unknown value, and so has all that follows
    cs_none, fixed_none, copies_none = prover.synthesize_keygen(None, Products(None, None, 10), 5)
    assert np.array_equal(copies, copies_none) and len(fixed) == len(fixed_none) == 0
    advice, first = prover.synthesize_witness(None, circuit, cs, 5, resident=False)
    C = [p * q % R_MOD for p, q in zip(A, B)]
    assert vc.ints(advice[2][:10]) == C and vc.ints(advice[0][:10]) == A
    want_d = [0] * 32
    want_d[1:11:2] = [(c + 1) % R_MOD for c in C[::2]]
    want_d[3] = 99
    assert vc.ints(advice[3]) == want_d and first == {0: 10, 1: 10, 2: 10, 3: 10}
    with pytest.raises(ValueError, match="10 values for 4 cells"):
        syn._Values(Value.unknown(10), 4)


def test_cells_carry_their_value_and_slice_it():
    A = field(14, 9)
    v = Value.from_ints(None, A)
    cells = syn.AssignedCells(("advice", 0), 3, 9, 2, v)
    assert cells.value() is v and cells[1:8:3].value().to_ints() == A[1:8:3] and cells[-1].value().to_ints() == [A[-1]]
    assert (cells[1:8:3].row, cells[1:8:3].stride, len(cells[1:8:3])) == (5, 6, 3)
    plain = syn.AssignedCells(("advice", 0), 3, 9, 2)                     # the positional constructor, repr and rows() as before
    assert repr(plain) == repr(cells) == "AssignedCells(advice[0], row 3, 9 x 2)" and plain.rows().tolist() == cells.rows().tolist()
    assert not plain.value().known and len(plain.value()) == 9 and len(plain[2:5].value()) == 3


def test_shuffle_gates_values_reproduces_shuffle_gates():
    """cannot pass without the feature: the witness of ShuffleGatesValues exists only as Values"""
    k = 6
    old, new = fe.ShuffleGates(k), fe.ShuffleGatesValues(k)
    cs, fixed, copies = prover.synthesize_keygen(None, old, k)
    cs2, fixed2, copies2 = prover.synthesize_keygen(None, new, k)
    assert all(np.array_equal(x, y) for x, y in zip(fixed, fixed2)) and np.array_equal(copies, copies2)
    advice, first = prover.synthesize_witness(None, old, cs, k, resident=False)
    (advice2, first2), n, i, _ = launches(lambda: prover.synthesize_witness(None, new, cs2, k, resident=False))
    assert first == first2 and all(np.array_equal(x, y) for x, y in zip(advice, advice2))
    assert (n, i) == (3, 1)                                               # denominators, quotients, z in canonical form; one inversion
    # and at the full height of k = 9: z returns to 1
    k = 9
    tall = fe.ShuffleGatesValues(k, height=(1 << k) - 7)
    assert tall.columns()[-1][(1 << k) - 7].to_ints() == [1]


# -- the host code under the sanitizers ----------------------------------------------------------------------------------------
def test_values_host_under_the_sanitizers(tmp_path):
    """a stand-alone program: nothing is preloaded into Python"""
    exe = tmp_path / "values_host_main"
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    cmd = ["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-g", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(rocm, "include"), "-I", CSRC,
           os.path.join(ROOT, "tests", "values_host_main.cpp"), os.path.join(CSRC, "values_host.cpp"), "-o", str(exe)]
    built = subprocess.run(cmd, capture_output=True, text=True, timeout=240)
    assert built.returncode == 0, built.stderr[-4000:]
    ran = subprocess.run([str(exe), "200"], capture_output=True, text=True, timeout=120)
    assert ran.returncode == 0 and not ran.stderr and ran.stdout.split() == ["ok", "200"], (ran.returncode, ran.stdout[-500:], ran.stderr[-3000:])
