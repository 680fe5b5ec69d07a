"""The integer half of Values without a GPU: the host twin h2_values_eval on TO_INT, TO_FIELD, EXTRACT, LT, AND, OR and XOR
against Python integers (tests/values_int_cases.py), the kinds the lowering tracks and refuses by name, the compiler's
conversions (inserted once, shared by hash-consing, re-inserted where a split gives up an integer), limbs and their launch
counts, `strict` and `take` by a Value, a seeded fuzz of expressions that cross between the kinds, LimbDecomposition through
the host assembly, and csrc/values_host.cpp under the address and undefined-behaviour sanitizers as a stand-alone program."""
import os
import random
import subprocess

import numpy as np
import pytest

import halo2_gpu_specific_amd as h2
import values_cases as vc
import values_int_cases as ic
from halo2_gpu_specific_amd import circuits_frontend as fe, prover, values as V
from halo2_gpu_specific_amd.values import Value
from values_cases import R_MOD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "halo2-gpu-specific_amd", "csrc")
CAPS = V.limits()
CODES = V.OP_CODES


def field(seed, count):
    rng = random.Random(seed)
    return [rng.randrange(R_MOD) for _ in range(count)]


def launches(fn):
    """(result of fn, evaluator launches, the programs launched) on the host backend"""
    before = V.HOST.values_launches
    del V.LAST_PROGRAMS[:]
    out = fn()
    return out, V.HOST.values_launches - before, list(V.LAST_PROGRAMS)


def count_ops(programs, name):
    return sum(op[0] == CODES[name] for p in programs for op in p.ops)


# -- the host twin against integers --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", ic.SIZES)
def test_host_twin_matches_the_integers(m):
    L = h2.lib()
    cases = ic.programs(max(ic.SIZES))
    assert len(cases) == 2 * len(ic.EXTRACT_LO) + 6 + 5
    for program in cases:
        assert program.decode(vc.run_host(L, program, m)) == program.expected(m), program.name


def test_the_named_edges_are_among_the_cases():
    """what the tables above are asked about is really there: (r - 1) | 1 == 0, an OR at or above r, 2^256 - 1 through TO_INT"""
    m = 16
    by_name = {p.name: p for p in ic.programs(max(ic.SIZES))}
    x, y = (leaf.values(m) for leaf in by_name["bitwise"].leaves)
    got = by_name["bitwise"].expected(m)
    assert (x[2], y[2]) == (R_MOD - 1, 1) and got[1][2] == 0 and got[3][2] == 1
    assert x[7] | y[7] >= R_MOD and got[1][7] == (x[7] | y[7]) - R_MOD and got[2][7] == (x[7] ^ y[7]) - R_MOD
    lt = by_name["lt"].expected(m)
    assert [lt[0][i] for i in range(5)] == [0, 1, 0, 0, 0] and [lt[1][i] for i in range(5)] == [1, 0, 1, 0, 0] and not any(lt[2])
    assert x[5] >> 224 != y[5] >> 224 and x[5] % (1 << 224) == y[5] % (1 << 224) and x[6] >> 32 == y[6] >> 32 and x[6] != y[6]
    raw = vc.ints(by_name["to_int"].leaves[0].data[by_name["to_int"].leaves[0].first:][:1])
    assert raw == [(1 << 256) - 1] and by_name["to_int"].expected(1)[0] == [((1 << 256) - 1) % R_MOD]


# -- kinds ---------------------------------------------------------------------------------------------------------------------------
def test_entry_points_refuse_kind_mismatches_by_name():
    L = h2.lib()
    m = 8
    data = vc.limbs(field(11, 32))
    out = np.zeros((m, 4), dtype=np.uint64)
    LEAF, CONST, SLOT, LAST = vc.LEAF, vc.CONST, vc.SLOT, vc.LAST
    to_int = (ic.TO_INT, 0, LEAF | 0, 0, 0)

    def run(ops, device):
        leaves = np.array([(data.ctypes.data, 0, 1, len(data), 0, 0)], dtype=V.VALUES_LEAF)
        ops = np.array(list(ops), dtype=np.uint32).reshape(-1, 5)
        outputs = np.array([(out.ctypes.data, 0, 0, 0)], dtype=V.VALUES_OUTPUT)
        consts = np.zeros((1, 4), dtype=np.uint64)
        args = (leaves.ctypes.data, 1, consts.ctypes.data, 1, ops.ctypes.data, len(ops), outputs.ctypes.data, 1, m)
        return L.h2_dev_values_eval(*(args + (None,))) if device else L.h2_values_eval(*args)

    bad = [([to_int, (vc.ADD, 0, SLOT | 0, LEAF | 0, 0)], b"op 1 takes a field value in operand a; slot 0 holds an integer"),
           ([to_int, (vc.MUL, 0, LEAF | 0, LAST, 0)], b"op 1 takes a field value in operand b; the last result is an integer"),
           ([to_int, (vc.SQR, 0, SLOT | 0, 0, 0)], b"op 1 takes a field value in operand a"),
           ([to_int, (vc.NEG, 0, LAST, 0, 0)], b"op 1 takes a field value in operand a"),
           ([to_int, (vc.SUB, 0, LEAF | 0, SLOT | 0, 0)], b"op 1 takes a field value in operand b; slot 0 holds an integer"),
           ([to_int, (ic.TO_INT, 0, SLOT | 0, 0, 0)], b"op 1 takes a field value in operand a; slot 0 holds an integer"),
           ([(vc.ADD, 2, LEAF | 0, CONST | 0, 0), (ic.EXTRACT, 0, SLOT | 2, 0, 8)], b"op 1 takes an integer in operand a; slot 2 holds a field value"),
           ([(vc.ADD, 2, LEAF | 0, CONST | 0, 0), (ic.TO_FIELD, 0, LAST, 0, 0)], b"op 1 takes an integer in operand a; the last result is a field value"),
           ([to_int, (vc.ADD, 1, LEAF | 0, CONST | 0, 0), (ic.LT, 0, SLOT | 0, SLOT | 1, 0)], b"op 2 takes an integer in operand b; slot 1 holds a field value"),
           ([(ic.EXTRACT, 0, LEAF | 0, 0, 8)], b"op 0 takes an integer in operand a; leaf 0 is a field value"),
           ([to_int, (ic.AND, 0, SLOT | 0, CONST | 0, 0)], b"op 1 takes an integer in operand b; constant 0 is a field value"),
           ([to_int, (ic.XOR, 0, LEAF | 0, SLOT | 0, 0)], b"op 1 takes an integer in operand a; leaf 0 is a field value"),
           ([to_int, (ic.OR, 0, SLOT | 0, LEAF | 0, 0)], b"op 1 takes an integer in operand b; leaf 0 is a field value"),
           ([to_int, (vc.SELECT, 0, LEAF | 0, SLOT | 0, LEAF | 0)], b"op 1 selects between a field value and an integer"),
           ([to_int, (vc.SELECT, 0, SLOT | 0, CONST | 0, SLOT | 0)], b"op 1 selects between a field value and an integer"),
           ([to_int, (ic.EXTRACT, 0, SLOT | 0, 256, 1)], b"op 1 extracts from bit 256: lo must be between 0 and 255"),
           ([to_int, (ic.EXTRACT, 0, SLOT | 0, 0, 0)], b"op 1 extracts 0 bits: n must be between 1 and 256"),
           ([to_int, (ic.EXTRACT, 0, SLOT | 0, 255, 257)], b"op 1 extracts 257 bits: n must be between 1 and 256")]
    bad += [([(code, 0, LEAF | 0, CONST | 0, 0)], b"op 0 has an unknown op code %d" % code) for code in list(range(7, 16)) + [23, 0xFE]]
    for device, name in ((False, b"h2_values_eval: "), (True, b"h2_dev_values_eval: ")):
        for ops, text in bad:
            assert run(ops, device) == 1, ops
            message = L.h2_last_error()
            assert message.startswith(name) and text in message, (ops, message)
    assert not out.any()
    # and what is allowed: either kind in ISZERO and in SELECT's condition, integer arms, an integer straight to an output
    good = [to_int, (ic.EXTRACT, 1, SLOT | 0, 255, 256), (vc.ISZERO, 2, SLOT | 1, 0, 0), (vc.SELECT, 0, SLOT | 2, SLOT | 0, SLOT | 1)]
    assert run(good, False) == 0 and vc.ints(out) == vc.ints(data[:m])          # v >> 255 is 0 below r: ISZERO 1, the first arm


# -- the compiler --------------------------------------------------------------------------------------------------------------------
def test_limbs_share_one_conversion_and_count_their_launches():
    A = field(1, 40)
    a = Value.from_ints(None, A)
    got, n, progs = launches(lambda: Value.materialize(a.limbs(8, 4)))
    assert n == 1 and count_ops(progs, "to_int") == 1 and count_ops(progs, "extract") == 4 and len(progs[0].ops) == 5
    assert [vc.ints(g) for g in got] == [[(v >> 8 * j) & 0xFF for v in A] for j in range(4)]
    got, n, progs = launches(lambda: Value.materialize((a * a).limbs(8, 32)))
    assert n == -(-32 // CAPS["outputs"]) and count_ops(progs, "to_int") == n      # once per launch
    assert [vc.ints(g) for g in got] == [[(v * v % R_MOD >> 8 * j) & 0xFF for v in A] for j in range(32)]
    # from_u64 -> limbs: no product at all -- the to_int of a compact leaf is a copy, the canonical outputs of integers plain stores
    c = Value.from_u64(None, [v & vc.MASK64 for v in A])
    got, n, progs = launches(lambda: Value.materialize(c.limbs(16, 4)))
    assert n == 1 and [op[0] for op in progs[0].ops] == [CODES["to_int"]] + [CODES["extract"]] * 4
    assert [vc.ints(g) for g in got] == [[(v & vc.MASK64) >> 16 * j & 0xFFFF for v in A] for j in range(4)]
    with pytest.raises(ValueError, match="bits \\* count <= 256"):
        a.limbs(8, 33)


def test_an_expression_mixing_kinds_gets_each_conversion_once():
    A, B = field(2, 33), field(3, 33)
    a, b = Value.from_ints(None, A), Value.from_ints(None, B)
    p = a * b
    low, flag = p.low(40), p.lt(b)                                    # two integer readers of p, one of b
    x = low * 3 + flag * low + (p & b) * p                            # three field readers of `low`, none converts p back
    got, n, progs = launches(x.to_ints)
    assert n == 1 and count_ops(progs, "to_int") == 2 and count_ops(progs, "to_field") == 3   # p, b; low, flag, p & b
    P = [u * v % R_MOD for u, v in zip(A, B)]
    assert got == [((u % (1 << 40)) * 3 + int(u < v) * (u % (1 << 40)) + (u & v) * u) % R_MOD for u, v in zip(P, B)]
    # there and back again is the value itself: a bit field of a bit field converts nothing in between
    got, n, progs = launches(p.low(100).bits(3, 20).to_ints)
    assert count_ops(progs, "to_int") == 1 and count_ops(progs, "to_field") == 0 and got == [u % (1 << 100) >> 3 & 0xFFFFF for u in P]
    # a select whose arms are integers stays one; a select between the kinds converts the integer arm
    s = Value.select(a.lt(b), a.low(8), b.low(8)) ^ 1
    got, n, progs = launches(s.to_ints)
    assert count_ops(progs, "to_field") == 0 and got == [((u if u < v else v) & 0xFF) ^ 1 for u, v in zip(A, B)]
    t = Value.select(a.bit(0), a.low(8), b)
    got, n, progs = launches(t.to_ints)
    assert count_ops(progs, "to_field") == 1 and got == [u & 0xFF if u & 1 else v for u, v in zip(A, B)]


def test_integer_expressions_split_at_the_op_cap_and_at_the_slot_cap():
    A, B = field(4, 21), field(5, 21)
    a, b = Value.from_ints(None, A), Value.from_ints(None, B)
    # a chain of integer ops alone, longer than one launch: every candidate to give up is an integer
    y, want = a.low(200), [u % (1 << 200) for u in A]
    for i in range(CAPS["ops"] + 30):
        if i % 2:
            y, want = y ^ b.low(100 + i % 50), [w ^ v % (1 << (100 + i % 50)) for w, v in zip(want, B)]
        else:
            y, want = (y & (a >> 3)) | 5, [w & (u >> 3) | 5 for w, u in zip(want, A)]
    planned = len(V.plan([y]))                                        # before the elements exist: afterwards y is read, not computed
    got, n, progs = launches(y.to_ints)
    assert n == planned > 1 and all(len(p.ops) <= CAPS["ops"] for p in progs) and got == [w % R_MOD for w in want]
    # slots + 1 integers, all read before AND after their xor: one live value more than the cap
    terms = [(a * b + i).low(64 + i) for i in range(CAPS["slots"] + 1)]
    u = terms[0]
    for t in terms[1:]:
        u = u ^ t
    v = u & terms[0]
    for t in terms[1:]:
        v = v | (u & t)
    dag = V._Dag()
    with pytest.raises(V._Overflow, match="slots"):
        V._schedule(dag, [dag.add(v)], CAPS)
    got, n, progs = launches(v.to_ints)
    assert n >= 2 and all(p.slots_used <= CAPS["slots"] for p in progs)
    want = []
    for p, q in zip(A, B):
        ts = [(p * q + i) % R_MOD % (1 << (64 + i)) for i in range(CAPS["slots"] + 1)]
        x = 0
        for t in ts:
            x ^= t
        acc = 0
        for t in ts:
            acc |= x & t
        want.append(acc)
    assert got == want


def test_six_integers_live_at_once():
    """register slot 0 and every LDS slot hold an integer: the compiler's program uses all the slots"""
    A = field(6, 19)
    a = Value.from_ints(None, A)
    parts = [a.bits(9 * i, 40 + i) for i in range(CAPS["slots"] - 1)]  # five bit fields and their xor, all read again afterwards
    u = parts[0]
    for t in parts[1:]:
        u = u ^ t
    v = u
    for t in parts:
        v = (v | t) ^ t
    got, n, progs = launches(v.to_ints)
    assert n == 1 and progs[0].slots_used == CAPS["slots"] == 6
    want = []
    for p in A:
        ts = [(p >> 9 * i) % (1 << (40 + i)) for i in range(5)]
        acc = 0
        for t in ts:
            acc ^= t
        for t in ts:
            acc = (acc | t) ^ t
        want.append(acc)
    assert got == want
    cap = ic.slot_cap_program(max(ic.SIZES), CAPS["slots"])
    assert cap.decode(vc.run_host(h2.lib(), cap, 257)) == cap.expected(257)


def test_unknown_propagates_through_every_new_method():
    u, a = Value.unknown(12), Value.from_ints(None, field(7, 12))
    results = [u.bits(3, 9), u >> 4, u >> 300, u.low(8), u.bit(0), u & a, a & u, u & 255, 255 & u, u | a, a | u, 1 | u, u ^ a, a ^ u, 7 ^ u,
               u.lt(a), a.lt(u), u.lt(5), u.le(a), a.le(u), u.gt(a), a.gt(u), u.ge(a), a.ge(u), a.take(u), u.take(a), u.take(u)]
    results += u.limbs(8, 4) + u.limbs(8, 4, strict=True)
    assert len(results) == 35 and all(not r.known and len(r) == 12 for r in results)
    assert len(u.take(a[:5])) == 5 and len(a.take(Value.unknown(3))) == 3


# -- strict and take -------------------------------------------------------------------------------------------------------------------
def test_strict_limbs_name_the_row_that_does_not_fit():
    A = [v % (1 << 32) for v in field(8, 50)]
    A[17] = 1 << 32
    A[30] = R_MOD - 1
    a = Value.from_ints(None, A)
    with pytest.raises(ValueError, match="element 17 of the 50 does not fit 4 limbs of 8 bits"):
        Value.materialize(a.limbs(8, 4, strict=True))
    with pytest.raises(ValueError, match="element 17 of the 50"):
        a.limbs(8, 4, strict=True)[2].to_ints()
    got, n, progs = launches(lambda: Value.materialize(a.low(32).limbs(8, 4, strict=True)))
    assert n == 2 and [vc.ints(g) for g in got] == [[(v % (1 << 32) >> 8 * j) & 0xFF for v in A] for j in range(4)]
    whole, n, _ = launches(lambda: Value.materialize(a.limbs(64, 4, strict=True)))             # 256 bits: nothing above to check
    assert n == 1 and [vc.ints(g) for g in whole] == [[(v >> 64 * j) & vc.MASK64 for v in A] for j in range(4)]


def test_take_by_a_value_of_integers():
    T, A = field(9, 40), field(10, 25)
    table, a = Value.from_ints(None, T), Value.from_ints(None, A)
    index = a.low(5)
    assert table.take(index).to_ints() == [T[v % 32] for v in A]
    assert (table * 2).take(a.bits(7, 5) + 3)[::3].to_ints() == [2 * T[(v >> 7) % 32 + 3] % R_MOD for v in A][::3]
    assert table.take(np.arange(39, -1, -1)).to_ints() == T[::-1]                                # host arrays as before
    at_len = Value.from_ints(None, [0, 39, 40, 1])
    with pytest.raises(IndexError, match="index 40 at row 2 is out of range for 40 elements"):
        table.take(at_len).to_ints()
    high = Value.from_ints(None, [3, 1 << 64, 5])                                                # the low word is in range
    with pytest.raises(IndexError, match="index %d at row 1 is out of range for 40 elements" % (1 << 64)):
        table.take(high).to_ints()
    with pytest.raises(IndexError, match="at row 0"):
        table.take(Value.from_ints(None, [-1])).to_ints()


# -- fuzz ----------------------------------------------------------------------------------------------------------------------------
FUZZ_SEEDS, FUZZ_ROWS = 300, 200


@pytest.mark.parametrize("chunk", range(6))
def test_fuzz_random_expressions_across_the_kinds(chunk):
    leaves = vc.fuzz_leaves(None, FUZZ_ROWS)
    leaf_ints = [x[4] for x in vc.fuzz_inputs(FUZZ_ROWS)]
    for seed in range(chunk * FUZZ_SEEDS // 6, (chunk + 1) * FUZZ_SEEDS // 6):
        value, want = ic.fuzz_expression(seed, leaves, leaf_ints)
        (got,), _, progs = launches(lambda: Value.materialize([value]))
        assert vc.ints(got) == want, seed
        assert count_ops(progs, "to_int") >= 1 and count_ops(progs, "to_field") >= 1 and count_ops(progs, "extract") >= 1, seed


# -- the front end -------------------------------------------------------------------------------------------------------------------
def limb_decomposition_columns(circuit):
    """the witness of LimbDecomposition by numpy and Python integers: [a, b, p] + limbs as lists of `height` integers"""
    a, b = circuit.witness_inputs()
    p = [int(x) * int(y) % (1 << (circuit.bits * circuit.words)) for x, y in zip(a, b)]
    return [[int(x) for x in a], [int(y) for y in b], p] + [[(v >> circuit.bits * j) % (1 << circuit.bits) for v in p] for j in range(circuit.words)]


def test_limb_decomposition_through_the_host_assembly():
    k = 9
    circuit = fe.LimbDecomposition(k)
    cs, fixed, copies = prover.synthesize_keygen(None, circuit, k)
    assert not any(v.known for v in circuit.without_witnesses().columns())
    assert (cs.num_advice, cs.num_fixed) == (7, 2)
    advice, first = prover.synthesize_witness(None, circuit, cs, k, resident=False)
    want, H = limb_decomposition_columns(circuit), circuit.height
    assert H == (1 << k) - 6 and first == {i: H for i in range(7)}
    for column, values in zip(advice, want):
        assert vc.ints(column[:H]) == values and not column[H:].any()
    assert vc.ints(fixed[0]) == [1] * H + [0] * 6 and vc.ints(fixed[1])[:256] == list(range(256))
    # other shapes: 3 limbs of 5 bits over 100 rows
    small = fe.LimbDecomposition(k, bits=5, words=3, height=100)
    cs, _, _ = prover.synthesize_keygen(None, small, k)
    advice, _ = prover.synthesize_witness(None, small, cs, k, resident=False)
    for column, values in zip(advice, limb_decomposition_columns(small)):
        assert vc.ints(column[:100]) == values


# -- the host code under the sanitizers ----------------------------------------------------------------------------------------
def test_values_int_host_under_the_sanitizers(tmp_path):
    """a stand-alone program: nothing is preloaded into Python"""
    exe = tmp_path / "values_int_host_main"
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    cmd = ["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-g", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(rocm, "include"), "-I", CSRC,
           os.path.join(ROOT, "tests", "values_int_host_main.cpp"), os.path.join(CSRC, "values_host.cpp"), "-o", str(exe)]
    built = subprocess.run(cmd, capture_output=True, text=True, timeout=240)
    assert built.returncode == 0, built.stderr[-4000:]
    ran = subprocess.run([str(exe), "200"], capture_output=True, text=True, timeout=120)
    assert ran.returncode == 0 and not ran.stderr and ran.stdout.split() == ["ok", "200"], (ran.returncode, ran.stdout[-500:], ran.stderr[-3000:])
