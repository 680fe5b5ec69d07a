"""The host side of prover.check_witness, without a GPU: the big-integer reference checker (tests/check_reference.py) on
hand-made circuits, the mapping of check records to MockProver's failures (sorting, truncation), and the argument checks
of the h2_dev_check_* entry points."""
import ctypes
import os
import sys

import numpy as np
import pytest

from check_reference import COPY, GATE, LOOKUP, SHUFFLE, reference_check

import halo2_gpu_specific_amd as h2
from halo2_gpu_specific_amd import circuit as hc
from halo2_gpu_specific_amd import check, circuits, prover

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import prover_fuzz  # noqa: E402


def tiny():
    """a * b = c at rows where q is on, c[r] + a[r + 1] = b[r - 1] everywhere q2 is on, a lookup of a into t, a shuffle of
    b into c, equality on a and c"""
    cs = hc.ConstraintSystem("tiny")
    a, b, c = cs.advice_column(), cs.advice_column(), cs.advice_column()
    q, q2, t = cs.fixed_column(), cs.fixed_column(), cs.fixed_column()
    cs.enable_equality(a)
    cs.enable_equality(c)
    qa, qb, qc = cs.query_advice(a), cs.query_advice(b), cs.query_advice(c)
    cs.create_gate("mul", [cs.query_fixed(q) * (qa * qb - qc)])
    cs.create_gate("rot", [cs.query_fixed(q2) * (qc + cs.query_advice(a, 1) - cs.query_advice(b, -1))])
    cs.lookup_any("in t", [cs.query_fixed(t)], [[[qa]], [[qb * 0 + qa + 0]]])
    cs.shuffle_group([("b to c", [qb], [qc])])
    return cs


def test_reference_checker_on_a_hand_made_circuit():
    cs = tiny()
    n = 16
    usable = n - (cs.blinding_factors() + 1)
    assert usable == 10
    # rows 0..9 usable: a = 1..10 (in t), b = 2, c = 2a; the shuffle b -> c fails unless the multisets agree
    a = [1 + r for r in range(usable)] + [0] * (n - usable)
    b = [2] * usable + [0] * (n - usable)
    c = [2 * v for v in a[:usable]] + [0] * (n - usable)
    q = [1] * usable + [0] * (n - usable)
    q2 = [0] * n
    t = list(range(1, 11)) + [1] * (n - 10)
    mapping = prover.permutation_mapping(2, n, [(0, 0, 1, 0)])        # a[0] = c[0]: 1 != 2
    got = reference_check(cs, n, [a, b, c], [q, q2, t], [], mapping)
    shuffle_rows = [r for r in range(usable)]                           # 2 occurs 10 times as input, once as shuffle
    assert got == ([(SHUFFLE, 0, 0, r) for r in shuffle_rows] + [(COPY, 0, 0, 0), (COPY, 1, 0, 0)])
    # break the gate at row 4, a lookup at row 6 (set 0 misses first), turn q2 on at row 3 (reads a[4], b[2])
    a2 = list(a)
    a2[6] = 77
    b2 = list(b)
    b2[4] = 3
    q2b = list(q2)
    q2b[3] = 1
    got = reference_check(cs, n, [a2, b2, c], [q, q2b, t], [], mapping, circuit=1)
    gates = [(GATE | 1 << 8, 0, 0, 4), (GATE | 1 << 8, 0, 0, 6), (GATE | 1 << 8, 1, 0, 3)]
    assert [g for g in got if g[0] & 0xFF == GATE] == gates
    assert [g for g in got if g[0] & 0xFF == LOOKUP] == [(LOOKUP | 1 << 8, 0, 0, 6)]
    # c[3] + a[4] = 8 + 5 = 13 != b[2] = 2: the rotation reads the rows around 3; rows past n wrap
    assert reference_check(cs, n, [a2, b2, c], [q, q2b, t], [], mapping, gate_rows=[3, 4, 99])[:2] == \
        [(GATE, 0, 0, 4), (GATE, 1, 0, 3)]


def test_reference_checker_on_examples():
    k = 6
    cs = circuits.lookup_api()
    adv, fixed, copies = circuits.lookup_api_synthesize(k)
    mapping = prover.permutation_mapping(len(cs.perm_columns), 1 << k, copies)
    assert reference_check(cs, 1 << k, adv, fixed, [], mapping) == []
    adv[2][1, 0] = 77
    assert (LOOKUP, 0, 0, 1) in reference_check(cs, 1 << k, adv, fixed, [], mapping)
    cs = circuits.shuffle_api_group()
    adv, fixed, copies = circuits.shuffle_api_group_synthesize(k, input1=(4, 1, 1, 3))
    got = reference_check(cs, 1 << k, adv, fixed, [], prover.permutation_mapping(0, 1 << k, copies))
    assert got and all(r[0] == SHUFFLE for r in got)


@pytest.mark.parametrize("seed", range(4))
def test_reference_checker_accepts_satisfiable_random_circuits(seed):
    cs, k, adv, fixed, copies, inst = prover_fuzz.random_case(seed, satisfiable=True)
    n = 1 << k
    assert reference_check(cs, n, adv, fixed, inst, prover.permutation_mapping(len(cs.perm_columns), n, copies)) == []


def test_records_to_failures_sorting_and_truncation():
    cs = tiny()
    recs = [(COPY, 1, 0, 5), (SHUFFLE, 0, 0, 2), (LOOKUP, 0, 1 << 16 | 0, 7), (GATE, 1, 0, 3), (GATE, 0, 0, 9),
            (GATE | 1 << 8, 0, 0, 1), (GATE, 0, 0, 2)]
    want = [prover.ConstraintNotSatisfied(0, "mul", 0, 2, 0), prover.ConstraintNotSatisfied(0, "mul", 0, 9, 0),
            prover.ConstraintNotSatisfied(1, "rot", 0, 3, 0), prover.Lookup("in t", 0, 1, 0, 7, 0),
            prover.Shuffle("b to c", 0, 0, 2, 0), prover.Permutation(("advice", 2), 5, 0),
            prover.ConstraintNotSatisfied(0, "mul", 0, 1, 1)]
    assert prover.check_failures(cs, recs) == want
    # the downloaded block: u64 count, padding, cap records; a count above cap keeps cap of them
    cap = 4
    words = np.zeros(4 + 4 * cap, dtype=np.uint32)
    words[:2] = np.array([9], dtype=np.uint64).view(np.uint32)
    words[4:] = np.array(recs[:cap], dtype=np.uint32).reshape(-1)
    failures, total = prover.check_result(cs, words, cap)
    assert total == 9 and failures == prover.check_failures(cs, recs[:cap])
    words[:2] = np.array([2], dtype=np.uint64).view(np.uint32)
    assert prover.check_result(cs, words, cap) == (prover.check_failures(cs, recs[:2]), 2)
    words[:2] = np.array([7], dtype=np.uint64).view(np.uint32)
    assert prover.check_result(cs, words[:4], 0) == ([], 7)


def test_assert_satisfied_message_names_gates_lookups_and_columns():
    cs = tiny()
    text = [check._describe_failure(f) for f in prover.check_failures(cs, [(GATE, 1, 0, 3), (LOOKUP, 0, 2 << 16 | 1, 7),
                                                                            (SHUFFLE, 0, 0, 2), (COPY, 0, 0, 5)])]
    assert text == ["gate 1 'rot' polynomial 0 is not satisfied at row 3",
                    "lookup 0 'in t' (input set 2, input 1): row 7 is not in the table",
                    "shuffle 'b to c' (group 0, unit 0): the value of row 2 is not shuffled",
                    "copy constraint of advice column 0 broken at row 5"]


def test_check_entry_points_reject_bad_arguments_without_a_device():
    L = h2.lib()
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.addressof(buf)
    INVALID = 1
    scratch = L.h2_check_scratch_bytes(1 << 10)
    assert scratch >= (1 << 10) * 4
    assert L.h2_dev_check_nonzero_rows(None, 8, p, p, None) == INVALID
    assert L.h2_dev_check_nonzero_rows(p, 1 << 31, p, p, None) == INVALID
    assert L.h2_dev_check_gates(None, p, p, 0, p, p, 4, None) == INVALID
    assert L.h2_dev_check_gates(p, p, p, 0, None, p, 4, None) == INVALID          # no count
    assert L.h2_dev_check_gates(p, p, p, 1 << 24, p, p, 4, None) == INVALID      # circuit index past 24 bits
    # a descriptor with a permutation part / an extended domain is not a gate program
    from halo2_gpu_specific_amd import evaluation as ev

    desc = ev.EvalHDesc()
    desc.k, desc.extended_k = 4, 5
    assert L.h2_dev_check_gates(ctypes.byref(desc), p, p, 0, p, p, 4, None) == INVALID
    desc.extended_k, desc.n_perm_sets = 4, 1
    assert L.h2_dev_check_gates(ctypes.byref(desc), p, p, 0, p, p, 4, None) == INVALID
    desc.n_perm_sets, desc.n_value_parts = 0, 1                                   # a value part and no array for it
    assert L.h2_dev_check_gates(ctypes.byref(desc), p, p, 0, p, p, 4, None) == INVALID
    ptrs = (ctypes.c_void_p * 1)(p)
    tags = (ctypes.c_uint32 * 1)(0)
    n = 1 << 10
    assert L.h2_dev_check_lookup(None, ptrs, tags, 1, n - 8, n, 0, 0, p, scratch, p, p, 4, None) == INVALID
    assert L.h2_dev_check_lookup(p, ptrs, None, 1, n - 8, n, 0, 0, p, scratch, p, p, 4, None) == INVALID
    assert L.h2_dev_check_lookup(p, (ctypes.c_void_p * 1)(None), tags, 1, n - 8, n, 0, 0, p, scratch, p, p, 4, None) == INVALID
    assert L.h2_dev_check_lookup(p, ptrs, tags, 1, n + 1, n, 0, 0, p, scratch, p, p, 4, None) == INVALID   # usable > n
    assert L.h2_dev_check_lookup(p, ptrs, tags, 1, n - 8, n, 0, 0, p, scratch - 1, p, p, 4, None) == INVALID
    assert L.h2_dev_check_lookup(p, ptrs, tags, 1, n - 8, n, 0, 0, p, scratch, p, None, 4, None) == INVALID  # records
    assert L.h2_dev_check_shuffle(p, None, n - 8, n, 0, 0, 0, p, scratch, p, p, 4, None) == INVALID
    assert L.h2_dev_check_shuffle(p, p, n - 8, n, 0, 0, 0, p, scratch // 2, p, p, 4, None) == INVALID
    assert L.h2_dev_check_shuffle(p, p, n - 8, 1 << 31, 0, 0, 0, p, 1 << 40, p, p, 4, None) == INVALID
    assert L.h2_dev_check_copies(None, 2, p, p, n, 0, p, p, 4, None) == INVALID
    assert L.h2_dev_check_copies(p, 2, p, None, n, 0, p, p, 4, None) == INVALID
    assert L.h2_dev_check_copies(p, 1 << 16, p, p, n, 0, p, p, 4, None) == INVALID
    assert L.h2_dev_check_copies(p, 2, p, p, n, 0, None, p, 4, None) == INVALID
