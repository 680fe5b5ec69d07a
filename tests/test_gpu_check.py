"""prover.check_witness / assert_satisfied (MockProver::verify on the device) against the big-integer checker of
tests/check_reference.py: satisfied witnesses of every example circuit give no failure; targeted corruptions and random
unsatisfiable circuits give exactly the reference's list."""
import os
import sys

import numpy as np
import pytest

from check_reference import reference_check
from h2util import R_MOD, to_mont
from test_plonk_host import S_TRAPDOOR

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import prover_fuzz  # noqa: E402

pytestmark = pytest.mark.gpu

BIG = 1 << 16


@pytest.fixture(scope="module")
def device():
    from halo2_gpu_specific_amd import prover

    return prover.Device()


_PARAMS = {}


@pytest.fixture(scope="module", autouse=True)
def params_released():
    """the parameters of this module go with it: a Params of 2^15 rows or more carries shifted-base tables in library memory
    until it is collected, and a live table changes what h2_msm_scratch_bytes reports to every later test of the process"""
    yield
    import gc

    _PARAMS.clear()
    gc.collect()


def setup(device, cs, k, fixed, copies):
    from halo2_gpu_specific_amd import prover

    if k not in _PARAMS:
        _PARAMS[k] = prover.Params.unsafe_setup(device, k, S_TRAPDOOR)
    return prover.keygen(device, _PARAMS[k], cs, fixed, copies)


def expected(pk, advice, fixed, instances=(), circuit=0, **kw):
    from halo2_gpu_specific_amd import prover

    return prover.check_failures(pk.cs, reference_check(pk.cs, pk.domain.n, advice, fixed, instances, pk.mapping, circuit, **kw))


def got(device, pk, advice, instances=(), **kw):
    from halo2_gpu_specific_amd import prover

    kw.setdefault("max_failures", BIG)
    return prover.check_witness(device, pk, advice, instances, **kw)


def example(which, k):
    from halo2_gpu_specific_amd import circuits

    return {
        "mini-plonk": lambda: (circuits.mini_plonk(), circuits.mini_plonk_synthesize(k)),
        "wide": lambda: (circuits.wide(2), circuits.wide_synthesize(k, 2)),
        "range-check": lambda: (circuits.range_check(0, 30, 2), circuits.range_check_synthesize(k, vmax=30, count=60)),
        "lookup-api": lambda: (circuits.lookup_api(), circuits.lookup_api_synthesize(k)),
        "lookup-api-set": lambda: (circuits.lookup_api_set(), circuits.lookup_api_set_synthesize(k)),
        "shuffle-api": lambda: (circuits.shuffle_api(), circuits.shuffle_api_synthesize(k)),
        "shuffle-api-group": lambda: (circuits.shuffle_api_group(), circuits.shuffle_api_group_synthesize(k)),
        "shuffle-gates": lambda: (circuits.shuffle_gates(), circuits.shuffle_gates_synthesize(k)),
    }[which]()


@pytest.mark.parametrize("which,k", [("mini-plonk", 5), ("wide", 7), ("range-check", 7), ("lookup-api", 6),
                                     ("lookup-api-set", 7), ("shuffle-api", 6), ("shuffle-api-group", 6), ("shuffle-gates", 6)])
def test_satisfied_examples_have_no_failures(device, which, k):
    cs, (adv, fixed, copies) = example(which, k)
    pk = setup(device, cs, k, fixed, copies)
    before = [c.copy() for c in adv]
    assert got(device, pk, adv) == ([], 0)
    # the caller's columns are unchanged (a range-checked column is completed on a copy)
    assert all(np.array_equal(a, b) for a, b in zip(adv, before))


@pytest.mark.parametrize("seed", range(8))
def test_satisfiable_random_circuits(device, seed):
    cs, k, adv, fixed, copies, inst = prover_fuzz.random_case(seed, satisfiable=True)
    pk = setup(device, cs, k, fixed, copies)
    assert got(device, pk, adv, inst) == ([], 0)
    assert expected(pk, adv, fixed, inst) == []


@pytest.mark.parametrize("seed", range(100, 112))
def test_unsatisfiable_random_circuits_match_the_reference(device, seed):
    cs, k, adv, fixed, copies, inst = prover_fuzz.random_case(seed, satisfiable=False)
    assert 5 <= k <= 9
    pk = setup(device, cs, k, fixed, copies)
    want = expected(pk, adv, fixed, inst)
    assert want
    assert got(device, pk, adv, inst) == (want, len(want))


def _gate_reads(e):
    from halo2_gpu_specific_amd import circuit as hc

    if isinstance(e, hc.Query):
        return [e]
    return [q for c in ("a", "b", "e") if hasattr(e, c) for q in _gate_reads(getattr(e, c))]


def test_one_advice_cell_breaks_the_gates_that_read_it(device):
    cs, k, adv, fixed, copies, inst = prover_fuzz.random_case(3, satisfiable=True)
    pk = setup(device, cs, k, fixed, copies)
    n = pk.domain.n
    # a column that a gate reads at a non-zero rotation where possible: the failures then sit at several rows
    reads = [q for _, polys in cs.gates for p in polys for q in _gate_reads(p) if q.name == "advice"]
    q = max(reads, key=lambda q: abs(q.rotation))
    bad = [c.copy() for c in adv]
    bad[q.column][n // 2, 0] ^= 5
    want = expected(pk, bad, fixed, inst)
    assert want and {f.row for f in want} >= {(n // 2 - q.rotation) % n}
    assert got(device, pk, bad, inst) == (want, len(want))


def test_one_copied_cell(device):
    from halo2_gpu_specific_amd import prover

    cs, (adv, fixed, copies) = example("mini-plonk", 5)
    pk = setup(device, cs, 5, fixed, copies)
    bad = [c.copy() for c in adv]
    bad[0][2, 0] += 1                       # row 2: a of the second raw_multiply, copied to row 3
    want = expected(pk, bad, fixed)
    perm = [f for f in want if isinstance(f, prover.Permutation)]
    assert perm == [prover.Permutation(("advice", 0), 2, 0), prover.Permutation(("advice", 0), 3, 0)]
    assert got(device, pk, bad) == (want, len(want))
    # the same witness as Montgomery columns, compact columns and device tensors
    mont = [to_mont([int(v) for v in c[:, 0]]) for c in bad]
    assert got(device, pk, mont, montgomery=True) == (want, len(want))
    assert got(device, pk, [c[:, 0].copy() for c in bad]) == (want, len(want))
    assert got(device, pk, [device.upload(c) for c in bad]) == (want, len(want))


def test_lookup_input_missing_from_the_table(device):
    from halo2_gpu_specific_amd import prover

    cs, (adv, fixed, copies) = example("lookup-api", 6)
    pk = setup(device, cs, 6, fixed, copies)
    bad = [c.copy() for c in adv]
    bad[2][1, 0] = 77
    want = expected(pk, bad, fixed)
    assert any(isinstance(f, prover.Lookup) and f.row == 1 for f in want)
    assert got(device, pk, bad) == (want, len(want))


def test_shuffle_that_is_not_a_permutation(device):
    from halo2_gpu_specific_amd import circuits, prover

    cs, (_, fixed, copies) = example("shuffle-api-group", 6)
    pk = setup(device, cs, 6, fixed, copies)
    bad, _, _ = circuits.shuffle_api_group_synthesize(6, input1=(4, 1, 1, 3))
    want = expected(pk, bad, fixed)
    assert want and all(isinstance(f, prover.Shuffle) for f in want)
    assert got(device, pk, bad) == (want, len(want))


def test_instance_value(device):
    from halo2_gpu_specific_amd import circuit as hc

    for seed in range(60):
        cs, k, adv, fixed, copies, inst = prover_fuzz.random_case(seed, satisfiable=True)
        if cs.num_instance and any(isinstance(q, hc.Instance) for _, polys in cs.gates for p in polys for q in _gate_reads(p)):
            break
    else:
        pytest.fail("no satisfiable random circuit whose gates read an instance column")
    pk = setup(device, cs, k, fixed, copies)
    bad = [list(inst[0]) + [0] * (6 - len(inst[0]))]
    bad[0][4] = (bad[0][4] + 1) % R_MOD
    want = expected(pk, adv, fixed, bad)
    assert want
    assert got(device, pk, adv, bad) == (want, len(want))


def test_seeds_truncation_and_circuit_instances(device):
    from halo2_gpu_specific_amd import prover

    cs, k, adv, fixed, copies, inst = prover_fuzz.random_case(105, satisfiable=False)
    pk = setup(device, cs, k, fixed, copies)
    want = expected(pk, adv, fixed, inst)
    assert got(device, pk, adv, inst, seed=1) == got(device, pk, adv, inst, seed=2) == (want, len(want))
    cap = len(want) // 3
    some, total = got(device, pk, adv, inst, max_failures=cap)
    assert total == len(want) and len(some) == cap and set(some) <= set(want)
    assert got(device, pk, adv, inst, max_failures=0) == ([], len(want))
    # two circuit instances, the second one satisfied: every record in one buffer, each with its circuit
    cs2, k2, good, fixed2, copies2, inst2 = prover_fuzz.random_case(3, satisfiable=True)
    pk2 = setup(device, cs2, k2, fixed2, copies2)
    bad = [c.copy() for c in good]
    bad[0][7, 0] ^= 1
    want2 = expected(pk2, bad, fixed2, inst2, circuit=2)
    assert want2
    assert got(device, pk2, [good, good, bad], [inst2, inst2, inst2]) == (want2, len(want2))
    assert all(f.circuit == 2 for f in want2) and isinstance(want2[0], (prover.ConstraintNotSatisfied, prover.Permutation))


def test_wide_circuit_at_k20(device, request):
    from halo2_gpu_specific_amd import circuits, prover

    k = 20
    request.addfinalizer(lambda: _PARAMS.pop(k, None))       # (its tables: see params_released)
    cs = circuits.wide(16)
    adv, fixed, copies = circuits.wide_synthesize(k, 16, compact=True)
    pk = setup(device, cs, k, fixed, copies)
    assert got(device, pk, adv) == ([], 0)
    prover.assert_satisfied(device, pk, adv)
    row = 123457
    adv[4 * 5 + 1][row] += 1                # b of quad 5: gate "mul3", polynomial 5
    assert got(device, pk, adv) == ([prover.ConstraintNotSatisfied(0, "mul3", 5, row, 0)], 1)
    with pytest.raises(ValueError, match="gate 0 'mul3' polynomial 5 is not satisfied at row %d" % row):
        prover.assert_satisfied(device, pk, adv)
