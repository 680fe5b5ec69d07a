"""The copy constraints' cycle mapping built on the device (csrc/permmap.hip, prover.permutation_mapping_device) against
prover.permutation_mapping, the host function the parent commit's keygen ran (pinned to the big-integer twin by
tests/test_perm_mapping_cases_host.py): every entry equal on every case of tests/perm_mapping_cases.py, the same bytes call
after call, out-of-bounds copies reported by their lowest index, and keygen through the device route giving the key, the
proof bytes and the check_witness verdicts of keygen through the host function."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import ref_plonk as rp
from h2util import ROOT, ints_to_arr
from perm_mapping_cases import CASES
from test_plonk_host import S_TRAPDOOR, lookup_shuffle_cs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def device():
    from halo2_gpu_specific_amd import prover

    return prover.Device()


@functools.lru_cache(maxsize=None)
def case(name):
    """(ncols, n, copies, the host function's (map_col, map_row)): computed once, read-only"""
    from halo2_gpu_specific_amd import prover

    ncols, n, copies = CASES[name]()
    want = prover.permutation_mapping(ncols, n, copies)
    for a in (copies,) + want:
        a.setflags(write=False)
    return ncols, n, copies, want


def on_device(device, ncols, n, copies):
    from halo2_gpu_specific_amd import prover

    map_col, map_row = prover.permutation_mapping_device(device, ncols, n, copies)
    assert tuple(map_col.shape) == tuple(map_row.shape) == (ncols * n,) and map_col.is_cuda and map_row.is_cuda
    with device.torch.cuda.stream(device.tstream):
        return tuple(t.cpu().numpy().view(np.uint32).reshape(ncols, n) for t in (map_col, map_row))


def first_difference(got, want):
    bad = np.flatnonzero((got[0] != want[0]).reshape(-1) | (got[1] != want[1]).reshape(-1))
    if not len(bad):
        return None
    c, r = divmod(int(bad[0]), want[0].shape[1])
    return "%d cells differ; the first is (%d, %d): (%d, %d), expected (%d, %d)" % (
        len(bad), c, r, got[0][c, r], got[1][c, r], want[0][c, r], want[1][c, r])


@pytest.mark.parametrize("name", list(CASES))
def test_device_mapping_equals_the_host_mapping(device, name):
    ncols, n, copies, want = case(name)
    got = on_device(device, ncols, n, copies)
    assert first_difference(got, want) is None
    again = on_device(device, ncols, n, copies)
    assert got[0].tobytes() == again[0].tobytes() and got[1].tobytes() == again[1].tobytes()


def test_copies_in_any_integer_form(device):
    """a list of tuples and a u32 array are the copies an int64 array is"""
    ncols, n, copies, want = case("random-7")
    for form in ([tuple(int(v) for v in row) for row in copies], copies.astype(np.uint32)):
        assert first_difference(on_device(device, ncols, n, form), want) is None


@pytest.mark.parametrize("what", ["row = n", "column = ncols", "a value past u32", "a negative value"])
def test_out_of_bounds_copies_name_the_lowest_index(device, what):
    from halo2_gpu_specific_amd import prover

    ncols, n, copies, want = case("random-2N")
    bad = copies.copy()
    first, second = 4097, 5000                                # past one workgroup's copies
    bad[second] = (0, n, 0, 0)
    bad[first] = {"row = n": (1, 3, 2, n), "column = ncols": (ncols, 0, 1, 1), "a value past u32": (0, 1 << 32, 0, 0),
                  "a negative value": (0, 0, -1, 0)}[what]
    with pytest.raises(ValueError, match=r"copy %d is out of bounds \(BoundsFailure\)" % first):
        prover.permutation_mapping_device(device, ncols, n, bad)
    # the next call on the same device is correct
    assert first_difference(on_device(device, ncols, n, copies), want) is None


def test_no_columns(device):
    from halo2_gpu_specific_amd import prover

    map_col, map_row = prover.permutation_mapping_device(device, 0, 16, np.zeros((0, 4), dtype=np.int64))
    assert map_col.numel() == map_row.numel() == 0
    with pytest.raises(ValueError, match="BoundsFailure"):
        prover.permutation_mapping_device(device, 0, 16, [(0, 0, 0, 1)])


# ---- keygen ----------------------------------------------------------------------------------------------------------
K = 8


def circuit(which):
    """-> (cs, advice, fixed, copies, instances)"""
    from halo2_gpu_specific_amd import circuits

    if which == "mini-plonk":
        adv, fixed, copies = circuits.mini_plonk_synthesize(K)
        return circuits.mini_plonk(), adv, fixed, copies, ()
    adv, fixed, copies, inst = rp.LookupShuffle.synthesize(K)
    return (lookup_shuffle_cs(), [ints_to_arr(c) for c in adv], [ints_to_arr(c) for c in fixed],
            np.array([(l[0], l[1], r[0], r[1]) for l, r in copies], dtype=np.int64), inst)


@pytest.fixture(scope="module")
def params(device):
    from halo2_gpu_specific_amd import prover

    return prover.Params.unsafe_setup(device, K, S_TRAPDOOR)


def key_facts(pk):
    from halo2_gpu_specific_amd.transcript import point_to_bytes

    return {"perm_commitments": [point_to_bytes(p).hex() for p in pk.perm_commitments], "transcript_repr": "%x" % pk.transcript_repr,
            "mapping": [np.ascontiguousarray(a, dtype=np.uint32).tobytes().hex() for a in pk.mapping]}


@pytest.mark.parametrize("which", ["mini-plonk", "lookup-shuffle"])
def test_keygen_through_the_device_equals_keygen_through_the_host_function(device, params, which, monkeypatch):
    from halo2_gpu_specific_amd import keygen, prover
    from halo2_gpu_specific_amd.rng import ProverRng

    cs, adv, fixed, copies, inst = circuit(which)
    n, ncols = 1 << K, len(cs.perm_columns)
    assert ncols and len(copies)
    host_mapping = prover.permutation_mapping(ncols, n, copies)
    hpk = prover.keygen(device, params, cs, fixed, None, mapping=host_mapping)
    # the default route neither calls the host function nor can import scipy
    with monkeypatch.context() as m:
        m.setattr(keygen, "permutation_mapping", lambda *a: pytest.fail("keygen called the host function"))
        for name in [name for name in sys.modules if name == "scipy" or name.startswith("scipy.")]:
            m.setitem(sys.modules, name, None)
        m.setitem(sys.modules, "scipy", None)
        pk = prover.keygen(device, params, cs, fixed, copies)
    assert all(a.shape == (ncols, n) and a.dtype == np.uint32 for a in pk.mapping)
    assert np.array_equal(pk.mapping[0], host_mapping[0]) and np.array_equal(pk.mapping[1], host_mapping[1])
    assert key_facts(pk) == key_facts(hpk)
    proof = prover.create_proof_ext(device, params, pk, adv, ProverRng(11), False, instances=inst)
    assert proof == prover.create_proof_ext(device, params, hpk, adv, ProverRng(11), False, instances=inst)
    # check_witness reads pk.mapping: nothing for the satisfying witness, a COPY failure at a changed cell of a cycle
    assert prover.check_witness(device, pk, adv, inst) == ([], 0)
    pos, row = next((int(c[0]), int(c[1])) for c in copies if cs.perm_columns[int(c[0])][0] == "advice")
    kind, index = cs.perm_columns[pos]
    bad = [c.copy() for c in adv]
    bad[index][row, 0] ^= 1
    failures, count = prover.check_witness(device, pk, bad, inst)
    assert prover.Permutation((kind, index), row, 0) in failures and count == len(failures)


_HOST_ROUTE = r"""
import json, sys
sys.path.insert(0, %r)
sys.path.insert(0, %r)
from halo2_gpu_specific_amd import keygen, prover
from test_gpu_perm_mapping import K, S_TRAPDOOR, circuit, key_facts
calls, host = [], keygen.permutation_mapping
def counted(*a):
    calls.append(1)
    return host(*a)
keygen.permutation_mapping = counted       # the name keygen.keygen reads: its own module's, not prover's re-export
D = prover.Device()
cs, adv, fixed, copies, inst = circuit("mini-plonk")
pk = prover.keygen(D, prover.Params.unsafe_setup(D, K, S_TRAPDOOR), cs, fixed, copies)
print("FACTS " + json.dumps({"calls": len(calls), "key": key_facts(pk)}))
"""


def test_host_route_knob_gives_the_same_key(device, params):
    """H2_PERM_MAPPING=host (read when keygen runs; a process of its own so that nothing else sees it)"""
    from halo2_gpu_specific_amd import prover

    cs, adv, fixed, copies, inst = circuit("mini-plonk")
    want = key_facts(prover.keygen(device, params, cs, fixed, copies))
    env = dict(os.environ, H2_PERM_MAPPING="host")
    out = subprocess.run([sys.executable, "-c", _HOST_ROUTE % (ROOT, os.path.join(ROOT, "tests"))], env=env, capture_output=True,
                         text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    facts = json.loads(next(line for line in out.stdout.splitlines() if line.startswith("FACTS "))[6:])
    assert facts["calls"] == 1 and facts["key"] == want
