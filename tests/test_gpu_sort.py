"""The sort on the device (csrc/sort.hip, h2_dev_sort_permutation) against the definition -- sorted(range(n), key=(k0[i], ...,
i)) over Python integers, tests/sort_cases.py -- element for element: every size around the wave, the workgroup, the tile and
the second level of the histogram's scan, crossed with the key sets that exercise the skipping rule, the limb boundaries,
stability and the three cell forms; the pass count in d_status[3]; promises kept and broken; two caller streams; h2_sort and
arithmetic.gpu_sort; Value.sort_by without a download; SortedAccessLog through check_witness, a proof and the verifier."""
import ctypes
import random

import numpy as np
import pytest
import torch

import sort_cases as sc
import stream_device as sd
import values_cases as vc
from sort_cases import R_MOD

pytestmark = pytest.mark.gpu

S_TRAPDOOR = 0x1D0C5F0A3B7E91C2A4D6F8091B2C3D4E5F60718293A4B5C6D7E8F9010203
GUARD = 8                                                        # words behind the permutation that must stay as they were


@pytest.fixture(scope="module")
def device():
    from halo2_gpu_specific_amd import prover

    return prover.Device()


@pytest.fixture(scope="module")
def tile(device):
    from halo2_gpu_specific_amd import values

    caps = values.sort_limits()
    assert caps["max_keys"] >= 4 and caps["status_words"] == 4
    return caps["tile"]


def run_device(L, keys, forms, bits, width=4, stream=None):
    """h2_dev_sort_permutation -> (the permutation, the status words); the keys are compared with what went up afterwards and
    the words behind the permutation with what they held"""
    n = len(keys[0])
    cells = [sd.to_device(sc.encode(column, form)) for column, form in zip(keys, forms)]
    kept = [c.clone() for c in cells]
    ptrs = np.array([c.data_ptr() for c in cells], dtype=np.uint64)
    forms, bits = np.array(forms, dtype=np.uint32), np.array(bits, dtype=np.uint32)
    perm = torch.full((n + GUARD,), -7, dtype=torch.int32 if width == 4 else torch.int64, device="cuda")
    status = torch.full((4,), 9, dtype=torch.int32, device="cuda")
    need = L.h2_sort_scratch_bytes(n, len(keys))
    scratch = torch.empty(need, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    rc = L.h2_dev_sort_permutation(ptrs.ctypes.data, forms.ctypes.data, bits.ctypes.data, len(keys), n, perm.data_ptr(), width,
                                   status.data_ptr(), scratch.data_ptr(), need, stream)
    torch.cuda.synchronize()
    assert rc == 0, L.h2_last_error()
    assert all(torch.equal(a, b) for a, b in zip(cells, kept)) and bool((perm[n:] == -7).all())
    return [int(v) for v in perm[:n].cpu().numpy()], [int(v) for v in status.cpu().numpy().view(np.uint32)]


# -- the kernels against the definition ----------------------------------------------------------------------------------------
def sizes():
    from halo2_gpu_specific_amd import values

    return sc.sizes(values.sort_limits()["tile"])


@pytest.mark.parametrize("n", sizes())
def test_device_matches_the_definition(device, tile, n):
    """every key set at n rows, each in every form it has: the permutation is the definition's and d_status[3] is the number of
    byte positions on which two cells differ -- 0 for equal keys, 1 for keys that differ in one byte, never a skip for n - 1
    equal keys and one other"""
    assert n < 1 << 20
    for case in sc.cases(n, tile):
        sc.check(case, lambda keys, forms, bits: run_device(device.L, keys, forms, bits))
    if n in (2, 257, 3 * tile + 77):                                           # the same at 8 bytes an index
        for case in sc.cases(n, tile):
            sc.check(case, lambda keys, forms, bits: run_device(device.L, keys, forms, bits, 8))


def test_second_level_size_is_derived_from_the_caps(tile):
    n = sc.second_level_rows(tile)
    words = lambda rows: 256 * -(-rows // tile)                                    # noqa: E731
    assert words(n - 1) <= 2 * tile < words(n) and n in sizes()


def test_sentinels_stability_and_both_index_widths(device, tile):
    sc.check(sc.sentinel_case(), lambda keys, forms, bits: run_device(device.L, keys, forms, bits))
    rng = random.Random(7)
    n = tile + 1
    four = [[(R_MOD - 1, 0, 1 << 64, 255)[rng.randrange(4)] for _ in range(n)]]
    want = sc.oracle(four)
    for width in (4, 8):
        for form in (sc.CANONICAL, sc.MONTGOMERY):
            perm, status = run_device(device.L, four, (form,), (0,), width)
            assert perm == want and status[0] == sc.OK
    # the twin, same input: the same permutation and the same status words
    assert sc.run_host(device.L, four, (sc.MONTGOMERY,), (0,)) == run_device(device.L, four, (sc.MONTGOMERY,), (0,))


def test_a_promise_that_holds_spares_the_passes_above_it(device, tile):
    """keys below 2^20 that vary in all three of their bytes: three passes with or without the promise (the bytes above agree),
    and with a promise of 16 bits the third byte is not looked at at all -- two passes, the order that of the low 16 bits"""
    rng = random.Random(9)
    n = 2 * tile + 1
    keys = [[rng.randrange(1 << 20) for _ in range(n)]]
    for form in (sc.CANONICAL, sc.MONTGOMERY, sc.COMPACT):
        assert run_device(device.L, keys, (form,), (0,)) == (sc.oracle(keys), [sc.OK, 0xFFFFFFFF, 0xFFFFFFFF, 3])
        assert run_device(device.L, keys, (form,), (20,)) == (sc.oracle(keys), [sc.OK, 0xFFFFFFFF, 0xFFFFFFFF, 3])
        assert run_device(device.L, keys, (form,), (24,))[1][3] == 3
    low = [[v & 0xFFFF for v in keys[0]]]
    assert run_device(device.L, low, (sc.CANONICAL,), (16,)) == (sc.oracle(low), [sc.OK, 0xFFFFFFFF, 0xFFFFFFFF, 2])
    assert run_device(device.L, low, (sc.CANONICAL,), (8,))[1][3] == 1               # (a broken promise: one pass all the same)


def test_a_broken_promise_is_reported_and_nothing_faults(device, tile):
    rng = random.Random(10)
    n = 3 * tile + 77
    keys = [[rng.randrange(1 << 12) for _ in range(n)], [rng.randrange(1 << 20) for _ in range(n)]]
    row = 2 * tile + 5
    keys[1][row] = keys[1][row + 300] = (1 << 250) + 1                             # the lowest breaking row is named, with its key
    keys[0][row + 300] = 1 << 12
    for forms in ((sc.CANONICAL, sc.MONTGOMERY), (sc.COMPACT, sc.CANONICAL)):
        perm, status = run_device(device.L, keys, forms, (12, 20))
        assert status == [sc.OUT_OF_RANGE, row, 1, 5] and sorted(perm) == list(range(n))
        assert sc.run_host(device.L, keys, forms, (12, 20))[1] == status
    perm, status = run_device(device.L, [[5, 1 << 9, 3]], (sc.CANONICAL,), (9,))   # bit 9 inside candidate byte 1
    assert status[:3] == [sc.OUT_OF_RANGE, 1, 0] and sorted(perm) == [0, 1, 2]
    perm, status = run_device(device.L, [[5, 1 << 63, 3]], (sc.COMPACT,), (63,))
    assert status[:3] == [sc.OUT_OF_RANGE, 1, 0]


# -- two caller streams ----------------------------------------------------------------------------------------------------------
class _SortAdapter:
    name, outputs, normalised = "sort_permutation", ("perm", "status"), False

    @staticmethod
    def call(L, stream, ptr, case):
        keys = np.array([ptr["key%d" % i] for i in range(len(case.forms))], dtype=np.uint64)
        forms, bits = np.array(case.forms, dtype=np.uint32), np.array(case.bits, dtype=np.uint32)
        need = L.h2_sort_scratch_bytes(case.n, len(case.forms))
        return L.h2_dev_sort_permutation(keys.ctypes.data, forms.ctypes.data, bits.ctypes.data, len(case.forms), case.n, ptr["perm"], 4,
                                         ptr["status"], ptr["scratch"], need, ctypes.c_void_p(stream)), None


class _SortCase:
    def __init__(self, keys, forms, bits):
        self.n, self.forms, self.bits = len(keys[0]), forms, bits
        self.inputs = {"key%d" % i: sc.encode(column, form) for i, (column, form) in enumerate(zip(keys, forms))}
        self.like = {"perm": ((self.n,), np.uint32), "status": ((4,), np.uint32)}
        self.scratch = {"scratch": lambda L: L.h2_sort_scratch_bytes(self.n, len(forms))}
        self.expect = {"perm": np.array(sc.oracle(keys), dtype=np.uint32),
                       "status": np.array([sc.OK, 0xFFFFFFFF, 0xFFFFFFFF, sc.expected_passes(keys, forms, bits)], dtype=np.uint32)}


def test_two_sorts_on_two_streams_with_two_scratch_blocks(device, tile):
    """different inputs of different shapes, each call with its own scratch: run one after the other (warm), then side by side
    from two threads, several rounds -- every result is the serial one"""
    rng = random.Random(12)
    n1, n2 = 5 * tile + 3, 3 * tile + 77
    one = _SortCase([[rng.randrange(R_MOD) for _ in range(n1)]], (sc.MONTGOMERY,), (0,))
    two = _SortCase([[rng.randrange(3) for _ in range(n2)], [rng.randrange(1 << 32) for _ in range(n2)]], (sc.COMPACT, sc.CANONICAL), (2, 32))
    rounds = 3
    bounds = [sd.Bound(_SortAdapter, case, device.L, snapshots=rounds) for case in (one, two)]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    for bound, stream in zip(bounds, streams):
        sd.warm(bound, stream)
    assert sd.run_pair(list(zip(bounds, streams)), rounds) == [[], []]


# -- the host-slice entry --------------------------------------------------------------------------------------------------------
def test_h2_sort_and_gpu_sort_on_host_vectors(device, tile):
    from halo2_gpu_specific_amd import arithmetic

    L = device.L
    rng = random.Random(13)
    for n in (1, 2, 256, tile + 1):
        values = [rng.randrange(R_MOD) for _ in range(n)]
        if n > 2:
            values[5] = values[n - 1]                                                 # a tie
        want = sc.encode(sorted(values), sc.MONTGOMERY)
        plain = sc.encode(values, sc.MONTGOMERY)
        assert L.h2_sort(plain.ctypes.data, n) == 0, L.h2_last_error()
        assert np.array_equal(plain, want)
        ptr = ctypes.c_void_p()
        assert L.h2_host_alloc_pinned(32 * n, ctypes.byref(ptr)) == 0
        try:
            pinned = np.ctypeslib.as_array(ctypes.cast(ptr, ctypes.POINTER(ctypes.c_uint64)), shape=(n, 4))
            pinned[:] = sc.encode(values, sc.MONTGOMERY)
            assert L.h2_sort(ptr, n) == 0, L.h2_last_error()
            assert np.array_equal(pinned, want)
            del pinned
        finally:
            assert L.h2_host_free_pinned(ptr) == 0
        if n & (n - 1) == 0:
            again = sc.encode(values, sc.MONTGOMERY)
            assert arithmetic.gpu_sort(again, n.bit_length() - 1) is again and np.array_equal(again, want)
    assert L.h2_sort(None, 0) == 0
    with pytest.raises(AssertionError):
        arithmetic.gpu_sort(sc.encode([1, 2, 3], sc.MONTGOMERY), 2)


# -- Value -----------------------------------------------------------------------------------------------------------------------
def test_value_sort_by_stays_on_the_device(device, tile, monkeypatch):
    from halo2_gpu_specific_amd import values
    from halo2_gpu_specific_amd.values import Value

    rng = random.Random(14)
    n = tile + 300
    A = [rng.randrange(1 << 10) for _ in range(n)]
    T = list(range(1, n + 1))
    P = [rng.randrange(R_MOD) for _ in range(n)]
    a, t, p = Value.from_u64(device, A), Value.from_u64(device, T), Value.from_ints(device, P)
    values._backend(device)
    Value.materialize([a + 0, p + 0])                                                  # the leaves are on the device from here on
    downloads = []
    real = device.download
    monkeypatch.setattr(device, "download", lambda tensor: downloads.append(tuple(tensor.shape)) or real(tensor))
    before = (device.values_sorts, device.values_launches)
    # whole leaves as keys and payloads: one sort, no evaluator launch at all
    sa, sp = Value.sort_by([a, t], [a, p], bits=[10, n.bit_length()])
    got = Value.materialize([sa, sp], montgomery=False)
    assert (device.values_sorts - before[0], device.values_launches - before[1]) == (1, 1)   # the launch widens the compact `sa`
    assert downloads == []
    order = sc.oracle([A, T])
    assert vc.ints(device.download(got[0])) == [A[i] for i in order] and vc.ints(device.download(got[1])) == [P[i] for i in order]
    assert len(downloads) == 2
    # a computed key, a computed payload, the permutation itself; a second materialisation sorts nothing
    before = (device.values_sorts, device.values_launches)
    perm = Value.argsort([a * 3 + 1, t])
    out = (p * 2).take(perm)
    assert out.to_ints() == [2 * P[i] % R_MOD for i in order] and perm.to_ints() == order
    # launches: the computed key, the computed payload, the gathered payload to canonical cells, the permutation widened
    assert device.values_sorts - before[0] == 1 and device.values_launches - before[1] == 4
    assert out.to_ints() == [2 * P[i] % R_MOD for i in order] and device.values_sorts - before[0] == 1
    assert p.sort().to_ints() == sorted(P) and a.sort(bits=10).to_ints() == sorted(A)
    # a broken promise: only the offending cell comes down
    del downloads[:]
    with pytest.raises(ValueError, match=r"argsort: key 0 at row %d is %d, which is not below 2\^4" % (next(i for i, v in enumerate(A) if v >= 16),
                                                                                                    next(v for v in A if v >= 16))):
        a.argsort(bits=4).to_ints()
    assert downloads == [(1,)]
    assert not Value.argsort([a, Value.unknown(n)]).known


# -- the circuit -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", (8, 10))
def test_sorted_access_log_checks_proves_and_verifies(device, k):
    """cannot pass without the feature: the sorted side of this witness exists only as Value.sort_by"""
    from halo2_gpu_specific_amd import check, circuits_frontend as fe, prover, verifier
    from halo2_gpu_specific_amd.rng import ProverRng
    from halo2_gpu_specific_amd.values import Value

    circuit = fe.SortedAccessLog(k, addr_bits=k - 4, device=device)
    H = circuit.height
    params = prover.Params.unsafe_setup(device, k, S_TRAPDOOR)
    cs, fixed, copies = prover.synthesize_keygen(device, circuit, k)
    pk = prover.keygen(device, params, cs, fixed, copies)
    sorts = device.values_sorts
    advice, _ = prover.synthesize_witness(device, circuit, pk, k, resident=True)
    assert device.values_sorts == sorts + 1
    want = sc.sorted_access_log_columns(circuit)
    for column, values in zip(advice, want):
        got = device.download(column)
        assert vc.ints(got[:len(values)]) == values and not got[len(values):].any()
    assert prover.check_witness(device, pk, advice) == ([], 0)
    proof = prover.create_proof_with_shplonk(device, params, pk, [device.clone(c) for c in advice], ProverRng(5))
    vk = verifier.VerifyingKey.from_proving_key(pk)
    assert verifier.verify_proof_with_shplonk(device, verifier.ParamsVerifier.from_params(params), vk, proof)
    # one sorted V at a read row altered (a row whose successor does not read the same address): exactly that gate, that row
    a, t, v, w, A, T, Vs, W, inv, s, d = want
    row = next(j for j in range(1, H - 1) if s[j - 1] == 1 and W[j] == 0 and (s[j] == 0 or W[j + 1] == 1))
    with device.torch.cuda.stream(device.tstream):
        advice[6][row, 0] ^= 1
    failures, total = prover.check_witness(device, pk, advice)
    gates = [(f.gate_name, f.row) for f in failures if isinstance(f, check.ConstraintNotSatisfied)]
    assert gates == [("a read returns the value before it", row - 1)] and total >= 1
    # the sorted side replaced by the unsorted log, everything after it computed from that: the gap leaves the table
    log = [Value.from_ints(device, col) for col in (a, t, v, w)]
    delta = log[0][1:] - log[0][:-1]
    flat_inv = delta.invert()
    flat_s = 1 - delta * flat_inv
    flat_d = Value.select(flat_s, log[1][1:] - log[1][:-1] - 1, delta - 1)
    unsorted = fe.SortedAccessLog(k, addr_bits=k - 4, device=device, columns=log + log + [flat_inv, flat_s, flat_d])
    bad, _ = prover.synthesize_witness(device, unsorted, pk, k, resident=True)
    failures, total = prover.check_witness(device, pk, bad)
    descents = {i for i in range(H - 1) if a[i + 1] < a[i]}                        # time ascends in the log: only these gaps are negative
    lookups = [f.row for f in failures if isinstance(f, check.Lookup) and f.name == "the gap is positive"]
    assert lookups and set(lookups) <= descents and total >= len(lookups)
    assert not any(isinstance(f, check.ConstraintNotSatisfied) and f.gate_name != "a read returns the value before it" for f in failures)
