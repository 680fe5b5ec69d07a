"""Rational (`Assigned`) cells resolved on the device (csrc/assigned.hip, prover.Rational / Device.resolve_rational).

Kernel: every row of every column against the big-integer reference of tests/assigned_cases.py (num * den^-1 mod r, 0 for a
zero denominator) -- equality of integers, no tolerance -- over the sizes at which the launch changes shape, the denominator
patterns a chain can meet, every combination of forms, sparse columns, bad row lists, many columns in a call, and the host
twin.  Proofs: the is-zero circuit proves from Rational columns to the bytes of the proof from the host-resolved witness.
None of this exists on the parent commit (no `Rational`, neither C entry)."""
import ctypes

import numpy as np
import pytest

import assigned_cases as A
from assigned_cases import CANONICAL as C, COMPACT as K, MONTGOMERY as M

pytestmark = pytest.mark.gpu

S_TRAPDOOR = 0x1D0C5F0A3B7E91C2A4D6F8091B2C3D4E5F60718293A4B5C6D7E8F9010203
GUARD = 64                                # rows on each side of every out column that no call may write
GUARD_WORD = 0x5A5A5A5A5A5A5A5A
# one wave, one workgroup, the switch from one element a lane to a chain; the second workgroup; several with a ragged tail
SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 6149)
_vp = ctypes.c_void_p


@pytest.fixture(scope="module")
def device():
    from halo2_gpu_specific_amd import prover

    return prover.Device()


def column(num, den, rows=None, nform=C, dform=C):
    return {"num": num, "den": den, "rows": rows, "nform": nform, "dform": dform}


def expected(col):
    if col["rows"] is None:
        return A.reference(col["num"], col["den"])
    return A.reference_sparse(col["num"], col["den"], col["rows"])


def call_arrays(cols, addr):
    """the parallel host arrays of a call; addr(array) -> where the operand lies (None for one without a cell)"""
    count = len(cols)
    num = (_vp * count)(*[addr(c["_num"]) for c in cols])
    den = (_vp * count)(*[addr(c["_den"]) for c in cols])
    rows = (_vp * count)(*[None if c["rows"] is None else addr(c["_rows"]) for c in cols])
    nforms = (ctypes.c_uint32 * count)(*[c["nform"] for c in cols])
    dforms = (ctypes.c_uint32 * count)(*[c["dform"] for c in cols])
    counts = (ctypes.c_uint64 * count)(*[0 if c["rows"] is None else len(c["rows"]) for c in cols])
    return num, nforms, den, dforms, rows, counts


def encode_operands(cols):
    for c in cols:
        c["_num"], c["_den"] = A.encode(c["num"], c["nform"]), A.encode(c["den"], c["dform"])
        if c["rows"] is not None:
            # (an empty list still needs an address to say "sparse": one index that is never read)
            c["_rows"] = np.array(list(c["rows"]) if len(c["rows"]) else [0], dtype=np.uint32)


def resolve_on_device(device, cols, n, out_form):
    """h2_dev_assigned_resolve on fresh uploads -> (status (cols, 4) u32, the out columns as integers); asserts the guard
    rows around every out column"""
    from halo2_gpu_specific_amd._lib import check

    torch = device.torch
    encode_operands(cols)
    staged = {}

    def addr(a):
        if a.shape[0] == 0:
            return None
        t = staged[id(a)] = device._assigned_operand(a)
        return t.data_ptr()

    arrays = call_arrays(cols, addr)
    with torch.cuda.stream(device.tstream):
        bufs = [torch.full((n + 2 * GUARD, 4), GUARD_WORD, dtype=torch.int64, device=device.dev) for _ in cols]
        status = torch.empty(len(cols) * 4, dtype=torch.int32, device=device.dev)
    outs = (_vp * len(cols))(*[b.data_ptr() + 32 * GUARD for b in bufs])
    check(device.L.h2_dev_assigned_resolve(*arrays, outs, len(cols), n, out_form, status.data_ptr(), device.stream),
          "h2_dev_assigned_resolve")
    got = []
    for b in bufs:
        host = device.download(b)
        assert (host[:GUARD] == np.uint64(GUARD_WORD)).all() and (host[GUARD + n:] == np.uint64(GUARD_WORD)).all(), "guard rows written"
        got.append(host[GUARD:GUARD + n])
    with torch.cuda.stream(device.tstream):
        st = status.cpu().numpy().view(np.uint32).reshape(len(cols), 4)
    return st, got


def check_columns(device, cols, n, out_form):
    """resolve and compare every row and every status with the reference"""
    st, got = resolve_on_device(device, cols, n, out_form)
    for i, (c, g) in enumerate(zip(cols, got)):
        zeros, first = A.zero_report(c["den"], c["rows"])
        assert list(st[i]) == [0, zeros, first, A.NONE], (i, list(st[i]))
        assert A.decode(g, out_form) == expected(c), "column %d of %d, n = %d" % (i, len(cols), n)


# ---- sizes and denominator patterns ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", SIZES)
def test_every_pattern_at_every_size(device, n):
    for p, name in enumerate(A.PATTERNS):
        num, den = A.pattern(name, n, seed=100 * n + p)
        check_columns(device, [column(num, den)], n, C)


@pytest.mark.parametrize("n", [(1 << 20) - 1, 1 << 20])
def test_both_sides_of_the_chain_length_switch(device, n):
    """the launch takes 8 elements a lane below 2^20 and 16 from there (the one switch below 2^21): checked on the device by
    out * den == num over seeded random field elements, so the host inverts nothing"""
    from halo2_gpu_specific_amd._lib import check

    assert A.chain_lanes(n) * (8 if n < 1 << 20 else 16) >= n > A.chain_lanes(n) * (4 if n < 1 << 20 else 8)
    D, L, torch = device, device.L, device.torch
    num, den = D.empty(n), D.empty(n)
    for t, key in ((num, b"n" * 32), (den, b"d" * 32)):
        check(L.h2_dev_random_fr(key, n, t.data_ptr(), D.stream), "h2_dev_random_fr")
    with torch.cuda.stream(D.tstream):
        den[n // 3] = 0                    # (out = 0 there; the product check below expects num = 0 in that row)
        num[n // 3] = 0
        assert int((den != 0).any(dim=1).sum()) == n - 1
        status = torch.empty(4, dtype=torch.int32, device=D.dev)
    out = D.empty(n)
    forms = (ctypes.c_uint32 * 1)(M)
    check(L.h2_dev_assigned_resolve((_vp * 1)(num.data_ptr()), forms, (_vp * 1)(den.data_ptr()), forms, None, None,
                                    (_vp * 1)(out.data_ptr()), 1, n, M, status.data_ptr(), D.stream), "h2_dev_assigned_resolve")
    back = D.eval_op(3, D.empty(n), out, den)                            # H2_OP_MUL
    with torch.cuda.stream(D.tstream):
        assert torch.equal(back, num)
        assert not bool(out[n // 3].any())
        assert status.cpu().numpy().view(np.uint32).tolist() == [0, 1, n // 3, A.NONE]


# ---- forms ----------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def small_cases():
    """(num, den, reference) per size, of values that fit a compact cell: shared by every combination of forms"""
    out = {}
    for n in (257, 2049):
        num, den = A.pattern("chain ends", n, seed=n, small=True)
        out[n] = (num, den, A.reference(num, den))
    return out


@pytest.mark.parametrize("n", [257, 2049])
@pytest.mark.parametrize("out_form", [C, M])
@pytest.mark.parametrize("dform", [C, M, K])
@pytest.mark.parametrize("nform", [C, M, K])
def test_every_combination_of_forms(device, small_cases, nform, dform, out_form, n):
    num, den, want = small_cases[n]
    st, got = resolve_on_device(device, [column(num, den, nform=nform, dform=dform)], n, out_form)
    assert list(st[0]) == [0, *A.zero_report(den), A.NONE]
    assert A.decode(got[0], out_form) == want


# ---- sparse columns -------------------------------------------------------------------------------------------------------

def sparse_column(n, rows, seed, nform=C, dform=C, zero_at=()):
    rng = np.random.Generator(np.random.PCG64(seed))
    small = K in (nform, dform)
    num, den = A.random_field(rng, n, small), A.random_field(rng, len(rows), small)
    for j in zero_at:
        den[j] = 0
    return column(num, den, rows=[int(r) for r in rows], nform=nform, dform=dform)


@pytest.mark.parametrize("n", [257, 2049])
def test_sparse_columns(device, n):
    rng = np.random.Generator(np.random.PCG64(n))
    third = np.sort(rng.choice(n, size=n // 3, replace=False))
    for i, rows in enumerate(([], [0], [n - 1], list(range(n)), third)):
        check_columns(device, [sparse_column(n, rows, seed=10 * n + i)], n, C)
    # the rows without a denominator are num in the OUTPUT form, whatever form num came in; a listed row may hold a zero
    for nform in (C, M, K):
        for out_form in (C, M):
            check_columns(device, [sparse_column(n, third, seed=n + nform, nform=nform, dform=(K, C, M)[nform], zero_at=(0, len(third) - 1))],
                          n, out_form)


@pytest.mark.parametrize("n", [257, 2049])
def test_bad_rows_are_reported_and_never_written_through(device, n):
    """an index equal to n and a repeated index: BAD_ROWS with the first bad index into rows, no write outside the column
    (resolve_on_device asserts the guard rows on both sides of every out column), and the good column next to them is
    resolved all the same"""
    rng = np.random.Generator(np.random.PCG64(n + 1))
    rows = [int(r) for r in np.sort(rng.choice(n - 1, size=n // 4, replace=False))]
    past = rows[:-1] + [n]                                   # the last index is n itself
    at = len(rows) // 2
    twice = rows[:at] + [rows[at - 1]] + rows[at + 1:]       # index `at` repeats its predecessor
    far = rows[:3] + [0xFFFFFFFF] + rows[4:]
    cols = [sparse_column(n, past, 1), sparse_column(n, twice, 2), sparse_column(n, far, 3, nform=K, dform=K), sparse_column(n, rows, 4)]
    st, got = resolve_on_device(device, cols, n, M)
    assert [int(st[i][0]) for i in range(4)] == [1, 1, 1, 0]
    assert [int(st[i][3]) for i in range(4)] == [len(rows) - 1, at, 3, A.NONE]
    assert A.decode(got[3], M) == expected(cols[3])
    # through the Python layer: device tensors (a host `rows` is refused before any device is asked)
    from halo2_gpu_specific_amd import prover

    good = prover.Rational(A.encode(cols[3]["num"], C), A.encode(cols[3]["den"], C), rows)
    good.rows = np.array(twice, dtype=np.uint32)              # (what validation would have refused)
    with pytest.raises(ValueError, match=r"fraction 0: rows\[%d\]" % at):
        device.resolve_rational([good], n, False, names=["fraction 0"])


# ---- several columns in one call ------------------------------------------------------------------------------------------

def mixed_columns(count, n, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    cols = []
    for i in range(count):
        nform, dform = (C, M, K)[i % 3], (M, K, C, C)[i % 4]
        small = K in (nform, dform)
        if i % 3 == 1:
            m = (0, 1, n // 5, n)[(i // 3) % 4]
            rows = np.sort(rng.choice(n, size=m, replace=False))
            cols.append(sparse_column(n, rows, seed + i, nform, dform, zero_at=(0,) if m > 2 else ()))
        else:
            num, den = A.pattern(A.PATTERNS[i % len(A.PATTERNS)], n, seed + i, small)
            cols.append(column(num, den, nform=nform, dform=dform))
    return cols


@pytest.mark.parametrize("count,n", [(1, 2049), (3, 2049), (17, 2049), (33, 300)])
def test_several_columns_in_one_call(device, count, n):
    """sizes of m, forms and patterns mixed; 33 columns are more than one launch takes (issued in slices)"""
    check_columns(device, mixed_columns(count, n, seed=7 * count), n, M if count % 2 else C)


def test_resolve_rational_strict_and_names(device):
    from halo2_gpu_specific_amd import prover

    n = 300
    cols = mixed_columns(2, n, seed=5)                        # canonical / Montgomery-free forms below: re-encode as one form
    rats, want = [], []
    for c in cols:
        rows = None if c["rows"] is None else np.array(c["rows"], dtype=np.uint32)
        rats.append(prover.Rational(A.encode(c["num"], C), A.encode(c["den"], C), rows))
        want.append(expected(c))
    num, den = A.pattern("lane", n, 9, small=True)
    rats.append(prover.Rational(A.encode(num, K), device.upload(A.encode(den, K), widen=False)))      # a resident operand
    want.append(A.reference(num, den))
    for montgomery in (False, True):
        outs = device.resolve_rational(rats, n, montgomery, input_montgomery=False)
        assert [A.decode(device.download(t), M if montgomery else C) for t in outs] == want
    zeros, first = A.zero_report(den)
    with pytest.raises(ValueError, match=r"slope: zero denominator at row %d \(%d in all\)" % (first, zeros)):
        device.resolve_rational(rats[2:], n, False, strict=True, names=["slope"])
    assert device.resolve_rational([], n, False) == []


# ---- the host twin --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [2049, 6149])
def test_host_twin_from_pageable_arrays(device, n):
    import halo2_gpu_specific_amd as h2
    from halo2_gpu_specific_amd import arithmetic

    cols = mixed_columns(5, n, seed=n)
    encode_operands(cols)
    arrays = call_arrays(cols, lambda a: a.ctypes.data if a.shape[0] else None)
    for out_form in (C, M):
        outs = [np.full((n + 2, 4), GUARD_WORD, dtype=np.uint64) for _ in cols]
        status = np.zeros(4 * len(cols), dtype=np.uint32)
        rc = h2.lib().h2_assigned_resolve(*arrays, (_vp * len(cols))(*[o.ctypes.data + 32 for o in outs]), len(cols), n, out_form,
                                          status.ctypes.data)
        assert rc == 0, h2.lib().h2_last_error()
        for i, (c, o) in enumerate(zip(cols, outs)):
            assert (o[0] == np.uint64(GUARD_WORD)).all() and (o[-1] == np.uint64(GUARD_WORD)).all()
            assert A.decode(o[1:-1], out_form) == expected(c), i
            assert list(status[4 * i:4 * i + 4]) == [0, *A.zero_report(c["den"], c["rows"]), A.NONE]
    # the reference's name over numpy columns (Montgomery cells in and out; None = a column of trivial denominators)
    num, den = A.pattern("chain ends", n, seed=3)
    got = arithmetic.batch_invert_assigned([A.encode(num, M), A.encode(num, M)], [A.encode(den, M), None])
    assert A.decode(got[0], M) == A.reference(num, den) and A.decode(got[1], M) == num


def test_host_twin_chunk_pipeline_equals_the_single_shot(device):
    """a dense column of page-locked memory from 2^21 rows on is resolved chunk by chunk (2^19 rows each) under its own
    transfers: the same bytes and the same status as the one-piece route the pageable copy of the same data takes -- the
    zero denominators sit in the second and the last chunk, so the first one's row is reported across a chunk's base"""
    import halo2_gpu_specific_amd as h2

    n = (1 << 21) + 5
    rng = np.random.Generator(np.random.PCG64(21))
    pinned = device.pinned_columns(2, n, compact=True) + device.pinned_columns(1, n)
    num, den, out = pinned
    num[:] = rng.integers(0, 1 << 63, size=n, dtype=np.uint64)
    den[:] = rng.integers(1, 1 << 63, size=n, dtype=np.uint64)
    first = (1 << 19) + 7
    den[[first, n - 1]] = 0
    results = []
    for a, b, o in ((num, den, out), (num.copy(), den.copy(), np.zeros((n, 4), dtype=np.uint64))):
        status = np.zeros(4, dtype=np.uint32)
        forms = (ctypes.c_uint32 * 1)(K)
        rc = h2.lib().h2_assigned_resolve((_vp * 1)(a.ctypes.data), forms, (_vp * 1)(b.ctypes.data), forms, None, None,
                                          (_vp * 1)(o.ctypes.data), 1, n, M, status.ctypes.data)
        assert rc == 0, h2.lib().h2_last_error()
        assert list(status) == [0, 2, first, A.NONE]
        results.append(o)
    assert np.array_equal(results[0], results[1])
    assert not results[0][first].any() and not results[0][n - 1].any() and results[0][first + 1].any()
    rows = [0, (1 << 19) - 1, 1 << 19, n - 2]                  # a few cells of the chunks' edges against big integers
    want = A.reference([int(num[r]) for r in rows], [int(den[r]) for r in rows])
    assert A.decode(results[0][rows], M) == want


# ---- proofs ---------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def setups(device):
    from halo2_gpu_specific_amd import prover, verifier

    made = {}

    def get(k):
        if k not in made:
            params = prover.Params.unsafe_setup(device, k, S_TRAPDOOR)
            made[k] = (params, verifier.ParamsVerifier.from_params(params))
        return made[k]

    return get


@pytest.mark.parametrize("k", [6, 9])
def test_proofs_from_rational_columns_equal_the_resolved_twins(device, setups, k):
    from halo2_gpu_specific_amd import prover, verifier
    from halo2_gpu_specific_amd.rng import ProverRng

    cs = A.is_zero_circuit()
    w = A.is_zero_witness(k, seed=k, blinding=cs.blinding_factors())
    params, pv = setups(k)
    # keygen: the selector as a fraction against the resolved column
    pk = prover.keygen(device, params, cs, w["fixed_resolved"], w["copies"])
    pk_r = prover.keygen(device, params, cs, w["fixed"], w["copies"])
    assert pk_r.fixed_commitments == pk.fixed_commitments and pk_r.transcript_repr == pk.transcript_repr
    twin = lambda: [c.copy() for c in w["resolved"]]          # noqa: E731
    for seed, use_gwc in ((1, True), (2, False)):
        want = prover.create_proof_ext(device, params, pk, twin(), ProverRng(seed), use_gwc)
        assert verifier.verify_proof_ext(device, pv, pk, want, (), use_gwc)
        for kind in ("dense", "compact", "sparse"):
            assert prover.create_proof_ext(device, params, pk_r, w[kind], ProverRng(seed), use_gwc) == want, kind
        fn = prover.create_proof if use_gwc else prover.create_proof_with_shplonk
        assert fn(device, params, pk, w["sparse"], ProverRng(seed)) == want
    # Montgomery residues in, under `montgomery`
    mont = lambda col: A.encode(A.ints(col), M)                # noqa: E731
    m_twin = [mont(c) for c in w["resolved"]]
    r = w["dense"][1]
    m_rational = [m_twin[0], prover.Rational(mont(r.num), mont(r.den)), m_twin[2]]
    assert prover.create_proof_ext(device, params, pk, m_rational, ProverRng(1), True, montgomery=True) == \
        prover.create_proof_ext(device, params, pk, [c.copy() for c in m_twin], ProverRng(1), True, montgomery=True)
    assert prover.create_proof_from_witness(device, params, pk, m_rational, ProverRng(1)) == \
        prover.create_proof_ext(device, params, pk, twin(), ProverRng(1), True)
    # v = 0 came as Rational(1, 0): the reference's unwrap under `strict_rationals`, the cell 0 without (every proof above)
    with pytest.raises(ValueError, match=r"advice column 1: zero denominator at row %d " % w["zero_rows"][0]):
        prover.create_proof(device, params, pk, w["dense"], ProverRng(1), strict_rationals=True)
    with pytest.raises(ValueError, match=r"advice column 1: zero denominator"):
        prover.check_witness(device, pk, w["compact"], strict_rationals=True)
    # check_witness: the same report from both witnesses, and the same failure when one inv cell is spoiled
    assert prover.check_witness(device, pk, twin()) == ([], 0)
    for kind in ("dense", "compact", "sparse"):
        assert prover.check_witness(device, pk, w[kind]) == ([], 0), kind
    row = next(i for i in range(2, w["n"]) if A.ints(w["resolved"][0][i:i + 1])[0])          # v != 0 there: inv matters
    bad_twin = twin()
    bad_twin[1][row] = A.limbs([(2 * A.ints(bad_twin[1][row:row + 1])[0]) % A.R_MOD])[0]
    bad_num = r.num.copy()
    bad_num[row, 0] = 2                                         # inv = 2 / v
    report = prover.check_witness(device, pk, bad_twin)
    assert report[1] >= 1 and all(f.row == row for f in report[0])
    assert prover.check_witness(device, pk, [w["dense"][0], prover.Rational(bad_num, r.den), w["dense"][2]]) == report


def test_two_circuit_instances_and_the_host_slice_device(device, setups):
    from halo2_gpu_specific_amd import host_api, prover, verifier
    from halo2_gpu_specific_amd.rng import ProverRng

    k = 6
    cs = A.is_zero_circuit()
    a = A.is_zero_witness(k, seed=11, blinding=cs.blinding_factors())
    b = A.is_zero_witness(k, seed=12, blinding=cs.blinding_factors())
    params, pv = setups(k)
    pk = prover.keygen(device, params, cs, a["fixed_resolved"], a["copies"])
    want = prover.create_proof_ext(device, params, pk, [[c.copy() for c in a["resolved"]], [c.copy() for c in b["resolved"]]],
                                   ProverRng(4), True, instances=[[], []])
    assert verifier.verify_proof_ext(device, pv, pk, want, [[], []], True, circuits=2)
    assert prover.create_proof_ext(device, params, pk, [a["dense"], b["sparse"]], ProverRng(4), True, instances=[[], []]) == want
    with pytest.raises(ValueError, match=r"circuit instance 1: advice column 1: zero denominator"):
        prover.create_proof_ext(device, params, pk, [a["sparse"], b["compact"]], ProverRng(4), True, instances=[[], []],
                                strict_rationals=True)
    # the literal drop-in: fixed and advice fractions through h2_assigned_resolve
    H = host_api.HostApiDevice()
    hparams = host_api.params_like(H, params)
    hpk = prover.keygen(H, hparams, cs, a["fixed"], a["copies"])
    single = prover.create_proof_ext(device, params, pk, [c.copy() for c in a["resolved"]], ProverRng(5), False)
    for kind in ("dense", "compact", "sparse"):
        assert prover.create_proof_ext(H, hparams, hpk, a[kind], ProverRng(5), False) == single, kind
    assert H.L.calls.get("h2_assigned_resolve") == 4


def test_a_range_checked_rational_origin(device, setups):
    """the origin of a range check given as fractions (value c / c): resolved first, then completed on the device as the
    resident column it has become -- to the bytes of the proof from the host columns"""
    from halo2_gpu_specific_amd import circuits, prover
    from halo2_gpu_specific_amd.rng import ProverRng

    k, vmax, step = 8, 61, 4
    cs = circuits.range_check(0, vmax, step)
    adv, fixed, copies = circuits.range_check_synthesize(k, vmin=0, vmax=vmax, count=150)
    params, _ = setups(k)
    pk = prover.keygen(device, params, cs, fixed, copies)
    want = prover.create_proof_ext(device, params, pk, [c.copy() for c in adv], ProverRng(3), True)
    rng = np.random.Generator(np.random.PCG64(8))
    c = rng.integers(1, 1 << 50, size=1 << k, dtype=np.uint64)
    origin = prover.Rational(adv[0][:, 0] * c, c)               # compact: value * c stays below 2^64
    pristine = adv[1].copy()
    assert prover.create_proof_ext(device, params, pk, [origin, adv[1]], ProverRng(3), True) == want
    assert np.array_equal(adv[1], pristine)
    assert prover.check_witness(device, pk, [origin, adv[1]]) == ([], 0)
