"""Range-check witness completion on the device (csrc/rangecheck.hip, prover.complete_range_check_witness_device).

Parity: the expected columns are prover.complete_range_check_witness run on host copies; the device's are equal bit for
bit (Montgomery columns after h2_dev_batch_unmont), rows at and past `usable` included, and -- independently of the host
code -- the usable rows of the companion are np.sort of the origin's.  Errors: the host path's ValueError, the columns
untouched, and the same call with good data succeeds.  Proofs: a circuit with a range check proves from resident columns,
from Montgomery residues and with the opt-in, to the bytes of the host-column proof (on the parent commit those intakes were
refused with a TypeError / ValueError)."""
import types

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

S_TRAPDOOR = 0x1D0C5F0A3B7E91C2A4D6F8091B2C3D4E5F60718293A4B5C6D7E8F9010203
BF = 5                                   # blinding factors of the range-check circuit: usable = n - 6
C, M, K = 0, 1, 2                        # canonical, Montgomery, compact
RANGES = {"u16": (0, 0xFFFF, 2), "3-40": (3, 40, 1), "5-5": (5, 5, 1), "0-61": (0, 61, 4), "2^20": (0, (1 << 20) + 3, 7)}
KS = {"u16": (16, 18, 20), "3-40": (7, 10, 13), "5-5": (7, 12), "0-61": (8, 11, 15, 19), "2^20": (18, 20)}
DISTS = ("uniform", "equal", "extremes", "padding")
FORMS = ((C, C), (M, M), (K, K), (C, M), (K, C), (M, K), (C, K), (K, M), (M, C))


@pytest.fixture(scope="module")
def device():
    from halo2_gpu_specific_amd import prover

    return prover.Device()


def fake_cs(*range_checks):
    """what complete_range_check_witness reads of a constraint system: the relations and the blinding factors"""
    return types.SimpleNamespace(range_checks=list(range_checks), blinding_factors=lambda: BF)


def n_values(vmin, vmax, step):
    return -(-(vmax - vmin) // step) + 1


def make_origin(k, vmin, vmax, step, dist, seed):
    """-> (origin (n, 4) canonical with every row below the planted ones in range and the rows to be planted zero, the
    first planted row); rows at and past `usable` hold arbitrary 64-bit values (the completion must leave them alone)"""
    n = 1 << k
    usable = n - (BF + 1)
    lo = usable - n_values(vmin, vmax, step)
    assert lo >= 1
    rng = np.random.Generator(np.random.PCG64(seed))
    col = np.zeros((n, 4), dtype=np.uint64)
    body = lo if vmin else lo - 1                         # (vmin > 0: the spare cell is a row of the column like any other)
    if dist == "uniform":
        col[:body, 0] = rng.integers(vmin, vmax + 1, size=body, dtype=np.uint64)
    elif dist == "equal":
        col[:body, 0] = vmin + (vmax - vmin) // 3
    elif dist == "extremes":
        col[:body, 0] = np.where(rng.integers(0, 2, size=body) == 1, vmax, vmin).astype(np.uint64)
    else:                                                 # a few assigned rows, then padding: zeros (vmin, where 0 is out of range)
        col[:body, 0] = vmin
        few = max(body // 50, 1)
        col[:few, 0] = rng.integers(vmin, vmax + 1, size=few, dtype=np.uint64)
    col[usable:, 0] = rng.integers(0, 1 << 63, size=n - usable, dtype=np.uint64)
    return col, lo


def to_device(device, col, form):
    """a canonical (n, 4) host column -> a device tensor in `form`"""
    from halo2_gpu_specific_amd._lib import check

    if form == K:
        return device.upload(np.ascontiguousarray(col[:, 0]), widen=False)
    t = device.upload(col)
    if form == M:
        check(device.L.h2_dev_batch_mont(t.data_ptr(), t.shape[0], device.stream), "h2_dev_batch_mont")
    return t


def to_host(device, t, form):
    """-> the canonical (n, 4) host column a device tensor in `form` stands for"""
    from halo2_gpu_specific_amd._lib import check

    if form == K:
        out = np.zeros((t.shape[0], 4), dtype=np.uint64)
        out[:, 0] = device.download(t)
        return out
    if form == M:
        t = device.clone(t)
        check(device.L.h2_dev_batch_unmont(t.data_ptr(), t.shape[0], device.stream), "h2_dev_batch_unmont")
    return device.download(t)


def run_pairs(device, k, specs, first_unassigned_known=False):
    """specs: [(range name, dist, (origin form, companion form))] completed in ONE call; checked against the host path"""
    from halo2_gpu_specific_amd import prover

    n = 1 << k
    usable = n - (BF + 1)
    host, relations, pairs, fu = [], [], [], {}
    for i, (rname, dist, (of, cf)) in enumerate(specs):
        vmin, vmax, step = RANGES[rname]
        origin, lo = make_origin(k, vmin, vmax, step, dist, seed=1000 * k + i)
        companion = np.zeros((n, 4), dtype=np.uint64)
        companion[:, 0] = np.arange(n, dtype=np.uint64) * np.uint64(3) + np.uint64(1)     # stale: every usable row is overwritten
        known = first_unassigned_known or vmin > 0
        if known:
            fu[2 * i] = lo - 1
        host += [origin, companion]
        relations.append((2 * i, 2 * i + 1, vmin, vmax, step))
        pairs.append((to_device(device, origin, of), to_device(device, companion, cf), of, cf, vmin, vmax, step,
                      lo - 1 if known else None))
    want = prover.complete_range_check_witness(fake_cs(*relations), n, [c.copy() for c in host], fu if fu else None)
    status = prover.range_check_complete_device(device, pairs, usable, n)
    assert status.shape == (len(specs), prover.RC_STATUS_WORDS)
    for i, (spec, p) in enumerate(zip(specs, pairs)):
        assert list(status[i][:3]) == [prover.RC_OK, 0xFFFFFFFF, i], (spec, status[i])
        got_origin, got_companion = to_host(device, p[0], p[2]), to_host(device, p[1], p[3])
        assert np.array_equal(got_origin, want[2 * i]), (k, spec, "origin")
        assert np.array_equal(got_companion, want[2 * i + 1]), (k, spec, "companion")
        # independent of the host code: sorted, and nothing but the low limb
        assert np.array_equal(got_companion[:usable, 0], np.sort(got_origin[:usable, 0])) and not got_companion[:usable, 1:].any()


@pytest.mark.parametrize("rname", list(RANGES))
def test_parity_with_the_host_completion(device, rname):
    """every k of the range x every distribution, the forms taken in turn (all nine pairings at the smallest k)"""
    turn = 0
    for k in KS[rname]:
        for dist in DISTS:
            for forms in (FORMS if k == KS[rname][0] else (FORMS[turn % len(FORMS)],)):
                run_pairs(device, k, [(rname, dist, forms)])
                turn += 1
    assert {7, 20} <= {k for ks in KS.values() for k in ks}


@pytest.mark.parametrize("k,specs", [
    (18, [("u16", "uniform", (C, C)), ("3-40", "padding", (M, K))]),
    (16, [("0-61", "extremes", (K, M)), ("u16", "equal", (M, M))]),
    (10, [("5-5", "equal", (C, K)), ("0-61", "uniform", (K, K))]),
    (20, [("2^20", "uniform", (C, M)), ("u16", "padding", (K, C))]),
    (12, [(r, d, f) for r, d, f in zip(["0-61", "3-40", "5-5"] * 4, DISTS * 3, FORMS + FORMS[:3])][:11]),   # more than one launch
])
def test_several_pairs_with_different_ranges_in_one_call(device, k, specs):
    run_pairs(device, k, specs)


def test_first_unassigned_known_skips_the_target_check(device):
    """with first_unassigned given the cells to be planted are not inspected: stale values there are overwritten, as on the host"""
    from halo2_gpu_specific_amd import prover

    k, (vmin, vmax, step) = 9, RANGES["0-61"]
    n = 1 << k
    usable = n - (BF + 1)
    origin, lo = make_origin(k, vmin, vmax, step, "uniform", seed=5)
    origin[lo:usable, 0] = 77                              # out of range, too: never read
    origin[lo + 1, 2] = 9
    want = prover.complete_range_check_witness(fake_cs((0, 1, vmin, vmax, step)), n, [origin.copy(), np.zeros((n, 4), np.uint64)], {0: lo - 1})
    for form in (C, M):
        adv = [to_device(device, origin, form), to_device(device, np.zeros((n, 4), np.uint64), form)]
        prover.complete_range_check_witness_device(device, fake_cs((0, 1, vmin, vmax, step)), n, adv, {0: lo - 1}, montgomery=form == M)
        assert all(np.array_equal(to_host(device, t, form), w) for t, w in zip(adv, want))


def error_case(which, k=9):
    """-> (relation, origin, first_unassigned, the host path's message)"""
    vmin, vmax, step = RANGES["0-61"]
    n = 1 << k
    usable = n - (BF + 1)
    origin, lo = make_origin(k, vmin, vmax, step, "uniform", seed=11)
    fu = None
    if which == "above vmax":
        origin[3, 0] = vmax + 9
        msg = "outside its range"
    elif which == "high limb":
        origin[lo - 2, 2] = 1
        msg = "outside its range"
    elif which == "does not fit":
        vmin, vmax, step = RANGES["u16"]
        msg = "does not fit"
    elif which == "first_unassigned == lo":
        fu, msg = {0: lo}, "does not fit"
    elif which == "cells in use":
        origin[usable - 3, 0] = 1
        msg = "already uses the cells"
    elif which == "spare cell in use":
        origin[lo - 1, 0] = 2
        msg = "already uses the cells"
    elif which == "half planted":
        origin[usable - 2, 0] = vmin + step                # what will be planted there, but the rest is still zero
        msg = "already uses the cells"
    else:
        raise KeyError(which)
    return (0, 1, vmin, vmax, step), origin, fu, msg


ERRORS = ["above vmax", "high limb", "does not fit", "first_unassigned == lo", "cells in use", "spare cell in use", "half planted"]


# (a compact column has no high limbs)
ERROR_CASES = [(w, f) for w in ERRORS for f in (C, M, K) if not (w == "high limb" and f == K)]


@pytest.mark.parametrize("which,form", ERROR_CASES, ids=["%s-%s" % (w, "cmk"[f]) for w, f in ERROR_CASES])
def test_errors_are_the_host_paths_and_leave_the_columns_alone(device, which, form):
    from halo2_gpu_specific_amd import prover

    k = 9
    n = 1 << k
    relation, origin, fu, msg = error_case(which, k)
    stale = np.zeros((n, 4), dtype=np.uint64)
    stale[:, 0] = 5
    with pytest.raises(ValueError, match=msg) as host_error:
        prover.complete_range_check_witness(fake_cs(relation), n, [origin.copy(), stale.copy()], fu)
    adv = [to_device(device, origin, form), to_device(device, stale, form)]
    with pytest.raises(ValueError) as device_error:
        prover.complete_range_check_witness_device(device, fake_cs(relation), n, adv, fu, montgomery=form == M)
    assert str(device_error.value) == str(host_error.value)
    # nothing was written (the host path writes nothing either in the cases it refuses before planting)
    assert np.array_equal(to_host(device, adv[0], form), origin) and np.array_equal(to_host(device, adv[1], form), stale)
    # the same call with good data succeeds, on the same library
    good_relation, good, good_fu = (0, 1) + RANGES["0-61"], make_origin(k, *RANGES["0-61"], "uniform", seed=11)[0], None
    want = prover.complete_range_check_witness(fake_cs(good_relation), n, [good.copy(), stale.copy()], good_fu)
    adv = [to_device(device, good, form), to_device(device, stale, form)]
    prover.complete_range_check_witness_device(device, fake_cs(good_relation), n, adv, good_fu, montgomery=form == M)
    got = [to_host(device, t, C if form == K else form) for t in adv]       # (a compact column comes back widened)
    assert all(np.array_equal(g, w) for g, w in zip(got, want))
    # ... and again on the completed columns: the planted values are recognised
    if form != K:
        prover.complete_range_check_witness_device(device, fake_cs(good_relation), n, adv, None, montgomery=form == M)
        assert all(np.array_equal(to_host(device, t, form), w) for t, w in zip(adv, want))


def test_status_records_name_the_pair_and_the_first_offending_row(device):
    from halo2_gpu_specific_amd import prover

    k = 10
    n = 1 << k
    usable = n - (BF + 1)
    vmin, vmax, step = RANGES["0-61"]
    good, lo = make_origin(k, vmin, vmax, step, "uniform", seed=3)
    bad = good.copy()
    bad[[40, 17, 300], 0] = vmax + 1
    used = good.copy()
    used[usable - 1, 0] = 9
    zeros = np.zeros((n, 4), dtype=np.uint64)
    cols = [to_device(device, c, C) for c in (good, zeros, bad, zeros, used, zeros, good, zeros, good, zeros)]
    pairs = [(cols[0], cols[1], C, C, vmin, vmax, step, None), (cols[2], cols[3], C, C, vmin, vmax, step, None),
             (cols[4], cols[5], C, C, vmin, vmax, step, None), (cols[6], cols[7], C, C, 0, 1 << 24, 1, None),
             (cols[8], cols[9], C, C, vmin, vmax, step, lo)]
    status = prover.range_check_complete_device(device, pairs, usable, n)
    assert [list(r[:3]) for r in status] == [[prover.RC_OK, 0xFFFFFFFF, 0], [prover.RC_OUT_OF_RANGE, 17, 1],
                                             [prover.RC_IN_USE, usable - 1, 2], [prover.RC_UNSUPPORTED, 0xFFFFFFFF, 3],
                                             [prover.RC_NO_FIT, lo, 4]]
    # a failing pair does not stop the others, and is itself left alone
    want = prover.complete_range_check_witness(fake_cs((0, 1, vmin, vmax, step)), n, [good.copy(), zeros.copy()])
    assert np.array_equal(device.download(cols[0]), want[0]) and np.array_equal(device.download(cols[1]), want[1])
    for t, before in zip(cols[2:], (bad, zeros, used, zeros, good, zeros, good, zeros)):
        assert np.array_equal(device.download(t), before)


def test_wide_range_cap(device):
    """vmax - vmin = 2^24 is past the counting sort's cap: the documented status from the C entry, a ValueError for resident
    columns; host columns keep the host path (which sorts)"""
    from halo2_gpu_specific_amd import prover, witness

    k = 8
    n = 1 << k
    cs = fake_cs((0, 1, 0, 1 << 24, 1 << 20))
    origin = np.zeros((n, 4), dtype=np.uint64)
    origin[:100, 0] = np.arange(100, dtype=np.uint64) * np.uint64(100000)
    adv = [to_device(device, origin, C), to_device(device, np.zeros((n, 4), np.uint64), C)]
    with pytest.raises(ValueError, match="2\\^24"):
        prover.complete_range_check_witness_device(device, cs, n, adv)
    assert np.array_equal(device.download(adv[0]), origin)
    host = witness._witness_sets(cs, n, [origin.copy(), np.zeros((n, 4), np.uint64)], (), False, None, device=device)[0][0]
    assert isinstance(host[1], np.ndarray) and np.array_equal(host[1][:n - 6, 0], np.sort(host[0][:n - 6, 0]))


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


def montgomery_host(device, col):
    return to_host_raw(device, to_device(device, col, M))


def to_host_raw(device, t):
    return device.download(t).copy()


@pytest.mark.parametrize("k,vmax,step,count", [(8, 61, 4, 150), (9, 100, 1, 300), (18, 0xFFFF, 2, 0xFFFF)])
def test_proofs_from_resident_montgomery_and_opt_in_witnesses(device, setups, k, vmax, step, count):
    from halo2_gpu_specific_amd import circuits, prover, verifier
    from halo2_gpu_specific_amd.rng import ProverRng

    cs = circuits.range_check(0, vmax, step)
    adv, fixed, copies = circuits.range_check_synthesize(k, vmin=0, vmax=vmax, count=count)
    params, pv = setups(k)
    pk = prover.keygen(device, params, cs, fixed, copies)
    pristine = [c.copy() for c in adv]
    mont = [montgomery_host(device, c) for c in adv]
    for seed, use_gwc in ((1, True), (2, False)):
        want = prover.create_proof_ext(device, params, pk, [c.copy() for c in adv], ProverRng(seed), use_gwc)
        assert verifier.verify_proof_ext(device, pv, pk, want, (), use_gwc)
        # device-tensor columns (on the parent commit: TypeError, "must be host columns")
        resident = [device.upload(c) for c in adv]
        assert prover.create_proof_ext(device, params, pk, resident, ProverRng(seed), use_gwc) == want
        # ... one of the two resident, the other a host column that is not written
        mixed = [device.upload(adv[0]), adv[1]]
        assert prover.create_proof_ext(device, params, pk, mixed, ProverRng(seed), use_gwc) == want
        # Montgomery residues (on the parent commit: ValueError, "needs canonical advice columns")
        m = [c.copy() for c in mont]
        assert prover.create_proof_ext(device, params, pk, m, ProverRng(seed), use_gwc, montgomery=True) == want
        assert all(np.array_equal(a, b) for a, b in zip(m, mont))
        if use_gwc:
            assert prover.create_proof_from_witness(device, params, pk, m, ProverRng(seed)) == want
        # the opt-in: host columns, completed on the device, unmodified
        assert prover.create_proof_ext(device, params, pk, adv, ProverRng(seed), use_gwc, range_checks_on_device=True) == want
        assert all(np.array_equal(a, b) for a, b in zip(adv, pristine))
        # compact host columns under the opt-in
        compact = [np.ascontiguousarray(c[:, 0]) for c in adv]
        assert prover.create_proof_ext(device, params, pk, compact, ProverRng(seed), use_gwc, range_checks_on_device=True) == want
    # check_witness: nothing to report on the resident forms, and the witness is not modified
    resident = [device.upload(c) for c in adv]
    assert prover.check_witness(device, pk, resident) == ([], 0)
    assert all(np.array_equal(device.download(t), c) for t, c in zip(resident, adv))
    assert prover.check_witness(device, pk, mont, montgomery=True) == ([], 0)
    assert prover.check_witness(device, pk, adv, range_checks_on_device=True) == ([], 0)
    assert all(np.array_equal(a, b) for a, b in zip(adv, pristine))
    # one row pushed out of range: reported as the host path reports it
    bad = [c.copy() for c in adv]
    bad[0][3, 0] = np.uint64(vmax + 9)
    with pytest.raises(ValueError, match="outside its range") as host_error:
        prover.check_witness(device, pk, bad)
    with pytest.raises(ValueError) as device_error:
        prover.check_witness(device, pk, [device.upload(c) for c in bad])
    assert str(device_error.value) == str(host_error.value)
    with pytest.raises(ValueError, match="outside its range"):
        prover.assert_satisfied(device, pk, [device.upload(c) for c in bad])
    with pytest.raises(ValueError, match="outside its range"):
        prover.create_proof_ext(device, params, pk, [device.upload(c) for c in bad], ProverRng(1), True)
    # the library is usable afterwards
    assert prover.create_proof_ext(device, params, pk, [device.upload(c) for c in adv], ProverRng(2), False) == want


def test_two_circuit_instances_with_their_own_first_unassigned(device, setups):
    from halo2_gpu_specific_amd import circuits, prover, verifier
    from halo2_gpu_specific_amd.rng import ProverRng

    k, vmax, step = 9, 100, 1
    cs = circuits.range_check(0, vmax, step)
    a, fixed, copies = circuits.range_check_synthesize(k, vmin=0, vmax=vmax, count=300)
    b, _, _ = circuits.range_check_synthesize(k, seed=77, vmin=0, vmax=vmax, count=120)
    params, pv = setups(k)
    pk = prover.keygen(device, params, cs, fixed, copies)
    fu = [{0: 300}, {0: 120}]
    want = prover.create_proof_ext(device, params, pk, [[c.copy() for c in a], [c.copy() for c in b]], ProverRng(4), True,
                                   instances=[[], []], first_unassigned=fu)
    assert verifier.verify_proof_ext(device, pv, pk, want, [[], []], True, circuits=2)
    resident = [[device.upload(c) for c in a], [device.upload(c) for c in b]]
    assert prover.create_proof_ext(device, params, pk, resident, ProverRng(4), True, instances=[[], []], first_unassigned=fu) == want
    assert prover.create_proof_ext(device, params, pk, [a, b], ProverRng(4), True, instances=[[], []], first_unassigned=fu,
                                   range_checks_on_device=True) == want
    # a first_unassigned that reaches into the planted cells of the SECOND instance only
    lo = (1 << k) - 6 - 101
    with pytest.raises(ValueError, match="does not fit"):
        prover.create_proof_ext(device, params, pk, [[device.upload(c) for c in a], [device.upload(c) for c in b]], ProverRng(4), True,
                                instances=[[], []], first_unassigned=[{0: 300}, {0: lo}])
