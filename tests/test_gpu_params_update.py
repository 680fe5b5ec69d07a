"""h2_dev_g1_mul_each and Params.update on the device: the per-point multiplication against Python integers, the update
against a fresh setup of the product of the trapdoors, verify_update's acceptance and every rejection it is there for, an
updated SRS through its file into a proof and a verifier, and the argument checks."""
import gc
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import ref_plonk as rp
from h2util import R_MOD, ROOT, points_to_arr, to_mont
from test_plonk_host import S_TRAPDOOR

pytestmark = pytest.mark.gpu

TAU = 0x0B5E55ED7A0C0FFEE1234567890ABCDEF0FEDCBA09876543210F1E2D3C4B5A69
BLOCK = 256                                                      # G1MUL_BLOCK (csrc/g1mul.hpp)
SIZES = [1, 63, 64, 65, BLOCK + 1]
H2_OK, H2_ERR_INVALID = 0, 1


@pytest.fixture(scope="module")
def device():
    from halo2_gpu_specific_amd import prover

    D = prover.Device()
    yield D
    gc.collect()


# ---- 1. the kernel -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mul_cases():
    """BLOCK + 1 (point, scalar) pairs and the expected products by ref_plonk's big-integer double-and-add; every size of the
    test is a prefix.  9 scalars against 7 points, both cycled: every combination occurs in the first 63 pairs."""
    rnd = random.Random(0x6D756C)
    P = rp.g1_mul(rp.G1, rnd.randrange(1, R_MOD))
    points = [rp.G1, P, None, rp.g1_mul(rp.G1, rnd.randrange(1, R_MOD)), rp.g1_neg(P), rp.g1_mul(rp.G1, rnd.randrange(1, R_MOD)),
              rp.g1_mul(rp.G1, 3)]
    scalars = [rnd.randrange(R_MOD), 0, 1, 2, R_MOD - 1, R_MOD - 2, 1 << 253, rnd.getrandbits(127) | 1 << 126,
               rnd.randrange(R_MOD)]
    n = max(SIZES)
    pts = [points[i % 7] for i in range(n)]
    ks = [scalars[i % 9] if i < 63 else rnd.randrange(R_MOD) for i in range(n)]
    want = [rp.g1_mul(p, k) if k else None for p, k in zip(pts, ks)]
    arr = lambda ps: points_to_arr([(0, 0) if p is None else p for p in ps])  # noqa: E731
    return arr(pts), to_mont(ks), arr(want)


@pytest.mark.parametrize("in_place", [False, True])
@pytest.mark.parametrize("n", SIZES)
def test_g1_mul_each_equals_big_integer_double_and_add(device, mul_cases, n, in_place):
    from halo2_gpu_specific_amd import params_update as pu

    D = device
    points, scalars, want = (a[:n] for a in mul_cases)
    d_points, d_scalars = D.upload(points), D.upload(scalars)
    with D.torch.cuda.stream(D.tstream):
        guard = D.torch.full((n + 1, 8), -1, dtype=D.torch.int64, device=D.dev)   # one row past the end: never written
    out = d_points if in_place else guard[:n]
    got = pu.g1_mul_each(D, d_points, d_scalars, out=out)
    assert got.data_ptr() == out.data_ptr()
    assert np.array_equal(D.download(got).reshape(n, 8), want)
    assert (D.download(guard[n:]) == np.uint64(2**64 - 1)).all()
    if not in_place:
        assert np.array_equal(D.download(d_points).reshape(n, 8), points)


def test_g1_mul_each_negated_point_gives_the_negated_product(device, mul_cases):
    """P and -P under one scalar (pairs 1 and 4 of the cases carry P and -P): y and q - y, the same x"""
    from halo2_gpu_specific_amd import params_update as pu

    D = device
    points, scalars, _ = mul_cases
    both = np.array([points[1], points[4]], dtype=np.uint64)
    k = np.array([scalars[8], scalars[8]], dtype=np.uint64)
    got = D.download(pu.g1_mul_each(D, D.upload(both), D.upload(k))).reshape(2, 8)
    from g1_ntt_reference import g1_neg

    assert got[0].any() and np.array_equal(g1_neg(got[0:1])[0], got[1])


def test_g1_mul_each_argument_checks(device):
    D = device
    with D.torch.cuda.stream(D.tstream):
        t = D.torch.zeros((4, 8), dtype=D.torch.int64, device=D.dev)
    p = t.data_ptr()
    L = D.L
    assert L.h2_dev_g1_mul_each(p, p, 0, p, D.stream) == H2_OK
    assert L.h2_dev_g1_mul_each(None, None, 0, None, D.stream) == H2_OK
    assert L.h2_dev_g1_mul_each(None, p, 4, p, D.stream) == H2_ERR_INVALID
    assert L.h2_dev_g1_mul_each(p, None, 4, p, D.stream) == H2_ERR_INVALID
    assert L.h2_dev_g1_mul_each(p, p, 4, None, D.stream) == H2_ERR_INVALID
    D.sync()
    assert not D.download(t).any()


# ---- 2. the update is the setup of the product ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def updated(device):
    """per k: (old, new, contribution) of unsafe_setup(S_TRAPDOOR).update(TAU)"""
    from halo2_gpu_specific_amd import prover

    made = {}

    def get(k):
        if k not in made:
            old = prover.Params.unsafe_setup(device, k, S_TRAPDOOR)
            made[k] = (old,) + tuple(old.update(device, TAU))
        return made[k]

    return get


@pytest.mark.parametrize("k", [1, 6, 7, 9, 15])
def test_update_equals_a_fresh_setup_of_the_product(device, k):
    """k = 15 is the smallest size at which the constructor builds the shifted-base tables: its table path sees a copied g"""
    from halo2_gpu_specific_amd import params_update as pu, prover

    D = device
    old = prover.Params.unsafe_setup(D, k, S_TRAPDOOR)
    before = [D.download(t).copy() for t in (old.g, old.g_lagrange)]
    s_g2_before = old.s_g2.copy()
    new, contribution = old.update(D, TAU)
    fresh = prover.Params.unsafe_setup(D, k, S_TRAPDOOR * TAU % R_MOD)
    assert new.k == k and new.n == 1 << k
    assert np.array_equal(D.download(new.g), D.download(fresh.g))
    assert np.array_equal(D.download(new.g_lagrange), D.download(fresh.g_lagrange))
    assert np.array_equal(new.s_g2, fresh.s_g2)
    assert contribution == pu.contribution_of(TAU) and len(contribution) == 64
    # the old object is untouched and shares no storage with the new one
    assert new.g.data_ptr() != old.g.data_ptr() and new.g_lagrange.data_ptr() != old.g_lagrange.data_ptr()
    assert np.array_equal(D.download(old.g), before[0]) and np.array_equal(D.download(old.g_lagrange), before[1])
    assert np.array_equal(old.s_g2, s_g2_before)
    if k == 15:
        assert old.table_bytes > 0 and new.table_bytes > 0
        # a commitment over the new object's tables equals the one over its plain points
        scalars = D.upload(to_mont([random.Random(k).randrange(R_MOD) for _ in range(1 << k)]))
        plain = prover.Params(D, k, D.clone(new.g), D.clone(new.g_lagrange), tables=False)
        assert D.msm_batch([scalars], new.g, 1 << k) == D.msm_batch([scalars], plain.g, 1 << k)
    del old, new, fresh
    gc.collect()


# ---- 3. verify_update --------------------------------------------------------------------------------------------------------------
def with_row(D, params, table, index, row, s_g2):
    """a copy of `params` (no tables) with one row of `table` replaced"""
    from halo2_gpu_specific_amd import prover

    g, gl = D.clone(params.g), D.clone(params.g_lagrange)
    with D.torch.cuda.stream(D.tstream):
        (g if table == "g" else gl)[index] = D.upload(np.asarray(row, dtype=np.uint64).reshape(1, 8))[0]
    out = prover.Params(D, params.k, g, gl, tables=False)
    out.s_g2 = s_g2
    return out


def test_verify_update_accepts_and_rejects(device, updated):
    from halo2_gpu_specific_amd import params_update as pu

    D, k = device, 6
    old, new, contribution = updated(k)
    report = pu.verify_update(D, old, new, contribution, seed=1)
    assert report.ok and report.base_kept and report.step and report.structure.ok, pu.describe(report)
    assert "update ok" in pu.describe(report)
    assert pu.assert_valid_update(D, old, new, contribution, seed=1).ok
    # a contribution made from another tau
    r = pu.verify_update(D, old, new, pu.contribution_of(TAU + 1), seed=2)
    assert (r.ok, r.base_kept, r.step, r.structure.ok) == (False, True, False, True)
    # new.g[0] replaced
    other = points_to_arr([rp.g1_mul(rp.G1, 77)])[0]
    r = pu.verify_update(D, old, with_row(D, new, "g", 0, other, new.s_g2), contribution, seed=3)
    assert (r.ok, r.base_kept, r.step) == (False, False, True)
    assert r.structure.powers is False and r.structure.first_bad_power == 0
    # new.g[5] replaced by another curve point
    r = pu.verify_update(D, old, with_row(D, new, "g", 5, other, new.s_g2), contribution, seed=4)
    assert (r.ok, r.base_kept, r.step) == (False, True, True)
    assert r.structure.powers is False and r.structure.first_bad_power == 4 and r.structure.points_total == 0
    with pytest.raises(pu.ParamsError) as err:
        pu.assert_valid_update(D, old, with_row(D, new, "g", 5, other, new.s_g2), contribution, seed=4)
    assert err.value.report.structure.first_bad_power == 4 and "update NOT ok" in str(err.value)
    # new.s_g2 left at the old value
    stale = with_row(D, new, "g", 0, D.download(new.g[0:1])[0], old.s_g2)
    r = pu.verify_update(D, old, stale, contribution, seed=5)
    assert (r.ok, r.base_kept, r.step) == (False, True, True)
    assert r.structure.powers is False and r.structure.lagrange
    # 64 zero bytes as the contribution: False, no exception
    r = pu.verify_update(D, old, new, bytes(64), seed=6)
    assert (r.ok, r.base_kept, r.step, r.structure.ok) == (False, True, False, True)
    # the old SRS offered as its own update
    r = pu.verify_update(D, old, old, contribution, seed=7)
    assert (r.ok, r.base_kept, r.step, r.structure.ok) == (False, True, False, True)


# ---- 4. end to end -----------------------------------------------------------------------------------------------------------------
def test_updated_srs_through_its_file_into_a_proof(device, updated, tmp_path):
    from halo2_gpu_specific_amd import circuits, formats, params_update as pu, prover, verifier
    from halo2_gpu_specific_amd.pairing import g2_compress
    from halo2_gpu_specific_amd.rng import ProverRng

    D, k, seed = device, 5, 20261018
    old = updated(k)[0]
    old_path, new_path = str(tmp_path / "old.params"), str(tmp_path / "new.params")
    formats.params_write(D, old, old_path, formats.params_additional_data(old))
    new, contribution = old.update(D, pu.tau_from_seed(seed))
    formats.params_write(D, new, new_path, g2_compress(new.s_g2))
    back, additional = formats.params_read(D, new_path, verify=True, seed=1)
    assert additional == g2_compress(new.s_g2) and additional != formats.params_additional_data(old)
    assert np.array_equal(D.download(back.g), D.download(new.g))
    assert np.array_equal(D.download(back.g_lagrange), D.download(new.g_lagrange))
    assert pu.verify_update(D, old, back, contribution, s_g2=additional, seed=2).ok
    # a proof under the updated SRS: accepted under its verifier, rejected under the old one's
    adv, fixed, copies = circuits.mini_plonk_synthesize(k)
    pk = prover.keygen(D, back, circuits.mini_plonk(), fixed, copies)
    proof = prover.create_proof(D, back, pk, adv, ProverRng(11))
    assert verifier.verify_proof(D, verifier.ParamsVerifier.from_params(back, additional), pk, proof)
    assert not verifier.verify_proof(D, verifier.ParamsVerifier.from_params(old), pk, proof)
    # the tool with the same seed on the same input: byte-identical files; and its --check of them
    tool = os.path.join(ROOT, "tools", "params_update.py")
    tool_out, tool_contribution = str(tmp_path / "tool.params"), str(tmp_path / "tool.contribution")
    res = subprocess.run([sys.executable, tool, old_path, tool_out, "--seed", str(seed), "--contribution", tool_contribution],
                         capture_output=True, text=True, timeout=280)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-3000:]
    assert "FOR TESTS ONLY" in res.stderr
    assert open(tool_out, "rb").read() == open(new_path, "rb").read()
    assert open(tool_contribution, "rb").read() == contribution
    res = subprocess.run([sys.executable, tool, "--check", old_path, tool_out, tool_contribution, "--seed", "3"],
                         capture_output=True, text=True, timeout=280)
    assert res.returncode == 0 and res.stdout.startswith("update ok"), res.stdout[-2000:] + res.stderr[-3000:]
    res = subprocess.run([sys.executable, tool, "--check", old_path, old_path, tool_contribution, "--seed", "3"],
                         capture_output=True, text=True, timeout=280)
    assert res.returncode == 1 and res.stdout.startswith("update NOT ok"), res.stdout[-2000:] + res.stderr[-3000:]


# ---- 5. argument checks ------------------------------------------------------------------------------------------------------------
def test_update_argument_checks(device, updated):
    from halo2_gpu_specific_amd import prover

    D = device
    old = updated(6)[0]
    with pytest.raises(ValueError, match="tau"):
        old.update(D, 0)
    with pytest.raises(ValueError, match="tau"):
        old.update(D, R_MOD)
    with pytest.raises(ValueError, match="at least 2 points"):
        single = prover.Params(D, 0, D.clone(old.g[:1]), D.clone(old.g_lagrange[:1]), tables=False)
        single.s_g2 = old.s_g2
        single.update(D, TAU)
    bare = prover.Params(D, 6, old.g, old.g_lagrange, tables=False)
    with pytest.raises(ValueError, match="carry no \\[s\\]G2"):
        bare.update(D, TAU)
    # ... and with one given, in either form verify accepts, the result is the same; a drawn tau gives a valid update
    from halo2_gpu_specific_amd import formats, params_update as pu

    a, ca = bare.update(D, TAU, s_g2=old.s_g2)
    b, cb = bare.update(D, TAU, s_g2=formats.params_additional_data(old))
    assert ca == cb and np.array_equal(a.s_g2, b.s_g2) and np.array_equal(D.download(a.g), D.download(b.g))
    drawn, contribution = old.update(D)
    assert contribution != ca and pu.verify_update(D, old, drawn, contribution, seed=8).ok
