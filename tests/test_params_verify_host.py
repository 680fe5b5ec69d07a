"""Params.verify without a GPU: the new entry point's declaration, export and argument checks; the masked scalar columns
(params_check.structure_scalars) on CPU tensors; and the two decisions at k = 3, fed with inner products computed by the
big-integer curve arithmetic of the tests (ref_plonk) and decided with the library's host pairing."""
import ctypes
import os
import re

import numpy as np
import pytest

import ref_plonk as rp
from g1_ntt_reference import omega
from h2util import R_MOD, ROOT

import halo2_gpu_specific_amd as h2
from halo2_gpu_specific_amd import params_check as pc
from halo2_gpu_specific_amd._lib import SYMBOLS

INVALID = 1
S_TRAPDOOR = 0x1D0C5F0A3B7E91C2A4D6F8091B2C3D4E5F60718293A4B5C6D7E8F9010203
K = 3
N = 1 << K


def test_entry_is_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "halo2_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bint\s+h2_dev_g1_check_points\s*\(", code)
    assert "poly/commitment.rs:262-275" in text
    for name in ("H2_SRS_NONCANONICAL", "H2_SRS_IDENTITY", "H2_SRS_OFF_CURVE", "H2_SRS_FORBID_IDENTITY"):
        assert name in code
    assert "h2_dev_g1_check_points" in SYMBOLS
    assert hasattr(h2.lib(), "h2_dev_g1_check_points")
    # the Python constants are the header's
    enums = dict(re.findall(r"(H2_SRS_[A-Z_]+)\s*=\s*(\d+)", code))
    assert (pc.NONCANONICAL, pc.IDENTITY, pc.OFF_CURVE) == tuple(int(enums["H2_SRS_" + n]) for n in
                                                               ("NONCANONICAL", "IDENTITY", "OFF_CURVE"))
    assert pc.FORBID_IDENTITY == int(enums["H2_SRS_FORBID_IDENTITY"])


def test_check_points_rejects_bad_arguments_without_a_device():
    L = h2.lib()
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.addressof(buf)
    assert L.h2_dev_g1_check_points(None, 4, 0, 1, p, p, 4, None) == INVALID        # null points with n > 0
    assert b"null" in L.h2_last_error()
    assert L.h2_dev_g1_check_points(p, 4, 0, 1, p, None, 4, None) == INVALID        # cap > 0 with null records
    assert b"null" in L.h2_last_error()
    assert L.h2_dev_g1_check_points(p, 4, 0, 1, None, p, 4, None) == INVALID        # nowhere to count
    assert L.h2_dev_g1_check_points(p, (1 << 28) + 1, 0, 1, p, p, 4, None) == INVALID
    assert b"2^28" in L.h2_last_error()
    assert L.h2_dev_g1_check_points(p, 4, 0, 2, p, p, 4, None) == INVALID           # a flag the header does not define
    assert b"flag" in L.h2_last_error()


# ---- structure_scalars ---------------------------------------------------------------------------------------------------
def _column(values):
    import torch

    a = np.array([[(v >> (64 * j)) & ((1 << 64) - 1) for j in range(4)] for v in values], dtype=np.uint64)
    return torch.from_numpy(a.view(np.int64))


def _values(t):
    return [int(l[0]) | int(l[1]) << 64 | int(l[2]) << 128 | int(l[3]) << 192 for l in t.numpy().view(np.uint64)]


def _random(seed, n=N):
    rng = np.random.default_rng(seed)
    return [int.from_bytes(rng.bytes(32), "little") % (R_MOD - 1) + 1 for _ in range(n)]       # never zero


@pytest.mark.parametrize("lo,hi", [(0, 8), (0, 1), (3, 5), (7, 8)])
def test_structure_scalars_on_cpu_tensors(lo, hi):
    r = _random(1)
    t = _column(r)
    a, b = (_values(x) for x in pc.structure_scalars(t, lo, hi))
    assert _values(t) == r                                    # the input is left alone
    assert a[N - 1] == 0 and b[0] == 0
    for i in range(N - 1):
        assert b[i + 1] == a[i]
    for i in range(N):
        inside = lo <= i < hi
        assert a[i] == (r[i] if inside and i < N - 1 else 0)
        if not lo < i <= hi:                                  # b is a one row down: zero outside [lo + 1, hi + 1)
            assert b[i] == 0
    m = _values(pc.mask_range(t, lo, hi))
    assert m == [r[i] if lo <= i < hi else 0 for i in range(N)]


# ---- the decisions at k = 3 -----------------------------------------------------------------------------------------------
def _msm(scalars, points):
    acc = None
    for s, P in zip(scalars, points):
        if s % R_MOD:
            acc = rp.g1_add(acc, rp.g1_mul(P, s))
    return acc


def _intt(e):
    w_inv, n_inv = pow(omega(K), -1, R_MOD), pow(N, -1, R_MOD)
    return [n_inv * sum(e[i] * pow(w_inv, i * j, R_MOD) for i in range(N)) % R_MOD for j in range(N)]


@pytest.fixture(scope="module")
def srs():
    """(g, g_lagrange) of k = 3 as host points: g[i] = [s^i] G, g_lagrange[i] = [n^-1 sum_j w^(-ij) s^j] G"""
    s = S_TRAPDOOR % R_MOD
    g = [rp.g1_mul(rp.G1, pow(s, i, R_MOD)) for i in range(N)]
    gl = [rp.g1_mul(rp.G1, c) for c in _intt([pow(s, j, R_MOD) for j in range(N)])]
    return g, gl


def _products(g, gl, seed=7):
    """A, B, C1, C2 as Params.verify forms them, the columns from structure_scalars itself"""
    a, b = (_values(x) for x in pc.structure_scalars(_column(_random(seed)), 0, N))
    e = _random(seed + 1)
    return _msm(a, g), _msm(b, g), _msm(_intt(e), g), _msm(e, gl)


def test_decisions_accept_a_true_srs(srs):
    import bn254_pairing as bp
    from halo2_gpu_specific_amd.pairing import g2_mul_generator

    g, gl = srs
    A, B, C1, C2 = _products(g, gl)
    assert pc.powers_decision(A, B, g2_mul_generator(S_TRAPDOOR))
    assert pc.lagrange_decision(C1, C2)
    # the same equation under the big-integer pairing of the tests
    assert bp.pairing_check([(A, bp.g2_mul(bp.G2, S_TRAPDOOR % R_MOD)), (rp.g1_neg(B), bp.G2)])
    # the 64 compressed bytes of an SRS file's additional_data name the same point
    from halo2_gpu_specific_amd.pairing import g2_compress

    assert pc.powers_decision(A, B, pc.parse_s_g2(g2_compress(g2_mul_generator(S_TRAPDOOR))))


def test_decisions_reject_swapped_powers(srs):
    from halo2_gpu_specific_amd.pairing import g2_mul_generator

    g, gl = srs
    g = list(g)
    g[5], g[6] = g[6], g[5]
    A, B, C1, C2 = _products(g, gl)
    assert not pc.powers_decision(A, B, g2_mul_generator(S_TRAPDOOR))
    assert not pc.lagrange_decision(C1, C2)                   # the basis no longer matches this g


def test_decisions_reject_another_s_g2(srs):
    from halo2_gpu_specific_amd.pairing import g2_mul_generator

    g, gl = srs
    A, B, C1, C2 = _products(g, gl)
    assert not pc.powers_decision(A, B, g2_mul_generator(S_TRAPDOOR + 1))
    assert pc.lagrange_decision(C1, C2)


def test_decisions_reject_swapped_lagrange_entries(srs):
    from halo2_gpu_specific_amd.pairing import g2_mul_generator

    g, gl = srs
    gl = list(gl)
    gl[1], gl[6] = gl[6], gl[1]
    A, B, C1, C2 = _products(g, gl)
    assert pc.powers_decision(A, B, g2_mul_generator(S_TRAPDOOR))
    assert not pc.lagrange_decision(C1, C2)


def test_report_text_and_error():
    rep = pc.ParamsReport(False, [("g", 77, pc.OFF_CURVE)], 1, None, None, None, None, True, {})
    err = pc.ParamsError(rep)
    assert err.report is rep and isinstance(err, ValueError)
    assert "g[77] off-curve" in str(err) and "NOT ok" in str(err)
    good = pc.ParamsReport(True, [], 0, True, None, True, None, True, {})
    assert pc.describe(good).startswith("parameters ok")


def test_bisect_finds_the_lowest_failing_term():
    for n in (1, 2, 8, 13):
        for bad in range(n):
            probes = []

            def fails(m):
                probes.append(m)
                return m > bad

            assert pc._bisect(n, fails) == bad
            assert len(probes) <= n.bit_length()
