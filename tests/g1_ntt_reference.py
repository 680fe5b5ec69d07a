"""The definitional G1 DFT on the CPU oracle: each output point is one MSM (oracle_multiexp_serial) over the scalars
n^-1 w^(-ij) (inverse) or w^(ij) (forward), normalised by oracle_g1_to_affine -- the reference for h2_dev_g1_ntt.
w = ROOT_OF_UNITY^(2^(28 - k)), the omega of EvaluationDomain::new.  Points: (n, 8) u64 affine Montgomery, identity (0, 0)."""
import numpy as np

from h2util import R_MOD, fr_mont

ROOT_OF_UNITY = 0x03DDB9F5166D18B798865EA93DD31F743215CF6DD39329C8D34F1ED960C37C9C
S = 28


def omega(k):
    return pow(ROOT_OF_UNITY, 1 << (S - k), R_MOD)


def dft_scalars(k, inverse):
    """the (n, n) matrix of scalars as canonical integers: row i holds the coefficients of output i"""
    n = 1 << k
    w = omega(k)
    if inverse:
        w = pow(w, -1, R_MOD)
    scale = pow(n, -1, R_MOD) if inverse else 1
    return [[scale * pow(w, i * j % n, R_MOD) % R_MOD for j in range(n)] for i in range(n)]


def g1_dft(oracle, points, k, inverse):
    points = np.ascontiguousarray(points, dtype=np.uint64).reshape(-1, 8)
    n = 1 << k
    assert points.shape[0] == n
    out = np.zeros((n, 8), dtype=np.uint64)
    for i, row in enumerate(dft_scalars(k, inverse)):
        coeffs = np.array([fr_mont(c) for c in row], dtype=np.uint64)
        out[i] = oracle.to_affine(oracle.multiexp_serial(coeffs, points))
    return out


def g1_mul(oracle, point, scalar):
    """[scalar] point (canonical scalar), affine"""
    return oracle.to_affine(oracle.g1_mul(np.ascontiguousarray(point, dtype=np.uint64), fr_mont(scalar % R_MOD)))


def g1_neg(points):
    """-P for affine Montgomery points (the identity stays (0, 0))"""
    from h2util import Q_MOD, int_to_limbs, limbs_to_int

    out = np.array(points, dtype=np.uint64).reshape(-1, 8).copy()
    for r in out:
        y = limbs_to_int(r[4:])
        r[4:] = int_to_limbs((Q_MOD - y) % Q_MOD)
    return out
