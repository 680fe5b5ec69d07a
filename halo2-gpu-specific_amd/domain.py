"""The scalar field's constants and EvaluationDomain's scalars (poly/domain.rs:44-149): what the prover and the host verifier share."""
import ctypes

from .transcript import R_MOD, fr_to_mont_limbs

ROOT_OF_UNITY = 0x03DDB9F5166D18B798865EA93DD31F743215CF6DD39329C8D34F1ED960C37C9C
DELTA = 0x09226B6E22C6F0CA64EC26AAD4C86E715B5F898E5E963F25870E56BBE533E9A2
ZETA = 0x30644E72E131A029048B6E193FD84104CC37A73FEC2BC5E9B8CA0B2D36636F23
S = 28
_vp = ctypes.c_void_p
_FR = ctypes.c_uint64 * 4


def _fr(v):
    """canonical integer -> Montgomery limbs for the C ABI"""
    return _FR(*fr_to_mont_limbs(v % R_MOD))


def _inv(v):
    return pow(v, -1, R_MOD)


class Domain:
    """EvaluationDomain::new (poly/domain.rs:44-149) -- the scalars only"""

    def __init__(self, k, degree):
        self.k, self.n = k, 1 << k
        self.quotient_poly_degree = degree - 1
        ek = k
        while (1 << ek) < self.n * self.quotient_poly_degree:
            ek += 1
        self.extended_k, self.extended_n = ek, 1 << ek
        self.extended_omega = pow(ROOT_OF_UNITY, 1 << (S - ek), R_MOD)
        self.omega = pow(self.extended_omega, 1 << (ek - k), R_MOD)
        self.omega_inv, self.extended_omega_inv = _inv(self.omega), _inv(self.extended_omega)
        self.ifft_divisor, self.extended_ifft_divisor = _inv(self.n), _inv(self.extended_n)
        self.g_coset, self.g_coset_inv = ZETA, ZETA * ZETA % R_MOD
        # t_evaluations: 1 / (ZETA^n * extended_omega^(n*i) - 1), i < 2^(extended_k - k)  (:91-131)
        t_len = 1 << (ek - k)
        zn, wn = pow(ZETA, self.n, R_MOD), pow(self.extended_omega, self.n, R_MOD)
        self.t_evaluations = [_inv((zn * pow(wn, i, R_MOD) - 1) % R_MOD) for i in range(t_len)]

    def rotate_omega(self, x, rot):
        return x * pow(self.omega if rot >= 0 else self.omega_inv, abs(rot), R_MOD) % R_MOD
