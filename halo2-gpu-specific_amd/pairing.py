"""G2 and the pairing check of the verifier -- host code of libhalo2_hip.so (csrc/pairing.cpp: h2_pairing_check,
h2_g2_mul_generator, h2_g2_mul, h2_g2_compress, h2_g2_decompress), usable with no device visible.

A G2 point is a numpy array of 16 u64: x.c0, x.c1, y.c0, y.c1 in Montgomery form, identity all zeros (the library's 128-byte
layout).  A G1 point is what the rest of the package uses on the host: (x, y) canonical integers, None for the identity.

The 64-byte G2 encoding (the SRS file's additional_data, ParamsVerifier files) extends the G1 convention of transcript.py to
Fq2: x.c0 then x.c1 little-endian, bit 7 of byte 63 the parity of the canonical y.c0 (of y.c1 when y.c0 is zero), identity =
zeros; "parity unpinned" like the G1 codec."""
import ctypes

import numpy as np

from ._lib import lib
from .transcript import Q_MOD, R_MOD

_M64 = (1 << 64) - 1


class PointError(ValueError):
    """a point the library refused: off the curve, outside the subgroup or not canonical"""


def _fq_mont(v):
    m = (v << 256) % Q_MOD
    return [(m >> (64 * i)) & _M64 for i in range(4)]


def g1_limbs(P):
    """(x, y) / None -> 8 u64 affine Montgomery, identity (0, 0)"""
    return [0] * 8 if P is None else _fq_mont(P[0]) + _fq_mont(P[1])


def g1_neg(P):
    return None if P is None else (P[0], (-P[1]) % Q_MOD)


def g2_mul_generator(s):
    """[s] G2 -- the s_g2 of Params::unsafe_setup (poly/commitment.rs:113-116)"""
    s %= R_MOD
    scalar = np.array([(s >> (64 * i)) & _M64 for i in range(4)], dtype=np.uint64)
    out = np.zeros(16, dtype=np.uint64)
    if lib().h2_g2_mul_generator(scalar.ctypes.data, out.ctypes.data) != 0:
        raise PointError(lib().h2_last_error().decode())
    return out


def g2_mul(point, scalar):
    """[scalar] point for a G2 point of the order-r subgroup -- the G2 side of an SRS update, [s]G2 -> [s tau]G2; PointError
    for a point off the twist or outside the subgroup"""
    point = np.ascontiguousarray(point, dtype=np.uint64).reshape(16)
    scalar %= R_MOD
    limbs = np.array([(scalar >> (64 * i)) & _M64 for i in range(4)], dtype=np.uint64)
    out = np.zeros(16, dtype=np.uint64)
    if lib().h2_g2_mul(point.ctypes.data, limbs.ctypes.data, out.ctypes.data) != 0:
        raise PointError(lib().h2_last_error().decode())
    return out


def g2_generator():
    return g2_mul_generator(1)


def g2_compress(point):
    point = np.ascontiguousarray(point, dtype=np.uint64).reshape(16)
    out = np.zeros(64, dtype=np.uint8)
    if lib().h2_g2_compress(point.ctypes.data, out.ctypes.data) != 0:
        raise PointError(lib().h2_last_error().decode())
    return out.tobytes()


def g2_decompress(data):
    if len(data) != 64:
        raise PointError("a compressed G2 point is 64 bytes, not %d" % len(data))
    raw = np.frombuffer(bytes(data), dtype=np.uint8).copy()
    out = np.zeros(16, dtype=np.uint64)
    if lib().h2_g2_decompress(raw.ctypes.data, out.ctypes.data) != 0:
        raise PointError(lib().h2_last_error().decode())
    return out


def pairing_check(pairs):
    """prod e(P_i, Q_i) == 1 for [(G1 point, G2 point)]; PointError for a point the library refuses"""
    g1 = np.array([g1_limbs(P) for P, _ in pairs], dtype=np.uint64).reshape(-1, 8)
    g2 = np.array([np.asarray(T, dtype=np.uint64).reshape(16) for _, T in pairs], dtype=np.uint64).reshape(-1, 16)
    ok = ctypes.c_int(0)
    if lib().h2_pairing_check(g1.ctypes.data, g2.ctypes.data, len(pairs), ctypes.byref(ok)) != 0:
        raise PointError(lib().h2_last_error().decode())
    return bool(ok.value)
