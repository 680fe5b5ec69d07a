"""The host pairing of the library (csrc/pairing.cpp behind h2_pairing_check, h2_g2_mul_generator, h2_g2_compress,
h2_g2_decompress) against the big-integer pairing of tests/bn254_pairing.py.  No device is needed or touched."""
import ctypes
import random

import numpy as np
import pytest

import bn254_pairing as bp
import ref_plonk as rp
from h2util import h2i, load_golden

import halo2_gpu_specific_amd as h2
from halo2_gpu_specific_amd import pairing

Q, R = bp.Q, bp.R
H2_ERR_INVALID = 1
_INV = pow(1 << 256, -1, Q)


def mont(v):
    m = (v << 256) % Q
    return [(m >> (64 * i)) & (2**64 - 1) for i in range(4)]


def g2_arr(T):
    if T is None:
        return np.zeros(16, dtype=np.uint64)
    return np.array(mont(T[0][0]) + mont(T[0][1]) + mont(T[1][0]) + mont(T[1][1]), dtype=np.uint64)


def g2_from_arr(a):
    v = [sum(int(a[4 * i + j]) << (64 * j) for j in range(4)) * _INV % Q for i in range(4)]
    return None if not any(v) else ((v[0], v[1]), (v[2], v[3]))


def raw_check(g1_rows, g2_rows):
    """h2_pairing_check on raw limb rows -> (status, ok)"""
    g1 = np.array(g1_rows, dtype=np.uint64).reshape(-1, 8)
    g2 = np.array(g2_rows, dtype=np.uint64).reshape(-1, 16)
    ok = ctypes.c_int(-1)
    rc = h2.lib().h2_pairing_check(g1.ctypes.data, g2.ctypes.data, len(g1), ctypes.byref(ok))
    return rc, ok.value


def check(pairs):
    return pairing.pairing_check([(P, g2_arr(T)) for P, T in pairs])


def test_pairing_check_agrees_with_the_big_integer_pairing_on_random_cases():
    rnd = random.Random(0xB254)
    decisions = []
    for case in range(20):
        a, b, c, d = (rnd.randrange(1, R) for _ in range(4))
        kind = case % 4
        if kind == 0:        # e(aG, bH) e(-abG, H) = 1
            pairs = [(rp.g1_mul(rp.G1, a), bp.g2_mul(bp.G2, b)), (rp.g1_neg(rp.g1_mul(rp.G1, a * b % R)), bp.G2)]
        elif kind == 1:      # a random pair of pairs
            pairs = [(rp.g1_mul(rp.G1, a), bp.g2_mul(bp.G2, b)), (rp.g1_mul(rp.G1, c), bp.g2_mul(bp.G2, d))]
        elif kind == 2:      # three pairs: ab + cd - (ab + cd) = 0
            pairs = [(rp.g1_mul(rp.G1, a), bp.g2_mul(bp.G2, b)), (rp.g1_mul(rp.G1, c), bp.g2_mul(bp.G2, d)),
                     (rp.g1_mul(rp.G1, (a * b + c * d) % R), bp.g2_mul(bp.G2, R - 1))]
        else:                # one pair alone
            pairs = [(rp.g1_mul(rp.G1, a), bp.g2_mul(bp.G2, b))]
        want = bp.pairing_check(pairs)
        assert check(pairs) == want, case
        decisions.append(want)
    assert any(decisions) and not all(decisions)


def test_bilinearity_and_off_by_one():
    rnd = random.Random(7)
    for _ in range(3):
        a, b = rnd.randrange(1, R), rnd.randrange(1, R)
        aP, bQ = rp.g1_mul(rp.G1, a), bp.g2_mul(bp.G2, b)
        assert check([(aP, bQ), (rp.g1_neg(rp.g1_mul(rp.G1, a * b % R)), bp.G2)])
        assert not check([(rp.g1_mul(rp.G1, a + 1), bQ), (rp.g1_neg(rp.g1_mul(rp.G1, a * b % R)), bp.G2)])
        assert not check([(aP, bp.g2_mul(bp.G2, (b + 1) % R)), (rp.g1_neg(rp.g1_mul(rp.G1, a * b % R)), bp.G2)])


def test_identity_on_either_side_contributes_one():
    P, T = rp.g1_mul(rp.G1, 5), bp.g2_mul(bp.G2, 11)
    assert check([]) and check([(None, T)]) and check([(P, None)]) and check([(None, None)])
    assert not check([(P, T)]) and not check([(P, T), (None, T), (P, None)])
    assert check([(P, T), (None, bp.G2), (rp.g1_neg(rp.g1_mul(rp.G1, 55)), bp.G2), (rp.G1, None)])


def test_invalid_points_are_refused_not_crashed_on():
    kat = load_golden("pairing_kat.json")
    L = h2.lib()
    good1, good2 = pairing.g1_limbs(rp.G1), g2_arr(bp.G2)
    assert raw_check([good1], [good2]) == (0, 0)
    # off-curve G1
    assert raw_check([pairing.g1_limbs((1, 3))], [good2])[0] == H2_ERR_INVALID and L.h2_last_error()
    # off-curve G2
    x, y = bp.G2
    bad2 = (x, ((y[0] + 1) % Q, y[1]))
    assert not bp.g2_on_curve(bad2)
    assert raw_check([good1], [g2_arr(bad2)])[0] == H2_ERR_INVALID
    # on the twist, outside the order-r subgroup
    (x0, x1), (y0, y1) = kat["outside_subgroup"]
    out = ((h2i(x0), h2i(x1)), (h2i(y0), h2i(y1)))
    assert bp.g2_on_curve(out) and bp.g2_mul(out, R) is not None
    assert raw_check([good1], [g2_arr(out)])[0] == H2_ERR_INVALID
    with pytest.raises(pairing.PointError):
        pairing.pairing_check([(rp.G1, g2_arr(out))])
    # non-canonical limbs: a coordinate of q or above, in G1 and in G2
    q_limbs = [(Q >> (64 * i)) & (2**64 - 1) for i in range(4)]
    assert raw_check([q_limbs + good1[4:]], [good2])[0] == H2_ERR_INVALID
    assert raw_check([[2**64 - 1] * 4 + good1[4:]], [good2])[0] == H2_ERR_INVALID
    nc = good2.copy()
    nc[12:16] = q_limbs
    assert raw_check([good1], [nc])[0] == H2_ERR_INVALID
    # null arguments
    ok = ctypes.c_int(0)
    assert L.h2_pairing_check(None, None, 1, ctypes.byref(ok)) == H2_ERR_INVALID
    assert L.h2_pairing_check(None, None, 0, None) == H2_ERR_INVALID
    assert L.h2_pairing_check(None, None, 0, ctypes.byref(ok)) == 0 and ok.value == 1


def test_g2_mul_generator():
    rnd = random.Random(3)
    for s in [0, 1, R - 1] + [rnd.randrange(R) for _ in range(4)]:
        assert g2_from_arr(pairing.g2_mul_generator(s)) == bp.g2_mul(bp.G2, s), s
    scalar = np.array([(R >> (64 * i)) & (2**64 - 1) for i in range(4)], dtype=np.uint64)
    out = np.zeros(16, dtype=np.uint64)
    assert h2.lib().h2_g2_mul_generator(scalar.ctypes.data, out.ctypes.data) == H2_ERR_INVALID
    assert h2.lib().h2_g2_mul_generator(None, out.ctypes.data) == H2_ERR_INVALID


def test_g2_compression_round_trips():
    rnd = random.Random(5)
    signs = set()
    for s in [0, 1, 2, R - 1, R - 2] + [rnd.randrange(R) for _ in range(4)]:
        P = pairing.g2_mul_generator(s)
        data = pairing.g2_compress(P)
        assert len(data) == 64
        assert np.array_equal(pairing.g2_decompress(data), P)
        if s:
            signs.add(data[63] >> 7)
            T = bp.g2_mul(bp.G2, s)
            assert data[:32] == T[0][0].to_bytes(32, "little")
            assert bytes(data[32:63]) + bytes([data[63] & 0x7F]) == T[0][1].to_bytes(32, "little")
            neg = pairing.g2_compress(g2_arr((T[0], bp.f2_sub((0, 0), T[1]))))         # -P: the other sign, the same x
            assert neg[:63] == data[:63] and neg[63] ^ data[63] == 0x80
        else:
            assert data == bytes(64)
    assert signs == {0, 1}
    # encodings that are no point
    with pytest.raises(pairing.PointError):
        pairing.g2_decompress(bytes(63) + b"\x80")                     # the identity with a sign
    with pytest.raises(pairing.PointError):
        pairing.g2_decompress(Q.to_bytes(32, "little") + bytes(32))    # x.c0 = q
    with pytest.raises(pairing.PointError):
        pairing.g2_decompress(bytes(32))
    refused = 0
    for i in range(1, 9):                                              # small x: about half have no y, the rest miss the subgroup
        try:
            pairing.g2_decompress(i.to_bytes(32, "little") + bytes(32))
        except pairing.PointError:
            refused += 1
    assert refused == 8
    with pytest.raises(pairing.PointError):                            # compress refuses a point off the curve
        pairing.g2_compress(g2_arr(((1, 2), (3, 4))))


def test_committed_known_answers():
    """tests/golden/pairing_kat.json (gen_pairing_kat.py, from bn254_pairing.py alone): decisions and multiples pinned
    independently of the code under test"""
    kat = load_golden("pairing_kat.json")

    def g1(p):
        return None if p is None else (h2i(p[0]), h2i(p[1]))

    def g2(t):
        return None if t is None else ((h2i(t[0][0]), h2i(t[0][1])), (h2i(t[1][0]), h2i(t[1][1])))

    accepts = []
    for case in kat["cases"]:
        got = check([(g1(p), g2(t)) for p, t in case["pairs"]])
        assert got == case["accept"]
        accepts.append(got)
    assert any(accepts) and not all(accepts)
    for entry in kat["g2_mul"]:
        assert g2_from_arr(pairing.g2_mul_generator(h2i(entry["scalar"]))) == g2(entry["point"])
