"""The host side of Params.update without a GPU: h2_g2_mul / pairing.g2_mul against the big-integer G2 of
tests/bn254_pairing.py, the update's decision (params_update.update_decision) on big-integer points, the argument checks of
h2_dev_g1_mul_each that run before a device is touched, and the header / binding-table agreement with the two new names."""
import random

import numpy as np

import bn254_pairing as bp
import ref_plonk as rp
from h2util import h2i, load_golden
from test_cpu_boundary import declared_symbols
from test_pairing_host import g2_arr, g2_from_arr

import halo2_gpu_specific_amd as h2
from halo2_gpu_specific_amd import pairing
from halo2_gpu_specific_amd._lib import SYMBOLS

R = bp.R
H2_OK, H2_ERR_INVALID = 0, 1


def limbs(v):
    return np.array([(v >> (64 * i)) & (2**64 - 1) for i in range(4)], dtype=np.uint64)


def raw_g2_mul(point, scalar_limbs):
    out = np.full(16, 0xA5, dtype=np.uint64)
    point = np.ascontiguousarray(point, dtype=np.uint64)
    return h2.lib().h2_g2_mul(point.ctypes.data, scalar_limbs.ctypes.data, out.ctypes.data), out


def test_g2_mul_agrees_with_the_big_integer_g2():
    rnd = random.Random(0x62AA)
    for a in [1, 2, R - 1, rnd.randrange(1, R), rnd.randrange(1, R)]:
        T = bp.g2_mul(bp.G2, a)
        for s in [0, 1, R - 1] + [rnd.randrange(R) for _ in range(3)]:
            assert g2_from_arr(pairing.g2_mul(g2_arr(T), s)) == bp.g2_mul(T, s), (a, s)
    # the identity is in the subgroup and stays the identity
    assert not pairing.g2_mul(np.zeros(16, dtype=np.uint64), 5).any()
    assert g2_from_arr(pairing.g2_mul(g2_arr(bp.G2), 0)) is None


def test_g2_mul_composes_with_the_generator_multiplication():
    rnd = random.Random(0x62AB)
    for _ in range(4):
        a, b = rnd.randrange(1, R), rnd.randrange(1, R)
        assert np.array_equal(pairing.g2_mul(pairing.g2_mul_generator(a), b), pairing.g2_mul_generator(a * b % R))
    assert np.array_equal(pairing.g2_mul(pairing.g2_generator(), 7), pairing.g2_mul_generator(7))


def test_g2_mul_refuses_what_it_must():
    import pytest

    good = g2_arr(bp.g2_mul(bp.G2, 9))
    assert raw_g2_mul(good, limbs(3))[0] == H2_OK
    # a scalar of r or above
    assert raw_g2_mul(good, limbs(R))[0] == H2_ERR_INVALID
    assert raw_g2_mul(good, limbs(2**256 - 1))[0] == H2_ERR_INVALID
    # on the twist, outside the order-r subgroup
    (x0, x1), (y0, y1) = load_golden("pairing_kat.json")["outside_subgroup"]
    out = ((h2i(x0), h2i(x1)), (h2i(y0), h2i(y1)))
    assert bp.g2_on_curve(out) and bp.g2_mul(out, R) is not None
    assert raw_g2_mul(g2_arr(out), limbs(3))[0] == H2_ERR_INVALID
    with pytest.raises(pairing.PointError):
        pairing.g2_mul(g2_arr(out), 3)
    # off the twist, and a coordinate that is not a canonical residue
    x, y = bp.G2
    assert raw_g2_mul(g2_arr((x, ((y[0] + 1) % bp.Q, y[1]))), limbs(3))[0] == H2_ERR_INVALID
    nc = good.copy()
    nc[0:4] = limbs(bp.Q)
    assert raw_g2_mul(nc, limbs(3))[0] == H2_ERR_INVALID
    # null arguments
    L = h2.lib()
    buf = np.zeros(16, dtype=np.uint64)
    assert L.h2_g2_mul(None, limbs(3).ctypes.data, buf.ctypes.data) == H2_ERR_INVALID
    assert L.h2_g2_mul(good.ctypes.data, None, buf.ctypes.data) == H2_ERR_INVALID
    assert L.h2_g2_mul(good.ctypes.data, limbs(3).ctypes.data, None) == H2_ERR_INVALID
    # in place
    p = good.copy()
    assert L.h2_g2_mul(p.ctypes.data, limbs(3).ctypes.data, p.ctypes.data) == H2_OK
    assert g2_from_arr(p) == bp.g2_mul(bp.G2, 27)


def test_update_decision_on_big_integer_points():
    from halo2_gpu_specific_amd import params_update as pu

    rnd = random.Random(0x0DEC)
    s, tau, other = (rnd.randrange(2, R) for _ in range(3))
    B = rp.g1_mul(rp.G1, rnd.randrange(2, R))               # a base point other than the generator
    sB, stB = rp.g1_mul(B, s), rp.g1_mul(B, s * tau % R)
    contribution = pu.contribution_of(tau)
    assert len(contribution) == 64 and g2_from_arr(pairing.g2_decompress(contribution)) == bp.g2_mul(bp.G2, tau)
    assert pu.update_decision(B, sB, B, stB, contribution) == (True, True)
    assert pu.update_decision(rp.G1, rp.g1_mul(rp.G1, s), rp.G1, rp.g1_mul(rp.G1, s * tau % R), contribution) == (True, True)
    # a contribution made from another tau
    assert pu.update_decision(B, sB, B, stB, pu.contribution_of(other)) == (True, False)
    # the base point replaced
    assert pu.update_decision(B, sB, rp.g1_mul(B, 2), stB, contribution) == (False, True)
    # g[1] not the product
    assert pu.update_decision(B, sB, B, rp.g1_mul(B, (s * tau + 1) % R), contribution) == (True, False)
    assert pu.update_decision(B, sB, B, sB, contribution) == (True, False)
    # 64 zero bytes (the identity), an encoding that does not decompress, and the identity as g[1]: False, no exception
    assert pu.update_decision(B, sB, B, stB, bytes(64)) == (True, False)
    assert pu.update_decision(B, sB, B, stB, b"\xff" * 64) == (True, False)
    assert pu.update_decision(B, sB, B, stB, contribution[:63]) == (True, False)
    assert pu.update_decision(B, None, B, None, contribution) == (True, False)
    assert pu.update_decision(B, sB, B, (1, 3), contribution) == (True, False)


def test_draw_tau_is_in_range_and_varies():
    from halo2_gpu_specific_amd import params_update as pu

    draws = {pu.draw_tau() for _ in range(8)}
    assert len(draws) == 8 and all(0 < t < R for t in draws)


def test_g1_mul_each_checks_its_arguments_without_a_device():
    L = h2.lib()
    p = 0x1000
    assert L.h2_dev_g1_mul_each(None, None, 0, None, None) == H2_OK
    assert L.h2_dev_g1_mul_each(None, p, 4, p, None) == H2_ERR_INVALID
    assert L.h2_dev_g1_mul_each(p, None, 4, p, None) == H2_ERR_INVALID
    assert L.h2_dev_g1_mul_each(p, p, 4, None, None) == H2_ERR_INVALID
    assert L.h2_dev_g1_mul_each(p, p, (1 << 31) + 1, p, None) == H2_ERR_INVALID
    assert b"h2_dev_g1_mul_each" in L.h2_last_error()


def test_header_binding_table_and_library_agree_on_the_new_names():
    L = h2.lib()
    names = declared_symbols()
    for name in ("h2_dev_g1_mul_each", "h2_g2_mul"):
        assert name in names and name in SYMBOLS and hasattr(L, name)
    assert sorted(SYMBOLS) == names
