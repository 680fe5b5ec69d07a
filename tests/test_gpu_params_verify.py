"""h2_dev_g1_check_points and Params.verify on the device: the screen against a Python-integer predicate on the same limbs,
valid parameters of several sizes, and every way of tampering with an SRS that the check is there to catch."""
import gc
import struct

import numpy as np
import pytest

from h2util import Q_MOD
from test_plonk_host import S_TRAPDOOR

pytestmark = pytest.mark.gpu

MONT_INV_Q = pow(1 << 256, -1, Q_MOD)
ONES = (1 << 64) - 1


@pytest.fixture(scope="module")
def device():
    from halo2_gpu_specific_amd import prover

    D = prover.Device()
    yield D
    gc.collect()


# ---- the screen -------------------------------------------------------------------------------------------------------------
def random_points(D, n, seed):
    from halo2_gpu_specific_amd import prover

    with D.torch.cuda.stream(D.tstream):
        t = D.torch.empty((n, 8), dtype=D.torch.int64, device=D.dev)
    prover.check(D.L.h2_dev_random_points(seed, n, t.data_ptr(), D.stream), "h2_dev_random_points")
    return t


def limbs_int(l):
    return int(l[0]) | int(l[1]) << 64 | int(l[2]) << 128 | int(l[3]) << 192


def predicate(row, forbid):
    """the kind a point fails with, or None -- Python integers on the stored limbs"""
    from halo2_gpu_specific_amd import params_check as pc

    X, Y = limbs_int(row[:4]), limbs_int(row[4:])
    if X >= Q_MOD or Y >= Q_MOD:
        return pc.NONCANONICAL
    if X == 0 and Y == 0:
        return pc.IDENTITY if forbid else None
    x, y = X * MONT_INV_Q % Q_MOD, Y * MONT_INV_Q % Q_MOD
    return None if (y * y - x * x * x - 3) % Q_MOD == 0 else pc.OFF_CURVE


def plant(host, index, how):
    """how = 0: y + 1 (stored limbs), 1: limbs all ones, 2: the identity"""
    if how == 0:
        y = limbs_int(host[index, 4:]) + 1
        host[index, 4:] = np.array([(y >> (64 * j)) & ONES for j in range(4)], dtype=np.uint64)
    elif how == 1:
        host[index] = np.uint64(ONES)
    else:
        host[index] = 0


def run_screen(D, t, table, flags, cap, room=None):
    """one call on a fresh buffer of `room` (>= cap) records filled with a sentinel -> (count, all `room` rows)"""
    from halo2_gpu_specific_amd import prover

    torch = D.torch
    room = cap if room is None else room
    with torch.cuda.stream(D.tstream):
        count = torch.zeros(1, dtype=torch.int64, device=D.dev)
        recs = torch.full((max(room, 1), 4), -1, dtype=torch.int32, device=D.dev)
    prover.check(D.L.h2_dev_g1_check_points(t.data_ptr(), t.shape[0], table, flags, count.data_ptr(), recs.data_ptr(), cap,
                                            D.stream), "h2_dev_g1_check_points")
    with torch.cuda.stream(D.tstream):
        return int(count.cpu()[0]), recs.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 1000])
def test_screen_equals_the_integer_predicate(device, n):
    from halo2_gpu_specific_amd import params_check as pc

    D = device
    clean = D.download(random_points(D, n, 0x5C4EE + n)).reshape(n, 8)
    assert all(predicate(row, True) is None for row in clean)
    assert run_screen(D, D.upload(clean), 0, pc.FORBID_IDENTITY, 8)[0] == 0
    positions = sorted({0, n - 1, 63, 64, 127, 128} & set(range(n)))      # both ends, both sides of wave boundaries
    for shift in range(3):                                                 # every kind at every position
        host = clean.copy()
        for j, index in enumerate(positions):
            plant(host, index, (j + shift) % 3)
        t = D.upload(host)
        for flags in (0, pc.FORBID_IDENTITY):
            want = {(kind, 3, 0, i) for i, row in enumerate(host) for kind in [predicate(row, bool(flags))] if kind is not None}
            count, recs = run_screen(D, t, 3, flags, 16)
            assert count == len(want), (n, shift, flags)
            assert {tuple(int(v) for v in r) for r in recs[:count]} == want, (n, shift, flags)
        kinds = {predicate(host[i], True) for i in positions}
        assert None not in kinds


def test_screen_covers_each_kind():
    """the plants give the three kinds (on a curve point y + 1 leaves the curve)"""
    from halo2_gpu_specific_amd import params_check as pc
    from halo2_gpu_specific_amd.pairing import g1_limbs

    host = np.array([g1_limbs((1, 2))] * 3, dtype=np.uint64)
    for how in range(3):
        plant(host, how, how)
    assert [predicate(r, True) for r in host] == [pc.OFF_CURVE, pc.NONCANONICAL, pc.IDENTITY]
    assert predicate(host[2], False) is None


def test_screen_count_stays_exact_after_the_buffer_fills(device):
    from halo2_gpu_specific_amd import params_check as pc

    D, n = device, 300
    host = D.download(random_points(D, n, 0xCA9)).reshape(n, 8).copy()
    bad = [3, 63, 64, 200, 299]
    for j, index in enumerate(bad):
        plant(host, index, j % 3)
    count, recs = run_screen(D, D.upload(host), 1, pc.FORBID_IDENTITY, cap=2, room=8)
    assert count == 5
    stored = [tuple(int(v) for v in r) for r in recs[:2]]
    assert len(set(stored)) == 2
    for kind, index, sub, row in stored:
        assert (index, sub) == (1, 0) and row in bad and kind == predicate(host[row], True)
    assert (recs[2:] == 0xFFFFFFFF).all()                                  # nothing stored at or past cap
    # cap = 0 counts without a buffer
    from halo2_gpu_specific_amd import prover

    with D.torch.cuda.stream(D.tstream):
        cnt = D.torch.zeros(1, dtype=D.torch.int64, device=D.dev)
    t = D.upload(host)
    prover.check(D.L.h2_dev_g1_check_points(t.data_ptr(), n, 0, pc.FORBID_IDENTITY, cnt.data_ptr(), None, 0, D.stream), "screen")
    with D.torch.cuda.stream(D.tstream):
        assert int(cnt.cpu()[0]) == 5


def test_screen_accumulates_over_tables(device):
    """two calls, one buffer, one download (params_check.screen_points)"""
    from halo2_gpu_specific_amd import params_check as pc

    D = device
    a = D.download(random_points(D, 100, 1)).reshape(100, 8).copy()
    b = D.download(random_points(D, 70, 2)).reshape(70, 8).copy()
    plant(a, 99, 0)
    plant(b, 0, 2)
    plant(b, 64, 1)
    recs, total = pc.screen_points(D, [D.upload(a), D.upload(b)])
    assert total == 3
    assert recs == [(0, 99, pc.OFF_CURVE), (1, 0, pc.IDENTITY), (1, 64, pc.NONCANONICAL)]


def test_screen_past_four_gibibytes(device):
    """point byte offsets above 2^32: the last points of 2^26 + 65"""
    from halo2_gpu_specific_amd import params_check as pc

    D, n = device, (1 << 26) + 65
    t = random_points(D, n, 0xB16)
    bad = [n - 1, n - 2, (1 << 26) - 1, 1 << 26]
    with D.torch.cuda.stream(D.tstream):
        for index in bad:
            t[index] = 0
    count, recs = run_screen(D, t, 0, pc.FORBID_IDENTITY, 8)
    assert count == len(bad)
    assert {tuple(int(v) for v in r) for r in recs[:count]} == {(pc.IDENTITY, 0, 0, i) for i in bad}
    assert run_screen(D, t, 0, 0, 8)[0] == 0
    del t


# ---- a valid SRS ------------------------------------------------------------------------------------------------------------
def assert_accepts(rep):
    assert rep.ok and rep.powers is True and rep.lagrange is True and rep.g0_is_generator is True
    assert rep.points == [] and rep.points_total == 0
    assert rep.first_bad_power is None and rep.first_bad_lagrange is None
    assert {"screen", "msm", "pairing", "total"} <= set(rep.timings)


@pytest.mark.parametrize("k", [1, 6, 8])
def test_valid_srs(device, k):
    from halo2_gpu_specific_amd import prover

    P = prover.Params.unsafe_setup(device, k, S_TRAPDOOR)
    Q = prover.Params(device, k, device.clone(P.g), device.clone(P.g_lagrange), tables=False)
    assert_accepts(Q.verify(device, s_g2=P.s_g2))
    assert_accepts(P.verify(device))                                       # self.s_g2
    assert P.assert_valid(device, seed=3).ok


def test_valid_srs_with_tables(device):
    """k = 15: the shifted scalar columns go through the shifted-base tables of g and g_lagrange"""
    from halo2_gpu_specific_amd import prover

    P = prover.Params.unsafe_setup(device, 15, S_TRAPDOOR)
    assert P.table_bytes > 0
    assert_accepts(P.verify(device))
    del P
    gc.collect()


# ---- tampering at k = 8 ---------------------------------------------------------------------------------------------------------
K = 8
N = 1 << K


@pytest.fixture(scope="module")
def base(device):
    from halo2_gpu_specific_amd import prover

    P = prover.Params.unsafe_setup(device, K, S_TRAPDOOR)
    return device.download(P.g).reshape(N, 8).copy(), device.download(P.g_lagrange).reshape(N, 8).copy(), P.s_g2


def fresh(device, g, gl):
    """parameters of their own from modified copies: never a write into a tensor that has a table"""
    from halo2_gpu_specific_amd import prover

    return prover.Params(device, K, device.upload(g.copy()), device.upload(gl.copy()), tables=False)


def test_off_curve_point_skips_the_structure_checks(device, base):
    from halo2_gpu_specific_amd import params_check as pc

    g, gl, s_g2 = base
    g = g.copy()
    plant(g, 77, 0)
    rep = fresh(device, g, gl).verify(device, s_g2=s_g2)
    assert rep.points == [("g", 77, pc.OFF_CURVE)] and rep.points_total == 1
    assert rep.powers is None and rep.lagrange is None and not rep.ok
    assert rep.first_bad_power is None and rep.first_bad_lagrange is None
    gl2 = gl.copy()
    plant(gl2, 9, 2)
    rep = fresh(device, g, gl2).verify(device, s_g2=s_g2)
    assert rep.points == [("g", 77, pc.OFF_CURVE), ("g_lagrange", 9, pc.IDENTITY)] and rep.points_total == 2
    many = g.copy()
    for i in range(100, 110):
        plant(many, i, 1)
    rep = fresh(device, many, gl).verify(device, s_g2=s_g2, max_failures=4)
    assert rep.points_total == 11 and len(rep.points) == 4 and rep.points == sorted(rep.points)


def test_swapped_powers(device, base):
    g, gl, s_g2 = base
    g = g.copy()
    g[[5, 6]] = g[[6, 5]]
    rep = fresh(device, g, gl).verify(device, s_g2=s_g2)
    assert rep.powers is False and rep.first_bad_power == 4
    assert rep.lagrange is False                                           # the basis no longer matches this g
    assert not rep.ok and rep.points_total == 0
    assert "locate" in rep.timings
    rep = fresh(device, g, gl).verify(device, s_g2=s_g2, locate=False)
    assert rep.powers is False and rep.lagrange is False
    assert rep.first_bad_power is None and rep.first_bad_lagrange is None


def test_swapped_lagrange_entries(device, base):
    g, gl, s_g2 = base
    gl = gl.copy()
    gl[[3, 200]] = gl[[200, 3]]
    rep = fresh(device, g, gl).verify(device, s_g2=s_g2)
    assert rep.powers is True and rep.lagrange is False and rep.first_bad_lagrange == 3
    assert rep.first_bad_power is None and not rep.ok


def test_last_lagrange_entry(device, base):
    """the location's upper end: only entry n - 1 is wrong"""
    g, gl, s_g2 = base
    gl = gl.copy()
    gl[N - 1] = gl[0]
    rep = fresh(device, g, gl).verify(device, s_g2=s_g2)
    assert rep.powers is True and rep.lagrange is False and rep.first_bad_lagrange == N - 1


def test_last_power(device, base):
    """the location's upper end: only g[n - 1] is wrong (term n - 2)"""
    g, gl, s_g2 = base
    g = g.copy()
    g[N - 1] = g[1]
    rep = fresh(device, g, gl).verify(device, s_g2=s_g2)
    assert rep.powers is False and rep.first_bad_power == N - 2


def test_basis_of_another_size(device, base):
    from halo2_gpu_specific_amd import prover

    g, gl, s_g2 = base
    big = prover.Params.unsafe_setup(device, K + 1, S_TRAPDOOR)
    gl9 = device.download(big.g_lagrange).reshape(-1, 8)[:N].copy()
    rep = fresh(device, g, gl9).verify(device, s_g2=s_g2)
    assert rep.powers is True and rep.lagrange is False and not rep.ok


def test_another_s_g2(device, base):
    from halo2_gpu_specific_amd.pairing import g2_compress, g2_mul_generator

    g, gl, _ = base
    wrong = g2_mul_generator(S_TRAPDOOR + 1)
    rep = fresh(device, g, gl).verify(device, s_g2=wrong)
    assert rep.powers is False and rep.first_bad_power == 0 and rep.lagrange is True and not rep.ok
    rep = fresh(device, g, gl).verify(device, s_g2=g2_compress(wrong), locate=False)      # the file's 64 bytes
    assert rep.powers is False and rep.lagrange is True


def test_no_s_g2(device, base):
    g, gl, _ = base
    rep = fresh(device, g, gl).verify(device)
    assert rep.powers is None and rep.lagrange is True and not rep.ok
    assert rep.first_bad_power is None


# ---- other ----------------------------------------------------------------------------------------------------------------------
def without_timings(rep):
    return rep._replace(timings=None)


def test_seeds(device, base):
    g, gl, s_g2 = base
    P = fresh(device, g, gl)
    assert without_timings(P.verify(device, s_g2=s_g2, seed=11)) == without_timings(P.verify(device, s_g2=s_g2, seed=11))
    assert_accepts(P.verify(device, s_g2=s_g2, seed=11))
    assert_accepts(P.verify(device, s_g2=s_g2, seed=12))
    bad = gl.copy()
    bad[[3, 200]] = bad[[200, 3]]
    T = fresh(device, g, bad)
    one, two = T.verify(device, s_g2=s_g2, seed=5), T.verify(device, s_g2=s_g2, seed=5)
    assert without_timings(one) == without_timings(two) and one.first_bad_lagrange == 3


def test_a_device_in_a_process_group_is_refused(device, base):
    from halo2_gpu_specific_amd import prover

    g, gl, s_g2 = base
    P = fresh(device, g, gl)
    D2 = prover.Device(force_collective=True)
    with pytest.raises(ValueError):
        P.verify(D2, s_g2=s_g2)


def test_params_read_verify(device, tmp_path):
    from halo2_gpu_specific_amd import formats, params_check as pc, prover

    P = prover.Params.unsafe_setup(device, K, S_TRAPDOOR)
    path = str(tmp_path / "params.bin")
    formats.params_write(device, P, path, formats.params_additional_data(P))
    Q, extra = formats.params_read(device, path, verify=True, seed=1)
    assert Q.k == K and extra == formats.params_additional_data(P)
    with device.torch.cuda.stream(device.tstream):
        assert device.torch.equal(Q.g, P.g) and device.torch.equal(Q.g_lagrange, P.g_lagrange)
    small, _ = formats.params_read(device, path, k=K - 2, verify=True, seed=1)
    assert small.k == K - 2
    raw = bytearray(open(path, "rb").read())
    at = lambda i: 4 + 32 * N + 32 * i                                      # noqa: E731  entry i of the g_lagrange block
    raw[at(10):at(11)], raw[at(20):at(21)] = raw[at(20):at(21)], raw[at(10):at(11)]
    bad = str(tmp_path / "swapped.bin")
    open(bad, "wb").write(bytes(raw))
    with pytest.raises(pc.ParamsError) as err:
        formats.params_read(device, bad, verify=True, seed=1)
    assert err.value.report.lagrange is False and err.value.report.first_bad_lagrange == 10
    assert err.value.report.powers is True
    formats.params_read(device, bad)                                        # the default reads it as before
    # a file without [s]G2 cannot be verified
    bare = str(tmp_path / "bare.bin")
    formats.params_write(device, P, bare, struct.pack("<I", 7))
    with pytest.raises(pc.ParamsError) as err:
        formats.params_read(device, bare, verify=True)
    assert err.value.report.powers is None and err.value.report.lagrange is True
