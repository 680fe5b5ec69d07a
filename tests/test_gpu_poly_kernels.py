"""The elementwise and scan kernels of csrc/poly.hip and csrc/scan.hip through their h2_dev_* entry points (and the host-vector
twins on the boundary sizes), on the cases of tests/poly_cases.py: every lane chain, workgroup block, recursion level, launch
slice and positional multiplier at its edge, bit for bit.

References: Python integers at every element up to a few thousand elements and for the prefix scans throughout; from 2^20
elements the C oracle at every element where it has the operation, with Python integers on windows of 40 elements around every
structural position.  Every output lies between two guard elements that have to come back untouched."""
import ctypes

import numpy as np
import pytest

import halo2_gpu_specific_amd as h2
import poly_cases as pc
from h2util import _ptr
from poly_cases import R_MOD

pytestmark = pytest.mark.gpu

POISON = np.uint64(0xA5A5A5A5A5A5A5A5)
FR = 32


def _dev(a):
    """upload (synchronous: the array is in place when this returns, whatever stream reads it next)"""
    import torch

    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()


def _host(t):
    assert h2.lib().h2_synchronize() == 0          # stream NULL = the library's own stream, which torch's does not order
    return t.cpu().numpy().view(np.uint64)


class Guarded:
    """a device buffer of `n` elements (poison, or `init`) between two poisoned guard elements"""

    def __init__(self, n, init=None, width=4):
        a = np.full((n + 2, width), POISON, dtype=np.uint64)
        if init is not None:
            a[1:n + 1] = init
        self.n, self.t = n, _dev(a)
        self.ptr = self.t.data_ptr() + 8 * width

    def read(self):
        a = _host(self.t)
        assert (a[0] == POISON).all() and (a[-1] == POISON).all(), "a guard element was written"
        return a[1:-1]


def _same(got, want_ints, what=""):
    """got: stored-form (n, 4) array; want_ints: canonical values"""
    want = pc.to_mont(want_ints)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not np.array_equal(got, want):
        bad = np.nonzero((got != want).any(axis=1))[0]
        i = int(bad[0])
        raise AssertionError("%s: %d elements differ, the first at %d: got %#x, want %#x"
                             % (what, len(bad), i, pc.from_mont(got[i:i + 1])[0], want_ints[i]))


def _sptr(v):
    a = pc.fr(v)
    return a, a.ctypes.data


# ---------------------------------------------------------------------------------------------- scans
SCAN_CASES = pc.scan_cases()


@pytest.mark.parametrize("case", SCAN_CASES, ids=[c.name for c in SCAN_CASES])
def test_scan(oracle, case):
    L = h2.lib()
    arr, s = case.make()
    want = pc.scan_reference(case, arr, s)
    keep, sp = _sptr(s)
    n = case.L + 1
    d_in, out = _dev(arr), Guarded(len(want))
    fn = {"kate": L.h2_dev_kate_division, "product": L.h2_dev_prefix_product, "sum": L.h2_dev_prefix_sum}[case.mode]
    assert fn(d_in.data_ptr(), n, sp, out.ptr, None) == 0, L.h2_last_error()
    got = out.read()
    _same(got, want, case.name)
    if case.mode == "kate":                         # the oracle too, at every element
        q = np.zeros((case.L, 4), dtype=np.uint64)
        oracle.lib.oracle_kate_division(_ptr(arr), n, _ptr(keep), _ptr(q))
        assert np.array_equal(got, q)
    if case.L > pc.HOST_TWIN_MAX:
        return
    res = np.full((len(want), 4), POISON, dtype=np.uint64)
    twin = {"kate": L.h2_kate_division, "product": L.h2_prefix_product, "sum": L.h2_prefix_sum}[case.mode]
    assert twin(arr.ctypes.data, n, sp, res.ctypes.data) == 0, L.h2_last_error()
    _same(res, want, case.name + " (host twin)")
    if case.mode == "kate":                         # q = a: the dividend is uploaded before the quotient comes back
        both = arr.copy()
        assert L.h2_kate_division(both.ctypes.data, n, sp, both.ctypes.data) == 0
        _same(both[:case.L], want, case.name + " (host twin, q = a)")
        assert np.array_equal(both[case.L], arr[case.L])


def test_scans_refuse_overlapping_device_buffers():
    """the refusals of tests/test_cpu_boundary.py on live buffers, and the calls that pass the check -- the ranges only touch, or
    n < 2 -- with their results.  (No in-place call is made to show what it would compute.)"""
    L = h2.lib()
    n = 2 * pc.SC_BLOCK + 2
    a = pc.rand_limbs(9100, n)
    keep, sp = _sptr(pc.rand_ints(9101, 1)[0])
    b = pc.from_mont(keep.reshape(1, 4))[0]
    buf = np.full((3 * n, 4), POISON, dtype=np.uint64)
    buf[n:2 * n] = a
    t = _dev(buf)
    base = t.data_ptr() + n * FR

    def refused(rc):
        return rc == 1 and b"must not overlap" in L.h2_last_error()

    kate = lambda q, n=n: L.h2_dev_kate_division(base, n, sp, q, None)
    assert refused(kate(base)) and refused(kate(base + FR)) and refused(kate(base - (n - 2) * FR))
    assert refused(kate(base + (n - 1) * FR)) and refused(kate(base, n=2))
    for fn in (L.h2_dev_prefix_product, L.h2_dev_prefix_sum):
        scan = lambda z, n=n: fn(base, n, sp, z, None)
        assert refused(scan(base)) and refused(scan(base + FR)) and refused(scan(base - (n - 1) * FR))
        assert refused(scan(base + (n - 2) * FR)) and refused(scan(base, n=2))
    assert np.array_equal(_host(t), buf)                       # a refusal writes nothing
    # accepted: q directly below a, then directly above it
    av = pc.from_mont(a)
    assert kate(base - (n - 1) * FR) == 0, L.h2_last_error()
    got = _host(t)
    _same(got[1:n], pc.kate_reference(av, b), "q ends where a begins")
    assert (got[0] == POISON).all() and np.array_equal(got[n:2 * n], a)
    assert kate(base + n * FR) == 0, L.h2_last_error()
    got = _host(t)
    _same(got[2 * n:3 * n - 1], pc.kate_reference(av, b), "q begins where a ends")
    assert (got[3 * n - 1] == POISON).all() and np.array_equal(got[n:2 * n], a)
    assert kate(base, n=1) == 0 and kate(base, n=0) == 0 and np.array_equal(_host(t)[n:2 * n], a)
    for fn, ref in ((L.h2_dev_prefix_product, pc.prefix_product_reference), (L.h2_dev_prefix_sum, pc.prefix_sum_reference)):
        t = _dev(buf)
        base = t.data_ptr() + n * FR
        assert fn(base, n, sp, base - n * FR, None) == 0, L.h2_last_error()       # z ends where f begins
        got = _host(t)
        _same(got[:n], ref(av[:n - 1], b), "z ends where f begins")
        assert np.array_equal(got[n:2 * n], a)
        assert fn(base, n, sp, base + (n - 1) * FR, None) == 0, L.h2_last_error()  # z begins at f[n - 1], which is not read
        got = _host(t)
        _same(got[2 * n - 1:3 * n - 1], ref(av[:n - 1], b), "z begins where f's read range ends")
        assert np.array_equal(got[n:2 * n - 1], a[:n - 1]) and (got[3 * n - 1] == POISON).all()
        assert fn(base, 1, sp, base, None) == 0                # n = 1: z[0] = init, f is not read
        assert np.array_equal(_host(t)[n], keep)


# ---------------------------------------------------------------------------------------------- batch inversion
BINV_CASES = pc.binv_cases()


@pytest.mark.parametrize("case", BINV_CASES, ids=[c.name for c in BINV_CASES])
def test_batch_invert(oracle, case):
    import torch

    L = h2.lib()
    n = case.n
    a = case.make()
    buf = Guarded(n, init=a)
    tmp = torch.empty((n, 4), dtype=torch.int64, device="cuda")
    assert L.h2_dev_batch_invert(buf.ptr, tmp.data_ptr(), n, None) == 0, L.h2_last_error()
    got = buf.read()
    want = a.copy()
    oracle.lib.oracle_batch_invert(_ptr(want), n)
    assert np.array_equal(got, want), int(np.nonzero((got != want).any(axis=1))[0][0])
    spans = [(0, n)] if n <= pc.BINV_PYTHON_MAX else pc.windows(n, pc.binv_window_positions(n, case.pattern))
    for lo, hi in spans:
        _same(got[lo:hi], pc.batch_invert_reference(pc.from_mont(a[lo:hi])), "%s [%d, %d)" % (case.name, lo, hi))
    if n <= pc.HOST_TWIN_MAX:
        twin = a.copy()
        assert L.h2_batch_invert(twin.ctypes.data, n) == 0, L.h2_last_error()
        assert np.array_equal(twin, want)


# ---------------------------------------------------------------------------------------------- Horner
def _run_batch(fn, batch, pointers, extra=()):
    count = len(batch.slots)
    ptrs = (ctypes.c_void_p * count)(*[pointers[s] for s in batch.slots])
    pts = pc.to_mont(batch.points)
    out = np.full((count, 4), POISON, dtype=np.uint64)
    assert fn(ptrs, count, batch.n, pts.ctypes.data, out.ctypes.data, *extra) == 0, h2.lib().h2_last_error()
    _same(out, [pc.horner(batch.polys[s], x) for s, x in zip(batch.slots, batch.points)], batch.name)


@pytest.mark.parametrize("batch", pc.horner_batches(), ids=lambda b: b.name)
def test_eval_polynomial_batch_slices_and_blocks(batch):
    """32769 evaluations are two launches per level (the second of one evaluation, reading its table row at an offset); two
    Horner blocks and one coefficient at the points 0, 1 and r - 1"""
    d = [_dev(pc.to_mont(p)) for p in batch.polys]
    _run_batch(h2.lib().h2_dev_eval_polynomial_batch, batch, [t.data_ptr() for t in d], (None,))


@pytest.mark.parametrize("batch", pc.horner_twin_batches(), ids=lambda b: b.name)
def test_eval_polynomial_batch_host_twin(batch):
    polys = [pc.to_mont(p) for p in batch.polys]
    _run_batch(h2.lib().h2_eval_polynomial_batch, batch, [p.ctypes.data for p in polys])


# ---------------------------------------------------------------------------------------------- lincomb
@pytest.mark.parametrize("count", pc.LINCOMB_COUNTS)
def test_lincomb_slices(count):
    """0 inputs (the memset), one slice, exactly one and two slices, and one input into the second and the third"""
    L = h2.lib()
    size = pc.LINCOMB_SIZE
    polys, coeffs = pc.lincomb_inputs(count)
    d = [_dev(pc.to_mont(p)) for p in polys]
    ptrs = (ctypes.c_void_p * max(count, 1))(*[t.data_ptr() for t in d])
    cf = pc.to_mont(coeffs)
    res = Guarded(size)
    assert L.h2_dev_lincomb(res.ptr, ptrs if count else None, cf.ctypes.data if count else None, count, size, None) == 0
    want = pc.lincomb_reference(polys, coeffs, size)
    _same(res.read(), want, "count %d" % count)
    if count <= pc.LINCOMB_MAX:
        return
    # the result aliasing a later input is refused before anything is written: here the first input of the second slice
    alias = d[pc.LINCOMB_MAX]
    assert L.h2_dev_lincomb(alias.data_ptr(), ptrs, cf.ctypes.data, count, size, None) == 1
    assert b"may only alias the first input" in L.h2_last_error()
    _same(_host(alias), polys[pc.LINCOMB_MAX], "a refused call wrote its result")
    # in place on input 0, over more than one slice
    assert L.h2_dev_lincomb(d[0].data_ptr(), ptrs, cf.ctypes.data, count, size, None) == 0
    _same(_host(d[0]), want, "in place, count %d" % count)
    for j in range(1, count):
        _same(_host(d[j]), polys[j], "input %d" % j)


# ---------------------------------------------------------------------------------------------- distribute_powers
@pytest.mark.parametrize("n", pc.DP_SIZES)
def test_distribute_powers(oracle, n):
    """a[i] *= g^i: every lane starts from g^(its first index) and steps by g^256; g = 0 keeps a[0] alone"""
    L = h2.lib()
    sz, vp = ctypes.c_size_t, ctypes.c_void_p
    oracle.lib.oracle_distribute_powers.argtypes, oracle.lib.oracle_distribute_powers.restype = [vp, sz, vp], None
    a = pc.rand_limbs(8450 + n, n)
    av = pc.from_mont(a)
    gens = pc.dp_generators()
    for name, g in gens.items():
        if n > (1 << 16) and name in ("one", "rm1"):
            continue            # at the large size: 0, the root of unity and the random generator
        keep, gp = _sptr(g)
        buf = Guarded(n, init=a)
        assert L.h2_dev_distribute_powers(buf.ptr, n, gp, None) == 0, L.h2_last_error()
        got = buf.read()
        _same(got, pc.distribute_powers_reference(av, g), "n %d, g %s" % (n, name))
        want = a.copy()
        oracle.lib.oracle_distribute_powers(_ptr(want), n, _ptr(keep))
        assert np.array_equal(got, want)


# ---------------------------------------------------------------------------------------------- permutation sigma and terms
@pytest.mark.parametrize("n", pc.PERM_SIZES)
def test_permutation_sigma_and_terms(n):
    """sigma = DELTA^c omega^r at the extreme map entries; the terms at the 8192-row block and 256-row lane-group edges, first
    and multiplying call, beta = 0, gamma = 0, and a row each whose numerator / denominator factor is zero"""
    import torch

    L = h2.lib()
    for coeffs in pc.PERM_COEFFS:
        c = pc.perm_case(n, coeffs)
        d_mc = torch.from_numpy(c.map_col.view(np.int32)).cuda()
        d_mr = torch.from_numpy(c.map_row.view(np.int32)).cuda()
        sig = Guarded(n)
        k_delta, p_delta = _sptr(pc.DELTA)
        k_omega, p_omega = _sptr(c.omega)
        assert L.h2_dev_permutation_sigma(sig.ptr, d_mc.data_ptr(), d_mr.data_ptr(), n, p_delta, p_omega, None) == 0
        sigma = pc.sigma_reference(c.map_col, c.map_row, pc.DELTA, c.omega)
        _same(sig.read(), sigma, c.name + " sigma")
        num, den = Guarded(n), Guarded(n)
        k_beta, p_beta = _sptr(c.beta)
        k_gamma, p_gamma = _sptr(c.gamma)
        want_n = want_d = None
        for j in range(2):
            d_v = _dev(pc.to_mont(c.values[j]))
            k_dp, p_dp = _sptr(c.delta_pows[j])
            assert L.h2_dev_permutation_terms(num.ptr, den.ptr, d_v.data_ptr(), sig.ptr, n, p_beta, p_gamma, p_dp, p_omega,
                                              1 if j == 0 else 0, None) == 0, L.h2_last_error()
            want_n, want_d = pc.perm_terms_reference(want_n, want_d, c.values[j], sigma, c.beta, c.gamma, c.delta_pows[j], c.omega, j == 0)
            _same(num.read(), want_n, "%s num after call %d" % (c.name, j))
            _same(den.read(), want_d, "%s den after call %d" % (c.name, j))
        assert want_n[c.num_zero_row] == 0 and want_d[c.den_zero_row] == 0


# ---------------------------------------------------------------------------------------------- eval_op
def _eval_op(op, res, l, r, l_rot, r_rot, size, cv):
    keep, cp = _sptr(cv)
    return h2.lib().h2_dev_eval_op(op, res, l, r, l_rot, r_rot, size, cp, None)


@pytest.mark.parametrize("op", sorted(pc.OPS.values()), ids=sorted(pc.OPS, key=pc.OPS.get))
def test_eval_op_edge_values(op):
    """each of the nine ops on {0, 1, 2, r - 2, r - 1, (r + 1) / 2} x itself, with c from the same set"""
    lv, rv = pc.edge_operands()
    size = len(lv)
    d_l, d_r = _dev(pc.to_mont(lv)), _dev(pc.to_mont(rv))
    for cv in pc.EDGE_VALUES:
        res = Guarded(size)
        rc = _eval_op(op, res.ptr, d_l.data_ptr() if op in pc.OPS_NEED_L else None, d_r.data_ptr() if op in pc.OPS_NEED_R else None,
                      0, 0, size, cv)
        assert rc == 0, h2.lib().h2_last_error()
        _same(res.read(), pc.eval_op_reference(op, lv, rv, 0, 0, size, cv), "op %d, c %#x" % (op, cv))


@pytest.mark.parametrize("size", pc.ROT_SIZES + (1,))
def test_eval_op_rotations_of_a_whole_turn_and_more(size):
    """|rot| >= size, up to the ends of int32: reduced as C's `%` reduces it, then taken modulo size"""
    lv, rv = pc.rand_ints(8900 + size, size), pc.rand_ints(8901 + size, size)
    d_l, d_r = _dev(pc.to_mont(lv)), _dev(pc.to_mont(rv))
    rots = pc.rotations(size)
    for k, rot in enumerate(rots):
        other = rots[(k + 1) % len(rots)]
        for op, c in ((pc.OPS["SUB"], 0), (pc.OPS["LCTHETA"], 3), (pc.OPS["MUL_C"], R_MOD - 2)):
            res = Guarded(size)
            assert _eval_op(op, res.ptr, d_l.data_ptr(), d_r.data_ptr(), rot, other, size, c) == 0, h2.lib().h2_last_error()
            _same(res.read(), pc.eval_op_reference(op, lv, rv, rot, other, size, c), "size %d, rotations %d / %d, op %d" % (size, rot, other, op))


def test_eval_op_in_place_and_the_rotated_alias():
    L = h2.lib()
    size = 257
    lv, rv = pc.rand_ints(8910, size), pc.rand_ints(8911, size)
    lm, rm = pc.to_mont(lv), pc.to_mont(rv)
    for op, c in ((pc.OPS["SUB"], 0), (pc.OPS["MUL"], 0), (pc.OPS["LCBETA"], R_MOD - 1), (pc.OPS["LCTHETA"], 2)):
        d_l, d_r = Guarded(size, init=lm), _dev(rm)                 # in place on l
        assert _eval_op(op, d_l.ptr, d_l.ptr, d_r.data_ptr(), 0, 0, size, c) == 0
        _same(d_l.read(), pc.eval_op_reference(op, lv, rv, 0, 0, size, c), "res = l, op %d" % op)
        d_l, d_r = _dev(lm), Guarded(size, init=rm)                 # on r
        assert _eval_op(op, d_r.ptr, d_l.data_ptr(), d_r.ptr, 0, 0, size, c) == 0
        _same(d_r.read(), pc.eval_op_reference(op, lv, rv, 0, 0, size, c), "res = r, op %d" % op)
        both = Guarded(size, init=lm)                               # on both
        assert _eval_op(op, both.ptr, both.ptr, both.ptr, 0, 0, size, c) == 0
        _same(both.read(), pc.eval_op_reference(op, lv, lv, 0, 0, size, c), "res = l = r, op %d" % op)
    # an un-rotated alias next to a rotated other operand
    d_l, d_r = Guarded(size, init=lm), _dev(rm)
    assert _eval_op(pc.OPS["SUM"], d_l.ptr, d_l.ptr, d_r.data_ptr(), 0, -3, size, 0) == 0
    _same(d_l.read(), pc.eval_op_reference(pc.OPS["SUM"], lv, rv, 0, -3, size, 0), "res = l, r rotated")
    # a rotated alias is refused, and nothing is written
    d_l, d_r = Guarded(size, init=lm), Guarded(size, init=rm)
    for args in ((d_l.ptr, d_l.ptr, d_r.ptr, 1, 0), (d_r.ptr, d_l.ptr, d_r.ptr, 0, -1), (d_l.ptr, d_l.ptr, d_l.ptr, 0, 2)):
        assert _eval_op(pc.OPS["SUM"], *args, size, 0) == 1 and b"rotated operand" in L.h2_last_error()
    assert np.array_equal(d_l.read(), lm) and np.array_equal(d_r.read(), rm)


# ---------------------------------------------------------------------------------------------- divide_by_vanishing, widen, max bits
@pytest.mark.parametrize("size,t_len", pc.vanishing_shapes())
def test_divide_by_vanishing_poly(size, t_len):
    L = h2.lib()
    a, t = pc.rand_limbs(9000 + size, size), pc.rand_limbs(9001 + t_len, t_len)
    av, tv = pc.from_mont(a), pc.from_mont(t)
    buf, d_t = Guarded(size, init=a), _dev(t)
    assert L.h2_dev_divide_by_vanishing_poly(buf.ptr, size, d_t.data_ptr(), t_len, None) == 0, L.h2_last_error()
    _same(buf.read(), [v * tv[i % t_len] % R_MOD for i, v in enumerate(av)], "size %d, t_len %d" % (size, t_len))


def test_divide_by_vanishing_poly_refuses_a_table_that_is_no_power_of_two():
    L = h2.lib()
    a = pc.rand_limbs(9002, 64)
    buf, d_t = Guarded(64, init=a), _dev(pc.rand_limbs(9003, 4))
    for t_len in (0, 3):
        assert L.h2_dev_divide_by_vanishing_poly(buf.ptr, 64, d_t.data_ptr(), t_len, None) == 1
        assert b"power of two" in L.h2_last_error()
    assert np.array_equal(buf.read(), a)


@pytest.mark.parametrize("n", pc.WIDEN_SIZES)
def test_widen_u64(n):
    import torch

    L = h2.lib()
    vals = pc.widen_values(n)
    assert 0 in vals or n < 3
    src = torch.from_numpy(np.array(vals, dtype=np.uint64).view(np.int64)).cuda()
    dst = Guarded(n)
    assert L.h2_dev_widen_u64(src.data_ptr(), n, dst.ptr, None) == 0, L.h2_last_error()
    got = dst.read()
    assert pc.raw_ints(got) == vals


def test_max_scalar_bits_past_the_capped_grid_and_the_sixteenth_column():
    """17 slots over three buffers of 524288 + 257 rows: the grid is capped at 256 workgroups, whose ninth grid-stride pass
    alone sees the one large value of buffer 0; the seventeenth slot takes a second launch; an all-zero column gives 0"""
    L = h2.lib()
    buffers, slots, want = pc.maxbits_case()
    n = pc.MAXBITS_ROWS_N
    cols = [_dev(pc.maxbits_column(b, n)) for b in buffers]
    count = len(slots)
    ptrs = (ctypes.c_void_p * count)(*[cols[s].data_ptr() for s in slots])
    out = (ctypes.c_uint32 * count)(*([0xFFFFFFFF] * count))
    words = _dev(np.full((count, 4), POISON, dtype=np.uint64))          # count * 32 bytes of scratch, not cleared
    assert L.h2_dev_max_scalar_bits(ptrs, count, n, words.data_ptr(), out, None) == 0, L.h2_last_error()
    assert list(out) == want
