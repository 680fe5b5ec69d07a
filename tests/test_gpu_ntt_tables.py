"""The tables an NTT plan builds on demand (csrc/ntt.hip: the divisor-scaled high twiddle tables, the coset scale tables) in
the library's memory accounting, and plan lookup from threads that hold no lock of their own.  Everything at 2^13, the
smallest size with a two-level twiddle table and two passes (5 + 8 bits): the scaled high table, the scale tables and the
inter-pass twiddle path all exist there.  Every output is compared with the oracle's FFT, bit for bit."""
import ctypes
import threading

import numpy as np
import pytest

import halo2_gpu_specific_amd as h2
from halo2_gpu_specific_amd import arithmetic as ar
from h2util import R_MOD, fr_mont

import ntt_matrix_cases as mc

pytestmark = pytest.mark.gpu

LOG_N = 13
N = 1 << LOG_N
SCALE_TABS_MAX = 32  # NttPlan::SCALE_TABS_MAX


def _vp(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def generator(i):
    """distinct coset generators, none a power of w"""
    return (7 + 2 * i) * pow(mc.ROOT_W, 5, R_MOD) % R_MOD


class Expected:
    """one input and its transforms by the oracle; a product with g^i per generator, computed once each"""
    _one = None

    @classmethod
    def get(cls, oracle):
        if cls._one is None:
            cls._one = cls(oracle)
        return cls._one

    def __init__(self, oracle):
        self.o = oracle
        self.ref = mc.Reference(oracle, LOG_N)
        self.w, self.w_inv = fr_mont(self.ref.w), fr_mont(self.ref.w_inv)
        self.x = oracle.random_fr(0x7AB1E5, N)
        self.fwd = oracle.best_fft(self.x.copy(), self.w, LOG_N)
        self.inv_unscaled = oracle.best_fft(self.x.copy(), self.w_inv, LOG_N)
        self._coset = {}
        for a in (self.x, self.fwd, self.inv_unscaled):
            a.setflags(write=False)

    def powers(self, base):
        out = np.empty((N, 4), dtype=np.uint64)  # base^i by doubling: log n elementwise products by a constant
        out[0] = fr_mont(1)
        m = 1
        while m < N:
            out[m : 2 * m] = self.o.eval_op(mc.OP_MUL_C, np.ascontiguousarray(out[:m]), None, 0, 0, fr_mont(pow(base, m, R_MOD)))
            m *= 2
        return out

    def inverse(self, d):
        """fft(x, w^-1) * d"""
        a = self.inv_unscaled.copy()
        self.ref.scale(a, d)
        return a

    def coset_forward(self, g):
        """fft(x[i] g^i, w)"""
        if g not in self._coset:
            self._coset[g] = self.o.best_fft(self.o.eval_op(mc.OP_MUL, self.x, self.powers(g), 0, 0, None), self.w, LOG_N)
        return self._coset[g]

    def coset_inverse(self, g_inv, d):
        """fft(x, w^-1)[i] * g_inv^i * d"""
        a = self.o.eval_op(mc.OP_MUL, self.inv_unscaled, self.powers(g_inv), 0, 0, None)
        self.ref.scale(a, d)
        return a


class Device:
    """one caller's buffers (torch's allocations: none of the library's memory) and the h2_dev_* calls on them"""

    def __init__(self, e):
        import torch

        self.torch, self.e, self.L = torch, e, h2.lib()
        self.dev = torch.device("cuda", 0)
        self.x = torch.from_numpy(e.x.copy().view(np.int64)).to(self.dev)
        self.buf = torch.empty((N, 4), dtype=torch.int64, device=self.dev)
        self.tmp = torch.empty((N, 4), dtype=torch.int64, device=self.dev)

    def _run(self, call):
        self.buf.copy_(self.x)
        self.torch.cuda.synchronize()
        rc = call(self.buf.data_ptr(), self.tmp.data_ptr())
        assert rc == 0, (rc, self.L.h2_last_error())
        assert self.L.h2_synchronize() == 0
        return self.buf.cpu().numpy().view(np.uint64)

    def forward(self):
        return self._run(lambda a, t: self.L.h2_dev_ntt(a, t, _vp(self.e.w), LOG_N, None))

    def inverse(self, d):
        return self._run(lambda a, t: self.L.h2_dev_intt(a, t, _vp(self.e.w_inv), _vp(fr_mont(d)), LOG_N, None))

    def coset_forward(self, g):
        return self._run(lambda a, t: self.L.h2_dev_coset_ntt(a, a, t, LOG_N, _vp(fr_mont(g)), _vp(self.e.w), None))

    def coset_inverse(self, g_inv, d):
        return self._run(lambda a, t: self.L.h2_dev_coset_intt(a, t, LOG_N, _vp(fr_mont(g_inv)), _vp(self.e.w_inv), _vp(fr_mont(d)), None))


def released_base(L, D):
    """the library's bytes with no plan held: after a warm-up transform and h2_release_plans"""
    D.forward()
    assert L.h2_release_plans() == 0
    return L.h2_library_memory_bytes()


def test_every_table_built_on_demand_is_accounted_and_released(oracle):
    """forward, inverse with two divisors (two scaled high tables), coset forward with three generators and coset inverse
    with two (generator, divisor) pairs (five scale tables): the oracle's values, the library's bytes grow by at least the
    tables' sizes, and after h2_release_plans they are back at the base exactly"""
    e = Expected.get(oracle)
    L, D = h2.lib(), Device(e)
    base = released_base(L, D)
    try:
        assert np.array_equal(D.forward(), e.fwd)
        plans_only = L.h2_library_memory_bytes()
        assert plans_only > base
        d1, d2 = e.ref.d, 0x0123456789ABCDEF0123456789ABCDEF0123456789ABCDEF0123456789ABCDEF % R_MOD
        for d in (d1, d2):
            assert np.array_equal(D.inverse(d), e.inverse(d)), "inverse, divisor %x" % d
        for i in range(3):
            assert np.array_equal(D.coset_forward(generator(i)), e.coset_forward(generator(i))), "coset forward %d" % i
        for i, d in ((3, d1), (4, d2)):
            g_inv = pow(generator(i), -1, R_MOD)
            assert np.array_equal(D.coset_inverse(g_inv, d), e.coset_inverse(g_inv, d)), "coset inverse %d" % i
        grown = L.h2_library_memory_bytes()
        # beyond the two plans (w and w^-1): two tables of n / 4096 and five of 4096 + n / 4096 elements
        assert grown - base >= 2 * (plans_only - base) + 32 * (2 * (N >> 12) + 5 * (4096 + (N >> 12)))
    finally:
        assert L.h2_release_plans() == 0
    assert L.h2_library_memory_bytes() == base


def test_scale_table_cap_holds_in_the_accounting(oracle):
    """forty generators through one plan: at most 32 scale tables are kept, so the library's bytes after the 40th equal
    those after the 32nd; the first generator (evicted by then) still transforms to the oracle's values at the same bytes"""
    e = Expected.get(oracle)
    L, D = h2.lib(), Device(e)
    base = released_base(L, D)
    try:
        at = {}
        for i in range(40):
            assert np.array_equal(D.coset_forward(generator(i)), e.coset_forward(generator(i))), "generator %d" % i
            at[i + 1] = L.h2_library_memory_bytes()
        assert at[SCALE_TABS_MAX] - at[1] == (SCALE_TABS_MAX - 1) * 32 * (4096 + (N >> 12))  # (a table each up to the cap)
        assert at[40] == at[SCALE_TABS_MAX]
        assert np.array_equal(D.coset_forward(generator(0)), e.coset_forward(generator(0)))
        assert L.h2_library_memory_bytes() == at[SCALE_TABS_MAX]
    finally:
        assert L.h2_release_plans() == 0
    assert L.h2_library_memory_bytes() == base


def test_plan_lookup_needs_no_lock_of_the_caller(oracle):
    """four threads of h2_dev_* transforms (their own buffers and generator), a fifth of host-slice h2_ntt calls and the
    main thread releasing the plans twice meanwhile: h2_release_plans skips what is in use, every status is 0 and every
    result the oracle's"""
    e = Expected.get(oracle)
    L = h2.lib()
    d = e.ref.d
    want_inv = e.inverse(d)
    want_coset = [e.coset_forward(generator(10 + i)) for i in range(4)]
    devices = [Device(e) for _ in range(4)]
    errors, started = [], [threading.Event() for _ in range(5)]

    def dev_worker(i):
        try:
            D = devices[i]
            for _ in range(3):
                assert np.array_equal(D.forward(), e.fwd), "forward"
                assert np.array_equal(D.inverse(d), want_inv), "inverse"
                assert np.array_equal(D.coset_forward(generator(10 + i)), want_coset[i]), "coset forward"
                started[i].set()
        except Exception as exc:  # noqa: BLE001
            errors.append((i, repr(exc)))
        finally:
            started[i].set()

    def host_worker():
        try:
            for _ in range(3):
                assert np.array_equal(ar.best_fft(e.x.copy(), e.w, LOG_N), e.fwd), "host-slice forward"
                started[4].set()
        except Exception as exc:  # noqa: BLE001
            errors.append(("host", repr(exc)))
        finally:
            started[4].set()

    threads = [threading.Thread(target=dev_worker, args=(i,)) for i in range(4)] + [threading.Thread(target=host_worker)]
    for t in threads:
        t.start()
    started[0].wait()
    rc1 = L.h2_release_plans()
    for ev in started:
        ev.wait()
    rc2 = L.h2_release_plans()
    for t in threads:
        t.join()
    assert not errors, errors
    assert (rc1, rc2) == (0, 0)
    assert L.h2_release_plans() == 0
