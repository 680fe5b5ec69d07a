"""Params (poly/commitment.rs:23-29): the SRS, both tables resident on the device, with its setup, derivation, check and update."""
import os
import weakref

import numpy as np

from ._lib import check
from .arithmetic import OP_CONSTANT, OP_MUL, OP_MUL_C, OP_SUM_C
from .device import g1_ntt
from .domain import ROOT_OF_UNITY, S, _fr
from .pairing import g2_mul_generator
from .parallel import msm_split_range
from .params_check import ParamsError, verify_params
from .params_update import update_params
from .transcript import Q_MOD, R_MOD


def _forget_tables(L, ptrs):
    for ptr in ptrs:
        L.h2_dev_bases_forget(ptr)


class Params:
    """poly/commitment.rs:23-29: k, n, g, g_lagrange -- both tables resident on the device"""

    def __init__(self, device, k, g, g_lagrange, tables=None):
        self.k, self.n = k, 1 << k
        self.g = g if not isinstance(g, np.ndarray) else device.upload(g)
        self.g_lagrange = g_lagrange if not isinstance(g_lagrange, np.ndarray) else device.upload(g_lagrange)
        assert self.g.shape[0] == self.n and self.g_lagrange.shape[0] == self.n
        self.table_bytes = 0
        if tables is None:
            tables = os.environ.get("H2_MSM_TABLES", "1") != "0"
        if tables:
            self.precompute_tables(device)

    def precompute_tables(self, device, digits=0):
        """Shifted-base tables of both point sets (h2_dev_bases_precompute, include/halo2_hip.h): every commitment of
        every proof made with these parameters adds all digits of a scalar into one bucket set -- 10-35 % off each MSM
        for digits x n x 64 B of HBM per table (12 GiB at k = 24) and ~0.25 s of doublings, once.  Skipped below 2^15
        rows (no gain) and when the tables would take more than half of the free device memory.  The tables live in
        library memory keyed by the tensors' addresses; they are dropped when this object is collected."""
        L = device.L
        # one proof over several ranks: this rank only ever commits its own contiguous range of the bases (the range
        # split of every MSM), so the tables cover that range only -- and their digit count is chosen for its length
        lo, hi = 0, self.n
        if device.group_size > 1:
            lo, hi = msm_split_range(self.n, device.group_size, device.group_rank)
        rows = hi - lo
        if rows < (1 << 15) or self.table_bytes:
            return False
        one = L.h2_dev_bases_precompute_bytes(rows, digits)
        free, _ = device.torch.cuda.mem_get_info(device.dev)
        # what the tables may take: half of the free memory, and under a memory budget (H2_DEVICE_MEM_BUDGET) a third of
        # it.  Each base set is optional on its own: g_lagrange first (the advice / product / multiplicity columns of a
        # wide circuit are committed against it; g only takes the h pieces, the random polynomial and the openings).
        room = free // 2 if device.mem_budget is None else min(free // 2, device.mem_budget // 3)
        which = [self.g_lagrange, self.g][:max(0, min(2, room // one))] if one else []
        if not which:
            return False
        device.sync()
        ptrs = [t.data_ptr() + 64 * lo for t in which]
        for ptr in ptrs:
            check(L.h2_dev_bases_precompute(ptr, rows, digits, device.stream), "h2_dev_bases_precompute")
        self.table_bytes = one * len(ptrs)
        weakref.finalize(self, _forget_tables, L, ptrs).atexit = False   # at interpreter exit the process frees them
        return True

    @staticmethod
    def unsafe_setup(device, k, s):
        """Params::unsafe_setup (poly/commitment.rs:56-124) with the toxic scalar `s` supplied by the caller instead of
        OsRng -- tests and benchmarks only, MUST NOT be used in production (as the reference says).
        g[i] = [s^i] G (:67-83), g_lagrange[i] = [(s^n - 1)/n * w^i / (s - w^i)] G (:85-112), all on the device."""
        D, L = device, device.L
        n = 1 << k
        s %= R_MOD
        omega = pow(ROOT_OF_UNITY, 1 << (S - k), R_MOD)
        # table of [2^j] G, j < 254 (affine; host big integers, 254 doublings)
        pts, P = [], (1, 2)
        for _ in range(254):
            pts.append(P)
            lam = 3 * P[0] * P[0] * pow(2 * P[1], -1, Q_MOD) % Q_MOD
            x3 = (lam * lam - 2 * P[0]) % Q_MOD
            P = (x3, (lam * (P[0] - x3) - P[1]) % Q_MOD)
        mq = lambda v: [((v << 256) % Q_MOD >> (64 * i)) & ((1 << 64) - 1) for i in range(4)]  # noqa: E731
        table = D.upload(np.array([mq(x) + mq(y) for x, y in pts], dtype=np.uint64))

        def powers(base):                       # [base^i]: the running product of a constant column
            f = D.eval_op(OP_CONSTANT, D.empty(n), c=base)
            out = D.empty(n)
            check(L.h2_dev_prefix_product(f.data_ptr(), n, _fr(1), out.data_ptr(), D.stream), "h2_dev_prefix_product")
            return out

        def fixed_base(scalars):
            with D.torch.cuda.stream(D.tstream):
                out = D.torch.empty((n, 8), dtype=D.torch.int64, device=D.dev)
            check(L.h2_dev_fixed_base_mul(scalars.data_ptr(), table.data_ptr(), n, out.data_ptr(), D.stream),
                  "h2_dev_fixed_base_mul")
            return out

        g = fixed_base(powers(s))
        w = powers(omega)
        t = D.eval_op(OP_SUM_C, D.empty(n), w, c=-s)                            # w^i - s
        check(L.h2_dev_batch_invert(t.data_ptr(), D.empty(n).data_ptr(), n, D.stream), "h2_dev_batch_invert")
        D.eval_op(OP_MUL, t, t, w)                                            # w^i / (w^i - s)
        multiplier = (pow(s, n, R_MOD) - 1) * pow(n, -1, R_MOD) % R_MOD
        D.eval_op(OP_MUL_C, t, t, c=-multiplier)                                # multiplier * w^i / (s - w^i)
        g_lagrange = fixed_base(t)
        D.sync()
        params = Params(D, k, g, g_lagrange)
        params.s_g2 = g2_mul_generator(s)       # additional_data of the setup (:113-116): what a ParamsVerifier needs of s
        return params

    @staticmethod
    def from_powers(device, k, g, tables=None):
        """Params from the powers g[i] = [s^i] G alone -- an SRS from a ceremony, or the prefix of a larger one: g_lagrange =
        n^-1 sum_j w^(-ij) g[j] (= [L_i(s)] G) by the G1 NTT on the device (h2_dev_g1_ntt).  g: (2^k, 8) u64 affine Montgomery,
        numpy or a device tensor (kept as it is); the shifted-base tables as the constructor builds them."""
        n = 1 << k
        if isinstance(g, np.ndarray):
            g = device.upload(np.ascontiguousarray(g, dtype=np.uint64))
        if tuple(g.shape) != (n, 8):
            raise ValueError("from_powers: g has shape %s, expected (%d, 8)" % (tuple(g.shape), n))
        g_lagrange = g1_ntt(device, g, k, inverse=True)
        device.sync()
        return Params(device, k, g, g_lagrange, tables)

    def downsize(self, device, k):
        """The parameters of 2^k rows, k <= self.k: g is a COPY of the first 2^k rows of this g (the library keys the
        shifted-base tables of a base set by its device address, so a view would collide with this object's entry) and
        g_lagrange is derived from it (from_powers).  k == self.k returns self."""
        if not 0 <= k <= self.k:
            raise ValueError("downsize: k = %d outside 0..%d" % (k, self.k))
        if k == self.k:
            return self
        with device.torch.cuda.stream(device.tstream):
            g = self.g[: 1 << k].clone()
        return Params.from_powers(device, k, g)

    def verify(self, device, s_g2=None, seed=None, locate=True, max_failures=64):
        """Checks these parameters on the device -> params_check.ParamsReport (the reference has no such step: Params::read
        unwraps `from_bytes` per point, poly/commitment.rs:262-275, and Params::verifier trusts the rest, :297-317).

          points    both tables through h2_dev_g1_check_points, the identity forbidden (s^i is never 0; an identity in
                    g_lagrange means s^n = 1): `points` = sorted (table, index, kind) of the first max_failures, `points_total`
                    the exact count.  Any bad point skips the structure checks (`powers` and `lagrange` None, `ok` False):
                    a point that failed the screen never reaches an MSM.
          powers    g[i + 1] = [s] g[i] against `s_g2` = [s]G2 -- 16 limbs, the 64 compressed bytes of an SRS file's
                    additional_data, or self.s_g2 when None -- by one random linear combination and one pairing.  Without any
                    [s]G2 `powers` is None: not a failure of the SRS, but `ok` is False.
          lagrange  g_lagrange is the basis that g, as given, implies (the convention of from_powers) by one random linear
                    combination; reported even when `powers` is False.
        A false accept has probability 1/r per check.  With `locate`, a failed check is bisected for `first_bad_power` (the
        lowest i with g[i + 1] != [s] g[i]) / `first_bad_lagrange` (the lowest i whose entry differs from the implied basis):
        at most k + 1 probes of one MSM batch each.  `g0_is_generator` (g[0] == (1, 2)) is information only: a ceremony may
        use another base point.  `timings`: milliseconds per phase.  `ok` = no bad point, `powers` True and `lagrange` True.

        The random key is 32 bytes of os.urandom; `seed` gives a deterministic one (rng.py's test-only stream): the same seed
        gives the same report.  A Device in a process group raises ValueError: one device is the scope.

        The check READS THE TENSORS self.g and self.g_lagrange.  The shifted-base tables were built from them at construction:
        a caller who writes into them afterwards has stale tables, and this check does not see that."""
        return verify_params(device, self, s_g2=s_g2, seed=seed, locate=locate, max_failures=max_failures)

    def assert_valid(self, device, **kw):
        """`verify`, raising params_check.ParamsError (a ValueError carrying `.report`) unless the report is ok"""
        report = self.verify(device, **kw)
        if not report.ok:
            raise ParamsError(report)
        return report

    def update(self, device, tau=None, tables=None, s_g2=None):
        """One ceremony contribution -> (new Params, contribution): the SRS of s tau from this SRS of s, without knowing s.
        new.g[i] = [tau^i] g[i] (h2_dev_g1_mul_each over a copy of g: this object stays valid), new.g_lagrange by
        from_powers, new.s_g2 = [tau] s_g2; `contribution` is the 64 compressed bytes of [tau]G2, what
        params_update.verify_update checks the pair (self, new) against.

        tau: an integer in [1, r); None draws 64 bytes of os.urandom, reduced mod r and redrawn when 0; 0 or a value outside
        the range raises ValueError.  Needs n >= 2 and an [s]G2 -- self.s_g2 (Params.unsafe_setup sets it) or `s_g2` in the
        forms `verify` accepts (16 limbs or the 64 bytes of an SRS file's additional_data) -- else ValueError; so does a
        Device in a process group.  `tables`: as the constructor's, for the new object.

        The column tau^i is zeroed on the device before it is released.  tau itself is a Python integer, which CANNOT be
        wiped: its digits may stay in this process's memory until it exits.  Make a contribution that matters in a process of
        its own that does nothing else (tools/params_update.py), and let it end."""
        return update_params(device, self, tau=tau, tables=tables, s_g2=s_g2)

    @staticmethod
    def synthetic(device, k, seed=0x48414C4F32):
        """Timing-only parameters: two tables of valid curve points with no common trapdoor, so proofs made
        with them exercise exactly the same work but cannot verify."""
        n = 1 << k
        tabs = []
        for i in range(2):
            with device.torch.cuda.stream(device.tstream):
                t = device.torch.empty((n, 8), dtype=device.torch.int64, device=device.dev)
            check(device.L.h2_dev_random_points(seed + i, n, t.data_ptr(), device.stream), "h2_dev_random_points")
            tabs.append(t)
        device.sync()
        return Params(device, k, tabs[0], tabs[1])
