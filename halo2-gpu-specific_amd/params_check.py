"""Checking parameters: `Params.verify` -- the points and the structure of an SRS, on the device.

The reference has no such step: `Params::read` unwraps `from_bytes` per point (poly/commitment.rs:262-275) and
`Params::verifier` trusts the rest (:297-317).  Here, in this order:

  points    every point of g and g_lagrange is a canonical residue pair on the curve and not the identity
            (h2_dev_g1_check_points, csrc/srscheck.hip).  Points that fail are never handed to an MSM: the structure checks
            are skipped.
  powers    g[i+1] = [s] g[i] for the s of `s_g2` = [s]G2: with n random r_i,  A = sum r_i g[i],  B = sum r_i g[i+1]  (i < n - 1)
            and e(A, [s]G2) = e(B, G2).  sum r_i (g[i+1] - s g[i]) = 0 happens with probability 1/r unless every term is zero.
  lagrange  g_lagrange[i] = n^-1 sum_j w^(-ij) g[j] (the convention of Params.from_powers), relative to g as given: with n
            random e_i and c = iNTT(e), linearity gives <c, g> = <e, iNTT_G1(g)>, so <c, g> and <e, g_lagrange> must be the
            same point.
All four inner products are one pipelined `msm_batch`; the pairing runs on the host (pairing.py).

When a structure check fails and `locate` is set, the same check restricted to a prefix [0, m) of its terms -- the scalars
outside the range zeroed (`structure_scalars`, `mask_range`) -- is bisected for the lowest failing index: at most k + 1
probes, each one MSM batch (and one pairing for the powers)."""
import os
import time
from collections import namedtuple

import numpy as np

from ._lib import check
from .domain import Domain
from .pairing import g1_limbs, g1_neg, g2_decompress, g2_generator, pairing_check
from .rng import ProverRng

NONCANONICAL, IDENTITY, OFF_CURVE = 0, 1, 2           # H2_SRS_* (include/halo2_hip.h): h2_check_record.kind
FORBID_IDENTITY = 1                                   # H2_SRS_FORBID_IDENTITY
KIND_NAMES = {NONCANONICAL: "noncanonical", IDENTITY: "identity", OFF_CURVE: "off-curve"}
TABLES = ("g", "g_lagrange")                          # h2_check_record.index

ParamsReport = namedtuple("ParamsReport", "ok points points_total powers first_bad_power lagrange first_bad_lagrange "
                                          "g0_is_generator timings")


class ParamsError(ValueError):
    """parameters that failed `Params.verify`; `.report` is the ParamsReport"""

    def __init__(self, report):
        self.report = report
        super().__init__(describe(report))


def describe(report):
    """one line per finding"""
    lines = []
    if report.points_total:
        lines.append("%d bad point(s): %s%s" % (
            report.points_total, ", ".join("%s[%d] %s" % (t, i, KIND_NAMES.get(kd, kd)) for t, i, kd in report.points[:8]),
            ", ..." if report.points_total > 8 else ""))
    for name, value, first, what in (("powers", report.powers, report.first_bad_power, "g[%d + 1] != [s] g[%d]"),
                                     ("lagrange", report.lagrange, report.first_bad_lagrange,
                                      "g_lagrange[%d] is not the basis that g implies")):
        if value is None:
            lines.append("%s: not checked%s" % (name, "" if report.points_total or name != "powers" else " (no [s]G2 given)"))
        elif value:
            lines.append("%s: ok" % name)
        else:
            lines.append("%s: FAILED%s" % (name, "" if first is None else
                                           ", first at " + what % ((first, first) if name == "powers" else first)))
    lines.append("g[0] is %sthe generator (1, 2)" % ("" if report.g0_is_generator else "not "))
    return ("parameters ok: " if report.ok else "parameters NOT ok: ") + "; ".join(lines)


# ---- the scalar columns (plain torch ops: device or CPU tensors of (n, 4) limbs) ----------------------------------------
def mask_range(r, lo, hi):
    """r with every row outside [lo, hi) zeroed (a new tensor)"""
    out = r.new_zeros(r.shape)
    out[lo:hi] = r[lo:hi]
    return out


def structure_scalars(r, lo, hi):
    """The two columns of the powers check restricted to the terms lo <= i < hi:  a = (r_0 .. r_{n-2}, 0) masked to the
    range, b = a shifted down by one row -- b[i + 1] = a[i], b[0] = 0.  Both go over the whole of g: <a, g> = sum r_i g[i],
    <b, g> = sum r_i g[i + 1].  The full check is lo = 0, hi = n."""
    n = r.shape[0]
    a = mask_range(r, lo, min(hi, n - 1))
    b = r.new_zeros(r.shape)
    b[1:] = a[:-1]
    return a, b


# ---- the decisions (host) ---------------------------------------------------------------------------------------------------
def powers_decision(A, B, s_g2):
    """e(A, [s]G2) e(-B, G2) == 1 for A = <a, g>, B = <b, g>: host points ((x, y) or None) and the 16-limb [s]G2"""
    return pairing_check([(A, s_g2), (g1_neg(B), g2_generator())])


def lagrange_decision(C1, C2):
    """<iNTT(e), g> and <e, g_lagrange> are the same affine point"""
    return C1 == C2


def parse_s_g2(s_g2):
    """the 16-limb point, or the 64 compressed bytes of an SRS file's additional_data -> 16 u64 limbs"""
    if isinstance(s_g2, (bytes, bytearray, memoryview)):
        return g2_decompress(bytes(s_g2))
    return np.ascontiguousarray(s_g2, dtype=np.uint64).reshape(16)


# ---- the device side ------------------------------------------------------------------------------------------------------
def screen_points(device, tables, flags=FORBID_IDENTITY, max_failures=64):
    """h2_dev_g1_check_points over `tables` (device tensors of (n, 8) limbs; record.index = position in the list) with one
    buffer and one download -> (sorted (table index, point index, kind) records, at most max_failures; the exact count)"""
    D, torch = device, device.torch
    cap = max(int(max_failures), 0)
    with torch.cuda.stream(D.tstream):
        blob = torch.zeros(4 * (cap + 1), dtype=torch.int32, device=D.dev)      # [u64 count, pad][cap x 16 B]
    for index, t in enumerate(tables):
        check(D.L.h2_dev_g1_check_points(t.data_ptr(), t.shape[0], index, flags, blob.data_ptr(), blob.data_ptr() + 16, cap,
                                         D.stream), "h2_dev_g1_check_points")
    with torch.cuda.stream(D.tstream):
        host = blob.cpu().numpy().view(np.uint32)
    total = int(host[0]) | int(host[1]) << 32
    records = host[4:4 + 4 * min(total, cap)].reshape(-1, 4)
    return sorted((int(r[1]), int(r[3]), int(r[0])) for r in records), total


def _random_column(device, key, n):
    t = device.empty(n)
    check(device.L.h2_dev_random_fr(key, n, t.data_ptr(), device.stream), "h2_dev_random_fr")
    return t


def _bisect(n, fails):
    """the lowest index whose term fails, given that the whole range does: the least m with fails(m) on prefixes [0, m)"""
    lo, hi = 0, n                       # [0, lo) passes (the empty sum), [0, hi) fails
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if fails(mid):
            hi = mid
        else:
            lo = mid
    return hi - 1


def verify_params(device, params, s_g2=None, seed=None, locate=True, max_failures=64):
    """`Params.verify` (params.py) -- see there and the module text"""
    D, torch = device, device.torch
    if D.group_size > 1 or D.force_collective:
        raise ValueError("Params.verify: one device is the scope -- not a Device in a process group")
    n, k = params.n, params.k
    timings = {}
    t_last = [time.perf_counter()]

    def phase(name):
        D.sync()
        now = time.perf_counter()
        timings[name] = timings.get(name, 0.0) + (now - t_last[0]) * 1e3
        t_last[0] = now

    # 1. points
    recs, total = screen_points(D, [params.g, params.g_lagrange], FORBID_IDENTITY, max_failures)
    points = [(TABLES[t], i, kind) for t, i, kind in recs]
    with torch.cuda.stream(D.tstream):
        g0 = params.g[0].cpu().numpy().view(np.uint64)
    g0_is_generator = g0.tolist() == g1_limbs((1, 2))
    phase("screen")
    if total:
        timings["total"] = sum(timings.values())
        return ParamsReport(False, points, total, None, None, None, None, g0_is_generator, timings)

    if s_g2 is None:
        s_g2 = getattr(params, "s_g2", None)
    if s_g2 is not None:
        s_g2 = parse_s_g2(s_g2)
    if seed is None:
        key_r, key_e = os.urandom(32), os.urandom(32)
    else:
        rng = ProverRng(seed)
        key_r, key_e = rng.random_poly_key(), rng.random_poly_key()
    dom = Domain(k, 2)
    r = _random_column(D, key_r, n) if s_g2 is not None else None
    e = _random_column(D, key_e, n)

    def products(lo, hi, with_powers, with_lagrange):
        """the inner products of both checks over the terms [lo, hi): (A, B, C1, C2), None where not asked for"""
        cols = []
        with torch.cuda.stream(D.tstream):
            if with_powers:
                cols += list(structure_scalars(r, lo, hi))
            if with_lagrange:
                em = mask_range(e, lo, hi)
                c = em.clone()
        phase("scalars")
        also = None
        if with_lagrange:
            cols.append(D.intt(c, dom))
            also = (em, params.g_lagrange)
            phase("intt")
        out = D.msm_batch(cols, params.g, n, also=also)
        phase("msm")
        A, B = (out[0], out[1]) if with_powers else (None, None)
        C1, C2 = (out[-2], out[-1]) if with_lagrange else (None, None)
        return A, B, C1, C2

    def decide_powers(A, B):
        ok = powers_decision(A, B, s_g2)
        phase("pairing")
        return ok

    # 2. and 3.: one batch of three or four MSMs, one pairing
    A, B, C1, C2 = products(0, n, s_g2 is not None, True)
    powers = decide_powers(A, B) if s_g2 is not None else None
    lagrange = lagrange_decision(C1, C2)

    # 4. location
    first_bad_power = first_bad_lagrange = None
    checked = dict(timings)
    if locate and powers is False:
        first_bad_power = _bisect(n, lambda m: not decide_powers(*products(0, m, True, False)[:2]))
    if locate and not lagrange:
        first_bad_lagrange = _bisect(n, lambda m: not lagrange_decision(*products(0, m, False, True)[2:]))
    located = sum(timings.values()) - sum(checked.values())      # the probes' phases, under one name
    timings.clear()
    timings.update(checked, locate=located)
    timings["total"] = sum(timings.values())
    ok = powers is True and lagrange
    return ParamsReport(ok, points, total, powers, first_bad_power, lagrange, first_bad_lagrange, g0_is_generator, timings)
