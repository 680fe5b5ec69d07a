"""Updating parameters: `Params.update` -- one ceremony contribution on the device -- and the check of one.

An SRS whose trapdoor s nobody should know is g[i] = [s^i] B with [s]G2.  Whoever holds it can make it the SRS of s tau for
a tau of their own: g[i] -> [tau^i] g[i], [s]G2 -> [tau]([s]G2).  From then on the trapdoor s tau is unknown as long as that
one tau is gone, whatever the earlier participants kept.  The reference has no such step: its only constructor of an SRS is
`Params::unsafe_setup`, whose caller knows s (poly/commitment.rs:56-124).

The update (`update_params`):
  1. the column tau^i by h2_dev_prefix_product, as Params.unsafe_setup builds s^i;
  2. h2_dev_g1_mul_each (csrc/g1mul.hip) over a COPY of g -- the old object stays valid, and the library keys the shifted-base
     tables of a base set by its device address;
  3. g_lagrange by Params.from_powers (the G1 NTT);
  4. [s tau]G2 = g2_mul([s]G2, tau) on the host.
The contribution that goes with the new SRS is the 64 compressed bytes of [tau]G2.

The check (`verify_update`) of (old, new, contribution), why it is enough:
  base_kept   new.g[0] == old.g[0] = B: the base point is the same.
  step        e(new.g[1], G2) == e(old.g[1], [tau]G2): with old.g[1] = [s] B this says new.g[1] = [s tau] B for the tau of
              the contribution (decompressed with the subgroup check; the identity or an encoding that does not decompress is
              a False here, not an exception).
  structure   new.verify(): new.g[i + 1] = [s'] new.g[i] for the s' of new.s_g2, and g_lagrange is the basis of new.g.  The
              first term of that chain is new.g[1] = [s'] B, so s' = s tau.
Together: the new SRS is exactly the setup of s tau over the same base point, with its [s tau]G2.  No [tau]G1 and no proof of
knowledge of tau are needed for the use served here -- "my own contribution is the last one I need to trust": the one who
updates knows that their tau was random and is gone, and checks with `verify_update` that the file they publish is the one
their tau made.  A multi-party transcript (who contributed, in which order, each knowing their tau) is out of scope.

tau in Python.  The column tau^i is zeroed on the device before it is released, but `tau` itself is a Python integer:
Python cannot wipe it, and copies of its digits may sit anywhere in the interpreter's heap until the process ends.  Run an
update that matters in a process of its own that does nothing else and exits (tools/params_update.py)."""
import hashlib
import os
import time
from collections import namedtuple

from ._lib import check
from .arithmetic import OP_CONSTANT
from .domain import _fr
from .pairing import PointError, g1_neg, g2_compress, g2_decompress, g2_generator, g2_mul, g2_mul_generator, pairing_check
from .params_check import ParamsError, describe as describe_params, parse_s_g2
from .transcript import Q_MOD, R_MOD

UpdateReport = namedtuple("UpdateReport", "ok base_kept step structure")

NO_S_G2 = "ParamsVerifier: these Params carry no [s]G2; pass the SRS file's additional_data"   # verifier.ParamsVerifier.from_params


def draw_tau():
    """a uniform tau in [1, r): 64 bytes of os.urandom reduced mod r (bias 2^-258), redrawn when 0"""
    while True:
        tau = int.from_bytes(os.urandom(64), "little") % R_MOD
        if tau:
            return tau


def tau_from_seed(seed):
    """a tau in [1, r) that is a function of `seed` alone -- FOR TESTS ONLY: whoever knows the seed knows tau"""
    digest = hashlib.blake2b(b"params_update test seed" + int(seed).to_bytes(16, "little", signed=True), digest_size=64).digest()
    return int.from_bytes(digest, "little") % (R_MOD - 1) + 1


def contribution_of(tau):
    """the 64 compressed bytes of [tau]G2"""
    return g2_compress(g2_mul_generator(tau))


def g1_mul_each(device, points, scalars, out=None):
    """h2_dev_g1_mul_each: out[i] = [scalars[i]] points[i] for (n, 8) affine Montgomery points and (n, 4) Montgomery scalars on
    the device -> `out` (a new tensor when None; `points` itself is allowed)"""
    D, torch = device, device.torch
    n = points.shape[0]
    if out is None:
        with torch.cuda.stream(D.tstream):
            out = torch.empty((n, 8), dtype=torch.int64, device=D.dev)
    check(D.L.h2_dev_g1_mul_each(points.data_ptr(), scalars.data_ptr(), n, out.data_ptr(), D.stream), "h2_dev_g1_mul_each")
    return out


def update_params(device, params, tau=None, tables=None, s_g2=None, timings=None):
    """`Params.update` (params.py) -- see there and the module text.  `timings`: a dict that receives the milliseconds of
    each phase (powers, scale, g1_ntt, g2_mul, total), with a synchronisation between them (tools/params_update.py --bench)."""
    D, L, torch = device, device.L, device.torch
    if D.group_size > 1 or D.force_collective:
        raise ValueError("Params.update: one device is the scope -- not a Device in a process group")
    if params.n < 2:
        raise ValueError("Params.update: n = %d; an SRS of at least 2 points is needed (g[1] carries the trapdoor)" % params.n)
    if s_g2 is None:
        s_g2 = getattr(params, "s_g2", None)
    if s_g2 is None:
        raise ValueError(NO_S_G2)
    s_g2 = parse_s_g2(s_g2)
    if tau is None:
        tau = draw_tau()
    if not 0 < tau < R_MOD:
        raise ValueError("Params.update: tau must be in [1, r)")
    n, k = params.n, params.k
    t_last = [time.perf_counter()]

    def phase(name):
        if timings is not None:
            D.sync()
            now = time.perf_counter()
            timings[name] = (now - t_last[0]) * 1e3
            t_last[0] = now

    if timings is not None:
        D.sync()
        t_last[0] = time.perf_counter()
    t_start = t_last[0]
    constant = D.eval_op(OP_CONSTANT, D.empty(n), c=tau)
    scalars = D.empty(n)
    check(L.h2_dev_prefix_product(constant.data_ptr(), n, _fr(1), scalars.data_ptr(), D.stream), "h2_dev_prefix_product")
    phase("powers")
    g = g1_mul_each(D, params.g, scalars)
    with torch.cuda.stream(D.tstream):
        constant.zero_()
        scalars.zero_()
    phase("scale")
    new = type(params).from_powers(D, k, g, tables)
    phase("g1_ntt")
    new.s_g2 = g2_mul(s_g2, tau)
    contribution = contribution_of(tau)
    phase("g2_mul")
    D.sync()                                     # the zeroing has run before the columns go back to the allocator
    del constant, scalars
    if timings is not None:
        timings["total"] = (time.perf_counter() - t_start) * 1e3
    return new, contribution


# ---- the check -----------------------------------------------------------------------------------------------------------
def _on_curve(P):
    return P is None or (0 <= P[0] < Q_MOD and 0 <= P[1] < Q_MOD and (P[1] * P[1] - P[0] * P[0] * P[0] - 3) % Q_MOD == 0)


def update_decision(old_g0, old_g1, new_g0, new_g1, contribution):
    """(base_kept, step) of `verify_update` on host points ((x, y) canonical integers, None for the identity) and the 64
    bytes of the contribution; no device.  A contribution that is the identity or does not decompress, and a g[1] that is
    the identity or not a curve point, give step = False."""
    base_kept = new_g0 == old_g0
    try:
        tau_g2 = g2_decompress(bytes(contribution))
    except PointError:
        return base_kept, False
    if not tau_g2.any() or old_g1 is None or new_g1 is None or not _on_curve(old_g1) or not _on_curve(new_g1):
        return base_kept, False
    try:
        return base_kept, pairing_check([(new_g1, g2_generator()), (g1_neg(old_g1), tau_g2)])
    except PointError:
        return base_kept, False


def _host_point(device, row):
    """one (8,) device row of affine Montgomery limbs -> (x, y) canonical integers, None for the identity"""
    limbs = device.download(row.reshape(1, 8)).reshape(8)
    r_inv = pow(1 << 256, -1, Q_MOD)
    x, y = (sum(int(limbs[4 * c + i]) << (64 * i) for i in range(4)) * r_inv % Q_MOD for c in range(2))
    return None if not limbs.any() else (x, y)


def verify_update(device, old, new, contribution, **verify_kw):
    """-> UpdateReport(ok, base_kept, step, structure) for the SRS `new` as an update of `old` by the tau of `contribution`
    (the module text says what each field establishes).  `structure` is the ParamsReport of new.verify(device, **verify_kw):
    pass s_g2= for a `new` read from a file, whose [s]G2 is the file's additional_data.  Sizes that differ give base_kept and
    step False."""
    if old.n != new.n or new.n < 2:
        base_kept = step = False
    else:
        base_kept, step = update_decision(_host_point(device, old.g[0]), _host_point(device, old.g[1]),
                                          _host_point(device, new.g[0]), _host_point(device, new.g[1]), contribution)
    structure = new.verify(device, **verify_kw)
    return UpdateReport(bool(base_kept and step and structure.ok), base_kept, step, structure)


def describe(report):
    """one line: the update's two findings, then params_check.describe of the structure"""
    return "%s: base point %s; step e(new.g[1], G2) = e(old.g[1], [tau]G2) %s; %s" % (
        "update ok" if report.ok else "update NOT ok", "kept" if report.base_kept else "CHANGED",
        "holds" if report.step else "FAILED", describe_params(report.structure))


class UpdateError(ParamsError):
    """an update that failed `verify_update`; `.report` is the UpdateReport"""

    def __init__(self, report):
        self.report = report
        ValueError.__init__(self, describe(report))


def assert_valid_update(device, old, new, contribution, **verify_kw):
    """`verify_update`, raising ParamsError (its subclass UpdateError, carrying `.report`) unless the report is ok"""
    report = verify_update(device, old, new, contribution, **verify_kw)
    if not report.ok:
        raise UpdateError(report)
    return report
