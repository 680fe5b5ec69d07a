"""verify_proof -- plonk/verifier.rs:34-507 over the product's own ConstraintSystem / Expression trees (circuit.py).

  ParamsVerifier        poly/commitment.rs:33-40, :296-320 (Params::verifier), :392-433 (write / read: formats.py)
  VerifyingKey          the verifying half of a ProvingKey: cs, domain, fixed / permutation commitments, transcript_repr
  pair_msm              verifier.rs:128-507 up to the `PairMSM` (poly/msm.rs:72-101), gwc/verifier.rs:17-95,
                        shplonk/verifier.rs:23-103 -- pure host code on Python integers
  verify_proof*         instance commitments on the device (verifier.rs:149-163, `commit_lagrange`: the verifier's only O(n)
                        step), pair_msm, `PairMSM::eval` as two device MSMs, the pairing check on the host
                        (multiopen.rs:29-55 `Decider`; csrc/pairing.cpp)
  BatchVerifier         verifier.rs:63-111

A rejected proof is the return value False; what was wrong with it is a typed error (VerifyError and its subclasses,
transcript.TranscriptError, pairing.PointError) that `pair_msm` raises and `verify_proof*` turn into False.
"""
import time

import numpy as np

from . import circuit as hc
from ._lib import check
from .pairing import PointError, g1_limbs, g1_neg, g2_decompress, g2_generator, pairing_check
from .cs_format import vk_digest
from .domain import DELTA, Domain
from .multiopen import _horner, _intermediate_sets, _lagrange_interpolate, _vanishing
from .transcript import (Blake2bRead, R_MOD, TranscriptError, fr_to_mont_limbs, g1_add_affine, point_from_bytes)

G1_GENERATOR = (1, 2)


class VerifyError(ValueError):
    """the proof, its instances or its key cannot be verified (plonk/error.rs)"""


class InvalidInstances(VerifyError):
    """Error::InvalidInstances: not one list of values per instance column (per circuit)"""


class InstanceTooLarge(VerifyError):
    """Error::InstanceTooLarge: more values than usable rows, or than the ParamsVerifier has Lagrange points"""


def _inv(v):
    v %= R_MOD
    if v == 0:
        raise VerifyError("a challenge hit a pole of the verifier's equations")
    return pow(v, -1, R_MOD)


# ---- keys and parameters ------------------------------------------------------------------------------------------------
class VerifyingKey:
    """What verification needs of a key: no polynomial, no device memory."""

    def __init__(self, cs, domain, fixed_commitments, perm_commitments, transcript_repr=None):
        self.cs, self.domain = cs, domain
        self.fixed_commitments, self.perm_commitments = list(fixed_commitments), list(perm_commitments)
        self.transcript_repr = (transcript_repr if transcript_repr is not None else
                                vk_digest(cs, domain, self.fixed_commitments, self.perm_commitments))

    @staticmethod
    def from_proving_key(pk):
        return VerifyingKey(pk.cs, pk.domain, pk.fixed_commitments, pk.perm_commitments, pk.transcript_repr)

    @staticmethod
    def from_info(info):
        """from formats.circuit_data_read(path): the commitments the file carries, no keygen and no device"""
        cs = info["cs"]
        return VerifyingKey(cs, Domain(info["k"], cs.degree()), [point_from_bytes(b) for b in info["fixed_commitments"]],
                            [point_from_bytes(b) for b in info["perm_commitments"]])


def _as_vk(vk):
    return vk if isinstance(vk, VerifyingKey) else VerifyingKey.from_proving_key(vk)


class ParamsVerifier:
    """poly/commitment.rs:33-40: k, the generators, [s]G2 and the first `public_inputs_size` points of g_lagrange (a device
    tensor, or a (size, 8) u64 array that is uploaded when a device first needs it)."""

    def __init__(self, k, s_g2, g_lagrange, public_inputs_size=None, g1=G1_GENERATOR, g2=None):
        self.k, self.n = k, 1 << k
        self.g1 = g1
        self.g2 = np.asarray(g2 if g2 is not None else g2_generator(), dtype=np.uint64).reshape(16)
        self.s_g2 = np.asarray(s_g2, dtype=np.uint64).reshape(16)
        self.g_lagrange = g_lagrange
        self.public_inputs_size = int(g_lagrange.shape[0]) if public_inputs_size is None else public_inputs_size
        if self.public_inputs_size > int(g_lagrange.shape[0]):
            raise ValueError("ParamsVerifier: %d public inputs over %d Lagrange points" % (self.public_inputs_size, g_lagrange.shape[0]))

    @staticmethod
    def from_params(params, additional_data=None, public_inputs_size=None):
        """Params::verifier (commitment.rs:296-320).  additional_data: the compressed [s]G2 that formats.params_read returns
        next to the Params; None takes the s_g2 that Params.unsafe_setup recorded."""
        if additional_data is not None:
            s_g2 = g2_decompress(additional_data)
        elif getattr(params, "s_g2", None) is not None:
            s_g2 = params.s_g2
        else:
            raise ValueError("ParamsVerifier: these Params carry no [s]G2; pass the SRS file's additional_data")
        size = params.n if public_inputs_size is None else public_inputs_size
        if size > params.n:
            raise ValueError("ParamsVerifier: public_inputs_size %d exceeds n = %d" % (size, params.n))
        return ParamsVerifier(params.k, s_g2, params.g_lagrange[:size], size)

    def lagrange_on(self, device):
        if isinstance(self.g_lagrange, np.ndarray):
            self.g_lagrange = device.upload(np.ascontiguousarray(self.g_lagrange, dtype=np.uint64))
        return self.g_lagrange

    def lagrange_host(self):
        """(size, 8) u64 on the host (formats.params_verifier_write)"""
        if isinstance(self.g_lagrange, np.ndarray):
            return self.g_lagrange
        return self.g_lagrange[:self.public_inputs_size].cpu().numpy().view(np.uint64)


# ---- PairMSM (poly/msm.rs) ---------------------------------------------------------------------------------------------
class MSM:
    """poly/msm.rs:13-70: scalar * base terms, merged per base; only the sum matters"""

    def __init__(self):
        self.terms = {}

    def append(self, scalar, base):
        if base is not None:
            self.terms[base] = (self.terms.get(base, 0) + scalar) % R_MOD

    def add_msm(self, other):
        for base, scalar in other.terms.items():
            self.append(scalar, base)

    def scale(self, factor):
        for base in self.terms:
            self.terms[base] = self.terms[base] * factor % R_MOD

    def items(self):
        return [(s, b) for b, s in self.terms.items() if s]

    def __len__(self):
        return len(self.terms)


class PairMSM:
    """poly/msm.rs:72-101: accepted when e(left, [s]G2) == e(right, G2)"""

    def __init__(self):
        self.left, self.right = MSM(), MSM()

    def scale(self, factor):
        self.left.scale(factor)
        self.right.scale(factor)

    def add_msm(self, other):
        self.left.add_msm(other.left)
        self.right.add_msm(other.right)


# ---- expressions at a point -------------------------------------------------------------------------------------------
def _evaluate(e, adv, fix, ins):
    """Expression::evaluate (plonk/circuit.rs:632-700) on the proof's evaluations"""
    stack, out = [(e, False)], []
    while stack:
        node, seen = stack.pop()
        if isinstance(node, hc.Constant):
            out.append(node.v % R_MOD)
        elif isinstance(node, hc.Advice):
            out.append(adv(node.column, node.rotation))
        elif isinstance(node, hc.Fixed):
            out.append(fix(node.column, node.rotation))
        elif isinstance(node, hc.Instance):
            out.append(ins(node.column, node.rotation))
        elif isinstance(node, (hc.Negated, hc.Scaled)):
            if not seen:
                stack += [(node, True), (node.e, False)]
            else:
                v = out.pop()
                out.append((-v if isinstance(node, hc.Negated) else v * node.c) % R_MOD)
        elif isinstance(node, (hc.Sum, hc.Product)):
            if not seen:
                stack += [(node, True), (node.b, False), (node.a, False)]
            else:
                b, a = out.pop(), out.pop()
                out.append((a + b if isinstance(node, hc.Sum) else a * b) % R_MOD)
        elif isinstance(node, hc.SelectorQuery):
            raise hc.SelectorNotCompiled("selector %d was not compiled away: a verifying key holds the constraint system "
                                         "after ConstraintSystem.compress_selectors" % node.selector.index)
        else:
            raise VerifyError("unknown expression node %r" % (node,))
    return out[0]


def _compress(values, theta):
    acc = 0
    for v in values:
        acc = (acc * theta + v) % R_MOD
    return acc


def _prod_and_sum(phi):
    """prod phi_j and sum_i prod_{j != i} phi_j"""
    prod = 1
    for v in phi:
        prod = prod * v % R_MOD
    total = 0
    for i in range(len(phi)):
        term = 1
        for j, v in enumerate(phi):
            if j != i:
                term = term * v % R_MOD
        total = (total + term) % R_MOD
    return prod, total


def _query_index(queries, what):
    table = {q: i for i, q in enumerate(queries)}

    def index(column, rotation):
        try:
            return table[(column, rotation)]
        except KeyError:
            raise VerifyError("the constraint system does not query %s column %d at rotation %d" % (what, column, rotation))

    return index


def _instance_sets(cs, instances, circuits):
    sets = [list(instances)] if circuits is None else [list(i) for i in instances]
    if circuits is not None and circuits != len(sets):
        raise InvalidInstances("%d circuits, %d instance lists" % (circuits, len(sets)))
    if not sets:
        raise InvalidInstances("a proof holds at least one circuit")
    for inst in sets:
        if len(inst) != cs.num_instance:
            raise InvalidInstances("%d instance columns given, the circuit has %d" % (len(inst), cs.num_instance))
    return sets


def pair_msm(vk, proof, instances=(), instance_commitments=None, use_gwc=False, circuits=None):
    """The host half of verification: reads the proof against the key and returns the PairMSM whose pairing equation decides
    it.  instances: the instance columns (lists of integers) of the one circuit, or with `circuits` = N a list of N such
    lists; instance_commitments: their commitments, one list per circuit (`commit_instances`).  Raises TranscriptError /
    VerifyError for a proof that cannot be read."""
    vk = _as_vk(vk)
    cs, dom = vk.cs, vk.domain
    n, bf = dom.n, cs.blinding_factors()
    sets = _instance_sets(cs, instances, circuits)
    ncirc = len(sets)
    for inst in sets:
        for vals in inst:
            if len(vals) > n - (bf + 1):
                raise InstanceTooLarge("%d instance values over %d usable rows" % (len(vals), n - (bf + 1)))
    if instance_commitments is None:
        instance_commitments = [[] for _ in sets]
    if len(instance_commitments) != ncirc or any(len(c) != cs.num_instance for c in instance_commitments):
        raise InvalidInstances("instance commitments do not match the instance columns")
    t = Blake2bRead(proof)
    t.common_scalar(vk.transcript_repr)
    for coms in instance_commitments:
        for P in coms:
            t.common_point(P)
    advice_commitments = [[t.read_point() for _ in range(cs.num_advice)] for _ in range(ncirc)]
    theta = t.squeeze_challenge_scalar()
    m_commitments = [[t.read_point() for _ in cs.lookups] for _ in range(ncirc)]
    beta = t.squeeze_challenge_scalar()
    gamma = t.squeeze_challenge_scalar()
    chunk = cs.degree() - 2
    ncols = len(cs.perm_columns)
    nsets = (ncols + chunk - 1) // chunk
    z_commitments = [[t.read_point() for _ in range(nsets)] for _ in range(ncirc)]
    lk_z_commitments = [[[t.read_point() for _ in sets_] for _, _, sets_ in cs.lookups] for _ in range(ncirc)]
    sh_commitments = [[t.read_point() for _ in cs.shuffles] for _ in range(ncirc)]
    random_commitment = t.read_point()
    y = t.squeeze_challenge_scalar()
    h_commitments = [t.read_point() for _ in range(dom.quotient_poly_degree)]
    x = t.squeeze_challenge_scalar()
    instance_evals = [[t.read_scalar() for _ in cs.instance_queries] for _ in range(ncirc)]
    advice_evals = [[t.read_scalar() for _ in cs.advice_queries] for _ in range(ncirc)]
    fixed_evals = [t.read_scalar() for _ in cs.fixed_queries]
    random_eval = t.read_scalar()
    sigma_evals = [t.read_scalar() for _ in cs.perm_columns]

    def read_set_evals(count):
        out = []
        for i in range(count):
            e = {"cur": t.read_scalar(), "next": t.read_scalar()}
            if i + 1 < count:
                e["last"] = t.read_scalar()
            out.append(e)
        return out

    z_evals = [read_set_evals(nsets) for _ in range(ncirc)]
    lk_evals = []
    for _ in range(ncirc):
        per = []
        for _, _, sets_ in cs.lookups:
            m_eval = t.read_scalar()
            per.append((m_eval, read_set_evals(len(sets_))))
        lk_evals.append(per)
    sh_evals = [[(t.read_scalar(), t.read_scalar()) for _ in cs.shuffles] for _ in range(ncirc)]

    # l_0, l_last, l_blind at x (verifier.rs:262-279; poly/domain.rs l_i_range)
    xn = pow(x, n, R_MOD)
    last_rot = -(bf + 1)
    n_inv = _inv(n)
    l_evals = []
    for rot in range(last_rot, 1):
        w = dom.rotate_omega(1, rot)
        l_evals.append((xn - 1) * w % R_MOD * n_inv % R_MOD * _inv(x - w) % R_MOD)
    l_last, l_blind, l_0 = l_evals[0], sum(l_evals[1:1 + bf]) % R_MOD, l_evals[1 + bf]
    l_active = (1 - (l_last + l_blind)) % R_MOD
    fi, ai, ii = (_query_index(cs.fixed_queries, "fixed"), _query_index(cs.advice_queries, "advice"),
                  _query_index(cs.instance_queries, "instance"))
    fix = lambda c, r: fixed_evals[fi(c, r)]  # noqa: E731

    def triples(evs):
        return [(evs[i]["cur"], evs[i]["next"], evs[i - 1]["last"] if i else None) for i in range(len(evs))]

    # the quotient's value at x from the gates and arguments in the order of evaluation.rs:1017-1219 == verifier.rs:281-383
    expected_h = 0
    for ci in range(ncirc):
        adv = lambda c, r, ci=ci: advice_evals[ci][ai(c, r)]  # noqa: E731
        ins = lambda c, r, ci=ci: instance_evals[ci][ii(c, r)]  # noqa: E731
        getters = {"advice": adv, "fixed": fix, "instance": ins}
        ev = lambda e: _evaluate(e, adv, fix, ins)  # noqa: E731
        exprs = [ev(p) for _, polys in cs.gates for p in polys]
        perm = triples(z_evals[ci])
        if perm:
            perm_vals = [getters[kd](ix, 0) for kd, ix in cs.perm_columns]
            exprs.append(l_0 * (1 - perm[0][0]) % R_MOD)
            exprs.append(l_last * (perm[-1][0] * perm[-1][0] - perm[-1][0]) % R_MOD)
            for i in range(1, len(perm)):
                exprs.append(l_0 * (perm[i][0] - perm[i][2]) % R_MOD)
            for i in range(len(perm)):
                left, right = perm[i][1], perm[i][0]
                cur = beta * x % R_MOD * pow(DELTA, i * chunk, R_MOD) % R_MOD
                for c in range(i * chunk, min((i + 1) * chunk, ncols)):
                    left = left * (perm_vals[c] + beta * sigma_evals[c] + gamma) % R_MOD
                    right = right * (perm_vals[c] + cur + gamma) % R_MOD
                    cur = cur * DELTA % R_MOD
                exprs.append(l_active * (left - right) % R_MOD)
        for (_, table, sets_), (m_eval, evs) in zip(cs.lookups, lk_evals[ci]):   # logup/verifier.rs
            zsets = triples(evs)
            tau = (_compress([ev(e) for e in table], theta) + beta) % R_MOD
            phis = [[(_compress([ev(e) for e in inputs], theta) + beta) % R_MOD for inputs in st] for st in sets_]
            exprs.append(l_0 * zsets[0][0] % R_MOD)
            exprs.append(l_last * zsets[-1][0] % R_MOD)
            prod, total = _prod_and_sum(phis[0])
            exprs.append(l_active * (((zsets[0][1] - zsets[0][0]) * tau + m_eval) * prod - tau * total) % R_MOD)
            for i in range(1, len(zsets)):
                exprs.append(l_0 * (zsets[i][0] - zsets[i][2]) % R_MOD)
            for i in range(1, len(zsets)):
                prod, total = _prod_and_sum(phis[i])
                exprs.append(l_active * ((zsets[i][1] - zsets[i][0]) * prod - total) % R_MOD)
        for group, (z, z_next) in zip(cs.shuffles, sh_evals[ci]):                # shuffle/verifier.rs
            a = b = 1
            for i, (_, inp, shf) in enumerate(group):
                ch = pow(beta, i + 1, R_MOD)
                a = a * (_compress([ev(e) for e in inp], theta) + ch) % R_MOD
                b = b * (_compress([ev(e) for e in shf], theta) + ch) % R_MOD
            exprs.append(l_0 * (1 - z) % R_MOD)
            exprs.append(l_last * (z * z - z) % R_MOD)
            exprs.append(l_active * (z_next * b - z * a) % R_MOD)
        for e in exprs:
            expected_h = (expected_h * y + e) % R_MOD
    expected_h = expected_h * _inv(xn - 1) % R_MOD

    # commitments as MSMs over the proof's points: the h pieces folded by x^n (vanishing/verifier.rs:93-117)
    commitments, queries = {}, []
    h_msm = MSM()
    for i, c in enumerate(h_commitments):
        h_msm.append(pow(xn, i, R_MOD), c)

    def single(P):
        m = MSM()
        m.append(1, P)
        return m

    def q(key, com, rot, ev_):
        commitments[key] = com
        queries.append((key, rot, dom.rotate_omega(x, rot), ev_))

    def open_sets(name, coms, evs):
        for i in range(len(coms)):
            q((name, i), coms[i], 0, evs[i]["cur"])
            q((name, i), coms[i], 1, evs[i]["next"])
        for i in reversed(range(len(coms) - 1)):
            q((name, i), coms[i], last_rot, evs[i]["last"])

    # the queries in the verifier's order (verifier.rs:385-470)
    for ci in range(ncirc):
        for (c, rot), e in zip(cs.instance_queries, instance_evals[ci]):
            q(("instance", ci, c), single(instance_commitments[ci][c]), rot, e)
        for (c, rot), e in zip(cs.advice_queries, advice_evals[ci]):
            q(("advice", ci, c), single(advice_commitments[ci][c]), rot, e)
        open_sets("z%d" % ci, [single(P) for P in z_commitments[ci]], z_evals[ci])
        for li, (m_eval, evs) in enumerate(lk_evals[ci]):
            q(("lookup_m", ci, li), single(m_commitments[ci][li]), 0, m_eval)
            open_sets("lookup_z%d_%d" % (ci, li), [single(P) for P in lk_z_commitments[ci][li]], evs)
        for i, (cur, nxt) in enumerate(sh_evals[ci]):
            q(("shuffle_z", ci, i), single(sh_commitments[ci][i]), 0, cur)
            q(("shuffle_z", ci, i), single(sh_commitments[ci][i]), 1, nxt)
    for (c, rot), e in zip(cs.fixed_queries, fixed_evals):
        q(("fixed", c), single(vk.fixed_commitments[c]), rot, e)
    for i, e in enumerate(sigma_evals):
        q(("sigma", i), single(vk.perm_commitments[i]), 0, e)
    q(("h",), h_msm, 0, expected_h)
    q(("random",), single(random_commitment), 0, random_eval)
    pair = PairMSM()
    if use_gwc:
        _gwc_pair(t, queries, commitments, pair)
    else:
        _shplonk_pair(t, queries, commitments, pair)
    t.expect_end()
    return pair


def _add_scaled(dst, msm, factor):
    for scalar, base in msm.items():
        dst.append(scalar * factor % R_MOD, base)


def _gwc_pair(t, queries, commitments, pair):
    """poly/multiopen/gwc/verifier.rs:17-95: left = sum_i u^i w_i; right = sum_i u^i (z_i w_i + C_i - [e_i] G)"""
    v = t.squeeze_challenge_scalar()
    u = t.squeeze_challenge_scalar()
    groups = {}
    for qu in queries:
        groups.setdefault(qu[1], []).append(qu)          # BTreeMap<Rotation, _> (gwc.rs:36-60)
    eval_multi = 0
    for rot in sorted(groups):
        group = groups[rot]
        z = group[0][2]
        wi = t.read_point()
        pair.scale(u)
        eval_multi = eval_multi * u % R_MOD
        pair.left.append(1, wi)
        pair.right.append(z, wi)
        m = len(group)
        for j, (key, _, _, e) in enumerate(group):
            vp = pow(v, m - 1 - j, R_MOD)
            _add_scaled(pair.right, commitments[key], vp)
            eval_multi = (eval_multi + vp * e) % R_MOD
    pair.right.append(-eval_multi % R_MOD, G1_GENERATOR)


def _shplonk_pair(t, queries, commitments, pair):
    """poly/multiopen/shplonk/verifier.rs:23-103"""
    sets, super_points = _intermediate_sets(queries)
    y = t.squeeze_challenge_scalar()
    v = t.squeeze_challenge_scalar()
    h1 = t.read_point()
    u = t.squeeze_challenge_scalar()
    h2 = t.read_point()
    r_outer, z_0, z_0_diff_inv = 0, None, None
    for i, rs in enumerate(sets):
        z_diff = _vanishing([p for p in super_points if p not in rs["points"]], u)
        if i == 0:
            z_0 = _vanishing(rs["points"], u)
            z_0_diff_inv = _inv(z_diff)
            z_diff = 1
        else:
            z_diff = z_diff * z_0_diff_inv % R_MOD
        pair.right.scale(v)
        r_inner, m = 0, len(rs["commitments"])
        for j, (key, evals) in enumerate(rs["commitments"]):
            r_eval = _horner(_lagrange_interpolate(rs["points"], evals), u)
            r_inner = (y * r_inner + r_eval) % R_MOD
            _add_scaled(pair.right, commitments[key], pow(y, m - 1 - j, R_MOD) * z_diff % R_MOD)
        r_outer = (v * r_outer + r_inner * z_diff) % R_MOD
    pair.right.append(-r_outer % R_MOD, G1_GENERATOR)
    pair.right.append(-z_0 % R_MOD, h1)
    pair.right.append(u, h2)
    pair.left.append(1, h2)


# ---- the evaluation half: the device and the pairing --------------------------------------------------------------------
def _values_array(vals):
    """instance values -> (m, 4) u64 canonical: a list of integers, or such an array as it is"""
    if isinstance(vals, np.ndarray) and vals.ndim == 2:
        return np.ascontiguousarray(vals, dtype=np.uint64)
    raw = b"".join((int(v) % R_MOD).to_bytes(32, "little") for v in vals)
    return np.frombuffer(raw, dtype=np.uint64).reshape(-1, 4).copy()


def commit_instances(device, params, vk, instance_sets):
    """The instance columns' commitments (verifier.rs:149-163, `params.commit_lagrange`) over the ParamsVerifier's Lagrange
    points: columns of one length share one Device.msm_batch.  instance_sets: one list of columns per circuit, for any number
    of proofs' circuits at once.  Returns the matching lists of points."""
    vk = _as_vk(vk)
    usable = vk.domain.n - (vk.cs.blinding_factors() + 1)
    by_len, out = {}, [[None] * len(inst) for inst in instance_sets]
    for si, inst in enumerate(instance_sets):
        for ci, vals in enumerate(inst):
            if len(vals) > usable or len(vals) > params.public_inputs_size:
                raise InstanceTooLarge("%d instance values: %d usable rows, %d Lagrange points" % (
                    len(vals), usable, params.public_inputs_size))
            if len(vals):
                by_len.setdefault(len(vals), []).append((si, ci, vals))
    bases = params.lagrange_on(device) if by_len else None
    for m, items in by_len.items():
        cols = []
        for _, _, vals in items:
            col = device.upload(_values_array(vals))
            check(device.L.h2_dev_batch_mont(col.data_ptr(), m, device.stream), "h2_dev_batch_mont")
            cols.append(col)
        for (si, ci, _), P in zip(items, device.msm_batch(cols, bases, m, 254)):
            out[si][ci] = P
    return out


def msm_eval(device, msm):
    """MSM::eval (poly/msm.rs:52-69) on the device: one windowed MSM over the ad-hoc bases, no table"""
    items = msm.items()
    if not items:
        return None
    scalars = device.upload(np.array([fr_to_mont_limbs(s) for s, _ in items], dtype=np.uint64))
    bases = device.upload(np.array([g1_limbs(b) for _, b in items], dtype=np.uint64))
    return device.msm(scalars, bases, len(items))


def msm_eval_host(msm):
    """the same sum on Python integers (small MSMs, tests, hosts without a device)"""
    acc = None
    for scalar, base in msm.items():
        P, e, term = base, scalar, None
        while e:
            if e & 1:
                term = g1_add_affine(term, P)
            P = g1_add_affine(P, P)
            e >>= 1
        acc = g1_add_affine(acc, term)
    return acc


def decide(params, left, right):
    """the `Decider`: e(left, [s]G2) e(-right, G2) == 1"""
    return pairing_check([(left, params.s_g2), (g1_neg(right), params.g2)])


def decide_host(params, pair):
    """a PairMSM decided without a device: both sums on Python integers, then the pairing check"""
    return decide(params, msm_eval_host(pair.left), msm_eval_host(pair.right))


def _sets_of(vk, instances, circuits):
    return _instance_sets(_as_vk(vk).cs, instances, circuits)


def verify_proof_ext(device, params, vk, proof, instances=(), use_gwc=True, circuits=None, timings=None, report=None):
    """verifier.rs:128-507 (`verify_proof_ext`): True iff the proof is accepted.  params: a ParamsVerifier; vk: a VerifyingKey
    (or a ProvingKey); instances / circuits as `pair_msm`.  timings: a dict that receives the seconds of the four phases;
    report: a dict that receives the reason of a rejection under "error"."""
    marks = [time.perf_counter()]
    try:
        vk = _as_vk(vk)
        if vk.domain.k != params.k:
            raise VerifyError("a key for k = %d under parameters of k = %d" % (vk.domain.k, params.k))
        sets = _sets_of(vk, instances, circuits)
        coms = commit_instances(device, params, vk, sets)
        if any(P is None for c in coms for P in c):
            raise TranscriptError("an instance column commits to the identity")
        marks.append(time.perf_counter())
        pair = pair_msm(vk, proof, sets, coms, use_gwc, circuits=len(sets))
        marks.append(time.perf_counter())
        left, right = msm_eval(device, pair.left), msm_eval(device, pair.right)
        marks.append(time.perf_counter())
        ok = decide(params, left, right)
        marks.append(time.perf_counter())
    except (VerifyError, TranscriptError, PointError) as e:
        if report is not None:
            report["error"] = e
        return False
    if timings is not None:
        for name, a, b in zip(PHASES, marks, marks[1:]):
            timings[name] = timings.get(name, 0.0) + (b - a)
    if not ok and report is not None:
        report["error"] = VerifyError("the opening equation does not hold")
    return ok


PHASES = ("instance commitments", "pair_msm", "msm evaluation", "pairing")


def verify_proof(device, params, vk, proof, instances=(), circuits=None, timings=None, report=None):
    """plonk/verifier.rs `verify_proof`: the GWC multiopen, the counterpart of prover.create_proof"""
    return verify_proof_ext(device, params, vk, proof, instances, True, circuits, timings, report)


def verify_proof_with_shplonk(device, params, vk, proof, instances=(), circuits=None, timings=None, report=None):
    """plonk/verifier.rs `verify_proof_with_shplonk`, the counterpart of prover.create_proof_with_shplonk"""
    return verify_proof_ext(device, params, vk, proof, instances, False, circuits, timings, report)


class BatchVerifier:
    """verifier.rs:63-111: many proofs under one ParamsVerifier, decided by ONE pairing check.  `process` queues a proof;
    `finalize` commits the instance columns of everything queued (Device.msm_batch, columns of one length together), folds
    each proof's PairMSM into the accumulator -- acc = r * acc + pair with a fresh scalar r from `rng` (a rng.ProverRng-style
    source with .fr(); seed it for reproducible tests, leave it on OS entropy otherwise) -- and evaluates the accumulator
    with exactly two device MSMs and one pairing check, however many proofs there are.

    False says that SOME proof failed (or could not be read); to find which, verify the proofs one by one."""

    def __init__(self, device, params, rng):
        self.device, self.params, self.rng = device, params, rng
        self.acc = PairMSM()
        self.queue, self.failed, self.timings = [], None, {}

    def process(self, vk, proof, instances=(), use_gwc=True, circuits=None, params=None):
        """params: the ParamsVerifier of this proof's k when it is not the batch's own (the Lagrange basis depends on k);
        it must come from the same setup, i.e. carry the same [s]G2"""
        params = self.params if params is None else params
        if not (np.array_equal(params.s_g2, self.params.s_g2) and np.array_equal(params.g2, self.params.g2)):
            raise ValueError("BatchVerifier: parameters of another setup")
        self.queue.append((_as_vk(vk), proof, instances, use_gwc, circuits, params))

    def accumulate(self, pair):
        """acc = r * acc + pair (verifier.rs:84-98); returns r"""
        r = self.rng.fr()
        self.acc.scale(r)
        self.acc.add_msm(pair)
        return r

    def finalize(self):
        marks = [time.perf_counter()]
        try:
            sets, spans = [], []
            for vk, _, instances, _, circuits, params in self.queue:
                if vk.domain.k != params.k:
                    raise VerifyError("a key for k = %d under parameters of k = %d" % (vk.domain.k, params.k))
                s = _sets_of(vk, instances, circuits)
                spans.append((len(sets), len(sets) + len(s)))
                sets += s
            # one commit pass per (key, parameters): the columns of every queued proof, grouped by length inside
            coms = [None] * len(sets)
            for vk, params in {(id(e[0]), id(e[5])): (e[0], e[5]) for e in self.queue}.values():
                idx = [i for (lo, hi), e in zip(spans, self.queue) if e[0] is vk and e[5] is params for i in range(lo, hi)]
                for i, c in zip(idx, commit_instances(self.device, params, vk, [sets[i] for i in idx])):
                    coms[i] = c
            if any(P is None for c in coms for P in c):
                raise TranscriptError("an instance column commits to the identity")
            marks.append(time.perf_counter())
            for (lo, hi), (vk, proof, _, use_gwc, _, _) in zip(spans, self.queue):
                self.accumulate(pair_msm(vk, proof, sets[lo:hi], coms[lo:hi], use_gwc, circuits=hi - lo))
            self.queue = []
            marks.append(time.perf_counter())
            left, right = msm_eval(self.device, self.acc.left), msm_eval(self.device, self.acc.right)
            marks.append(time.perf_counter())
            ok = decide(self.params, left, right)
            marks.append(time.perf_counter())
        except (VerifyError, TranscriptError, PointError) as e:
            self.failed = e
            return False
        for name, a, b in zip(PHASES, marks, marks[1:]):
            self.timings[name] = self.timings.get(name, 0.0) + (b - a)
        return ok
