"""The two multi-open schemes (poly/multiopen/gwc; shplonk.rs:58-135, shplonk/prover.rs:89-225): the host arithmetic on a handful
of points, which the verifier shares, and the provers over a device that is duck-typed here (any object with Device's methods)."""
from .domain import _inv
from .transcript import R_MOD


def _intermediate_sets(queries):
    """construct_intermediate_sets (poly/multiopen/shplonk.rs:58-135) on (key, rotation, point, eval) tuples:
    BTreeMap / BTreeSet iteration orders become sorted()."""
    rot_point = {}
    for _, rot, point, _ in queries:
        assert rot_point.setdefault(rot, point) == point
    super_point_set = [rot_point[r] for r in sorted(rot_point)]
    order, rotsets = [], {}
    for key, rot, _, _ in queries:
        if key not in rotsets:
            rotsets[key] = set()
            order.append(key)
        rotsets[key].add(rot)
    groups = {}
    for key in order:
        groups.setdefault(tuple(sorted(rotsets[key])), []).append(key)
    evals = {(key, rot): e for key, rot, _, e in queries}
    sets = [{"points": [rot_point[r] for r in rots],
             "commitments": [(key, [evals[(key, r)] for r in rots]) for key in groups[rots]]}
            for rots in sorted(groups)]
    return sets, super_point_set


def _lagrange_interpolate(points, evals):
    """arithmetic.rs:849-903 on host integers (at most a handful of points)"""
    n = len(points)
    out = [0] * n
    for j in range(n):
        num, den = [1], 1
        for m in range(n):
            if m != j:
                num = [((num[i - 1] if i else 0) - points[m] * (num[i] if i < len(num) else 0)) % R_MOD
                       for i in range(len(num) + 1)]
                den = den * (points[j] - points[m]) % R_MOD
        c = evals[j] * _inv(den) % R_MOD
        for i in range(n):
            out[i] = (out[i] + c * num[i]) % R_MOD
    return out


def _horner(coeffs, x):
    acc = 0
    for c in reversed(coeffs):
        acc = (acc * x + c) % R_MOD
    return acc


def _vanishing(roots, z):
    acc = 1
    for r in roots:
        acc = acc * (z - r) % R_MOD
    return acc


def _gwc(D, params, transcript, queries, polys, n):
    """poly/multiopen/gwc/prover.rs:20-175: per opening point, batch = sum_i v^(m-1-i) p_i, witness =
    (batch - batch(z)) / (X - z).  The reference's cuda branch (:57-151) uploads every p_i again for its eval_mul_c /
    eval_sum pair; here they never left the device and one lincomb forms the batch.  One proof over several ranks: every
    vector pass runs on the rank's coefficient range (Device.*_range(s)); the commitments are range-split anyway."""
    v = transcript.squeeze_challenge_scalar()
    quotient_sum = D.quotient_sum if D.row_range(n) == (0, n) else None
    groups = {}
    for qu in queries:
        groups.setdefault(qu[1], []).append(qu)          # BTreeMap<Rotation, Vec<Q>> (gwc.rs:40-49)
    witnesses = []
    for rot in sorted(groups):
        group = groups[rot]
        z, m = group[0][2], len(group)
        vpow = [pow(v, m - 1 - i, R_MOD) for i in range(m)]
        at_z = sum(c * e for c, (_, _, _, e) in zip(vpow, group)) % R_MOD                       # = batch(z)
        if quotient_sum:                   # (host vectors: the fold, the subtraction and the division in one call)
            witnesses.append(quotient_sum(n, [([polys[key] for key, _, _, _ in group], vpow, [at_z], [z])])[0])
            continue
        batch = D.lincomb_range(D.empty(n), [polys[key] for key, _, _, _ in group], vpow, n)
        D.sub_low_range(batch, [at_z], n)
        witnesses.append(D.kate_division_ranges(batch, n, z, D.empty(n)))
    for P in D.msm_batch(witnesses, params.g, n, 254):
        transcript.write_point(P)


def _shplonk(D, params, transcript, queries, polys, n):
    """poly/multiopen/shplonk/prover.rs:89-225.  Every fold `acc * c + p` of the reference is a linear combination
    with powers of the challenge; the device computes each one in a single pass (h2_dev_lincomb) and the host
    adjusts the <= 3 low coefficients the low-degree equivalents r_i(X) touch.  One proof over several ranks: every
    vector pass runs on the rank's coefficient range; a Kate division exchanges one field element per rank."""
    y = transcript.squeeze_challenge_scalar()
    sets, super_points = _intermediate_sets(queries)
    for rs in sets:
        rs["low"] = [_lagrange_interpolate(rs["points"], e) for _, e in rs["commitments"]]
    v = transcript.squeeze_challenge_scalar()
    R = len(sets)
    vpow = [pow(v, R - 1 - r, R_MOD) for r in range(R)]
    # a device whose vectors live on the HOST computes the whole sum in one call (h2_quotient_sum: the combinations, the
    # subtractions and the synthetic divisions stay on the device, h(X) crosses PCIe once)
    quotient_sum = D.quotient_sum if D.row_range(n) == (0, n) else None
    # quotient contribution of every rotation set: (sum_i y^(m-1-i) (p_i - r_i)) / prod (X - point)
    quotients, fused_sets = [], []
    ping, pong = D.empty(n), D.empty(n)
    for r, rs in enumerate(sets):
        m = len(rs["commitments"])
        ypow = [pow(y, m - 1 - i, R_MOD) for i in range(m)]
        width = len(rs["points"])
        low = [sum(ypow[i] * rs["low"][i][j] for i in range(m)) % R_MOD for j in range(width)]
        if quotient_sum:        # v^(R-1-r) goes into the set's coefficients: division is linear, the field elements are the same
            fused_sets.append(([polys[key] for key, _ in rs["commitments"]], [vpow[r] * c % R_MOD for c in ypow],
                               [vpow[r] * c % R_MOD for c in low], rs["points"]))
            continue
        n_x = D.lincomb_range(D.empty(n), [polys[key] for key, _ in rs["commitments"]], ypow, n)
        D.sub_low_range(n_x, low, n)
        cur = n_x
        for pt in rs["points"]:
            nxt = ping if cur is not ping else pong
            D.kate_division_ranges(cur, n, pt, nxt)
            cur = nxt
        quotients.append(D.clone(cur))
    if quotient_sum:
        h_x, _ = quotient_sum(n, fused_sets)
    else:
        h_x = D.lincomb_range(D.empty(n), quotients, vpow, n)
    del quotients
    transcript.write_point(D.msm(h_x, params.g, n))
    u = transcript.squeeze_challenge_scalar()
    zt_eval = _vanishing(super_points, u)
    # linearisation: l(X) = sum_r v^(R-1-r) z_r sum_i y^(m-1-i) (p_i - r_i(u)) - zt(u) h(X), then / (X - u) / z_0
    z_diffs = [_vanishing([p for p in super_points if p not in rs["points"]], u) for rs in sets]
    scale = _inv(z_diffs[0])
    lin_polys, lin_coeffs, const = [], [], 0
    for r, rs in enumerate(sets):
        m = len(rs["commitments"])
        for i, (key, _) in enumerate(rs["commitments"]):
            c = vpow[r] * z_diffs[r] % R_MOD * pow(y, m - 1 - i, R_MOD) % R_MOD * scale % R_MOD
            lin_polys.append(polys[key])
            lin_coeffs.append(c)
            const = (const + c * _horner(rs["low"][i], u)) % R_MOD
    lin_polys.append(h_x)
    lin_coeffs.append((-zt_eval * scale) % R_MOD)
    if quotient_sum:
        pong, rem = quotient_sum(n, [(lin_polys, lin_coeffs, [const], [u])], remainders=True)
        if rem[0] != 0:
            raise AssertionError("shplonk: l(u) != 0")
    else:
        l_x = D.lincomb_range(ping, lin_polys, lin_coeffs, n)
        D.sub_low_range(l_x, [const], n)
        if D.eval_polynomial_ranges([l_x], n, [u])[0] != 0:
            raise AssertionError("shplonk: l(u) != 0")   # the reference's must_be_zero (prover.rs:213-214)
        D.kate_division_ranges(l_x, n, u, pong)
    transcript.write_point(D.msm(pong, params.g, n))
