"""tests/stream_cases.py is what it claims to be, without a GPU: every adapter's expected output equals the entry point's
definition in Python integers at a reduced size, and two builds of an adapter from different seeds have identical shapes,
table lengths and vector sizes (so that mixing them up on the device can only give wrong values) and different outputs."""
import numpy as np
import pytest

import ref_plonk as rp
import stream_cases as S
from h2util import MONT_R, Q_MOD, R_MOD, arr_to_ints, arr_to_points, from_mont

NAMES = [a.name for a in S.ADAPTERS]
P = R_MOD


def _i(a):
    return from_mont(a)


def _one(a):
    return from_mont(a)[0]


def _pt(xy):
    return None if xy == (0, 0) else xy


def _chacha_block(key, counter):
    """RFC 8439's block function with a 64-bit counter in words 12-13 and a zero nonce -> the 64 keystream bytes"""
    def rotl(v, c):
        return ((v << c) | (v >> (32 - c))) & 0xFFFFFFFF

    init = [0x61707865, 0x3320646E, 0x79622D32, 0x6B206574] + [int.from_bytes(key[4 * j:4 * j + 4], "little") for j in range(8)] + \
           [counter & 0xFFFFFFFF, counter >> 32, 0, 0]
    x = list(init)

    def qr(a, b, c, d):
        x[a] = (x[a] + x[b]) & 0xFFFFFFFF; x[d] = rotl(x[d] ^ x[a], 16)
        x[c] = (x[c] + x[d]) & 0xFFFFFFFF; x[b] = rotl(x[b] ^ x[c], 12)
        x[a] = (x[a] + x[b]) & 0xFFFFFFFF; x[d] = rotl(x[d] ^ x[a], 8)
        x[c] = (x[c] + x[d]) & 0xFFFFFFFF; x[b] = rotl(x[b] ^ x[c], 7)

    for _ in range(10):
        qr(0, 4, 8, 12); qr(1, 5, 9, 13); qr(2, 6, 10, 14); qr(3, 7, 11, 15)
        qr(0, 5, 10, 15); qr(1, 6, 11, 12); qr(2, 7, 8, 13); qr(3, 4, 9, 14)
    return b"".join(((a + b) & 0xFFFFFFFF).to_bytes(4, "little") for a, b in zip(x, init))


# ---- the definitions: case -> (outputs, host results) as Python integers (lists per tensor) ----------------------------------
def _def_kate(c):
    return {"q": rp.kate_division(_i(c.inputs["a"]), _one(c.p["b"]))}, {}


def _def_scan(op):
    def define(c):
        z = [_one(c.p["init"])]
        for v in _i(c.inputs["f"]):
            z.append(op(z[-1], v) % P)
        return {"z": z}, {}
    return define


def _def_evalp(c):
    return {}, {"value": [rp.eval_poly(_i(c.inputs["poly"]), _one(c.p["point"]))]}


def _def_evalpb(c):
    pts = _i(c.p["points"])
    return {}, {"values": [rp.eval_poly(_i(c.inputs["poly%d" % j]), pts[j]) for j in range(S.EVALP_BATCH)]}


def _def_binv(c):
    return {"a": [pow(v, -1, P) if v else 0 for v in _i(c.inputs["a"])]}, {}


def _def_lincomb(c):
    co = _i(c.p["coeffs"])
    polys = [_i(c.inputs["p%d" % j]) for j in range(S.LINCOMB_COUNT)]
    return {"res": [sum(k * p[i] for k, p in zip(co, polys)) % P for i in range(c.dims["size"])]}, {}


def _def_evalop(c):
    l, r, k, n = _i(c.inputs["l"]), _i(c.inputs["r"]), _one(c.p["c"]), c.dims["size"]
    return {"res": [l[(i + 1) % n] * r[(i - 2) % n] % P for i in range(n)], "l": [(l[i] * k + r[i]) % P for i in range(n)]}, {}


def _def_vanish(c):
    """h[i] *= t_evaluations[i mod t_len] (poly/domain.rs:352-371), and t_evaluations are the inverses of X^n - 1 on the coset"""
    a, t = _i(c.inputs["a"]), _i(c.inputs["t"])
    dom = rp.Domain(S.VANISH_K, S.VANISH_J)
    assert c.dims["size"] == dom.extended_n and len(t) == 1 << (dom.extended_k - dom.k)
    assert t == [pow((pow(rp.ZETA * pow(dom.extended_omega, i, P) % P, dom.n, P) - 1) % P, -1, P) for i in range(len(t))]
    return {"a": [a[i] * t[i % len(t)] % P for i in range(len(a))]}, {}


def _def_mont(c):
    return {"a": [v * MONT_R % P for v in arr_to_ints(c.inputs["a"])]}, {}


def _def_unmont(c):
    return {"a": _i(c.inputs["a"])}, {}


def _def_widen(c):
    return {"dst": [int(v) for v in c.inputs["src"]]}, {}


def _def_powers(c):
    g = _one(c.p["g"])
    return {"a": [v * pow(g, i, P) % P for i, v in enumerate(_i(c.inputs["a"]))]}, {}


def _def_sigma(c):
    delta, omega = _one(c.p["delta"]), _one(c.p["omega"])
    assert delta == S.DELTA
    return {"sigma": [pow(delta, int(mc), P) * pow(omega, int(mr), P) % P for mc, mr in zip(c.inputs["map_col"], c.inputs["map_row"])]}, {}


def _def_terms(c):
    beta, gamma, dp, omega = (_one(c.p[k]) for k in ("beta", "gamma", "delta_pow", "omega"))
    num, den, value, sigma = (_i(c.inputs[k]) for k in ("num", "den", "value", "sigma"))
    n = c.dims["n"]
    return {"num": [num[i] * (dp * pow(omega, i, P) * beta + gamma + value[i]) % P for i in range(n)],
            "den": [den[i] * (beta * sigma[i] + gamma + value[i]) % P for i in range(n)]}, {}


def _def_random(c):
    out, m253 = [], (1 << 253) - 1
    for i in range(c.dims["n"]):
        block = _chacha_block(c.p["key"], i)
        out.append(((int.from_bytes(block[:32], "little") & m253) + ((int.from_bytes(block[32:], "little") & m253) << 253)) % P)
    return {"out": out}, {}


def _def_maxbits(c):
    return {}, {"bits": [max(v.bit_length() for v in arr_to_ints(c.inputs["c%d" % j])) for j in range(S.MAX_BITS_COLUMNS)]}


def _def_compress(c):
    return {"bytes": [rp.point_to_bytes(_pt(xy)) for xy in arr_to_points(c.inputs["points"])]}, {}


def _def_decompress(c):
    return {"points": [rp.point_from_bytes(bytes(row)) or (0, 0) for row in c.inputs["bytes"]]}, {}


def _def_msm(c):
    acc = None
    for k, xy in zip(_i(c.inputs["scalars"]), arr_to_points(c.inputs["bases"])):
        acc = rp.g1_add(acc, rp.g1_mul(_pt(xy), k))
    return {}, {"point": [acc or (0, 0)]}


def _def_muleach(c):
    return {"out": [rp.g1_mul(_pt(xy), k) or (0, 0) for k, xy in zip(_i(c.inputs["scalars"]), arr_to_points(c.inputs["points"]))]}, {}


def _def_ntt(c):
    return {"a": rp.fft(_i(c.inputs["a"]), _one(c.p["omega"]))}, {}


def _def_coset(c):
    g = _one(c.p["g"])
    return {"out": rp.fft([v * pow(g, t, P) % P for t, v in enumerate(_i(c.inputs["coeffs"]))], _one(c.p["omega"]))}, {}


def _def_coset_inv(c):
    """the coefficients of the polynomial with the values `a` on g H: the inverse transform, then a[t] * g^-t"""
    g_inv, d = _one(c.p["g_inv"]), _one(c.p["divisor"])
    assert d * (1 << c.dims["k"]) % P == 1
    coeffs = rp.fft(_i(c.inputs["a"]), _one(c.p["omega_inv"]))
    return {"a": [v * d % P * pow(g_inv, t, P) % P for t, v in enumerate(coeffs)]}, {}


def _def_evalh(c):
    from evalh_cases import python_evaluate_h

    return {"values": python_evaluate_h(c.kw)}, {}


def _def_gates(c):
    """the gate polynomials in integers (a stored form is zero exactly when its value is): every listed row, every part"""
    col = {k: arr_to_ints(v) for k, v in c.inputs.items() if k not in ("records", "row_count")}
    n = 1 << c.dims["k"]
    want = []
    for row in range(n):
        if col["values"][row] == 0:
            continue
        part0 = (col["advice0"][row] - col["fixed0"][row]) % P
        parts = (part0, col["advice1"][(row + 1) % n] * col["fixed1"][row] % P, part0 * col["advice2"][row] % P)
        want += [(part, row) for part, v in enumerate(parts) if v]
    return {"records": sorted(want)}, {}


def _def_logup(c):
    """m[r] = the number of usable input rows holding the value of table row r, for the LOWEST r with that value"""
    usable, n = c.dims["usable"], c.dims["n"]
    table = arr_to_ints(c.inputs["table"])
    m = [0] * n
    for j in range(S.LOGUP_INPUTS):
        for v in arr_to_ints(c.inputs["in%d" % j])[:usable]:
            m[table[:usable].index(v)] += 1
    return {"m": m}, {}


def _def_permmap(c):
    d = c.dims
    copies = [((int(a), int(b)), (int(x), int(y))) for a, b, x, y in c.inputs["copies"]]
    mapping = rp.permutation_mapping(d["ncols"], d["n"], copies)
    cells = [mapping[col][row] for col in range(d["ncols"]) for row in range(d["n"])]
    return {"map_col": [t[0] for t in cells], "map_row": [t[1] for t in cells], "status": [0, 0xFFFFFFFF]}, {}


DEFINITIONS = {
    "kate_division": _def_kate, "prefix_product": _def_scan(lambda a, b: a * b), "prefix_sum": _def_scan(lambda a, b: a + b),
    "eval_polynomial": _def_evalp, "eval_polynomial_batch": _def_evalpb, "batch_invert": _def_binv, "lincomb": _def_lincomb,
    "eval_op": _def_evalop, "divide_by_vanishing_poly": _def_vanish, "batch_mont": _def_mont, "batch_unmont": _def_unmont,
    "widen_u64": _def_widen, "distribute_powers": _def_powers, "permutation_sigma": _def_sigma, "permutation_terms": _def_terms,
    "random_fr": _def_random, "max_scalar_bits": _def_maxbits, "points_compress": _def_compress, "points_decompress": _def_decompress,
    "ntt": _def_ntt, "coset_ntt": _def_coset, "coset_intt": _def_coset_inv, "msm": _def_msm, "g1_mul_each": _def_muleach,
    "evaluate_h_generated": _def_evalh, "evaluate_h_interpreter": _def_evalh, "check_gates": _def_gates,
    "logup_multiplicity": _def_logup, "permutation_mapping": _def_permmap,
}
# how an expected tensor reads as the integers of its definition
RAW = {"widen_u64": arr_to_ints, "batch_mont": arr_to_ints, "batch_unmont": arr_to_ints}         # canonical on one side
POINTS = {("points_decompress", "points"), ("g1_mul_each", "out"), ("msm", "point")}


def _read(name, key, array):
    if (name, key) in POINTS:
        return arr_to_points(array)
    if name == "points_compress":
        return [bytes(row) for row in array]
    if name == "check_gates":
        blob = np.asarray(array).view(np.uint32)
        total = int(blob[:2].copy().view(np.uint64)[0])
        recs = blob[4:].reshape(-1, 4)
        assert (recs[:total, 0] == (S.H2_CHECK_GATE | S.CIRCUIT << 8)).all() and (recs[:total, 2] == 0).all()
        assert (recs[total:] == S.SENTINEL).all()
        return sorted((int(r[1]), int(r[3])) for r in recs[:total])
    if name in RAW:
        return RAW[name](array)
    if array.dtype != np.uint64:
        return [int(v) for v in np.asarray(array).reshape(-1)]
    return from_mont(array)


def test_every_entry_point_of_the_issue_has_an_adapter_or_a_reason():
    assert len(NAMES) == len(set(NAMES)) == 29 and set(DEFINITIONS) == set(NAMES)
    for name in ("kate_division", "prefix_product", "prefix_sum", "eval_polynomial", "eval_polynomial_batch", "points_decompress",
                 "evaluate_h_generated", "evaluate_h_interpreter", "check_gates"):
        assert name in S.BY_NAME
    assert {a.name for a in S.ADAPTERS if a.waits} >= {"prefix_product", "prefix_sum", "eval_polynomial", "eval_polynomial_batch",
                                                      "max_scalar_bits", "points_decompress", "msm"}


@pytest.mark.parametrize("name", NAMES)
def test_expected_output_is_the_definition_in_integers(name):
    a = S.BY_NAME[name]
    c = S.built(name, 1, small=True)
    outputs, host = DEFINITIONS[name](c)
    assert set(outputs) == set(a.outputs) == set(c.expect) and set(host) == set(c.host)
    norm = a.normalise(c, dict(c.host))
    for key, want in outputs.items():
        assert _read(name, key, c.expect[key]) == want, key
    for key, want in host.items():
        assert _read(name, key, np.asarray(norm[key])) == want, key


@pytest.mark.parametrize("name", NAMES)
def test_two_seeds_same_shapes_different_outputs(name):
    """at the size the device tests run"""
    c1, c2 = S.built(name, 1), S.built(name, 2)
    assert c1.signature() == c2.signature()
    assert set(c1.scratch) == set(c2.scratch)
    L = S.host_lib()
    for key in c1.scratch:
        try:
            assert c1.scratch[key](L) == c2.scratch[key](L)
        except AttributeError:
            pass                                       # a size only libhalo2_hip.so states: a function of the dims compared above
    differ = [not np.array_equal(c1.expect[k], c2.expect[k]) for k in c1.expect if k != "status"]
    differ += [not np.array_equal(c1.host[k], c2.host[k]) for k in c1.host]
    assert differ and all(differ)
    for k in c1.inputs:
        if k not in ("t", "records", "row_count"):   # (the domain's constants, the caller-zeroed blocks)
            assert not np.array_equal(c1.inputs[k], c2.inputs[k]), k


def test_a_decoy_is_valid_wherever_the_real_case_is():
    """what bounds an index inside a kernel is a size or a table entry: both are equal or in range for every seed"""
    for seed in (1, 2):
        c = S.built("permutation_sigma", seed)
        assert c.inputs["map_col"].max() < S.PERM_COLUMNS and c.inputs["map_row"].max() < c.dims["n"]
        c = S.built("permutation_mapping", seed)
        cp, d = c.inputs["copies"], c.dims
        assert cp[:, [0, 2]].max() < d["ncols"] and cp[:, [1, 3]].max() < d["n"] and len(cp) == d["copies"]
        c = S.built("logup_multiplicity", seed)
        keys = set(S.H.keys_of(c.inputs["table"][:c.dims["usable"]]))
        assert all(set(S.H.keys_of(c.inputs["in%d" % j][:c.dims["usable"]])) <= keys for j in range(S.LOGUP_INPUTS))
        c = S.built("points_decompress", seed)
        assert S.host_lib().o.points_decompress(c.inputs["bytes"])[1] == 0
        for name in ("evaluate_h_generated", "evaluate_h_interpreter"):
            kw = S.built(name, seed).kw
            assert (len(kw["calculations"]), len(kw["constants"]), len(kw["rotations"]), len(kw["value_parts"])) == (40, 6, 5, 6)
            assert [len(kw[t]) for t in S.COLUMN_TABLES] == [2, 3, 1, 3, 5, 4, 2, 2]
            assert [len(l[1]) for l in kw["lookups"]] == [1, 3] and len(kw["shuffles"]) == 2
