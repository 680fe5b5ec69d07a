"""The field and G1 primitives of csrc/field.hpp, ec.hpp and ec_quad.hpp, checked one by one against plain Python integers.

tests/arith_conformance.hip runs one kernel per primitive over an operand table this module writes; every expected value is
computed here with `pow` and `%` (G1 with tests/ref_plonk.py's affine g1_add / g1_neg / g1_mul), never with the C oracle or
the header's own host path.  The harness is built three ways: g++ (the host path: the 4 x u64 CIOS product, the portable
column scans -- CPU suite), hipcc for gfx950 (the inline-asm carry chains and the generated schedules of fp_mul_gen.hpp --
the code the product runs) and hipcc for gfx950 with -DH2_PORTABLE_MUL (the portable device path).

The cases are those random data almost never reach: Montgomery reductions whose every digit is 2^32 - 1, sums that land
exactly on p, 2p or 4p, the non-canonical operands the contracts allow (anything below 2^254 for the products, any 256-bit
value for fp_mul_wide / fp_mul_const / the conversions, below 4p for the lazy domain), the shortest and longest Kaliski runs
of fp_inv, and one point added to itself in two XYZZ representations -- each next to a few thousand random cases.  A case
that claims to be exceptional is checked to be so (test_exceptional_cases_are_what_they_are_named), and every batch is
checked for its layout on the device (mixed branches per wave, neighbouring quads on different branches, fp_inv once with
whole waves holding one value), so that a harness that drops or reorders cases cannot pass.
"""
import concurrent.futures
import functools
import os
import random
import struct
import subprocess

import pytest

from ref_plonk import G1, Q, R as R_MOD, g1_add, g1_mul, g1_neg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "halo2-gpu-specific_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "arith_conformance.hip")
HIPCC = "/opt/rocm/bin/hipcc"

RM = 1 << 256                      # the Montgomery radix R
FIELDS = {"Fr": R_MOD, "Fq": Q}
FIELD_ID = {"Fr": 0, "Fq": 1}
SEED = 0x5EED_A417
N_RANDOM = 2500                    # random cases per field primitive, on top of the edge cases
WAVE = 64
IN_BYTES, OUT_BYTES = 272, 128     # struct In / struct Out of the harness

FIELD_OPS = ["fp_add", "fp_sub", "fp_neg", "fp_dbl", "fp_reduce_once", "fp_mul", "fp_sqr", "fp_mul2", "fp_mul_wide",
             "fp_mul_const", "fp_const_pair", "fp_to_mont", "fp_from_mont", "fp_lazy_red2p", "fp_lazy_add", "fp_lazy_sub",
             "fp_lazy_add_red", "fp_lazy_sub_red", "fp_lazy_canon", "fp_inv", "fp_pow_u32"]
G1_OPS = ["xyzz_from_affine", "xyzz_madd", "xyzz_add", "xyzz_double", "xyzz_double_affine", "xyzz_mul_u32", "xyzz_to_jacobian"]
QUAD_OPS = {"xyzz_add_q": "xyzz_add", "xyzz_double_q": "xyzz_double", "xyzz_mul_u32_q": "xyzz_mul_u32"}  # -> its scalar twin


class Case:
    """one operand record: `ops` are the 256-bit operands v[0..7] as integers, `k` the 32-bit scalar, `flag` the negate flag;
    `claim` is what the case says it is, as (kind, value) -- checked by test_exceptional_cases_are_what_they_are_named"""
    __slots__ = ("label", "ops", "k", "flag", "claim", "kind")

    def __init__(self, label, ops, k=0, flag=0, claim=None, kind="general"):
        self.label, self.ops, self.k, self.flag, self.claim, self.kind = label, tuple(ops), k, flag, claim, kind

    def describe(self):
        ops = ", ".join("0x%x" % v for v in self.ops)
        extra = (" k=0x%x" % self.k if self.k else "") + (" negate" if self.flag else "")
        return "'%s' (%s)%s" % (self.label, ops, extra)


# ---- Montgomery arithmetic with Python integers ---------------------------------------------------------------------------
def redc_parts(t, p):
    """the REDC of t: (m, (t + m p) / R) with m = -t p^-1 mod R -- the digits of m are the device's eight m_i, the second
    value what a product holds before its final conditional subtraction"""
    m = (-t * pow(p, -1, RM)) % RM
    return m, (t + m * p) >> 256


def ones_digits(m):
    return sum(1 for i in range(8) if (m >> (32 * i)) & 0xFFFFFFFF == 0xFFFFFFFF)


def kaliski_rounds(v, p):
    """the number of rounds of fp_inv's loop for the input v (the four cases of field.hpp, counting only)"""
    u, k = p, 0
    while v:
        if not u & 1:
            u >>= 1
        elif not v & 1:
            v >>= 1
        elif u > v:
            u = (u - v) >> 1
        else:
            v = (v - u) >> 1
        k += 1
    return k


def sqrt_mod_2_256(c):
    """a root of x^2 = c mod 2^256 for c = 1 mod 8 (Hensel, one bit at a time), chosen below 2^254"""
    assert c % 8 == 1
    x = 1
    for b in range(3, 256):
        if (x * x - c) % (1 << (b + 1)):
            x += 1 << (b - 1)
    assert x * x % RM == c
    x %= 1 << 255                      # the roots are +-x and +-x + 2^255
    return min(x, (1 << 255) - x)


def patterns():
    """all-ones limbs, alternating limbs and bits, values just below 2^254 and 2^256"""
    out = [(1 << (32 * k)) - 1 for k in range(1, 9)]
    alt_lo = sum(0xFFFFFFFF << (64 * i) for i in range(4))
    out += [alt_lo, alt_lo << 32, int("55" * 32, 16), int("aa" * 32, 16), int("33" * 32, 16), int("cc" * 32, 16)]
    out += [alt_lo & ((1 << 254) - 1), (alt_lo << 32) & ((1 << 254) - 1), int("aa" * 32, 16) >> 2]
    out += [(1 << 254) - 1, (1 << 254) - 2, (1 << 254) - (1 << 32), (1 << 254) - (1 << 224), (1 << 253), (1 << 253) - 1]
    out += [RM - 1, RM - 2, RM - (1 << 32), RM - (1 << 224), 1 << 255, (1 << 255) - 1]
    return out


# ---- the field cases ---------------------------------------------------------------------------------------------------
def field_pools(p):
    ri = pow(RM, -1, p)
    edges = [0, 1, 2, p - 1, p - 2, (p - 1) // 2, (p + 1) // 2, RM % p, ri]
    mult = [c * p + d for c in range(1, 6) for d in (-1, 0, 1)]
    every = sorted(set(edges + patterns() + mult))
    return {
        "canon": edges + [v for v in every if v < p and v not in edges],
        "2p": [v for v in every if v < 2 * p],
        "4p": [v for v in every if v < 4 * p],
        "254": [v for v in every if v < 1 << 254],
        "256": [v for v in every if v < RM],
    }


BOUND = {"canon": lambda p: p, "2p": lambda p: 2 * p, "4p": lambda p: 4 * p, "254": lambda p: 1 << 254, "256": lambda p: RM}


def rand_in(rnd, dom, p):
    """uniform below the domain's bound, or (one in four) within 2^64 of it"""
    b = BOUND[dom](p)
    return b - 1 - rnd.randrange(1 << 64) if rnd.random() < 0.25 else rnd.randrange(b)


def pairs(pool_a, pool_b, label="edge"):
    return [Case(label, (a, b)) for a in pool_a for b in pool_b]


def ones_products(rnd, p, count, a_dom=1 << 254, b_dom=1 << 254):
    """(a, b) with a b = p mod 2^256: the reduction digits m_i of a b are all 2^32 - 1"""
    out = []
    while len(out) < count:
        b = rnd.randrange(1, b_dom) | 1
        a = p * pow(b, -1, RM) % RM
        if a < a_dom:
            out.append((a, b))
    return out


def landing(rnd, p, dom_bound, targets, sign, n_each=3):
    """(a, b) below dom_bound with a + b (sign +1) or a - b (sign -1) equal to each target exactly"""
    out = []
    for name, t in targets:
        lo, hi = (max(0, t - dom_bound + 1), min(t, dom_bound - 1)) if sign > 0 else (max(0, t), min(dom_bound - 1, dom_bound - 1 + t))
        assert lo <= hi, (name, t)
        for a in [lo, hi] + [rnd.randint(lo, hi) for _ in range(n_each - 2)]:
            b = t - a if sign > 0 else a - t
            out.append(Case("%s=%s" % ("sum" if sign > 0 else "diff", name), (a, b), claim=("sum" if sign > 0 else "diff", t)))
    return out


def build_field_cases(op, p, rnd):
    pools = field_pools(p)
    ri = pow(RM, -1, p)
    C, rc = [], []                                     # edge / exceptional cases, random cases
    if op in ("fp_add", "fp_sub"):
        C += pairs(pools["canon"], pools["canon"])
        if op == "fp_add":
            C += landing(rnd, p, p, [("0", 0), ("p-1", p - 1), ("p", p), ("p+1", p + 1), ("2p-2", 2 * p - 2)], +1)
        else:
            C += landing(rnd, p, p, [("0", 0), ("-1", -1), ("1", 1), ("-(p-1)", -(p - 1)), ("p-1", p - 1)], -1)
        rc = [Case("random", (rnd.randrange(p), rnd.randrange(p))) for _ in range(N_RANDOM)]
    elif op in ("fp_neg", "fp_dbl"):
        C += [Case("edge", (a,)) for a in pools["canon"]]
        if op == "fp_dbl":
            C += [Case("2a=p-1", ((p - 1) // 2,), claim=("sum", p - 1)), Case("2a=p+1", ((p + 1) // 2,), claim=("sum", p + 1)),
                  Case("2a=2p-2", (p - 1,), claim=("sum", 2 * p - 2))]
        rc = [Case("random", (rnd.randrange(p),)) for _ in range(N_RANDOM)]
    elif op == "fp_reduce_once":
        C += [Case("edge", (a,)) for a in pools["2p"]]
        C += [Case("value=%s" % n, (v,), claim=("value", v)) for n, v in [("0", 0), ("p-1", p - 1), ("p", p), ("p+1", p + 1), ("2p-1", 2 * p - 1)]]
        rc = [Case("random", (rand_in(rnd, "2p", p),)) for _ in range(N_RANDOM)]
    elif op in ("fp_mul", "fp_sqr", "fp_mul2"):
        pool = pools["254"]
        if op == "fp_mul":
            C += pairs(pool, pool)
            C += [Case("pre=p", (p, b), claim=("pre", p)) for b in pool if b % p]                 # (p b + (R - b) p) / R = p
            for a, b in ones_products(rnd, p, 24):
                C += [Case("ones-digits", (a, b), claim=("ones", 8)), Case("ones-digits", (b, a), claim=("ones", 8))]
            rc = [Case("random", (rand_in(rnd, "254", p), rand_in(rnd, "254", p))) for _ in range(N_RANDOM)]
        elif op == "fp_sqr":
            C += [Case("edge", (a,)) for a in pool]
            # a^2 = c p mod 2^256: c = 1 mod 8 / p mod 8 -- for Fr (p = 1 mod 8) every digit is all-ones; for Fq (p = 7 mod 8)
            # p itself is no square mod 2^256, the best is c = 7: m = R - 7, digits 1..7 all-ones (digit 0 cannot be: a^2 = 1 mod 8)
            best = 8 if p % 8 == 1 else 7
            for c in range(1, 400):
                if (c * p) % 8 == 1 and len(C) < len(pool) + 12:
                    a = sqrt_mod_2_256(c * p % RM)
                    if ones_digits(redc_parts(a * a, p)[0]) == best:
                        C.append(Case("ones-digits", (a,), claim=("ones", best)))
            rc = [Case("random", (rand_in(rnd, "254", p),)) for _ in range(N_RANDOM)]
        else:
            small = [0, 1, p - 1, (1 << 254) - 1, RM % p, p]
            C += [Case("edge", (a, b, c, d)) for a in small for b in small for c in small for d in small[:3]]
            prods = ones_products(rnd, p, 16)
            for (a, b), (c, d) in zip(prods[::2], prods[1::2]):                 # two products of all-ones digits: m = R - 2
                C.append(Case("two-ones-products", (a, b, c, d), claim=("ones", 7)))
            for a, b in prods[:6]:
                C.append(Case("ones-digits+0", (a, b, 0, 0), claim=("ones", 8)))
                C.append(Case("0+ones-digits", (0, 0, a, b), claim=("ones", 8)))
            got = 0
            while got < 24:                                                    # a b + c d = p mod 2^256, all four below 2^254
                a, b, c = (rnd.randrange(1 << 254) for _ in range(3))
                c |= 1
                d = (p - a * b) * pow(c, -1, RM) % RM
                if d < 1 << 254:
                    C.append(Case("ones-digits-sum", (a, b, c, d), claim=("ones", 8)))
                    got += 1
            rc = [Case("random", tuple(rand_in(rnd, "254", p) for _ in range(4))) for _ in range(N_RANDOM)]
    elif op == "fp_mul_wide":
        C += pairs(pools["256"], pools["canon"])
        for a, b in ones_products(rnd, p, 24, a_dom=RM, b_dom=p):
            C.append(Case("ones-digits", (a, b), claim=("ones", 8)))
        rc = [Case("random", (rand_in(rnd, "256", p), rnd.randrange(p))) for _ in range(N_RANDOM)]
    elif op == "fp_mul_const":
        wm = [0, 1, 2, p - 1, RM % p, ri] + [rnd.randrange(p) for _ in range(6)]
        C += [Case("edge", (x,) + const_pair(w, p)) for x in pools["256"] for w in wm]
        got = 0
        while got < 32:   # x w' = t mod 2^256 with t < 2^200: the quotient summed over anti-diagonals >= 6 only is one short
            w, q = const_pair(rnd.randrange(p), p)
            if q & 1:
                x = rnd.randrange(1 << 200) * pow(q, -1, RM) % RM
                C.append(Case("short-quotient", (x, w, q), claim=("short", 0)))
                got += 1
        rc = [Case("random", (rand_in(rnd, "256", p),) + const_pair(rnd.randrange(p), p)) for _ in range(N_RANDOM)]
    elif op == "fp_const_pair":
        C += [Case("edge", (w,)) for w in pools["canon"]]
        rc = [Case("random", (rnd.randrange(p),)) for _ in range(N_RANDOM)]
    elif op in ("fp_to_mont", "fp_from_mont"):
        C += [Case("edge", (a,)) for a in pools["256"]]
        C += [Case("value=%dp" % c, (c * p,), claim=("value", c * p)) for c in range(1, 6)]
        if op == "fp_to_mont":    # a R^2 mod p = p mod 2^256: the product inside takes all-ones digits
            rr = RM * RM % p
            C.append(Case("ones-digits", (p * pow(rr, -1, RM) % RM,), claim=("ones", 8)))
        else:
            C.append(Case("ones-digits", (p,), claim=("ones", 8)))
        rc = [Case("random", (rand_in(rnd, "256", p),)) for _ in range(N_RANDOM)]
    elif op in ("fp_lazy_red2p", "fp_lazy_canon"):
        C += [Case("edge", (a,)) for a in pools["4p"]]
        C += [Case("value=%s" % n, (v,), claim=("value", v)) for n, v in
              [("0", 0), ("p-1", p - 1), ("p", p), ("2p-1", 2 * p - 1), ("2p", 2 * p), ("2p+1", 2 * p + 1), ("3p-1", 3 * p - 1),
               ("3p", 3 * p), ("3p+1", 3 * p + 1), ("4p-1", 4 * p - 1)]]
        C += [Case("in [3p,4p)", (3 * p + rnd.randrange(p),), claim=("range", 3)) for _ in range(16)]
        rc = [Case("random", (rand_in(rnd, "4p", p),)) for _ in range(N_RANDOM)]
    elif op in ("fp_lazy_add", "fp_lazy_add_red"):
        C += pairs(pools["2p"], pools["2p"])
        C += landing(rnd, p, 2 * p, [("0", 0), ("p", p), ("2p-1", 2 * p - 1), ("2p", 2 * p), ("2p+1", 2 * p + 1), ("4p-2", 4 * p - 2)], +1)
        rc = [Case("random", (rand_in(rnd, "2p", p), rand_in(rnd, "2p", p))) for _ in range(N_RANDOM)]
    elif op in ("fp_lazy_sub", "fp_lazy_sub_red"):
        C += pairs(pools["2p"], pools["2p"])
        C += landing(rnd, p, 2 * p, [("0", 0), ("-1", -1), ("1", 1), ("2p-1", 2 * p - 1), ("-(2p-1)", -(2 * p - 1)), ("-p", -p)], -1)
        rc = [Case("random", (rand_in(rnd, "2p", p), rand_in(rnd, "2p", p))) for _ in range(N_RANDOM)]
    elif op == "fp_inv":
        C += [Case("edge", (a,)) for a in pools["canon"]]
        C += [Case("2^%d" % j, (1 << j,)) for j in range(254)]
        C += [Case("2^%d R" % j, ((1 << j) * RM % p,)) for j in range(64)]
        C += [Case("zero as p", (p,), claim=("value", p))]            # the residue 0 in its non-canonical form
        C += [Case("kaliski-shortest", (1,), claim=("kaliski", 254)), Case("kaliski-longest", (1 << 253,), claim=("kaliski", 507))]
        rc = [Case("random", (rnd.randrange(p),)) for _ in range(N_RANDOM // 2)]
    elif op == "fp_pow_u32":
        es = [0, 1, 2, 3, 1 << 31, (1 << 32) - 1]
        C += [Case("edge", (a,), k=e) for a in pools["canon"] for e in es]
        rc = [Case("random", (rnd.randrange(p),), k=rnd.choice(es + [rnd.randrange(1 << 32)])) for _ in range(N_RANDOM // 4)]
    else:
        raise AssertionError(op)
    cases = C + rc
    rnd.shuffle(cases)                           # every wave mixes edge, exceptional and random cases
    if len(cases) % WAVE == 0:
        cases.append(rc[0])
    return cases


def const_pair(w_mont, p):
    """what fp_mul_const reads for the twiddle w_mont: the plain value and floor(w_plain 2^256 / p)"""
    w = w_mont * pow(RM, -1, p) % p
    return w, (w << 256) // p


def inv_uniform_cases(p, rnd):
    """fp_inv as k_batch_invert calls it: whole waves hold one value (the last, partial wave too)"""
    values = [1, 2, p - 1, 1 << 253, RM % p, p, 0, (1 << 17) * RM % p] + [rnd.randrange(p) for _ in range(4)]
    cases = [Case("uniform", (v,)) for v in values for _ in range(WAVE)]
    return cases + [Case("uniform", (values[-1],))] * 37


# ---- G1 --------------------------------------------------------------------------------------------------------------
def mont(v):
    return v * RM % Q


def xyzz_rep(P, lam):
    """the affine point P as XYZZ (lam^2 x, lam^3 y, lam^2, lam^3), Montgomery form; the identity as xyzz_identity()"""
    if P is None:
        return (0, mont(1), 0, 0)
    l2, l3 = lam * lam % Q, lam * lam * lam % Q
    return tuple(mont(v) for v in (l2 * P[0] % Q, l3 * P[1] % Q, l2, l3))


def affine_rep(P):
    return (0, 0) if P is None else (mont(P[0]), mont(P[1]))


def xyzz_value(c):
    """the affine point a Montgomery-form XYZZ record stands for (None: the identity, zz = 0)"""
    x, y, zz, zzz = (v * pow(RM, -1, Q) % Q for v in c)
    if zz == 0:
        return None
    return x * pow(zz, -1, Q) % Q, y * pow(zzz, -1, Q) % Q


def round_robin(groups):
    """one case of each kind in turn: neighbouring quads (and the lanes of every wave) take different branches"""
    out, i = [], 0
    while any(groups):
        g = groups[i % len(groups)]
        if g:
            out.append(g.pop(0))
        i += 1
    return out


def build_g1_cases(rnd):
    pts = [G1] + [g1_mul(G1, rnd.randrange(1, R_MOD)) for _ in range(23)]
    pt = lambda: rnd.choice(pts)                                            # noqa: E731
    lam = lambda: rnd.randrange(2, Q)                                       # noqa: E731
    stale = (mont(5), mont(7), 0, mont(11))                                 # an identity (zz = 0) with leftover coordinates
    n = 40
    out = {}
    # a + b: the identity cases, P + P and P - P in two representations, and general sums
    ident, same, opp, gen = [], [], [], []
    for i in range(n):
        P, Qp = pt(), pt()
        z = xyzz_rep(None, 1) if i % 2 else stale
        ident.append(Case(["O+P", "P+O", "O+O"][i % 3], [z + xyzz_rep(P, lam()), xyzz_rep(P, lam()) + z, z + z][i % 3], kind="identity",
                          claim=("identity-operand", 0)))
        l1, l2 = lam(), lam()
        same.append(Case("P+P", xyzz_rep(P, l1) + xyzz_rep(P, l1 if i % 8 == 0 else l2), kind="P+P", claim=("P+P", i % 8 != 0)))
        opp.append(Case("P-P", xyzz_rep(P, l1) + xyzz_rep(g1_neg(P), l2), kind="P-P", claim=("P-P", 1)))
        gen.append(Case("general", xyzz_rep(P, lam() if i % 4 else 1) + xyzz_rep(Qp if Qp != P else G1 if P != G1 else pts[1], lam()),
                        kind="general"))
    out["xyzz_add"] = round_robin([ident, same, opp, gen])
    # 2 P
    dbl = []
    for i in range(2 * n):
        if i % 2 == 0:
            dbl.append(Case("O", xyzz_rep(None, 1) if i % 4 else stale, kind="identity"))
        else:
            dbl.append(Case("2P", xyzz_rep(pt(), lam() if i % 8 != 1 else 1), kind="general"))
    out["xyzz_double"] = dbl
    # [k] P
    mul = []
    for i in range(2 * n):
        P = pt()
        k = [0, 1, 2, 3, 1 << 31, (1 << 32) - 1, rnd.randrange(1 << 32), rnd.randrange(1 << 8)][i % 8]
        rep = xyzz_rep(None, 1) if i % 11 == 5 else xyzz_rep(P, lam() if i % 3 else 1)
        mul.append(Case("[k]P", rep, k=k, kind="O" if i % 11 == 5 else "k=%d" % k))
    out["xyzz_mul_u32"] = mul
    # acc + (+-) q
    madd = []
    for i in range(2 * n):
        P, Qp = pt(), pt()
        sel = i % 8
        if sel == 0:
            madd.append(Case("acc=q", xyzz_rep(P, lam()) + affine_rep(P), kind="P+P", claim=("madd-same", 0)))
        elif sel == 1:
            madd.append(Case("acc=-q", xyzz_rep(g1_neg(P), lam()) + affine_rep(P), kind="P-P", claim=("madd-opp", 0)))
        elif sel == 2:
            madd.append(Case("acc=q, negate", xyzz_rep(P, lam()) + affine_rep(P), flag=1, kind="P-P", claim=("madd-opp", 1)))
        elif sel == 3:
            madd.append(Case("acc=-q, negate", xyzz_rep(g1_neg(P), lam()) + affine_rep(P), flag=1, kind="P+P", claim=("madd-same", 1)))
        elif sel == 4:
            madd.append(Case("O+q", (stale if i % 16 == 4 else xyzz_rep(None, 1)) + affine_rep(P), flag=i & 1, kind="identity"))
        elif sel == 5:
            madd.append(Case("acc+O", xyzz_rep(P, lam()) + affine_rep(None), flag=i & 1, kind="identity"))
        else:
            Qp = Qp if Qp != P else g1_add(P, G1)
            madd.append(Case("general", xyzz_rep(P, lam() if sel == 6 else 1) + affine_rep(Qp), flag=i & 1, kind="general"))
    out["xyzz_madd"] = madd
    out["xyzz_from_affine"] = [Case("O" if i % 4 == 0 else "P", affine_rep(None if i % 4 == 0 else pt()), flag=(i >> 1) & 1,
                                    kind="identity" if i % 4 == 0 else "general") for i in range(n)]
    out["xyzz_double_affine"] = [Case("2P", affine_rep(pt()), kind="general") for _ in range(n)]
    out["xyzz_to_jacobian"] = [Case("O" if i % 4 == 0 else "P", (xyzz_rep(None, 1) if i % 8 else stale) if i % 4 == 0 else xyzz_rep(pt(), lam()),
                                    kind="identity" if i % 4 == 0 else "general") for i in range(n)]
    for name, cases in out.items():
        while len(cases) % 16 == 0:                  # neither the cases nor the lanes of the quad form fill whole waves
            cases.append(cases[0])
    return out


@functools.lru_cache(maxsize=None)
def all_batches():
    """[(op, field, layout, cases)] for every build; the quad batches reuse their scalar twin's cases, in the same order"""
    rnd = random.Random(SEED)
    batches = []
    for field, p in FIELDS.items():
        for op in FIELD_OPS:
            batches.append((op, field, "mixed", build_field_cases(op, p, rnd)))
        batches.append(("fp_inv", field, "uniform", inv_uniform_cases(p, rnd)))
    g1 = build_g1_cases(rnd)
    for op in G1_OPS:
        batches.append((op, "Fq", "mixed", g1[op]))
    for op, twin in QUAD_OPS.items():
        batches.append((op, "Fq", "quad", g1[twin]))
    return batches


# ---- expected values ----------------------------------------------------------------------------------------------------
def check_field(op, p, c, r):
    """-> None when the result r (four integers) meets the contract for the case c, else what was wanted"""
    ri = pow(RM, -1, p)
    a = c.ops[0]
    b = c.ops[1] if len(c.ops) > 1 else 0
    got = r[0]

    def exact(want):
        return None if got == want else "0x%x" % want

    def lazy(want, bound):
        return None if got < bound and got % p == want % p else "a value below 0x%x congruent to 0x%x" % (bound, want % p)

    if op == "fp_add":
        return exact((a + b) % p)
    if op == "fp_sub":
        return exact((a - b) % p)
    if op == "fp_neg":
        return exact(-a % p)
    if op == "fp_dbl":
        return exact(2 * a % p)
    if op in ("fp_reduce_once", "fp_lazy_canon"):
        return exact(a % p)
    if op == "fp_mul":
        return exact(a * b * ri % p)
    if op == "fp_sqr":
        return exact(a * a * ri % p)
    if op == "fp_mul2":
        return exact((a * b + c.ops[2] * c.ops[3]) * ri % p)
    if op == "fp_mul_wide":
        return lazy(a * b * ri, 2 * p)
    if op == "fp_mul_const":
        return lazy(a * b, 2 * p)
    if op == "fp_const_pair":
        w, wq = r[0], r[1]
        ok = w == a * ri % p and (w << 256) == wq * p + a
        return None if ok else "w_plain 0x%x, wq 0x%x" % const_pair(a, p)
    if op == "fp_to_mont":
        return exact(a * RM % p)
    if op == "fp_from_mont":
        return exact(a * ri % p)
    if op == "fp_lazy_red2p":
        return lazy(a, 2 * p)
    if op == "fp_lazy_add":
        return exact(a + b)
    if op == "fp_lazy_sub":
        return exact(a - b + 2 * p)
    if op in ("fp_lazy_add_red", "fp_lazy_sub_red"):
        return lazy(a + b if op == "fp_lazy_add_red" else a - b, 2 * p)
    if op == "fp_inv":
        return exact(0 if a % p == 0 else RM * RM * pow(a, -1, p) % p)
    if op == "fp_pow_u32":
        return exact(pow(a * ri % p, c.k, p) * RM % p)
    raise AssertionError(op)


def g1_expected(op, c):
    if op == "xyzz_from_affine":
        P = None if c.ops[:2] == (0, 0) else tuple(v * pow(RM, -1, Q) % Q for v in c.ops[:2])
        return g1_neg(P) if c.flag else P
    if op == "xyzz_madd":
        Qp = None if c.ops[4:6] == (0, 0) else tuple(v * pow(RM, -1, Q) % Q for v in c.ops[4:6])
        return g1_add(xyzz_value(c.ops[:4]), g1_neg(Qp) if c.flag else Qp)
    if op in ("xyzz_add", "xyzz_add_q"):
        return g1_add(xyzz_value(c.ops[:4]), xyzz_value(c.ops[4:8]))
    if op in ("xyzz_double", "xyzz_double_q"):
        P = xyzz_value(c.ops[:4])
        return g1_add(P, P)
    if op == "xyzz_double_affine":
        P = tuple(v * pow(RM, -1, Q) % Q for v in c.ops[:2])
        return g1_add(P, P)
    if op in ("xyzz_mul_u32", "xyzz_mul_u32_q"):
        return g1_mul(xyzz_value(c.ops[:4]), c.k)
    if op == "xyzz_to_jacobian":
        return xyzz_value(c.ops[:4])
    raise AssertionError(op)


def check_g1(op, c, r, want):
    """XYZZ results: canonical coordinates, the identity exactly when zz = 0, else zz^3 = zzz^2 and (x / zz, y / zzz) the
    big-integer point; xyzz_to_jacobian: (x / z^2, y / z^3)"""
    if any(v >= Q for v in r):
        return "canonical coordinates"
    ri = pow(RM, -1, Q)
    x, y, z2, z3 = (v * ri % Q for v in r)
    if op == "xyzz_to_jacobian":
        if want is None:
            return None if z2 == 0 else "the identity (z = 0)"
        if z2 == 0:
            return str(want)
        return None if (x * pow(z2, -2, Q) % Q, y * pow(z2, -3, Q) % Q) == want else str(want)
    if want is None:
        return None if z2 == 0 else "the identity (zz = 0)"
    if z2 == 0 or pow(z2, 3, Q) != pow(z3, 2, Q):
        return "%s with zz^3 = zzz^2 != 0" % (want,)
    return None if (x * pow(z2, -1, Q) % Q, y * pow(z3, -1, Q) % Q) == want else str(want)


# ---- building and running the harness -----------------------------------------------------------------------------------
BUILDS = {
    "host": ["g++", "-O2", "-std=c++17", "-x", "c++", "-I", CSRC],
    "gfx950": [HIPCC, "-O2", "-std=c++17", "--offload-arch=gfx950", "-I", CSRC],
    "gfx950-portable": [HIPCC, "-O2", "-std=c++17", "--offload-arch=gfx950", "-DH2_PORTABLE_MUL", "-I", CSRC],
}


def compile_build(build, out_dir, timeout=240):
    exe = os.path.join(out_dir, "arith_conformance_" + build.replace("-", "_"))
    res = subprocess.run(BUILDS[build] + [SRC, "-o", exe], capture_output=True, text=True, timeout=timeout)
    assert res.returncode == 0, "%s build of arith_conformance.hip failed:\n%s" % (build, res.stderr[-4000:])
    return exe


def batches_for(build):
    return [b for b in all_batches() if build != "host" or b[2] != "quad"]


def encode(batches):
    buf = bytearray(b"ACF1" + struct.pack("<I", len(batches)))
    for op, field, _, cases in batches:
        buf += op.encode().ljust(32, b"\0") + struct.pack("<II", FIELD_ID[field], len(cases))
        for c in cases:
            ops = c.ops + (0,) * (8 - len(c.ops))
            buf += b"".join(v.to_bytes(32, "little") for v in ops) + struct.pack("<4I", c.k, c.flag, 0, 0)
    assert len(buf) == 8 + sum(40 + IN_BYTES * len(b[3]) for b in batches)
    return bytes(buf)


def run_build(exe, build, work_dir, timeout=180):
    """-> {(op, field): [(layout, cases, results)]}; asserts that every batch comes back with one result per case and lane"""
    batches = batches_for(build)
    inp, outp = os.path.join(work_dir, build + ".in"), os.path.join(work_dir, build + ".out")
    with open(inp, "wb") as f:
        f.write(encode(batches))
    res = subprocess.run([exe, inp, outp], capture_output=True, text=True, timeout=timeout)
    assert res.returncode == 0, "%s harness failed (exit %d):\n%s%s" % (build, res.returncode, res.stdout[-2000:], res.stderr[-4000:])
    with open(outp, "rb") as f:
        data = f.read()
    assert data[:4] == b"ACF1" and struct.unpack_from("<I", data, 4)[0] == len(batches)
    pos, results = 8, {}
    for op, field, layout, cases in batches:
        name = data[pos:pos + 32].rstrip(b"\0").decode()
        fid, n_out = struct.unpack_from("<II", data, pos + 32)
        pos += 40
        lanes = 4 if layout == "quad" else 1
        assert (name, fid) == (op, FIELD_ID[field]), (name, fid, op, field)
        assert n_out == len(cases) * lanes, "%s[%s]: %d results for %d cases x %d lanes" % (op, field, n_out, len(cases), lanes)
        rec = data[pos:pos + n_out * OUT_BYTES]
        assert len(rec) == n_out * OUT_BYTES, "%s[%s]: truncated output" % (op, field)
        pos += n_out * OUT_BYTES
        outs = [tuple(int.from_bytes(rec[i * OUT_BYTES + 32 * j:i * OUT_BYTES + 32 * (j + 1)], "little") for j in range(4))
                for i in range(n_out)]
        results.setdefault((op, field), []).append((layout, cases, outs))
    assert pos == len(data), "trailing output"
    return results


def failures(op, field, results, scalar_results=None, limit=6):
    """the cases of (op, field) whose results break the contract, as messages that name the primitive and the operands"""
    bad = []
    for layout, cases, outs in results[(op, field)]:
        lanes = 4 if layout == "quad" else 1
        assert len(outs) == len(cases) * lanes
        twin = None
        if layout == "quad":
            twin = scalar_results[(QUAD_OPS[op], field)][0][2]
            assert len(twin) == len(cases)
        memo = {}
        for i, c in enumerate(cases):
            for lane in range(lanes):
                r = outs[i * lanes + lane]
                if op.startswith("fp_"):
                    want = check_field(op, FIELDS[field], c, r)
                else:
                    if i not in memo:
                        memo[i] = g1_expected(op, c)
                    want = check_g1(op, c, r, memo[i])
                    if want is None and twin is not None and r != twin[i]:
                        want = "limb for limb the scalar %s result (%s)" % (QUAD_OPS[op], ", ".join("0x%x" % v for v in twin[i]))
                if want is not None:
                    where = " [%s layout%s]" % (layout, ", lane %d" % lane if lanes > 1 else "")
                    bad.append("%s[%s] %s%s: got (%s), want %s" % (op, field, c.describe(), where,
                                                                  ", ".join("0x%x" % v for v in r), want))
                    if len(bad) >= limit:
                        return bad
    return bad


PRIMS = [(op, f) for op in FIELD_OPS for f in FIELDS] + [(op, "Fq") for op in G1_OPS]
QUAD_PRIMS = [(op, "Fq") for op in QUAD_OPS]
IDS = ["%s-%s" % p for p in PRIMS]


# ---- the suite ----------------------------------------------------------------------------------------------------------
def test_exceptional_cases_are_what_they_are_named():
    """each case that claims to be exceptional is: sums landing on their target, products with all-ones reduction digits
    or a value of exactly p before the final subtraction, the Kaliski extremes, P + P in two representations, ..."""
    seen = {}
    for op, field, layout, cases in all_batches():
        p = FIELDS[field]
        for c in cases:
            if c.claim is None:
                continue
            kind, v = c.claim
            seen[(op, kind)] = seen.get((op, kind), 0) + 1
            a = c.ops[0]
            if kind == "sum":
                ok = (a + (c.ops[1] if len(c.ops) > 1 else a)) == v
            elif kind == "diff":
                ok = a - c.ops[1] == v
            elif kind == "value":
                ok = a == v
            elif kind == "range":
                ok = v * p <= a < (v + 1) * p
            elif kind == "pre":
                ok = redc_parts(a * c.ops[1], p)[1] == v and a < 1 << 254 and c.ops[1] < 1 << 254
            elif kind == "ones":
                # the product the primitive reduces: a b (+ c d), a a, a R^2 mod p (fp_to_mont), a 1 (fp_from_mont)
                t = {"fp_sqr": a * a, "fp_to_mont": a * (RM * RM % p), "fp_from_mont": a}.get(op)
                if t is None:
                    t = a * c.ops[1] + (c.ops[2] * c.ops[3] if op == "fp_mul2" else 0)
                lim = RM if op in ("fp_mul_wide", "fp_to_mont", "fp_from_mont") else 1 << 254
                ok = ones_digits(redc_parts(t, p)[0]) == v and all(x < lim for x in c.ops)
            elif kind == "short":
                w, q = c.ops[1], c.ops[2]
                ok = a * q % RM < 7 << 224 and q == (w << 256) // p
            elif kind == "kaliski":
                ok = kaliski_rounds(a, p) == v
            elif kind == "identity-operand":
                ok = xyzz_value(c.ops[:4]) is None or xyzz_value(c.ops[4:]) is None
            elif kind == "P+P":
                ok = xyzz_value(c.ops[:4]) == xyzz_value(c.ops[4:]) is not None and (c.ops[:4] != c.ops[4:]) == v
            elif kind == "P-P":
                P, T = xyzz_value(c.ops[:4]), xyzz_value(c.ops[4:])
                ok = P is not None and T == g1_neg(P) and c.ops[2] != c.ops[6]
            elif kind in ("madd-same", "madd-opp"):
                acc, qa = xyzz_value(c.ops[:4]), tuple(x * pow(RM, -1, Q) % Q for x in c.ops[4:6])
                q_signed = g1_neg(qa) if c.flag else qa
                ok = acc == (q_signed if kind == "madd-same" else g1_neg(q_signed)) and c.ops[2] != mont(1)
            else:
                raise AssertionError(kind)
            assert ok, "%s[%s] case %s is not what it is named (%s)" % (op, field, c.describe(), c.claim)
    # the Kaliski extremes: n = 254 rounds is the least possible, 2n = 508 the most; the longest case is within one of it
    for p in FIELDS.values():
        assert min(kaliski_rounds(1 << j, p) for j in range(254)) == 254 == kaliski_rounds(1, p)
    for key in [("fp_add", "sum"), ("fp_sub", "diff"), ("fp_mul", "pre"), ("fp_mul", "ones"), ("fp_sqr", "ones"), ("fp_mul2", "ones"),
                ("fp_mul_wide", "ones"), ("fp_mul_const", "short"), ("fp_to_mont", "ones"), ("fp_lazy_red2p", "range"),
                ("fp_lazy_add", "sum"), ("fp_lazy_sub_red", "diff"), ("fp_inv", "kaliski"), ("xyzz_add", "P+P"), ("xyzz_add", "P-P"),
                ("xyzz_madd", "madd-same"), ("xyzz_madd", "madd-opp"), ("xyzz_add", "identity-operand")]:
        assert seen.get(key, 0) > 0, key


def test_batch_layout():
    """no batch fills whole waves; every wave of the scalar batches mixes branches; neighbouring quads take different
    branches; fp_inv runs once with whole waves holding one value"""
    for op, field, layout, cases in all_batches():
        lanes = 4 if layout == "quad" else 1
        assert len(cases) % WAVE and (len(cases) * lanes) % WAVE, (op, field, len(cases))
        if op.startswith("xyzz_") and op != "xyzz_double_affine":        # (which has no branch)
            per_wave = WAVE // lanes
            for w in range(0, len(cases) - 1, per_wave):
                assert len({c.kind for c in cases[w:w + per_wave]}) > 1, (op, w)
            if layout == "quad" or op == "xyzz_add":
                assert all(a.kind != b.kind for a, b in zip(cases, cases[1:])), op
        elif layout == "uniform":
            full = len(cases) // WAVE * WAVE
            assert all(len({c.ops for c in cases[w:w + WAVE]}) == 1 for w in range(0, len(cases), WAVE))
            assert len({c.ops for c in cases[:full:WAVE]}) == full // WAVE
        else:
            waves = [cases[w:w + WAVE] for w in range(0, len(cases), WAVE)]
            assert all(len({c.ops for c in wv}) > 1 for wv in waves if len(wv) > 1), (op, field)
    assert {(op, f, lay) for op, f, lay, _ in all_batches() if op == "fp_inv"} == {("fp_inv", f, lay) for f in FIELDS for lay in ("mixed", "uniform")}


@pytest.fixture(scope="module")
def host_results(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("arith_host"))
    return run_build(compile_build("host", d, timeout=120), "host", d, timeout=120)


@pytest.mark.parametrize("op,field", PRIMS, ids=IDS)
def test_host_build(host_results, op, field):
    bad = failures(op, field, host_results)
    assert not bad, "\n".join(bad)


@pytest.fixture(scope="module")
def device_results(tmp_path_factory):
    """both device builds, compiled side by side, each run once over every batch"""
    d = str(tmp_path_factory.mktemp("arith_device"))
    builds = ["gfx950", "gfx950-portable"]
    with concurrent.futures.ThreadPoolExecutor(2) as pool:
        exes = dict(zip(builds, pool.map(lambda b: compile_build(b, d, timeout=240), builds)))
    return {b: run_build(exes[b], b, d, timeout=180) for b in builds}


DEVICE_PARAMS = [(b, op, f) for b in ("gfx950", "gfx950-portable") for op, f in PRIMS + QUAD_PRIMS]


@pytest.mark.gpu
@pytest.mark.parametrize("build,op,field", DEVICE_PARAMS, ids=["%s-%s-%s" % p for p in DEVICE_PARAMS])
def test_device_build(device_results, build, op, field):
    res = device_results[build]
    bad = failures(op, field, res, scalar_results=res)
    assert not bad, "\n".join(bad)
