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

The arithmetic of the fixed NTT pass (k_ntt_pass8) is here primitive by primitive as well, since whole transforms of random
data reach its corners about once in 2^30 products: fp_mul_chunk<2> (both fields), fp_mul_chunk_planes<AH> with the entry's
words in vector registers and in scalar registers (Fr, AH = 1 and 2; the scalar form in the device builds only, one entry per
wave read through the constant address space, every lane its own x), fp_chunk_table<1> and <2> word for word,
fp_lazy_sub_off<1> and <4> (fp_lazy_sub_from4p), fp_lazy_first_pair_of in its three forms, fp_lazy_last_pair_loose_head and
_add, fp_chunk_handover<true> and <false> on four values, and jacobian_to_xyzz of the G1 folds.  A case of a chunk product
carries its whole table entry as free data (a wider record), and the expected value is the exact integer of field.hpp's
formula, r = (S + m p) / 2^(32 (CL + 1)) with S = sum X_k T_k and m = -S / p mod 2^(32 (CL + 1)), T_k read from the entry
as it stands; the pairs and the hand-over are the 256-bit integers of their formulas around it, all four outputs compared.
Their cases: x at 0, 1, p - 1, 2p - 1, 4p - 1, 5p + (p >> 29), 2^256 - 1 and the limb patterns, w at 1, -1 and powers of the
2^28-th root of unity, the entry at the bound of the schedule's column sums (which no w produces), at least 256 products per
form and field that come out AT OR ABOVE p (x w = v mod p for a small v gives v + p) and products below p whose top limb is
that of p -- what tells a hand-over that subtracts by the top limb from the right one; both ends of the ranges of the
subtractions, differences that borrow through all eight limbs or land on M p; every operand of a first pair at both ends
of its form's range, FIRST_PAIR_2P and _4P compared bit for bit on operands below 2p; the loose last pair's largest rows,
asserted below 2^256 before they are written; and for the hand-over whole waves that do not take its one branch, that take it
for one lane and one slot, and that take it on every lane with lanes below p next to lanes above.
"""
import concurrent.futures
import functools
import os
import random
import struct
import subprocess

import pytest

from ref_plonk import G1, Q, R as R_MOD, ROOT_OF_UNITY, g1_add, g1_mul, g1_neg

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
WIDE_IN_BYTES, WIDE_OUT_BYTES = 400, 256   # struct InW (four operands and a table entry) / struct OutW (a table entry)

FIELD_OPS = ["fp_add", "fp_sub", "fp_neg", "fp_dbl", "fp_reduce_once", "fp_mul", "fp_sqr", "fp_mul2", "fp_mul_wide",
             "fp_mul_const", "fp_const_pair", "fp_to_mont", "fp_from_mont", "fp_lazy_red2p", "fp_lazy_add", "fp_lazy_sub",
             "fp_lazy_add_red", "fp_lazy_sub_red", "fp_lazy_canon", "fp_inv", "fp_pow_u32"]
G1_OPS = ["xyzz_from_affine", "xyzz_madd", "xyzz_add", "xyzz_double", "xyzz_double_affine", "xyzz_mul_u32", "xyzz_to_jacobian"]
QUAD_OPS = {"xyzz_add_q": "xyzz_add", "xyzz_double_q": "xyzz_double", "xyzz_mul_u32_q": "xyzz_mul_u32"}  # -> its scalar twin
# the NTT's chunk products, lazy pairs and hand-over (both fields), the plane forms of the product (Fr; with the entry in scalar
# registers: device builds only, one entry per wave) and the G1 conversion of the folds
NTT_OPS = ["fp_mul_chunk2", "fp_chunk_table1", "fp_chunk_table2", "fp_lazy_sub_off1", "fp_lazy_sub_from4p", "fp_lazy_first_pair_2p",
           "fp_lazy_first_pair_4p", "fp_lazy_first_pair_canon", "fp_lazy_last_pair_loose_head", "fp_lazy_last_pair_loose_add",
           "fp_chunk_handover", "fp_chunk_handover_nobranch"]
PLANE_OPS = ["fp_mul_chunk_planes_ah1", "fp_mul_chunk_planes_ah2"]
SPLANE_OPS = ["fp_mul_chunk_splanes_ah1", "fp_mul_chunk_splanes_ah2"]
CHUNK_LIMBS = {"fp_mul_chunk2": 2, **{op: 1 for op in PLANE_OPS + SPLANE_OPS}}          # chunk product -> CL
FIRST_PAIR_OPS = {"fp_lazy_first_pair_2p": "2p", "fp_lazy_first_pair_4p": "4p", "fp_lazy_first_pair_canon": "canon"}
HANDOVER_OPS = ["fp_chunk_handover", "fp_chunk_handover_nobranch"]
WIDE_IN = set(CHUNK_LIMBS) | set(FIRST_PAIR_OPS)          # ops whose cases carry an entry (struct InW)
WIDE_OUT = {"fp_chunk_table1": 1, "fp_chunk_table2": 2}   # ops that write one (struct OutW) -> CL
MIN_OVER_P = 256                   # chunk products at or above p, per form and field


class Case:
    """one operand record: `ops` are the 256-bit operands v[0..7] as integers, `k` the 32-bit scalar, `flag` the negate flag;
    `claim` is what the case says it is, as (kind, value) -- checked by test_exceptional_cases_are_what_they_are_named;
    `tab` is the table entry of a chunk product, the residues T_k as integers, free data like the operands, and `w` the plain
    multiplier it tabulates, where it tabulates one"""
    __slots__ = ("label", "ops", "k", "flag", "claim", "kind", "tab", "w")

    def __init__(self, label, ops, k=0, flag=0, claim=None, kind="general", tab=(), w=None):
        self.label, self.ops, self.k, self.flag, self.claim, self.kind = label, tuple(ops), k, flag, claim, kind
        self.tab, self.w = tuple(tab), w

    def describe(self):
        ops = ", ".join("0x%x" % v for v in self.ops)
        extra = (" k=0x%x" % self.k if self.k else "") + (" negate" if self.flag else "")
        if self.tab:
            extra += " entry [%s]" % ", ".join("0x%x" % v for v in self.tab)
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


def landing(rnd, p, dom_bound, targets, sign, n_each=3, b_bound=None):
    """(a, b) below dom_bound (b below b_bound, where that is another) with a + b (sign +1) or a - b (sign -1) equal to each
    target exactly"""
    out = []
    b_bound = dom_bound if b_bound is None else b_bound
    for name, t in targets:
        lo, hi = (max(0, t - b_bound + 1), min(t, dom_bound - 1)) if sign > 0 else (max(0, t), min(dom_bound - 1, b_bound - 1 + t))
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


# ---- the NTT's chunk products, lazy pairs and hand-over: the exact integers of field.hpp's formulas --------------------------
M32 = 0xFFFFFFFF


def p_loose(p):
    """what a chunk product stays below: p (1 + 2^-29)"""
    return p + (p >> 29)


def top_of(p):
    """the least value whose top limb is MOD[7]"""
    return (p >> 224) << 224


def chunk_table(w, cl, p):
    """the entry of the plain multiplier w: T_k = w 2^(32 cl k + 32 (cl + 1)) mod p"""
    return tuple(w * (1 << (32 * cl * k + 32 * (cl + 1))) % p for k in range(8 // cl))


def chunk_bound_entry(cl, p):
    """the entry the schedule's column bounds are taken at: every limb 2^32 - 1, the top limb that of p - 1; no w gives it"""
    return ((((p - 1) >> 224) << 224) | ((1 << 224) - 1),) * (8 // cl)


def entry_words(tab, cl):
    """the entry as FpChunk<cl> holds it, limb-major: w[l (8 / cl) + k] = limb l of T_k"""
    return [(t >> (32 * limb)) & M32 for limb in range(8) for t in tab]


def chunk_exact(x, tab, cl, p):
    """fp_mul_chunk<cl> bit for bit: S = sum X_k T_k over the chunks X_k of cl limbs, r = (S + m p) / 2^(32 (cl + 1)) with
    m = -S p^-1 mod 2^(32 (cl + 1)); T_k as the entry holds it"""
    bits = 32 * cl
    assert len(tab) == 8 // cl and 0 <= x < RM
    s = sum(((x >> (bits * k)) & ((1 << bits) - 1)) * t for k, t in enumerate(tab))
    rk = 1 << (bits + 32)
    m = -s * pow(p, -1, rk) % rk
    assert (s + m * p) % rk == 0
    return (s + m * p) >> (bits + 32)


def twiddles(p):
    """1, -1 and powers of the 2^28-th root of unity; Fq has none (q - 1 = 2 (odd)), there powers of 3 stand in"""
    if p == R_MOD:
        assert pow(ROOT_OF_UNITY, 1 << 27, p) == p - 1
        pw = [pow(ROOT_OF_UNITY, e, p) for e in (1, 2, 3, 1 << 13, (1 << 13) + 1, 1 << 26, 3 << 26, (1 << 27) + 1, (1 << 28) - 1)]
    else:
        pw = [pow(3, e, p) for e in (1, 2, 3, 1 << 13, (1 << 13) + 1, 1 << 26, 3 << 26, (1 << 27) + 1, (p - 1) // 2 - 1)]
    return [1, p - 1] + pw


def chunk_x_edges(p):
    out = []
    for x in [0, 1, p - 1, 2 * p - 1, 4 * p - 1, 5 * p + (p >> 29), RM - 1] + patterns():
        if x not in out:
            out.append(x)
    return out


def chunk_special(rnd, p, cl, w, kind, i):
    """x with x w = v ("over-p": the exact product is v + p) or = p - v ("top-below-p": the top limb of p on a value below
    p) for a small positive v, in the i-th of the representatives x0 + j p below 2^256.  (An x so small that S itself is
    v 2^(32 (cl + 1)), such as x = v for w = 1, gives v and not v + p: drawn again)"""
    tab = chunk_table(w, cl, p)
    while True:
        v = rnd.randrange(1, 1 << 200)
        x0 = (v if kind == "over-p" else p - v) * pow(w, -1, p) % p
        x = x0 + i % ((RM - 1 - x0) // p + 1) * p
        if kind != "over-p" or chunk_exact(x, tab, cl, p) >= p:
            return Case(kind, (x,), tab=tab, w=w, claim=(kind, v))
        i += 1


def chunk_random(rnd, p, cl, x=None):
    """a random x with a random twiddle's entry, or (one in four) with an entry of free limbs within the schedule's bound"""
    x = rand_in(rnd, "256", p) if x is None else x
    if rnd.random() < 0.25:
        return Case("random, free entry", (x,), tab=tuple(rnd.randrange(top_of(p) + (1 << 224)) for _ in range(8 // cl)))
    w = rnd.randrange(p)
    return Case("random", (x,), tab=chunk_table(w, cl, p), w=w)


def finish(C, rc, rnd):
    cases = C + rc
    rnd.shuffle(cases)                           # every wave mixes edge, exceptional and random cases
    if len(cases) % WAVE == 0:
        cases.append(rc[0])
    return cases


def build_chunk_cases(p, rnd, cl):
    W, X = twiddles(p), chunk_x_edges(p)
    C = [Case("edge", (x,), tab=chunk_table(w, cl, p), w=w) for x in X for w in W]
    C += [Case("entry-bound", (x,), tab=chunk_bound_entry(cl, p), claim=("entry-bound", cl)) for x in X]
    ws = W + [rnd.randrange(1, p) for _ in range(8)]
    C += [chunk_special(rnd, p, cl, ws[i % len(ws)], "over-p", i) for i in range(MIN_OVER_P + 32)]
    C += [chunk_special(rnd, p, cl, ws[i % len(ws)], "top-below-p", i) for i in range(64)]
    return finish(C, [chunk_random(rnd, p, cl) for _ in range(N_RANDOM)], rnd)


def build_splane_cases(p, rnd):
    """the chunk product with its entry in scalar registers: every wave holds ONE entry, another in every wave, and 64
    different x -- the twiddle waves mix edge operands, products at or above p and random ones"""
    cl, X = 1, chunk_x_edges(p)
    tw = twiddles(p)
    while len(tw) < 48:
        w = pow(ROOT_OF_UNITY, rnd.randrange(1 << 28), p)
        if w not in tw:
            tw.append(w)

    def wave(tab, w, lanes, size=WAVE):
        xs = {c.ops: c for c in lanes}
        while len(xs) < size:
            x = rand_in(rnd, "256", p)
            xs.setdefault((x,), Case("random", (x,), tab=tab, w=w))
        out = list(xs.values())[:size]
        rnd.shuffle(out)
        return out

    cases = []
    for i, w in enumerate(tw):
        tab = chunk_table(w, cl, p)
        lanes = [chunk_special(rnd, p, cl, w, "over-p", 10 * i + j) for j in range(10)]
        lanes += [chunk_special(rnd, p, cl, w, "top-below-p", 2 * i + j) for j in range(2)]
        lanes += [Case("edge", (X[(16 * i + j) % len(X)],), tab=tab, w=w) for j in range(16)]
        cases += wave(tab, w, lanes)
    bound = chunk_bound_entry(cl, p)
    cases += wave(bound, None, [Case("entry-bound", (x,), tab=bound, claim=("entry-bound", cl)) for x in X])
    for i in range(N_RANDOM // WAVE + 1):         # the random cases: a random twiddle's entry or a free one per wave
        c = chunk_random(rnd, p, cl)
        cases += wave(c.tab, c.w, [c], size=WAVE if i else 37)   # (the partial wave is the last one below)
    return cases[WAVE * len(tw) + WAVE + 37:] + cases[:WAVE * len(tw) + WAVE + 37]


def count_borrows(a, b):
    """how many of the eight limb subtractions of a - b borrow"""
    n = bw = 0
    for i in range(8):
        bw = 1 if ((a >> (32 * i)) & M32) - ((b >> (32 * i)) & M32) - bw < 0 else 0
        n += bw
    return n


def build_sub_off_cases(op, p, rnd):
    """fp_lazy_sub_off<1> over the two ranges it is used at (canonical operands: the first pair; a below 4p and b a product:
    the loose last pair) and fp_lazy_sub_off<4> (fp_lazy_sub_from4p: a a product, b a row below 4p)"""
    pools, pl = field_pools(p), p_loose(p)
    small = [0, 5, M32 - 1, 1 << 32, (7 << 224) | 3]                                          # a + 1 carries into no limb
    C = [Case("borrow-all", (a, a + 1), claim=("borrows", 8)) for a in small]                 # the difference is -1
    C += [Case("borrow-7", (t << 224, 1), claim=("borrows", 7)) for t in (1, 2, p >> 224)]
    if op == "fp_lazy_sub_off1":
        C += pairs(pools["canon"], pools["canon"])
        C += landing(rnd, p, p, [("0", 0), ("-1", -1), ("1", 1), ("-(p-1)", -(p - 1)), ("p-1", p - 1)], -1)   # 0 lands on p
        C += landing(rnd, p, 4 * p, [("4p-1", 4 * p - 1), ("p", p), ("3p", 3 * p), ("-(p-1)", -(p - 1)), ("0", 0)], -1, b_bound=pl)
        rc = [Case("random", (rnd.randrange(p), rnd.randrange(p))) for _ in range(N_RANDOM)]
        rc += [Case("random", (rnd.randrange(p, 4 * p), rnd.randrange(pl))) for _ in range(N_RANDOM // 4)]
    else:
        pa = [v for v in pools["2p"] if v < pl] + [pl - 1, pl - 2]
        C += pairs(pa, pools["4p"])
        C += landing(rnd, p, pl, [("0", 0), ("-1", -1), ("1", 1), ("-(4p-1)", -(4 * p - 1)), ("p+(p>>29)-1", pl - 1), ("-p", -p),
                                  ("-2p", -2 * p), ("-3p", -3 * p)], -1, b_bound=4 * p)                       # 0 lands on 4p
        rc = [Case("random", (pl - 1 - rnd.randrange(1 << 64) if rnd.random() < 0.25 else rnd.randrange(pl), rand_in(rnd, "4p", p)))
              for _ in range(N_RANDOM)]
    m = 1 if op == "fp_lazy_sub_off1" else 4
    for c in C + rc:
        assert 0 < c.ops[0] - c.ops[1] + m * p < RM, c.describe()          # the contract: b < a + M p, the result below 2^256
    return finish(C, rc, rnd)


def lazy_red2p(a, p):
    return a - 2 * p if a >= 2 * p else a


def first_pair_exact(form, ops, tab, p):
    """fp_lazy_first_pair_of<2>: the four 256-bit results, with y3 the chunk product of x2 - x3 + 2p"""
    x0, x1, x2, x3 = ops
    if form == "canon":
        y0, y1, y2 = x0 + x1, x0 - x1 + p, x2 + x3
    else:
        if form == "4p":
            x0, x1, x2, x3 = (lazy_red2p(v, p) for v in ops)
        y0, y1, y2 = lazy_red2p(x0 + x1, p), x0 - x1 + (0 if x0 >= x1 else 2 * p), lazy_red2p(x2 + x3, p)
    y3 = chunk_exact(x2 - x3 + 2 * p, tab, 2, p)
    return y0 + y2, y1 + y3, y0 - y2 + 2 * p, y1 - y3 + 2 * p


def first_pair_cases(form, p, rnd):
    b = BOUND[form](p)
    edges = [v for v in field_pools(p)["4p"] if v < b]

    def case(label, ops, tab, w, claim=None):
        assert all(0 <= v < b for v in ops) and all(0 <= v < RM for v in first_pair_exact(form, ops, tab, p)), (label, ops)
        return Case(label, ops, tab=tab, w=w, claim=claim)

    def r():
        return rand_in(rnd, form, p)

    tabs = [(chunk_table(w, 2, p), w) for w in twiddles(p)] + [(chunk_bound_entry(2, p), None)]
    C = []
    for tab, w in tabs[:4] + tabs[-1:]:                                        # every operand at both ends of the form's range
        for m in range(16):
            C.append(case("ends", tuple((b - 1) if m >> i & 1 else 0 for i in range(4)), tab, w))
    for i in range(32):
        tab, w = tabs[i % len(tabs)]
        x = [0, b - 1, r()][i % 3]
        C.append(case("x2=x3", (r(), r(), x, x), tab, w, claim=("x2-x3", 0)))
        C.append(case("x2-x3 at its maximum", (r(), r(), b - 1, 0), tab, w, claim=("x2-x3", b - 1)))
    for i in range(256):
        tab, w = tabs[i % len(tabs)]
        C.append(case("edge", tuple(rnd.choice(edges) for _ in range(4)), tab, w))
    rc = []
    for _ in range(N_RANDOM):
        w = rnd.randrange(p)
        rc.append(case("random", (r(), r(), r(), r()), chunk_table(w, 2, p), w))
    return C, rc


def first_pair_batches(p, rnd):
    """the three forms; FIRST_PAIR_4P runs every case of FIRST_PAIR_2P too: operands that ARE below 2p give the same 256-bit
    values in both forms (field.hpp)"""
    c2, r2 = first_pair_cases("2p", p, rnd)
    c4, r4 = first_pair_cases("4p", p, rnd)
    cc, rcn = first_pair_cases("canon", p, rnd)
    return {"fp_lazy_first_pair_2p": finish(list(c2), list(r2), rnd), "fp_lazy_first_pair_4p": finish(c2 + c4, r2 + r4, rnd),
            "fp_lazy_first_pair_canon": finish(cc, rcn, rnd)}


def loose_pair_cases(op, p, rnd):
    """the loose last pair: x0 below 2p, the products x1', y2 and n3 below p (1 + 2^-29); _add takes what _head made of x0, x1'"""
    pl = p_loose(p)
    xs, prods = [0, 1, p, 2 * p - 1], [0, 1, p - 1, p, pl - 1]

    def case(label, x0, x1, y2, n3, claim=None):
        assert 0 <= x0 < 2 * p and all(0 <= v < pl for v in (x1, y2, n3))
        y0, y1 = x0 + x1, x0 - x1 + 2 * p
        if op == "fp_lazy_last_pair_loose_head":
            assert 0 <= y0 < RM and 0 <= y1 < RM
            return Case(label, (x0, x1), claim=claim)
        assert all(0 <= v < RM for v in (y0 + y2, y1 - n3 + p, y0 - y2 + 2 * p, y1 + n3)), (label, x0, x1, y2, n3)
        return Case(label, (y0, y1, y2, n3), claim=claim)

    if op == "fp_lazy_last_pair_loose_head":
        C = [case("edge", x0, x1, 0, 0, claim=None if x0 != 2 * p - 1 else ("sum", 2 * p + pl - 2) if x1 == pl - 1 else ("value", x0))
             for x0 in xs for x1 in prods]
        rc = [case("random", rand_in(rnd, "2p", p), rnd.randrange(pl), 0, 0) for _ in range(N_RANDOM)]
    else:
        C = [case("edge", x0, x1, y2, n3) for x0 in xs for x1 in prods for y2 in prods for n3 in prods]
        # the largest rows: y0 + y2 with x1' at its maximum, y1 + n3 with x1' = 0
        C += [case("largest outputs", 2 * p - 1, x1, pl - 1, pl - 1, claim=("largest", 2 * p - 1 + x1 + pl - 1)) for x1 in (0, pl - 1)]
        rc = [case("random", rand_in(rnd, "2p", p), rnd.randrange(pl), rnd.randrange(pl),
                   rnd.randrange(pl) if rnd.random() < 0.75 else pl - 1 - rnd.randrange(1 << 64)) for _ in range(N_RANDOM)]
    return finish(C, rc, rnd)


def handover_wave_kind(wave, p):
    """(lanes with a value at or above MOD[7] << 224, such values, lanes with a value at or above p)"""
    hot = [sum(1 for v in c.ops if v >= top_of(p)) for c in wave]
    return sum(1 for h in hot if h), sum(hot), sum(1 for c in wave if any(v >= p for v in c.ops))


def handover_cases(p, rnd):
    """fp_chunk_handover on four values per lane (N = 4): below MOD[7] << 224 (no lane of such a wave takes the branch), with the
    top limb of p but below p (the branch is taken and the value comes back as it is), and p, p + v, p (1 + 2^-29) - 1.  The
    first waves are laid out whole: none taken, one lane and one slot, every lane"""
    top, pl = top_of(p), p_loose(p)

    def below():
        return top - 1 - rnd.randrange(1 << 64) if rnd.random() < 0.1 else rnd.randrange(top)

    def special(i):
        return [p, pl - 1, p + 1, top, p - 1, p + rnd.randrange(1, p >> 29), top + rnd.randrange(p - top)][i % 7]

    def lane(values=(), label="random"):
        """the given values at slots drawn at random, values below MOD[7] << 224 in the others"""
        ops = [below() for _ in range(4)]
        for v, s in zip(values, rnd.sample(range(4), len(values))):
            ops[s] = v
        return Case(label, ops)

    def claimed(v, kind):
        ops = [v] + [below() for _ in range(3)]
        return Case(kind, ops, claim=("value", v) if kind == "exactly p" else (kind, 0))

    cases = [lane() for _ in range(2 * WAVE)]                                             # two waves that do not take the branch
    for v in (p, top + rnd.randrange(p - top)):                                           # one lane, one slot: above p / below p
        w = [lane() for _ in range(WAVE)]
        w[rnd.randrange(WAVE)] = lane((v,), "one lane")
        cases += w
    for k in range(2):                                                                    # every lane, below and above p mixed
        cases += [lane([top + rnd.randrange(p - top)] if i % 3 == k else [special(i + j) for j in range(1 + i % 4)], "every lane")
                  for i in range(WAVE)]
    C = [claimed(p, "exactly p") for _ in range(8)] + [claimed(top + rnd.randrange(p - top), "top-limb-below-p") for _ in range(32)]
    C += [claimed(v, "top-limb-below-p") for v in (top, p - 1)]
    C += [lane([special(i + j) for j in range(1 + i % 4)], "edge") for i in range(200)]
    return cases + finish(C, [lane() for _ in range(N_RANDOM)], rnd)


def build_ntt_cases(op, p, rnd):
    if op == "fp_mul_chunk2":
        return build_chunk_cases(p, rnd, 2)
    if op in WIDE_OUT:
        ws = field_pools(p)["canon"] + [w * RM % p for w in twiddles(p)]
        return finish([Case("edge", (w,)) for w in ws], [Case("random", (rnd.randrange(p),)) for _ in range(N_RANDOM // 4)], rnd)
    if op in ("fp_lazy_sub_off1", "fp_lazy_sub_from4p"):
        return build_sub_off_cases(op, p, rnd)
    return loose_pair_cases(op, p, rnd)


def build_jacobian_cases(rnd):
    """jacobian_to_xyzz: (x z^2, y z^3, z) with z = 1 and generic, the identity (z = 0) and y = 0, as they stand"""
    pts = [G1] + [g1_mul(G1, rnd.randrange(1, R_MOD)) for _ in range(7)]
    cases = []
    for i in range(90):
        (x, y), z = pts[i % len(pts)], 1 if i % 5 == 0 else rnd.randrange(2, Q)
        X, Y = x * z * z % Q, y * z * z * z % Q
        kind = ["P", "identity", "y=0"][i % 3]
        ops = {"P": (X, Y, z), "identity": [(0, 1, 0), (X, Y, 0), (5, 7, 0)][i // 3 % 3], "y=0": (X, 0, z)}[kind]
        cases.append(Case(kind, tuple(mont(v) for v in ops), kind=kind, claim=("jacobian-z", 1) if z == 1 and kind == "P" else None))
    return cases + cases[:11]


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
    # (the NTT's primitives come last, so that the cases above are those they were before these existed)
    for field, p in FIELDS.items():
        first_pair, handover = first_pair_batches(p, rnd), handover_cases(p, rnd)      # (the two hand-overs run the same cases)
        for op in NTT_OPS:
            cases = first_pair[op] if op in FIRST_PAIR_OPS else handover if op in HANDOVER_OPS else build_ntt_cases(op, p, rnd)
            batches.append((op, field, "mixed", cases))
    for op in PLANE_OPS:
        batches.append((op, "Fr", "mixed", build_chunk_cases(R_MOD, rnd, 1)))
    for op in SPLANE_OPS:
        batches.append((op, "Fr", "wave-entry", build_splane_cases(R_MOD, rnd)))
    batches.append(("jacobian_to_xyzz", "Fq", "mixed", build_jacobian_cases(rnd)))
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

    def exact_all(want):
        want = tuple(want)
        want += (0,) * (len(r) - len(want))
        return None if tuple(r) == want else "(%s)" % ", ".join("0x%x" % v for v in want)

    if op in CHUNK_LIMBS:
        return exact(chunk_exact(a, c.tab, CHUNK_LIMBS[op], p))
    if op in WIDE_OUT:                               # the entry word for word, eight words to a 256-bit result
        words = entry_words(chunk_table(a * ri % p, WIDE_OUT[op], p), WIDE_OUT[op])
        return exact_all(sum(w << (32 * j) for j, w in enumerate(words[i:i + 8])) for i in range(0, len(words), 8))
    if op == "fp_lazy_sub_off1":
        return exact(a - b + p)
    if op == "fp_lazy_sub_from4p":
        return exact(a - b + 4 * p)
    if op in FIRST_PAIR_OPS:
        return exact_all(first_pair_exact(FIRST_PAIR_OPS[op], c.ops, c.tab, p))
    if op == "fp_lazy_last_pair_loose_head":
        return exact_all((a + b, a - b + 2 * p))
    if op == "fp_lazy_last_pair_loose_add":
        y0, y1, y2, n3 = c.ops
        return exact_all((y0 + y2, y1 - n3 + p, y0 - y2 + 2 * p, y1 + n3))
    if op in HANDOVER_OPS:
        return exact_all(v - p if v >= p else v for v in c.ops)
    if op == "jacobian_to_xyzz":
        z = c.ops[2] * ri % p
        return exact_all((c.ops[0], c.ops[1], z * z * RM % p, z * z * z * RM % p))
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
    return [b for b in all_batches() if build != "host" or b[2] not in ("quad", "wave-entry")]


def in_bytes(op):
    return WIDE_IN_BYTES if op in WIDE_IN else IN_BYTES


def out_bytes(op):
    return WIDE_OUT_BYTES if op in WIDE_OUT else OUT_BYTES


def encode(batches):
    buf = bytearray(b"ACF2" + struct.pack("<I", len(batches)))
    for op, field, _, cases in batches:
        buf += op.encode().ljust(32, b"\0") + struct.pack("<II", FIELD_ID[field], len(cases))
        for c in cases:
            if op in WIDE_IN:             # four operands and the entry's words (FpChunk<2>: the first 32 of the 64)
                cl = CHUNK_LIMBS.get(op, 2)
                words = entry_words(c.tab, cl)
                assert len(c.ops) <= 4 and len(c.tab) == 8 // cl and len(words) == 64 // cl
                ops = c.ops + (0,) * (4 - len(c.ops))
                buf += b"".join(v.to_bytes(32, "little") for v in ops) + struct.pack("<64I", *words + [0] * (64 - len(words)))
            else:
                assert not c.tab
                ops = c.ops + (0,) * (8 - len(c.ops))
                buf += b"".join(v.to_bytes(32, "little") for v in ops)
            buf += struct.pack("<4I", c.k, c.flag, 0, 0)
    assert len(buf) == 8 + sum(40 + in_bytes(b[0]) * len(b[3]) for b in batches)
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
    assert data[:4] == b"ACF2" and struct.unpack_from("<I", data, 4)[0] == len(batches)
    pos, results = 8, {}
    for op, field, layout, cases in batches:
        name = data[pos:pos + 32].rstrip(b"\0").decode()
        fid, n_out = struct.unpack_from("<II", data, pos + 32)
        pos += 40
        lanes = 4 if layout == "quad" else 1
        ob = out_bytes(op)
        assert (name, fid) == (op, FIELD_ID[field]), (name, fid, op, field)
        assert n_out == len(cases) * lanes, "%s[%s]: %d results for %d cases x %d lanes" % (op, field, n_out, len(cases), lanes)
        rec = data[pos:pos + n_out * ob]
        assert len(rec) == n_out * ob, "%s[%s]: truncated output" % (op, field)
        pos += n_out * ob
        outs = [tuple(int.from_bytes(rec[i * ob + 32 * j:i * ob + 32 * (j + 1)], "little") for j in range(ob // 32))
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
        same_in_2p = {}
        if op == "fp_lazy_first_pair_4p":          # its cases below 2p are FIRST_PAIR_2P's: the same 256-bit values in both forms
            _, cases_2p, outs_2p = results[("fp_lazy_first_pair_2p", field)][0]
            same_in_2p = {(c.ops, c.tab): r for c, r in zip(cases_2p, outs_2p)}
            assert sum(1 for c in cases if (c.ops, c.tab) in same_in_2p) >= len(same_in_2p) > N_RANDOM
        memo = {}
        for i, c in enumerate(cases):
            for lane in range(lanes):
                r = outs[i * lanes + lane]
                if op.startswith("fp_") or op == "jacobian_to_xyzz":
                    want = check_field(op, FIELDS[field], c, r)
                    if want is None and same_in_2p.get((c.ops, c.tab), r) != r:
                        want = "what FIRST_PAIR_2P gives (%s)" % ", ".join("0x%x" % v for v in same_in_2p[(c.ops, c.tab)])
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
PRIMS += [(op, f) for op in NTT_OPS for f in FIELDS] + [(op, "Fr") for op in PLANE_OPS] + [("jacobian_to_xyzz", "Fq")]
DEVICE_ONLY_PRIMS = [(op, "Fq") for op in QUAD_OPS] + [(op, "Fr") for op in SPLANE_OPS]   # the device builds only
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
            seen[(op, field, kind)] = seen.get((op, field, kind), 0) + 1
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
            elif kind in ("over-p", "top-below-p"):
                # the exact product of a twiddle's entry: at or above p (the hand-over's subtraction is needed), or below p with
                # the top limb of p (a test of the top limb alone would subtract)
                cl = CHUNK_LIMBS[op]
                r = chunk_exact(a, c.tab, cl, p)
                ok = 0 < v < 1 << 200 and c.tab == chunk_table(c.w, cl, p) and r < p_loose(p)
                ok = ok and (r == v + p if kind == "over-p" else r == p - v and r >> 224 == p >> 224)
            elif kind == "entry-bound":
                words = entry_words(c.tab, v)
                ok = v == CHUNK_LIMBS[op] and len(words) == 64 // v and all(w == M32 for w in words[:56 // v])
                ok = ok and all(w == (p - 1) >> 224 for w in words[56 // v:])
            elif kind == "borrows":
                ok = count_borrows(a, c.ops[1]) == v
            elif kind == "x2-x3":
                form = FIRST_PAIR_OPS[op]           # (FIRST_PAIR_4P runs FIRST_PAIR_2P's cases too)
                ok = c.ops[2] - c.ops[3] == v and v in (0, BOUND[form](p) - 1, 2 * p - 1 if form == "4p" else 0)
            elif kind == "largest":
                y0, y1, y2, n3 = c.ops
                ok = y0 + y2 == v and y2 == n3 == p_loose(p) - 1 and y0 + y1 == 2 * (2 * p - 1) + 2 * p and max(v, y1 + n3) < RM
            elif kind == "top-limb-below-p":
                ok = a >> 224 == p >> 224 and a < p
            elif kind == "jacobian-z":
                ok = c.ops[2] == mont(v)
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
    # the NTT's primitives, per field: every form of the chunk product has its products at or above p
    forms = [(op, f) for op in CHUNK_LIMBS for f in (FIELDS if op == "fp_mul_chunk2" else ["Fr"])]
    assert len(forms) == 6
    for op, f in forms:
        assert seen.get((op, f, "over-p"), 0) >= MIN_OVER_P and seen.get((op, f, "top-below-p"), 0) >= 64, (op, f)
        assert seen.get((op, f, "entry-bound"), 0) >= len(chunk_x_edges(FIELDS[f])) >= 7 + 24, (op, f)
    for f in FIELDS:
        for op, kind, least in [("fp_lazy_sub_off1", "diff", 30), ("fp_lazy_sub_from4p", "diff", 24), ("fp_lazy_sub_off1", "borrows", 8),
                                ("fp_lazy_sub_from4p", "borrows", 8), ("fp_lazy_last_pair_loose_head", "value", 4),
                                ("fp_lazy_last_pair_loose_head", "sum", 1), ("fp_lazy_last_pair_loose_add", "largest", 2),
                                ("fp_chunk_handover", "value", 8), ("fp_chunk_handover", "top-limb-below-p", 34),
                                ("fp_chunk_handover_nobranch", "value", 8), ("fp_chunk_handover_nobranch", "top-limb-below-p", 34)]:
            assert seen.get((op, f, kind), 0) >= least, (op, f, kind)
        for op in FIRST_PAIR_OPS:
            assert seen.get((op, f, "x2-x3"), 0) >= 64, (op, f)
    assert seen.get(("jacobian_to_xyzz", "jacobian-z"), 0) > 0


def test_chunk_products_are_within_their_contract():
    """the exact formula itself, on every chunk-product case: the result is below 2^256; congruent to x w where the entry is
    a twiddle's; below p (1 + 2^-29) where every T_k is below p or the entry is at its bound; FIRST_PAIR_2P and _4P agree on
    operands below 2p; and the builders are deterministic"""
    n_same = 0
    for op, field, _, cases in all_batches():
        p = FIELDS[field]
        for c in cases:
            if op in CHUNK_LIMBS:
                cl, x = CHUNK_LIMBS[op], c.ops[0]
                r = chunk_exact(x, c.tab, cl, p)
                assert r < RM, c.describe()
                if c.w is not None:
                    assert c.tab == chunk_table(c.w, cl, p) and r % p == x * c.w % p, c.describe()
                if all(t < p for t in c.tab) or c.tab == chunk_bound_entry(cl, p):
                    assert r < p_loose(p), c.describe()
            elif op == "fp_lazy_first_pair_4p" and all(v < 2 * p for v in c.ops):
                assert first_pair_exact("4p", c.ops, c.tab, p) == first_pair_exact("2p", c.ops, c.tab, p)
                n_same += 1
    assert n_same > 2 * N_RANDOM
    assert encode(all_batches.__wrapped__()) == encode(all_batches())


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
        elif layout == "wave-entry":
            # the entry in scalar registers: one entry per wave, another in every wave, x different in every lane -- and the
            # products at or above p spread over many waves, next to lanes that stay below
            waves = [cases[w:w + WAVE] for w in range(0, len(cases), WAVE)]
            assert all(len({c.tab for c in wv}) == 1 and len({c.ops for c in wv}) == len(wv) for wv in waves), (op, field)
            assert len({wv[0].tab for wv in waves}) == len(waves) > 64
            over = [sum(1 for c in wv if c.claim and c.claim[0] == "over-p") for wv in waves]
            assert sum(1 for n in over if 0 < n < WAVE // 2) >= 32 and 0 in over
        else:
            waves = [cases[w:w + WAVE] for w in range(0, len(cases), WAVE)]
            assert all(len({c.ops for c in wv}) > 1 for wv in waves if len(wv) > 1), (op, field)
            if op in CHUNK_LIMBS or op in FIRST_PAIR_OPS:
                assert all(len({c.tab for c in wv}) > 1 for wv in waves if len(wv) > 1), (op, field)
            if op in HANDOVER_OPS:
                # whole waves of fp_chunk_handover<true>'s one branch: not taken; taken for one lane and one slot (a value at or
                # above p, and one that only has p's top limb); taken by every lane, with lanes below p next to lanes above
                p = FIELDS[field]
                kinds = [handover_wave_kind(wv, p) for wv in waves if len(wv) == WAVE]
                assert kinds.count((0, 0, 0)) >= 2 and (1, 1, 1) in kinds and (1, 1, 0) in kinds, (op, field)
                assert sum(1 for hot, _, above in kinds if hot == WAVE and WAVE // 4 < above < WAVE) >= 2, (op, field)
                assert sum(1 for hot, _, _ in kinds if 0 < hot < WAVE) > N_RANDOM // WAVE // 2, (op, field)
    first_pair, handover = {}, {}
    for op, f, _, cases in all_batches():
        if op in FIRST_PAIR_OPS:
            first_pair[(op, f)] = {(c.ops, c.tab) for c in cases}
        if op in HANDOVER_OPS:
            handover.setdefault(f, []).append(cases)
    for f in FIELDS:
        assert first_pair[("fp_lazy_first_pair_2p", f)] <= first_pair[("fp_lazy_first_pair_4p", f)]
        assert len(handover[f]) == 2 and handover[f][0] is handover[f][1]                 # <false> runs the cases of <true>
    assert {(op, f, lay) for op, f, lay, _ in all_batches() if lay == "wave-entry"} == {(op, "Fr", "wave-entry") for op in SPLANE_OPS}
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


DEVICE_PARAMS = [(b, op, f) for b in ("gfx950", "gfx950-portable") for op, f in PRIMS + DEVICE_ONLY_PRIMS]


@pytest.mark.gpu
@pytest.mark.parametrize("build,op,field", DEVICE_PARAMS, ids=["%s-%s-%s" % p for p in DEVICE_PARAMS])
def test_device_build(device_results, build, op, field):
    res = device_results[build]
    bad = failures(op, field, res, scalar_results=res)
    assert not bad, "\n".join(bad)
