"""The operand ranges of the fixed NTT pass (csrc/ntt_pass.hip k_ntt_pass8, csrc/field.hpp) with two more reductions left out:

  the stage pairs with twiddles (unit4_mul, every pass) take the row x2 as LDS holds it, strictly below 4p, next to the product
  x3' = x3 wa < p (1 + 2^-29): the sum x2 + x3' and the difference taken the other way round, x3' - x2 + 4p, are operands of
  products (any 256-bit value) and stay below 2^256 = 5.29 p; the second product is -y3 and unit4_add subtracts where it added;

  the first stage pair of a pass that loads the caller's data (fp_lazy_first_pair_canon) takes canonical residues, below p, and
  reduces nothing: bare sums below 2p, the difference x0 - x1 + p in (0, 2p).

Part 1 states the bounds as exact rationals and propagates exact-integer intervals (the model of
tests/test_ntt_lazy_bounds_host.py, whose operations assert what they rely on) through a whole pass from every entry bound: no
value reaches 2^256, 4p - x2 stays above zero, every row written to LDS is strictly below 4p.

Part 2 runs the portable bodies of field.hpp (tests/ntt_lazy_ranges_host.cpp, g++) on the end points -- 0, p - 1, 2p - 1, 4p - 1
for the rows, the products' largest value p + floor(p / 2^29) -- in every combination and on seeded random operands, against
the same arithmetic on Python integers: the same 256-bit values, and the butterflies' residues."""
import itertools
import os
import random
import struct
import subprocess
from fractions import Fraction

import pytest

from test_ntt_lazy_bounds_host import (M_CHUNK, OMEGA_28, P, TOP, Iv, add, add_red, canon, first_pair, hull, i_add, i_add_red,
                                       i_mul_chunk, i_red2p, i_sub, i_sub_red, mul_chunk, mul_wide, red2p, sub, sub_red)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ part 1: the bounds
def test_the_constants_the_ranges_rest_on():
    chunk = Fraction(P) * (1 + Fraction(1, 1 << 29))           # fp_mul_chunk: r < p (1 + 2^-29) ...
    assert chunk.denominator != 1 and M_CHUNK == chunk.numerator // chunk.denominator     # ... so r <= M_CHUNK, an integer
    assert Fraction(529, 100) < Fraction(TOP, P) < Fraction(530, 100)                     # 2^256 = 5.29 p
    assert 4 * P - 1 + chunk < TOP                             # x2 + x3': a bare 8-limb addition
    assert chunk + 4 * P < TOP                                 # x3' - x2 + 4p at x2 = 0
    assert 2 * P - 1 + chunk >= TOP - 4 * P                    # (why k_ntt_pass keeps its reduction: products below 2p, sum up to 6p)
    csrc = open(os.path.join(ROOT, "halo2-gpu-specific_amd", "csrc", "field.hpp")).read()
    fr = csrc[csrc.index("struct FrParams"):csrc.index("struct FqParams")]
    for name, mult in (("MOD", 1), ("MOD2", 2), ("MOD4", 4)):
        body = fr[fr.index("%s[8] = {" % name):]
        limbs = [int(v.strip().rstrip("u"), 16) for v in body[body.index("{") + 1:body.index("}")].split(",")]
        assert sum(v << (32 * i) for i, v in enumerate(limbs)) == mult * P, name


def sub_off(a, b, m):
    """fp_lazy_sub_off<m>: a - b + m p; strictly positive at its lowest and inside the 256 bits (Iv) at its highest"""
    assert a.lo - b.hi + m * P > 0, "a - b + %d p may wrap" % m
    return Iv(a.lo - b.hi + m * P, a.hi - b.lo + m * P)


def first_pair_canon(x):
    assert x.hi < P, "the canonical first pair takes residues below p"
    y0, y1, y2 = add(x, x), sub_off(x, x, 1), add(x, x)
    assert max(y0.hi, y1.hi, y2.hi) < 2 * P
    y3 = mul_chunk(sub(x, x))
    return hull(add(y0, y2), add(y1, y3), sub(y0, y2), sub(y1, y3))


def unit4(x, unit):
    """unit4_mul + unit4_add of k_ntt_pass8 on four rows with one bound, as they are now"""
    assert x.hi < 4 * P, "a row in LDS is strictly below 4p: 4p - x2 > 0"
    x0 = red2p(x)
    if unit:
        x1 = x2 = x3 = red2p(x)
        y2, n3 = red2p(add(x2, x3)), mul_chunk(sub(x3, x2))
    else:
        x1 = x3 = mul_chunk(x)
        s, n = add(x, x3), sub_off(x3, x, 4)          # x2 as loaded
        assert 4 * P - x.hi > 0 and s.hi < TOP and n.hi < TOP
        y2, n3 = mul_chunk(s), mul_chunk(n)
    y0, y1 = add_red(x0, x1), sub_red(x0, x1)
    return hull(add(y0, y2), sub(y1, n3), sub(y0, y2), add(y1, n3))


def pass_rows(rows):
    assert rows.hi < 4 * P
    for _ in (2, 4):                                  # the two rounds in LDS: unit twiddles for part of the lanes
        rows = hull(unit4(rows, True), unit4(rows, False))
        assert rows.hi < 4 * P, "a row in LDS may reach 4p"
    rows = unit4(rows, False)                         # the last stage pair: never a unit
    assert rows.hi < 4 * P
    return rows


ENTRIES = {
    "the caller's data, canonical": lambda: first_pair_canon(Iv(0, P - 1)),
    "the caller's data after pre3, reductions kept": lambda: first_pair(Iv(0, 4 * P - 1), True),
    "a store product": lambda: first_pair(Iv(0, M_CHUNK), False),
    "a load product": lambda: first_pair(Iv(0, 2 * P - 1), False),
}


@pytest.mark.parametrize("name", sorted(ENTRIES))
def test_a_pass_stays_strictly_below_4p_from_every_entry(name):
    rows = pass_rows(ENTRIES[name]())
    assert rows.hi < 4 * P < TOP
    assert mul_chunk(rows).hi == M_CHUNK < 2 * P      # multiplied at the store
    assert mul_wide(rows).hi < 2 * P                  # handed on and multiplied at the next pass's load
    assert canon(rows).hi == P - 1                    # the last pass


def test_the_model_refuses_what_the_kernel_must_not_do():
    with pytest.raises(AssertionError):
        unit4(Iv(0, 4 * P), False)                    # a row AT 4p: 4p - x2 may be zero
    with pytest.raises(AssertionError):
        first_pair_canon(Iv(0, P))                    # an operand at p: not canonical
    with pytest.raises(AssertionError):
        add(Iv(0, 4 * P - 1), Iv(0, 2 * P - 1))       # k_ntt_pass's products are below 2p only: x2 + x3' leaves the 256 bits


def test_a_three_pass_transform_chains_the_bounds():
    rows = pass_rows(first_pair_canon(Iv(0, P - 1)))
    rows = pass_rows(first_pair(mul_chunk(rows), False))
    rows = pass_rows(first_pair(mul_wide(rows), False))
    assert canon(rows).hi == P - 1


# ------------------------------------------------------------------ the same operations on integers
def i_sub_off(a, b, m):
    assert 0 < a - b + m * P < TOP
    return a - b + m * P


def i_first_pair_canon(x, w):
    x0, x1, x2, x3 = x
    assert max(x) < P
    y0, y1, y2 = i_add(x0, x1), i_sub_off(x0, x1, 1), i_add(x2, x3)
    assert max(y0, y1, y2) < 2 * P
    y3 = i_mul_chunk(i_sub(x2, x3), w)
    return [i_add(y0, y2), i_add(y1, y3), i_sub(y0, y2), i_sub(y1, y3)]


def i_unit4(x, ws, products_given):
    """-> the four rows, then the operands of the last two products"""
    wa, wb, wc = ws
    x0, x1, x2, x3 = x
    assert max(x0, x2) < 4 * P
    x0 = i_red2p(x0)
    if not products_given:
        x1, x3 = i_mul_chunk(x1, wa), i_mul_chunk(x3, wa)
    assert max(x1, x3) <= M_CHUNK
    s, n = i_add(x2, x3), i_sub_off(x3, x2, 4)
    y0, y1 = i_add_red(x0, x1), i_sub_red(x0, x1)
    y2, n3 = i_mul_chunk(s, wb), i_mul_chunk(n, wc)
    return [i_add(y0, y2), i_sub(y1, n3), i_sub(y0, y2), i_add(y1, n3), s, n]


# ------------------------------------------------------------------ part 2: the portable code of field.hpp
def operand_sets():
    """(mode, x0 .. x3, (wa, wb, wc)) rows; modes as in tests/ntt_lazy_ranges_host.cpp"""
    w_i = pow(OMEGA_28, 1 << 22, P)              # index 1 of stage 1, a fourth root of unity: the first pair's twiddle
    w8 = tuple(pow(OMEGA_28, e << 20, P) for e in (2, 1, 5))   # a unit of stages 2, 3 of an 8-bit pass: wa = w^(2r), wb = w^r, wc = w^(r + h)
    rows = []
    for x in itertools.product([0, 1, P - 1], repeat=4):
        rows.append((0, x, (1, 1, w_i)))
    edge_rows = [0, P - 1, 2 * P - 1, 4 * P - 1]
    for x in itertools.product(edge_rows, repeat=4):
        rows.append((1, x, w8))
    for x0, x2 in itertools.product(edge_rows, repeat=2):
        for x1, x3 in itertools.product([0, P - 1, M_CHUNK], repeat=2):
            rows.append((2, (x0, x1, x2, x3), w8))
    rng = random.Random(0x1A2E)
    for i in range(1500):
        ws = tuple(rng.randrange(P) for _ in range(3))
        rows.append((0, tuple(rng.randrange(P) for _ in range(4)), (1, 1, (w_i, ws[2])[i & 1])))
        rows.append((1, tuple(rng.randrange(4 * P) for _ in range(4)), ws))
        rows.append((2, (rng.randrange(4 * P), rng.randrange(M_CHUNK + 1), rng.randrange(4 * P), rng.randrange(M_CHUNK + 1)), ws))
    return rows


def test_portable_pairs_of_field_hpp(tmp_path):
    exe = tmp_path / "ntt_lazy_ranges_host"
    src = os.path.join(ROOT, "tests", "ntt_lazy_ranges_host.cpp")
    csrc = os.path.join(ROOT, "halo2-gpu-specific_amd", "csrc")
    res = subprocess.run(["g++", "-O2", "-std=c++17", "-I", csrc, src, "-o", str(exe)], capture_output=True, text=True, timeout=240)
    assert res.returncode == 0, res.stderr[-4000:]
    rows = operand_sets()
    recs = bytearray()
    for mode, x, ws in rows:
        recs += struct.pack("<II", mode, 0) + b"".join(v.to_bytes(32, "little") for v in x)
        recs += b"".join((w * TOP % P).to_bytes(32, "little") for w in ws)
    inp, outp = tmp_path / "in.bin", tmp_path / "out.bin"
    inp.write_bytes(bytes(recs))
    res = subprocess.run([str(exe), str(inp), str(outp)], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, (res.returncode, res.stderr[-2000:])
    data = outp.read_bytes()
    assert len(data) == 192 * len(rows)
    for i, (mode, x, ws) in enumerate(rows):
        got = [int.from_bytes(data[192 * i + 32 * j : 192 * i + 32 * j + 32], "little") for j in range(6)]
        a, b, c, d = x
        if mode == 0:
            assert got == i_first_pair_canon(x, ws[2]) + [0, 0], (i, [hex(v) for v in x])
            want = [a + b + c + d, a - b + ws[2] * (c - d), a + b - c - d, a - b - ws[2] * (c - d)]
        else:
            assert got == i_unit4(x, ws, mode == 2), (i, mode, [hex(v) for v in x])
            assert got[4] < TOP and 0 < got[5] < TOP
            wa, wb, wc = ws
            if mode == 2:
                wa = 1
            u, v, s, t = a + wa * b, a - wa * b, wb * (c + wa * d), wc * (c - wa * d)
            want = [u + s, v + t, u - s, v - t]      # rows p, p + h, p + 2h, p + 3h of the two stages
        assert all(v < 4 * P for v in got[:4]), (i, mode)
        assert [v % P for v in got[:4]] == [v % P for v in want], (i, mode)
