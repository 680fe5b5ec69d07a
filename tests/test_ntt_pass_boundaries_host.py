"""The values two NTT passes hand over (csrc/ntt_pass.hip k_ntt_pass8 / k_ntt_pass, csrc/field.hpp), without a GPU.

  The LAST stage pair of a pass before the last (k_ntt_pass8, stages 6 and 7: never a unit twiddle) leaves its four results
  unreduced, because a product -- the store product of the same kernel or the next pass's load product, any 256-bit operand --
  is the first thing that reads them (fp_lazy_last_pair_loose_head / _add).  With e = 2^-29 and x0 below 2p:
      y0 = x0 + x1'          below 3p (1 + e)          y1 = x0 - x1' + 2p     in [p (1 - e), 4p)
      y0 + y2  < 4p (1 + e)      y0 - y2 + 2p  in (0, 5p + 3e p)      y1 - n3 + p  in (0, 5p)      y1 + n3  < 5p (1 + e)
  all below 2^256 = 5.29 p, none below 4p: not rows of a tile (the x2 role needs a row strictly below 4p).

  Every store product (fp_mul_chunk, below p (1 + e)) is followed by fp_chunk_handover, which subtracts p where the top limb
  says the value may be at or above p: the next pass loads CANONICAL residues and its first stage pair is the one of the
  caller's data (FIRST_PAIR_CANON).

Part 1 states the bounds as exact rationals and propagates exact-integer intervals (the model of
tests/test_ntt_lazy_bounds_host.py and tests/test_ntt_lazy_ranges_host.py) through the three passes of a 2^24 transform.
Part 2 runs the portable bodies of field.hpp (tests/ntt_pass_boundaries_host.cpp, g++; once more under AddressSanitizer /
UndefinedBehaviorSanitizer) on the end points against the same arithmetic on Python integers.
Part 3: operands x with x w = v (mod p), v = 1, 2, 3, make fp_mul_chunk return v + p (checked on Python integers first): the
hand-over returns v."""
import itertools
import os
import random
import struct
import subprocess
from fractions import Fraction

import pytest

from test_ntt_lazy_bounds_host import (M_CHUNK, OMEGA_28, P, TOP, Iv, add, canon, first_pair, hull, i_add, i_mul_chunk, i_red2p,
                                       i_sub, mul_chunk, mul_wide, red2p, sub)
from test_ntt_lazy_ranges_host import first_pair_canon, i_sub_off, sub_off, unit4

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E = Fraction(1, 1 << 29)


# ------------------------------------------------------------------ part 1: the bounds
def loose_pair(x):
    """unit4_mul + unit4_add of the last stage pair of a pass before the last, on four rows with one bound -> the four results"""
    assert x.hi < 4 * P, "a row in LDS is strictly below 4p"
    x0 = red2p(x)
    x1 = x3 = mul_chunk(x)
    y2, n3 = mul_chunk(add(x, x3)), mul_chunk(sub_off(x3, x, 4))
    y0, y1 = add(x0, x1), sub(x0, x1)
    return y0, y1, (add(y0, y2), sub_off(y1, n3, 1), sub(y0, y2), add(y1, n3))


def test_the_bounds_of_the_loose_pair_as_exact_fractions():
    chunk = Fraction(P) * (1 + E)
    assert M_CHUNK == chunk.numerator // chunk.denominator and chunk.denominator != 1     # a product is at most M_CHUNK
    assert Fraction(529, 100) < Fraction(TOP, P) < Fraction(530, 100)
    y0, y1, rows = loose_pair(Iv(0, 4 * P - 1))
    assert y0.hi == 2 * P - 1 + M_CHUNK and y0.hi < 3 * P * (1 + E)
    assert y1.lo == 2 * P - M_CHUNK and y1.lo >= P * (1 - E) and y1.hi == 4 * P - 1
    r0, r1, r2, r3 = rows
    assert r0.hi < 4 * P * (1 + E)
    assert 0 < r2.lo and r2.hi < 5 * P + 3 * E * P
    assert r1.lo == 3 * P - 2 * M_CHUNK and r1.lo >= P * (1 - 2 * E) > 0 and r1.hi < 5 * P      # y1 - n3 + p stays positive
    assert r3.hi < 5 * P * (1 + E)
    assert all(r.hi < TOP for r in rows)                      # (Iv asserts it too)
    assert all(r.hi >= 4 * P for r in rows)                   # none is below 4p: a product's operand and nothing else


def test_the_model_refuses_a_loose_result_as_a_row_of_a_tile():
    rows = hull(*loose_pair(Iv(0, 4 * P - 1))[2])
    assert mul_chunk(rows).hi == M_CHUNK and mul_wide(rows).hi < 2 * P       # both readers take them
    with pytest.raises(AssertionError):
        unit4(rows, False)                                    # the x2 role: 4p - x2 may be negative
    with pytest.raises(AssertionError):
        canon(rows)                                           # nor the last pass's store


def pass_rows(rows, loose):
    assert rows.hi < 4 * P
    for _ in (2, 4):
        rows = hull(unit4(rows, True), unit4(rows, False))
        assert rows.hi < 4 * P
    if loose:
        return hull(*loose_pair(rows)[2])
    rows = unit4(rows, False)
    assert rows.hi < 4 * P
    return rows


def handover(a):
    """fp_chunk_handover after a store product"""
    assert a.hi <= M_CHUNK < 2 * P
    return Iv(0, P - 1)


def test_a_three_pass_transform_chains_the_bounds():
    """2^24 as it runs: the caller's data -> loose pair -> store product, canonical -> the canonical first pair again -> loose
    pair -> the last pass's load product -> its pairs as they were -> canonical"""
    rows = pass_rows(first_pair_canon(Iv(0, P - 1)), True)
    rows = pass_rows(first_pair_canon(handover(mul_chunk(rows))), True)
    assert rows.hi >= 4 * P
    rows = pass_rows(first_pair(mul_wide(rows), False), False)
    assert canon(rows).hi == P - 1


# ------------------------------------------------------------------ the same operations on integers
def i_loose(x0, x1p, y2, n3):
    """-> the four results, then y0 and y1; every step asserts that nothing wraps"""
    assert x0 < 2 * P and max(x1p, y2, n3) <= M_CHUNK
    y0, y1 = i_add(x0, x1p), i_sub(x0, x1p)
    assert y1 > 0
    return [i_add(y0, y2), i_sub_off(y1, n3, 1), i_sub(y0, y2), i_add(y1, n3), y0, y1]


def i_last_pair(x, ws):
    wa, wb, wc = ws
    x0, x1, x2, x3 = x
    assert max(x) < 4 * P
    x1p, x3p = i_mul_chunk(x1, wa), i_mul_chunk(x3, wa)
    y2, n3 = i_mul_chunk(i_add(x2, x3p), wb), i_mul_chunk(i_sub_off(x3p, x2, 4), wc)
    return i_loose(i_red2p(x0), x1p, y2, n3)


# ------------------------------------------------------------------ part 2 and 3: the portable code of field.hpp
FLAGS = ["-O2", "-std=c++17"]
SANITIZE = ["-O1", "-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def exe(request, tmp_path_factory):
    out = str(tmp_path_factory.mktemp("ntt_pass_boundaries_host") / "ntt_pass_boundaries_host")
    src = os.path.join(ROOT, "tests", "ntt_pass_boundaries_host.cpp")
    csrc = os.path.join(ROOT, "halo2-gpu-specific_amd", "csrc")
    flags = SANITIZE if request.param == "sanitized" else FLAGS
    res = subprocess.run(["g++", *flags, "-I", csrc, src, "-o", out], capture_output=True, text=True, timeout=240)
    assert res.returncode == 0, res.stderr[-4000:]
    return out


def run(exe, tmp_path, rows):
    """rows of (mode, (x0 .. x3), (wa, wb, wc) plain) -> six integers per row"""
    recs = bytearray()
    for mode, x, ws in rows:
        recs += struct.pack("<II", mode, 0) + b"".join(v.to_bytes(32, "little") for v in x)
        recs += b"".join((w * TOP % P).to_bytes(32, "little") for w in ws)
    inp, outp = tmp_path / "in.bin", tmp_path / "out.bin"
    inp.write_bytes(bytes(recs))
    res = subprocess.run([exe, str(inp), str(outp)], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0 and not res.stderr, (res.returncode, res.stderr[-3000:])
    data = outp.read_bytes()
    assert len(data) == 192 * len(rows)
    return [[int.from_bytes(data[192 * i + 32 * j : 192 * i + 32 * j + 32], "little") for j in range(6)] for i in range(len(rows))]


W8 = tuple(pow(OMEGA_28, e << 20, P) for e in (2 * 37, 37, 37 + 64))   # stages 6, 7 of an 8-bit pass at r = 37: w^(2r), w^r, w^(r + h)


def loose_operand_sets():
    rows = []
    for x in itertools.product([0, 4 * P - 1], repeat=4):                       # the end points of the rows
        rows.append((1, x, W8))
    for x in itertools.product([0, P - 1, 2 * P - 1, 2 * P, 4 * P - 1], repeat=4):
        rows.append((1, x, W8))
    for x0 in (0, 2 * P - 1, 2 * P, 4 * P - 1):                                 # the products at 0 and at their upper bound
        for prods in itertools.product([0, P - 1, M_CHUNK], repeat=3):
            rows.append((2, (x0,) + prods, W8))
    rng = random.Random(0xB0DA)
    for _ in range(1000):
        ws = tuple(rng.randrange(P) for _ in range(3))
        rows.append((1, tuple(rng.randrange(4 * P) for _ in range(4)), ws))
        rows.append((2, (rng.randrange(4 * P),) + tuple(rng.randrange(M_CHUNK + 1) for _ in range(3)), ws))
    return rows


def test_the_loose_pair_against_python_integers(exe, tmp_path):
    rows = loose_operand_sets()
    lowest = None
    for (mode, x, ws), got in zip(rows, run(exe, tmp_path, rows)):
        a, b, c, d = x
        if mode == 1:
            want = i_last_pair(x, ws)
            wa, wb, wc = ws
            u, v, s, t = a + wa * b, a - wa * b, wb * (c + wa * d), wc * (c - wa * d)
            res = [u + s, v + t, u - s, v - t]                # rows p, p + h, p + 2h, p + 3h of the two stages
        else:
            want = i_loose(i_red2p(a), b, c, d)               # x1', y2 and n3 = -y3 given
            res = [a + b + c, a - b - d, a + b - c, a - b + d]
        assert got == want, (mode, [hex(v) for v in x])       # the exact integers: no wrap below 0, none at 2^256
        assert all(0 <= v < TOP for v in got)
        assert [v % P for v in got[:4]] == [v % P for v in res], (mode, [hex(v) for v in x])
        lowest = got[1] if lowest is None else min(lowest, got[1])
    assert lowest == 3 * P - 2 * M_CHUNK > 0                  # y1 - n3 + p at x0 = 0 and both products at their upper bound


# twiddles as the tables hold them: butterfly twiddles of an 8-bit pass of 2^24 and inter-pass twiddles of its middle pass
TABLE_W = [pow(OMEGA_28, e, P) for e in (1 << 20, 3 << 20, 127 << 20, 16, 5 * 16, 0xFFFF * 16, 0x1234 * 16)]


def handover_operand_sets():
    rows, want = [], []
    for w in TABLE_W:
        w_inv = pow(w, -1, P)
        for v in (1, 2, 3):
            x = v * w_inv % P
            for k in range(6):                                # every representative of x a 256-bit operand can be
                if x + k * P < TOP:
                    rows.append((3, (x + k * P, 0, 0, 0), (w, 1, 1)))
                    want.append((v + P, v))
        for u in (P - 1, (P >> 224) << 224, 0):               # below p with p's top limb, and zero: left as they are
            rows.append((3, (u * w_inv % P, 0, 0, 0), (w, 1, 1)))
            want.append((u, u))
    rng = random.Random(0xCA707)
    for _ in range(500):
        w, x = rng.randrange(1, P), rng.randrange(TOP)
        r = i_mul_chunk(x, w)
        rows.append((3, (x, 0, 0, 0), (w, 1, 1)))
        want.append((r, r % P))
    return rows, want


def test_the_operands_that_leave_the_product_at_or_above_p():
    """on Python integers, before the compiled code is asked: x w = v (mod p) for a small v leaves the product at v + p"""
    rows, want = handover_operand_sets()
    above = 0
    for (_, x, ws), (raw, _) in zip(rows, want):
        assert i_mul_chunk(x[0], ws[0]) == raw
        above += raw >= P
    assert above >= 3 * len(TABLE_W) * 5


def test_the_hand_over_is_canonical(exe, tmp_path):
    rows, want = handover_operand_sets()
    for (_, x, ws), (raw, res), got in zip(rows, want, run(exe, tmp_path, rows)):
        assert got[0] == raw, hex(x[0])                       # fp_mul_chunk as it is: v + p where the test says so
        assert got[1] == res < P, hex(x[0])                   # with the branch
        assert got[2] == res, hex(x[0])                       # the form without one
