"""Generates tests/golden/pairing_kat.json from the big-integer pairing of tests/bn254_pairing.py alone (nothing of the
product is imported): pairing-check cases with their decisions, G2 scalar multiples of the generator, and one twist point
outside the order-r subgroup.  Integers are hex strings; a G1 point is [x, y], a G2 point [[x.c0, x.c1], [y.c0, y.c1]],
null the identity.

usage: python tests/golden/gen_pairing_kat.py"""
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import bn254_pairing as bp  # noqa: E402
import ref_plonk as rp  # noqa: E402


def fq2_sqrt(a):
    """a root of a in Fq2 = Fq[u] / (u^2 + 1), or None (q = 3 mod 4; by the norm)"""
    q = bp.Q
    a0, a1 = a
    root = lambda v: (lambda s: s if s * s % q == v % q else None)(pow(v % q, (q + 1) // 4, q))  # noqa: E731
    if a1 == 0:
        s = root(a0)
        if s is not None:
            return (s, 0)
        s = root(-a0)
        return None if s is None else (0, s)
    n = root(a0 * a0 + a1 * a1)
    if n is None:
        return None
    half = pow(2, -1, q)
    x0 = root((a0 + n) * half)
    if x0 is None:
        x0 = root((a0 - n) * half)
    if x0 is None:
        return None
    x = (x0, a1 * pow(2 * x0, -1, q) % q)
    return x if bp.f2_mul(x, x) == (a0 % q, a1 % q) else None


def twist_point_outside_subgroup(rnd):
    while True:
        x = (rnd.randrange(bp.Q), rnd.randrange(bp.Q))
        y = fq2_sqrt(bp.f2_add(bp.f2_mul(bp.f2_mul(x, x), x), bp.B2))
        if y is not None and bp.g2_mul((x, y), bp.R) is not None:
            assert bp.g2_on_curve((x, y))
            return (x, y)


def h(v):
    return "%x" % v


def g1_json(P):
    return None if P is None else [h(P[0]), h(P[1])]


def g2_json(T):
    return None if T is None else [[h(T[0][0]), h(T[0][1])], [h(T[1][0]), h(T[1][1])]]


def main():
    rnd = random.Random(0x50414952)
    cases = []
    for i in range(8):
        a, b = rnd.randrange(1, bp.R), rnd.randrange(1, bp.R)
        c = a * b % bp.R if i % 2 == 0 else (a * b + 1 + i) % bp.R
        pairs = [(rp.g1_mul(rp.G1, a), bp.g2_mul(bp.G2, b)), (rp.g1_neg(rp.g1_mul(rp.G1, c)), bp.G2)]
        if i == 4:
            pairs.append((None, bp.g2_mul(bp.G2, 7)))
        if i == 6:
            pairs.append((rp.g1_mul(rp.G1, 9), None))
        cases.append({"pairs": [[g1_json(P), g2_json(T)] for P, T in pairs], "accept": bp.pairing_check(pairs)})
    assert [c["accept"] for c in cases] == [True, False] * 4
    scalars = [0, 1, 2, bp.R - 1] + [rnd.randrange(bp.R) for _ in range(4)]
    out = {"cases": cases, "g2_mul": [{"scalar": h(s), "point": g2_json(bp.g2_mul(bp.G2, s))} for s in scalars],
           "outside_subgroup": g2_json(twist_point_outside_subgroup(rnd))}
    with open(os.path.join(HERE, "pairing_kat.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
