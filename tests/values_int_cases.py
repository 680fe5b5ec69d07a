"""Cases shared by tests/test_values_int_host.py (the host twin) and tests/test_gpu_values_int.py (the kernel) for the integer
half of the fused evaluator: programs for the C ABI that use TO_INT, TO_FIELD, EXTRACT, LT, AND, OR and XOR, with an interpreter
over Python integers as their oracle (a value is the integer in [0, r) whatever its kind: the kinds only say how the evaluator
holds it), and a seeded generator of random Value expressions that cross between the kinds.  Everything here is deterministic;
expected values are computed once per (case, m) and cached."""
import functools
import random

import numpy as np

import values_cases as vc
from values_cases import (ADD, CANONICAL, COMPACT, CONST, ISZERO, LAST, LEAF, MONTGOMERY, MUL, NEG, NO_SLOT, R, R_MOD, SELECT, SLOT, SQR,
                          SUB, Leaf, limbs)
from halo2_gpu_specific_amd.values import Value

TO_INT, TO_FIELD, EXTRACT, LT, AND, OR, XOR = range(16, 23)
SIZES = (1, 2, 255, 256, 257)
EXTRACT_LO = (0, 1, 31, 32, 33, 63, 64, 65, 127, 128, 223, 224, 253, 255)
EXTRACT_N = (1, 31, 32, 33, 64, 254, 256)
POWERS = (1, 31, 32, 33, 63, 64, 65, 127, 128, 191, 192, 224, 252, 253)


def edge_integers(rng, count, wide=False):
    """`count` integers below r drawn from {0, 1, r - 1, 2^j - 1, 2^j, random}, the named ones first; `wide`: any 256-bit
    integer, with 2^256 - 1, r, r + 1, 2^254 and 2^255 among them"""
    special = [0, 1, R_MOD - 1] + [v for j in POWERS for v in ((1 << j) - 1, 1 << j)]
    if wide:
        special += [(1 << 256) - 1, R_MOD, R_MOD + 1, 1 << 254, 1 << 255]
    out = [rng.randrange(1 << 256 if wide else R_MOD) for _ in range(count)]
    for at, v in zip(range(0, count, 2), special):
        out[at] = v
    return out


def interpret(leaves, constants, ops, outputs, m):
    """the program over Python integers -> one list of m integers per output"""
    leaf_values = [leaf.values(m) for leaf in leaves]
    slots, last = {}, None

    def operand(word):
        kind, index = word & 0xFF000000, word & 0xFFFFFF
        if kind == LEAF:
            return leaf_values[index]
        if kind == CONST:
            return [constants[index] % R_MOD] * m
        return slots[index] if kind == SLOT else last

    binary = {ADD: lambda p, q: (p + q) % R_MOD, SUB: lambda p, q: (p - q) % R_MOD, MUL: lambda p, q: p * q % R_MOD,
              LT: lambda p, q: int(p < q), AND: lambda p, q: p & q, OR: lambda p, q: (p | q) % R_MOD, XOR: lambda p, q: (p ^ q) % R_MOD}
    for op, dst, a, b, c in ops:
        x = operand(a)
        if op in binary:
            r = [binary[op](p, q) for p, q in zip(x, operand(b))]
        elif op == SQR:
            r = [p * p % R_MOD for p in x]
        elif op == NEG:
            r = [-p % R_MOD for p in x]
        elif op == ISZERO:
            r = [int(p == 0) for p in x]
        elif op in (TO_INT, TO_FIELD):
            r = list(x)
        elif op == EXTRACT:
            r = [(p >> b) % (1 << c) for p in x]
        else:
            assert op == SELECT
            r = [q if p else s for p, q, s in zip(x, operand(b), operand(c))]
        last = r
        if dst != NO_SLOT:
            slots[dst] = r
    return [slots[slot] for slot, _ in outputs]


class Program(vc.Program):
    @functools.lru_cache(maxsize=None)
    def expected(self, m):
        return interpret(self.leaves, self.constants, self.ops, self.outputs, m)


@functools.lru_cache(maxsize=None)
def buffers(m_max):
    """canonical (any 256-bit integers), reduced canonical x and y, Montgomery and compact buffers of 3 m_max + 8 elements"""
    rng = random.Random(0x494E54)
    n = 3 * m_max + 8
    wide = edge_integers(rng, n, wide=True)
    x = edge_integers(rng, n)
    y = [rng.randrange(R_MOD) for _ in range(n)]
    mont = edge_integers(rng, n)
    # the pairs LT and the bitwise ops are asked about, from row 0 on
    top, bottom = 1 << 224, 1
    pairs = [(R_MOD - 1, 0), (0, R_MOD - 1), (R_MOD - 1, 1), (5, 5), (R_MOD - 1, R_MOD - 1), (x[5], x[5] ^ top), (x[6] | bottom, (x[6] | bottom) - 1),
             (0x30 << 248, 0x0F << 248),                       # both below r, their OR and XOR above it
             (0, 0), (1 << 253, (1 << 253) - 1)]
    assert all(p < R_MOD and q < R_MOD for p, q in pairs) and (pairs[7][0] | pairs[7][1]) >= R_MOD
    for at, (p, q) in enumerate(pairs):
        x[at], y[at] = p, q
    return {"wide": limbs(wide), "x": limbs(x), "y": limbs(y), "montgomery": limbs([v * R % R_MOD for v in mont]),
            "compact": np.array(vc.edge_compact(rng, n), dtype=np.uint64)}


@functools.lru_cache(maxsize=None)
def programs(m_max):
    """the hand cases, over buffers long enough for m_max rows at every stride used"""
    B = buffers(m_max)
    out = []
    sources = [Leaf(B["wide"], CANONICAL), Leaf(B["montgomery"], MONTGOMERY), Leaf(B["x"], CANONICAL, 1, 2), Leaf(B["compact"], COMPACT)]
    # EXTRACT at every lo x n of the table: one TO_INT, at most `outputs` extracts per program; leaf and output forms rotate
    count = 0
    for lo in EXTRACT_LO:
        for chunk in (EXTRACT_N[:4], EXTRACT_N[4:]):
            ops = [(TO_INT, 0, LEAF | 0, 0, 0)] + [(EXTRACT, 1 + i, SLOT | 0, lo, n) for i, n in enumerate(chunk)]
            outputs = [(1 + i, (count + i) % 2) for i in range(len(chunk))]
            out.append(Program("extract lo %d n %s" % (lo, chunk), [sources[count % 4]], [], ops, outputs))
            count += 1
    # every leaf form x every output form, for an integer result, a field result computed from it, and the TO_INT itself
    for name, leaf in (("canonical", Leaf(B["wide"], CANONICAL, 2, 3)), ("montgomery", Leaf(B["montgomery"], MONTGOMERY, 1, 2)),
                       ("compact", Leaf(B["compact"], COMPACT, 1, 1))):
        for form in (CANONICAL, MONTGOMERY):
            ops = [(TO_INT, 0, LEAF | 0, 0, 0), (EXTRACT, 1, SLOT | 0, 3, 100), (TO_FIELD, NO_SLOT, SLOT | 1, 0, 0), (MUL, 2, LAST, LEAF | 0, 0),
                   (ISZERO, 3, SLOT | 1, 0, 0)]
            out.append(Program("forms %s -> %d" % (name, form), [leaf], [], ops, [(0, form), (1, form), (2, form), (3, form)]))
    # TO_INT of a canonical leaf that holds 2^256 - 1 (row 0 of this view) and of a compact leaf, in both output forms
    at = next(i for i, v in enumerate(vc.ints(B["wide"])) if v == (1 << 256) - 1)
    ops = [(TO_INT, 0, LEAF | 0, 0, 0), (TO_INT, 1, LEAF | 1, 0, 0)]
    out.append(Program("to_int", [Leaf(B["wide"], CANONICAL, at, 1), Leaf(B["compact"], COMPACT)], [], ops,
                       [(0, CANONICAL), (0, MONTGOMERY), (1, CANONICAL), (1, MONTGOMERY)]))
    # LT both ways, on integers from LAST and from slots
    xy = [Leaf(B["x"], CANONICAL), Leaf(B["y"], CANONICAL)]
    ops = [(TO_INT, 0, LEAF | 0, 0, 0), (TO_INT, NO_SLOT, LEAF | 1, 0, 0), (LT, 2, SLOT | 0, LAST, 0), (TO_INT, 1, LEAF | 1, 0, 0),
           (LT, 3, SLOT | 1, SLOT | 0, 0), (LT, 4, SLOT | 0, SLOT | 0, 0)]
    out.append(Program("lt", xy, [], ops, [(2, CANONICAL), (3, MONTGOMERY), (4, CANONICAL)]))
    # AND, OR, XOR, and ISZERO of an integer: (r - 1) | 1 = r = 0
    ops = [(TO_INT, 0, LEAF | 0, 0, 0), (TO_INT, 1, LEAF | 1, 0, 0), (AND, 2, SLOT | 0, SLOT | 1, 0), (OR, 3, SLOT | 0, SLOT | 1, 0),
           (XOR, 4, SLOT | 0, SLOT | 1, 0), (ISZERO, 5, SLOT | 3, 0, 0)]
    out.append(Program("bitwise", xy, [], ops, [(2, CANONICAL), (3, MONTGOMERY), (4, CANONICAL), (5, CANONICAL)]))
    # SELECT: an integer condition over integer arms (an integer result) and over field arms; a constant through TO_INT
    ops = [(TO_INT, 0, LEAF | 0, 0, 0), (TO_INT, 1, LEAF | 1, 0, 0), (LT, 2, SLOT | 0, SLOT | 1, 0), (SELECT, 3, SLOT | 2, SLOT | 0, SLOT | 1),
           (SELECT, 4, SLOT | 2, LEAF | 1, CONST | 0), (TO_INT, NO_SLOT, CONST | 1, 0, 0), (AND, 5, LAST, SLOT | 3, 0),
           (SELECT, 2, LEAF | 0, SLOT | 5, SLOT | 3)]
    out.append(Program("select", xy, [R_MOD - 1, (1 << 130) - 1], ops, [(3, CANONICAL), (4, MONTGOMERY), (5, MONTGOMERY), (2, CANONICAL)]))
    out.append(slot_cap_program(m_max, 6))
    return out


def slot_cap_program(m_max, slots):
    """an integer in every slot (register slot 0 and every LDS slot), many ops over slot 0 alone, then every slot read again"""
    B = buffers(m_max)
    ops = [(TO_INT, 0, LEAF | 0, 0, 0)] + [(EXTRACT, s, SLOT | 0, 7 * s, 256 - 40 * s) for s in range(1, slots)]
    ops += [(XOR, 0, SLOT | 0, SLOT | 1, 0), (EXTRACT, 0, SLOT | 0, 1, 250)] * 10
    for s in range(1, slots):
        ops.append((XOR if s % 2 else OR, 0, SLOT | 0, SLOT | s, 0))
    return Program("integer slot cap", [Leaf(B["x"], CANONICAL)], [], ops, [(0, CANONICAL), (slots - 1, MONTGOMERY)])


def grid_stride_program(m, seed=11):
    """EXTRACT, LT, XOR and both output forms over m rows of random cells -> (program, its integer oracle for a slice of rows)"""
    rng = np.random.Generator(np.random.PCG64(seed))
    canonical = rng.integers(0, 1 << 64, size=(m + 3, 4), dtype=np.uint64)            # any 256-bit integers
    compact = rng.integers(0, 1 << 64, size=2 * m, dtype=np.uint64)
    leaves = [Leaf(canonical, CANONICAL, 3, 1), Leaf(compact, COMPACT, 1, 2)]
    ops = [(TO_INT, 0, LEAF | 0, 0, 0), (TO_INT, 1, LEAF | 1, 0, 0), (EXTRACT, 2, SLOT | 0, 37, 64), (LT, 3, SLOT | 2, SLOT | 1, 0),
           (XOR, 4, SLOT | 0, SLOT | 1, 0)]
    program = Program("long", leaves, [], ops, [(2, CANONICAL), (3, MONTGOMERY), (4, MONTGOMERY)])

    def want(rows):
        x = [v % R_MOD for v in vc.ints(canonical[3:][rows])]
        y = [int(v) for v in compact[1::2][rows]]
        field = [(p >> 37) % (1 << 64) for p in x]
        return [field, [int(f < q) for f, q in zip(field, y)], [(p ^ q) % R_MOD for p, q in zip(x, y)]]

    return program, want


# -- random Value expressions that cross between the kinds ------------------------------------------------------------------------
def fuzz_expression(seed, leaves, leaf_ints, max_nodes=30):
    """a random DAG over the four leaves of values_cases.fuzz_inputs -> (Value, its integers).  The last steps are, by
    construction, a field product taken as an integer (to_int), a bit field of it (an integer op) and a field sum over that
    (to_field): every expression holds an integer op and crosses between the kinds both ways"""
    rng = random.Random(0x1217 + seed)
    pool = list(zip(leaves, leaf_ints))
    for _ in range(rng.randrange(1, max_nodes - 3)):
        kind = rng.choice(["add", "sub", "mul", "sqr", "neg", "select", "iszero", "const", "bits", "bits", "shr", "low", "bit", "and", "or",
                           "xor", "lt", "le", "gt", "ge", "mask"])
        (x, xi), (y, yi), (z, zi) = (rng.choice(pool) for _ in range(3))
        if kind == "add":
            node = (x + y, [(p + q) % R_MOD for p, q in zip(xi, yi)])
        elif kind == "sub":
            node = (x - y, [(p - q) % R_MOD for p, q in zip(xi, yi)])
        elif kind == "mul":
            node = (x * y, [p * q % R_MOD for p, q in zip(xi, yi)])
        elif kind == "sqr":
            node = (x.square(), [p * p % R_MOD for p in xi])
        elif kind == "neg":
            node = (-x, [-p % R_MOD for p in xi])
        elif kind == "select":
            node = (Value.select(x, y, z), [q if p else s for p, q, s in zip(xi, yi, zi)])
        elif kind == "iszero":
            node = (x.is_zero(), [int(p == 0) for p in xi])
        elif kind == "const":
            k = rng.choice([0, 1, R_MOD - 1, rng.randrange(1 << 256), -3])
            node = (x * k, [p * k % R_MOD for p in xi])
        elif kind == "bits":
            lo, n = rng.choice(EXTRACT_LO + (7, 100)), rng.choice(EXTRACT_N + (8, 16))
            node = (x.bits(lo, n), [(p >> lo) % (1 << n) for p in xi])
        elif kind == "shr":
            k = rng.randrange(0, 256)
            node = (x >> k, [p >> k for p in xi])
        elif kind == "low":
            n = rng.randrange(1, 257)
            node = (x.low(n), [p % (1 << n) for p in xi])
        elif kind == "bit":
            i = rng.randrange(0, 254)
            node = (x.bit(i), [(p >> i) & 1 for p in xi])
        elif kind == "and":
            node = (x & y, [p & q for p, q in zip(xi, yi)])
        elif kind == "or":
            node = (x | y, [(p | q) % R_MOD for p, q in zip(xi, yi)])
        elif kind == "xor":
            node = (x ^ y, [(p ^ q) % R_MOD for p, q in zip(xi, yi)])
        elif kind == "lt":
            node = (x.lt(y), [int(p < q) for p, q in zip(xi, yi)])
        elif kind == "le":
            node = (x.le(y), [int(p <= q) for p, q in zip(xi, yi)])
        elif kind == "gt":
            node = (x.gt(y), [int(p > q) for p, q in zip(xi, yi)])
        elif kind == "ge":
            node = (x.ge(y), [int(p >= q) for p, q in zip(xi, yi)])
        else:
            k = rng.choice([0xFF, (1 << 64) - 1, R_MOD - 1, 1 << 200])
            node = (k ^ x if rng.random() < 0.5 else x & k, None)
            node = (node[0], [(p ^ k) % R_MOD for p in xi] if node[0]._node.kind == "xor" else [p & k for p in xi])
        pool.append(node)
    (x, xi), (y, yi) = pool[-1], rng.choice(pool)
    lo, n = rng.randrange(0, 200), rng.randrange(1, 65)
    value, want = (x * y).bits(lo, n), [(p * q % R_MOD >> lo) % (1 << n) for p, q in zip(xi, yi)]
    for other, oi in pool[-3:-1]:
        value, want = value + other, [(p + q) % R_MOD for p, q in zip(want, oi)]
    return value, want
