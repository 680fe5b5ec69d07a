"""Cases shared by tests/test_values_host.py (the host twin) and tests/test_gpu_values.py (the kernel): programs for the C ABI
of the fused evaluator (h2_values_eval / h2_dev_values_eval) with an interpreter over Python integers as their oracle, and a
seeded generator of random Value expressions.  Everything here is deterministic; expected values are computed once per
(case, m) and cached."""
import functools
import random

import numpy as np

from halo2_gpu_specific_amd import values as V
from halo2_gpu_specific_amd.values import Value

R_MOD = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001
MASK64 = (1 << 64) - 1
R = (1 << 256) % R_MOD
R_INV = pow(R, -1, R_MOD)
CANONICAL, MONTGOMERY, COMPACT = 0, 1, 2
ADD, SUB, MUL, SQR, NEG, SELECT, ISZERO = range(7)
LEAF, CONST, SLOT, LAST = (k << 24 for k in range(4))
NO_SLOT = 0xFFFFFFFF
SIZES = (1, 2, 255, 256, 257)


def limbs(values):
    return np.array([[(v >> (64 * j)) & MASK64 for j in range(4)] for v in values], dtype=np.uint64).reshape(len(values), 4)


def ints(a):
    return [int.from_bytes(row.tobytes(), "little") for row in np.ascontiguousarray(a, dtype=np.uint64)]


def edge_field(rng, count, wide=False):
    """`count` integers below r -- or, `wide`, below 2^256 with 2^256 - 1, r and r + 1 among them: 0, 1, r - 1 first"""
    special = [0, 1, R_MOD - 1, 2, R_MOD - 2] + ([(1 << 256) - 1, R_MOD, R_MOD + 1, 1 << 255] if wide else [])
    out = [rng.randrange(1 << 256 if wide else R_MOD) for _ in range(count)]
    for at, v in zip(range(0, count, 3), special):
        out[at] = v
    return out


def edge_compact(rng, count):
    out = [rng.randrange(1 << 64) for _ in range(count)]
    for at, v in zip(range(0, count, 2), [0, 1, MASK64, 1 << 63]):
        out[at] = v
    return out


class Leaf:
    """a buffer (numpy) in a form, read from `first` on every `stride` elements; values(m): the integers mod r it stands for"""

    def __init__(self, data, form, first=0, stride=1):
        self.data, self.form, self.first, self.stride = data, form, first, stride

    def values(self, m):
        picked = self.data[self.first:self.first + (m - 1) * self.stride + 1:self.stride]
        if self.form == COMPACT:
            return [int(v) for v in picked]
        return [(v * R_INV if self.form == MONTGOMERY else v) % R_MOD for v in ints(picked)]


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

    for op, dst, a, b, c in ops:
        x = operand(a)
        if op in (ADD, SUB, MUL):
            y = operand(b)
            r = [(p + q) % R_MOD if op == ADD else (p - q) % R_MOD if op == SUB else p * q % R_MOD for p, q in zip(x, y)]
        elif op == SQR:
            r = [p * p % R_MOD for p in x]
        elif op == NEG:
            r = [-p % R_MOD for p in x]
        elif op == ISZERO:
            r = [int(p == 0) for p in x]
        else:
            r = [q if p else s for p, q, s in zip(x, operand(b), operand(c))]
        last = r
        if dst != NO_SLOT:
            slots[dst] = r
    return [slots[slot] for slot, _ in outputs]


class Program:
    def __init__(self, name, leaves, constants, ops, outputs):
        self.name, self.leaves, self.constants, self.ops, self.outputs = name, leaves, constants, ops, outputs

    @functools.lru_cache(maxsize=None)
    def expected(self, m):
        return interpret(self.leaves, self.constants, self.ops, self.outputs, m)

    def tables(self, m, address, out_address):
        """the C tables: `address(leaf index)` and `out_address(output index)` give the base pointers"""
        leaves = np.zeros(len(self.leaves), dtype=V.VALUES_LEAF)
        for i, leaf in enumerate(self.leaves):
            leaves[i] = (address(i), leaf.first, leaf.stride, len(leaf.data), leaf.form, 0)
        constants = limbs(self.constants) if self.constants else np.zeros((0, 4), dtype=np.uint64)
        ops = np.array(self.ops, dtype=np.uint32).reshape(len(self.ops), 5).view(V.VALUES_OP).reshape(-1)
        outputs = np.zeros(len(self.outputs), dtype=V.VALUES_OUTPUT)
        for i, (slot, form) in enumerate(self.outputs):
            outputs[i] = (out_address(i), 0, slot, form)
        return leaves, constants, ops, outputs

    def decode(self, arrays):
        """the output arrays as integers mod r"""
        return [[v * R_INV % R_MOD for v in ints(a)] if form == MONTGOMERY else ints(a) for a, (_, form) in zip(arrays, self.outputs)]


def run_host(L, program, m):
    """h2_values_eval -> the raw output arrays"""
    outs = [np.full((m, 4), 0x5A5A5A5A5A5A5A5A, dtype=np.uint64) for _ in program.outputs]
    leaves, constants, ops, outputs = program.tables(m, lambda i: program.leaves[i].data.ctypes.data, lambda i: outs[i].ctypes.data)
    rc = L.h2_values_eval(leaves.ctypes.data, len(leaves), constants.ctypes.data, len(constants), ops.ctypes.data, len(ops),
                          outputs.ctypes.data, len(outputs), m)
    assert rc == 0, L.h2_last_error()
    return outs


def run_device(D, program, m):
    """h2_dev_values_eval -> the raw output arrays, downloaded"""
    torch = D.torch
    with torch.cuda.stream(D.tstream):
        bufs = [torch.from_numpy(leaf.data.view(np.int64)).to(D.dev) for leaf in program.leaves]
        outs = [torch.full((m, 4), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device=D.dev) for _ in program.outputs]
    leaves, constants, ops, outputs = program.tables(m, lambda i: bufs[i].data_ptr(), lambda i: outs[i].data_ptr())
    rc = D.L.h2_dev_values_eval(leaves.ctypes.data, len(leaves), constants.ctypes.data, len(constants), ops.ctypes.data, len(ops),
                                outputs.ctypes.data, len(outputs), m, D.stream)
    assert rc == 0, D.L.h2_last_error()
    return [D.download(t) for t in outs]


@functools.lru_cache(maxsize=None)
def programs(m_max):
    """the hand cases, over buffers long enough for m_max rows at every stride used"""
    rng = random.Random(0x56414C)
    n = 3 * m_max + 8
    canonical = limbs(edge_field(rng, n, wide=True))
    montgomery = limbs([v * R % R_MOD for v in edge_field(rng, n)])
    compact = np.array(edge_compact(rng, n), dtype=np.uint64)
    consts = [0, 1, R_MOD - 1, (1 << 256) - 1, R_MOD, 0x1234567890ABCDEF]
    out = []
    # every op over every form; leaf 0 and leaf 3 are ONE buffer at different strides; constants that need reducing
    leaves = [Leaf(canonical, CANONICAL), Leaf(compact, COMPACT), Leaf(montgomery, MONTGOMERY), Leaf(canonical, CANONICAL, 1, 2),
              Leaf(compact, COMPACT, 2, 3), Leaf(montgomery, MONTGOMERY, 5, 3)]
    ops = [(ADD, 0, LEAF | 0, LEAF | 1, 0), (SUB, 1, LEAF | 2, LEAF | 3, 0), (MUL, 2, SLOT | 0, SLOT | 1, 0),
           (SQR, 3, LEAF | 4, 0, 0), (NEG, 4, LEAF | 5, 0, 0), (ISZERO, 5, LEAF | 0, 0, 0),
           (SELECT, 0, SLOT | 5, SLOT | 3, SLOT | 4), (MUL, 1, SLOT | 0, CONST | 3, 0), (ADD, NO_SLOT, SLOT | 1, CONST | 2, 0),
           (SUB, 3, LAST, CONST | 5, 0), (ISZERO, 4, LEAF | 1, 0, 0), (MUL, 5, LEAF | 1, LEAF | 1, 0)]
    out.append(Program("every op", leaves, consts, ops, [(2, CANONICAL), (3, MONTGOMERY), (4, CANONICAL), (5, MONTGOMERY)]))
    # the edge operands against each other: x * (r - 1), x + (r - 1), x - x, 0 - x, (2^64 - 1)^2
    ops = [(MUL, 0, LEAF | 0, CONST | 2, 0), (ADD, 1, LEAF | 0, CONST | 2, 0), (SUB, 2, LEAF | 1, LEAF | 1, 0),
           (SUB, 3, CONST | 0, LEAF | 1, 0), (ADD, 2, SLOT | 2, SLOT | 3, 0), (MUL, 3, SLOT | 0, SLOT | 1, 0)]
    out.append(Program("edges", [Leaf(canonical, CANONICAL), Leaf(compact, COMPACT)], consts, ops, [(2, CANONICAL), (3, CANONICAL)]))
    # strides and offsets 1, 2, 3 of all three forms, summed
    leaves = [Leaf(buf, form, first, stride) for buf, form in ((canonical, CANONICAL), (compact, COMPACT), (montgomery, MONTGOMERY))
              for first, stride in ((0, 1), (1, 2), (2, 3))]
    ops = [(ADD, 0, LEAF | 0, LEAF | 1, 0)] + [(ADD, 0, SLOT | 0, LEAF | i, 0) for i in range(2, 9)]
    out.append(Program("strides", leaves, [], ops, [(0, MONTGOMERY)]))
    # a constant and a leaf straight to the outputs, in both forms
    ops = [(ADD, 0, CONST | 3, CONST | 0, 0), (ADD, 1, LEAF | 0, CONST | 0, 0)]
    out.append(Program("copies", [Leaf(canonical, CANONICAL, 3, 2)], consts, ops, [(0, CANONICAL), (0, MONTGOMERY), (1, CANONICAL), (1, MONTGOMERY)]))
    return out


def slot_cap_program(m_max, slots):
    """writes every slot, then many other ops over slot 0 alone, then reads each slot again: what a slot held must survive"""
    rng = random.Random(5)
    data = limbs(edge_field(rng, m_max))
    ops = [(ADD, s, LEAF | 0, CONST | s, 0) for s in range(slots)]
    ops += [(MUL, 0, SLOT | 0, SLOT | 0, 0), (ADD, 0, SLOT | 0, CONST | 1, 0)] * 20
    for s in range(1, slots):
        ops.append((MUL, 0, SLOT | 0, SLOT | s, 0))
    return Program("slot cap", [Leaf(data, CANONICAL)], list(range(3, 3 + slots)), ops, [(0, CANONICAL), (slots - 1, CANONICAL)])


# -- random Value expressions ------------------------------------------------------------------------------------------------
def fuzz_inputs(m):
    """four leaves of mixed forms as (numpy data, form, first, stride, integers): shared by every seed"""
    rng = random.Random(0xF022 + m)
    a = edge_field(rng, m, wide=True)
    b = edge_compact(rng, 2 * m + 1)
    c = edge_field(rng, m)
    d = edge_field(rng, 3 * m)
    return [(limbs(a), CANONICAL, 0, 1, [v % R_MOD for v in a]),
            (np.array(b, dtype=np.uint64), COMPACT, 1, 2, b[1::2][:m]),
            (limbs([v * R % R_MOD for v in c]), MONTGOMERY, 0, 1, c),
            (limbs(d), CANONICAL, 2, 3, d[2::3][:m])]


def fuzz_leaves(device, m, upload=None):
    out = []
    for data, form, first, stride, _ in fuzz_inputs(m):
        data = upload(data) if upload else data
        base = Value.from_u64(device, data) if form == COMPACT else Value.from_limbs(device, data, montgomery=form == MONTGOMERY)
        out.append(base[first:first + (m - 1) * stride + 1:stride])
    return out


def fuzz_expression(seed, leaves, leaf_ints, max_nodes=40):
    """a random DAG of at most `max_nodes` nodes over the four leaves -> (Value, its integers); divisions and selects included"""
    rng = random.Random(seed)
    pool = list(zip(leaves, leaf_ints))
    for _ in range(rng.randrange(1, max_nodes - 3)):
        kind = rng.choice(["add", "sub", "mul", "mul", "sqr", "neg", "div", "select", "iszero", "const", "pow", "inv"])
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
        elif kind == "div":
            node = (x / y, [p * pow(q, -1, R_MOD) % R_MOD if q else 0 for p, q in zip(xi, yi)])
        elif kind == "inv":
            node = (x.invert(), [pow(p, -1, R_MOD) if p else 0 for p in xi])
        elif kind == "select":
            node = (Value.select(x, y, z), [q if p else s for p, q, s in zip(xi, yi, zi)])
        elif kind == "iszero":
            node = (x.is_zero(), [int(p == 0) for p in xi])
        elif kind == "pow":
            e = rng.randrange(0, 6)
            node = (x ** e, [pow(p, e, R_MOD) for p in xi])
        else:
            k = rng.choice([0, 1, R_MOD - 1, rng.randrange(1 << 256), -3])
            node = (k - x if rng.random() < 0.5 else x * k, None)
            node = (node[0], [(k - p) % R_MOD for p in xi] if node[0]._node.kind == "sub" else [p * k % R_MOD for p in xi])
        pool.append(node)
    # the result mixes the last nodes, so that most of the pool is live
    value, want = pool[-1]
    for other, oi in pool[-3:-1]:
        value, want = value + other, [(p + q) % R_MOD for p, q in zip(want, oi)]
    return value, want
