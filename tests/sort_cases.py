"""Cases of the sort (csrc/sort.hip, its host twin, Value.argsort) shared by tests/test_sort_host.py and tests/test_gpu_sort.py:
key columns as Python integers, their encodings in the three cell forms, the definition -- sorted(range(n), key=(k0[i], k1[i],
..., i)) over Python integers -- and the number of passes that move data, counted from the bytes themselves."""
import random

import numpy as np

R_MOD = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001
MONT_R = (1 << 256) % R_MOD
CANONICAL, MONTGOMERY, COMPACT = 0, 1, 2
OK, OUT_OF_RANGE = 0, 1
SENTINELS = (0, 1, (1 << 64) - 1, 1 << 64, (1 << 128) - 1, 1 << 128, 1 << 192, R_MOD - 1)


def oracle(keys):
    """the definition: equal tuples keep ascending row order"""
    return sorted(range(len(keys[0])), key=lambda i: tuple(k[i] for k in keys) + (i,))


def encode(values, form):
    """a key column of Python integers as the cells of `form`"""
    if form == COMPACT:
        return np.array(values, dtype=np.uint64)
    if form == MONTGOMERY:
        values = [v * MONT_R % R_MOD for v in values]
    return np.frombuffer(b"".join(v.to_bytes(32, "little") for v in values), dtype=np.uint64).reshape(len(values), 4).copy()


def candidate_bytes(form, bits):
    return ((bits or (64 if form == COMPACT else 254)) + 7) // 8


def expected_passes(keys, forms, bits):
    """byte positions, below each key's promise, on which two cells differ"""
    passes = 0
    for column, form, b in zip(keys, forms, bits):
        for byte in range(candidate_bytes(form, b)):
            passes += len({(v >> 8 * byte) & 0xFF for v in column}) > 1
    return passes


def second_level_rows(tile):
    """the smallest n whose 256 x ceil(n / tile) counters no longer fit one workgroup of the scan (2 x tile words)"""
    return (2 * tile // 256) * tile + 1


def sizes(tile):
    return (0, 1, 2, 63, 64, 65, 255, 256, 257, tile - 1, tile, tile + 1, 2 * tile + 1, 3 * tile + 77, second_level_rows(tile))


class Case:
    def __init__(self, name, keys, forms=None, bits=None, passes=None):
        self.name, self.keys = name, keys
        self.forms = forms or [(CANONICAL,) * len(keys)]            # every tuple of forms gives the same permutation
        self.bits = bits or (0,) * len(keys)
        self.passes = passes                                         # what the case is ABOUT, where the count is the point
        self.n = len(keys[0])


def shuffled(rng, values):
    values = list(values)
    rng.shuffle(values)
    return values


def cases(n, tile):
    """the key sets of the issue at n rows (those that need a row, two rows or a fixed n only there)"""
    rng = random.Random(0x50525 + n)
    base = rng.randrange(1 << 200) << 40 & ~(0xFFFF << 56)      # bytes 0 .. 4 and 7, 8 clear
    all_forms = [(CANONICAL,), (MONTGOMERY,), (COMPACT,)]
    wide_forms = [(CANONICAL,), (MONTGOMERY,)]
    out = [Case("all equal", [[base + 5] * n], wide_forms, passes=0)]
    if n == 0:
        return out + [Case("two keys, no rows", [[], []], [(CANONICAL, COMPACT)], passes=0)]
    out.append(Case("all equal, compact", [[77] * n], all_forms, passes=0))
    top = shuffled(rng, [(i % 0x31) << 248 for i in range(n)])
    out.append(Case("top byte only", [top], wide_forms, passes=1 if n >= 2 else 0))
    out.append(Case("byte 0 only", [shuffled(rng, [base + i % 256 for i in range(n)])], wide_forms, passes=1 if n >= 2 else 0))
    cross = shuffled(rng, [base + ((i * 37) % 65536 << 56) for i in range(n)])
    out.append(Case("bytes 7 and 8 only", [cross], wide_forms, passes=(0 if n < 2 else 1 if n <= 7 else 2)))
    low = shuffled(rng, [(i * 40503) % (1 << 64) for i in range(n)])
    out.append(Case("below 2^64 in every form", [low], all_forms))
    if n >= 2:
        odd = [base] * n
        odd[rng.randrange(n)] = base + 1
        out.append(Case("all equal but one", [odd], wide_forms, passes=1))
        out.append(Case("0x00 and 0xff in one position", [shuffled(rng, [base + (0xFF << 16) * (i & 1) for i in range(n)])],
                        wide_forms, passes=1))
    rand = [rng.randrange(R_MOD) for _ in range(n)]
    out.append(Case("random 254-bit", [rand], wide_forms))
    out.append(Case("sorted 254-bit", [sorted(rand)]))
    out.append(Case("reversed 254-bit", [sorted(rand, reverse=True)]))
    primary = [rng.randrange(3) for _ in range(n)]
    second = [rng.randrange(1 << 16) for _ in range(n)]
    out.append(Case("two keys", [primary, second], [(CANONICAL, CANONICAL), (COMPACT, MONTGOMERY), (MONTGOMERY, COMPACT)]))
    out.append(Case("three keys", [primary, [v & 3 for v in second], rand], [(COMPACT, CANONICAL, MONTGOMERY)]))
    out.append(Case("a promise that holds", [second], all_forms, bits=(16,)))
    if n == tile + 1:
        out.append(Case("four distinct values", [[(R_MOD - 1, 0, 1 << 64, 255)[rng.randrange(4)] for _ in range(n)]], wide_forms))
    return out


def sentinel_case():
    """0, 1, the values on either side of every limb boundary and r - 1, each three times"""
    return Case("sentinels", [shuffled(random.Random(24), SENTINELS * 3)], [(CANONICAL,), (MONTGOMERY,)])


def run_host(L, keys, forms, bits, width=4):
    """h2_sort_permutation -> (the permutation, the status words)"""
    n = len(keys[0])
    cells = [encode(column, form) for column, form in zip(keys, forms)]
    ptrs = np.array([c.ctypes.data for c in cells], dtype=np.uint64)
    forms, bits = np.array(forms, dtype=np.uint32), np.array(bits, dtype=np.uint32)
    perm = np.zeros(n, dtype=np.uint32 if width == 4 else np.uint64)
    status = np.zeros(4, dtype=np.uint32)
    rc = L.h2_sort_permutation(ptrs.ctypes.data, forms.ctypes.data, bits.ctypes.data, len(keys), n, perm.ctypes.data, width,
                               status.ctypes.data)
    assert rc == 0, L.h2_last_error()
    return [int(v) for v in perm], [int(v) for v in status]


def check(case, run):
    """every tuple of forms of `case` through run(keys, forms, bits) against the definition and the pass count"""
    want = oracle(case.keys)
    for forms in case.forms:
        perm, status = run(case.keys, forms, case.bits)
        assert perm == want, (case.name, case.n, forms)
        passes = expected_passes(case.keys, forms, case.bits)
        assert status == [OK, 0xFFFFFFFF, 0xFFFFFFFF, passes], (case.name, case.n, forms, status)
        assert case.passes is None or passes == case.passes, (case.name, case.n, passes)


def sorted_access_log_columns(circuit):
    """the witness of circuits_frontend.SortedAccessLog by Python integers: [a, t, v, w, A, T, V, W] of `height` elements and
    [inv, s, d] of height - 1"""
    a, t, v, w = ([int(x) for x in col] for col in circuit.witness_inputs())
    H, memory = circuit.height, {}
    for row in range(H):                                                      # the replay, once more, on plain integers
        if w[row]:
            memory[a[row]] = v[row]
        else:
            assert v[row] == memory.get(a[row], 0)
    order = sorted(range(H), key=lambda i: (a[i], t[i]))
    A, T, Vs, W = ([col[i] for i in order] for col in (a, t, v, w))
    delta = [(A[i + 1] - A[i]) % R_MOD for i in range(H - 1)]
    inv = [pow(x, -1, R_MOD) if x else 0 for x in delta]
    s = [(1 - x * y) % R_MOD for x, y in zip(delta, inv)]
    d = [(T[i + 1] - T[i] - 1) % R_MOD if s[i] else (delta[i] - 1) % R_MOD for i in range(H - 1)]
    return [a, t, v, w, A, T, Vs, W, inv, s, d]
