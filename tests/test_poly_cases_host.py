"""tests/poly_cases.py without a GPU: its structural constants are the ones in the sources, every case that claims a property has
it, and where the C oracle has the operation its output equals the Python-integer expectation on the small cases -- the two
references of tests/test_gpu_poly_kernels.py kept honest against each other."""
import ctypes
import os
import re

import numpy as np
import pytest

import poly_cases as pc
from h2util import ROOT, _ptr
from poly_cases import R_MOD

CSRC = os.path.join(ROOT, "halo2-gpu-specific_amd", "csrc")


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _one(pattern, text):
    found = re.findall(pattern, text)
    assert len(found) == 1, (pattern, found)
    return found[0]


# ---------------------------------------------------------------------------------------------- constants
def test_scan_constants_are_the_sources():
    scan = _src("scan.hip")
    assert int(_one(r"constexpr int SC_ITEMS = (\d+);", scan)) == pc.SC_ITEMS
    lanes = int(_one(r"constexpr int SC_BLOCK = (\d+) \* SC_ITEMS;", scan))
    assert lanes == pc.SC_LANES and lanes * pc.SC_ITEMS == pc.SC_BLOCK
    assert set(re.findall(r"__launch_bounds__\((\d+)\) k_scan_\w+", scan)) == {str(pc.SC_LANES)}
    assert pc.SCAN_LENGTHS == (1, 2, 3, 4, 5, 1023, 1024, 1025, 2048, 2049, 1 << 20, (1 << 20) + 1)
    # the level structure the two large lengths exist for: level 2 exactly one block; one element more adds a third level
    assert pc.scan_blocks(1 << 20) == [1024, 1] and pc.scan_blocks((1 << 20) + 1) == [1025, 2, 1]
    assert pc.scan_blocks(1024) == [1] and pc.scan_blocks(1025) == [2, 1]


def test_poly_constants_are_the_sources():
    poly = _src("poly.hip")
    assert int(_one(r"const size_t base = \(size_t\)blockIdx\.x \* (\d+);", poly)) == pc.HORNER_BLOCK
    assert int(_one(r"for \(size_t j0 = 0; j0 < count; j0 \+= (\d+)\)", poly)) == pc.EVAL_BATCH_SLICE
    assert int(_one(r"std::min<size_t>\((\d+), count - j0\)", poly)) == pc.EVAL_BATCH_SLICE
    assert int(_one(r"constexpr int LINCOMB_MAX = (\d+);", poly)) == pc.LINCOMB_MAX
    assert _one(r"blockIdx\.x \* \((\d+ \* \d+)\) \+ threadIdx\.x;\s+if \(base >= n\)", poly) == "256 * %d" % pc.DP_ITEMS
    assert _one(r"k_distribute_powers, dim3\(\(unsigned\)\(\(n \+ (\d+)\) / (\d+)\)\)", poly) == (str(pc.DP_BLOCK - 1), str(pc.DP_BLOCK))
    assert int(_one(r"constexpr int PT_ITEMS = (\d+);", poly)) == pc.PT_ITEMS and pc.PT_BLOCK == 8192
    assert _one(r"blockIdx\.x \* \((\d+) \* PT_ITEMS\)", poly) == "256"
    assert int(_one(r"constexpr int MAXBITS_COLS = (\d+);", poly)) == pc.MAXBITS_COLS
    assert _one(r"std::min<size_t>\(\(n \+ (\d+)\) / (\d+), (\d+)\);", poly) == (
        str(pc.MAXBITS_ROWS - 1), str(pc.MAXBITS_ROWS), str(pc.MAXBITS_GRID))
    assert pc.DP_SIZES == (1, 255, 256, 257, 2047, 2048, 2049, 4097, (1 << 20) + 1)
    assert pc.PERM_SIZES == (1, 255, 256, 257, 8191, 8192, 8193, 8192 + 257)
    assert pc.LINCOMB_COUNTS == (0, 1, 8, 9, 16, 17)


def test_batch_invert_constants_are_the_sources():
    h = _src("batchinv.hpp")
    assert int(_one(r"size_t chunk = (\d+);", h)) == pc.BINV_CHUNK_MAX
    assert _one(r"while \(chunk > (\d+) && n / chunk < (\d+)\) chunk /= 2;", h) == (str(pc.BINV_CHUNK_MIN), str(pc.BINV_FILL))
    assert _one(r"if \(nthreads < (\d+)\) nthreads = n < (\d+) \? n : (\d+);", h) == (str(pc.BINV_FLOOR),) * 3
    assert pc.BINV_SIZES == (1, 255, 256, 257, 2040, 2041, 2049, (1 << 20) - 1, 1 << 20, 1 << 21, 1 << 22)
    # the chain length each size exists for (elements of the longest chain), and the forced 256 lanes
    longest = {n: len(pc.chain(n, 0)) for n in pc.BINV_SIZES}
    assert longest == {1: 1, 255: 1, 256: 1, 257: 2, 2040: 8, 2041: 8, 2049: 8, (1 << 20) - 1: 8, 1 << 20: 16, 1 << 21: 32, 1 << 22: 64}
    assert pc.batch_invert_threads(2040) == 256 and (2040 + 7) // 8 == 255          # 255 chains of 8 forced up to a workgroup
    assert pc.batch_invert_threads(2041) == 256 and pc.batch_invert_threads(2049) == 257   # one lane in a second workgroup
    assert pc.batch_invert_threads(1) == 1 and pc.batch_invert_threads(255) == 255


# ---------------------------------------------------------------------------------------------- claims
def test_scan_cases_cover_every_length_and_their_claims_hold():
    cases = pc.scan_cases()
    assert len({c.name for c in cases}) == len(cases)
    for mode in ("kate", "product", "sum"):
        assert {c.L for c in cases if c.mode == mode} == set(pc.SCAN_LENGTHS)
    # three levels in all three modes, and the exact level edge
    for L in pc.SCAN_LARGE:
        assert {c.mode for c in cases if c.L == L} == {"kate", "product", "sum"}
    for c in cases:
        if c.claim is None:
            continue
        kind, p = c.claim
        assert 0 <= p < c.L and pc.position_class_holds(kind, p, c.L), c.name
    # every class of position is planted somewhere, the level-2 ones at the large lengths
    kinds = {c.claim[0] for c in cases if c.claim}
    assert kinds == {"inside_lane", "lane_last", "block_last", "block1_first", "level2_block_last", "level2_block1_first", "last"}
    small = [c for c in cases if c.L <= pc.HOST_TWIN_MAX]
    for c in small:
        arr, scalar = c.make()
        assert arr.shape == (c.L + 1 if c.mode == "kate" else c.L, 4)
        if c.claim:        # one zero factor: everything after it is zero, nothing before
            vals = pc.from_mont(arr)
            p = c.claim[1]
            assert [i for i, v in enumerate(vals) if v == 0] == [p] and scalar != 0
            z = pc.scan_reference(c, arr, scalar)
            assert all(z[: p + 1]) and not any(z[p + 1:]), c.name


def test_scan_closed_forms():
    """the inputs whose expected values have a closed form: the monomial X^(n-1) gives q[i] = b^(n-2-i); a constant factor c
    gives z[i] = init c^i; ones with init 0 sum to z[i] = i; r - 1 wraps at every step"""
    for c in pc.scan_cases():
        if c.L > pc.HOST_TWIN_MAX:
            continue
        arr, s = c.make()
        want = pc.scan_reference(c, arr, s)
        n = c.L + 1
        if c.mode == "kate" and "-monomial-" in c.name:
            assert want == [pow(s, n - 2 - i, R_MOD) for i in range(n - 1)], c.name
        elif c.mode == "kate" and "-zero-" in c.name:
            assert not any(want)
        elif c.mode == "product" and "-constant-" in c.name:
            cv = pc.from_mont(arr[:1])[0]
            assert want == [s * pow(cv, i, R_MOD) % R_MOD for i in range(n)], c.name
        elif c.mode == "product" and "-ones-" in c.name:
            assert want == [s] * n
        elif c.mode == "sum" and "-ones-" in c.name:
            assert s == 0 and want == list(range(n))
        elif c.mode == "sum" and "-rm1-" in c.name:
            assert want == [(s - i) % R_MOD for i in range(n)]


def test_batch_invert_patterns_hold_under_the_thread_count():
    for n in pc.BINV_SIZES:
        nt = pc.batch_invert_threads(n)
        first_t, last_t, ends_t = pc.binv_lanes(n)
        assert first_t < min(nt, 256) and last_t == nt - 1 and last_t // 256 == (nt - 1) // 256   # first / last workgroup
        for pattern in ("chain_zero_first_wg", "chain_zero_last_wg"):
            t = first_t if pattern.endswith("first_wg") else last_t
            planted = pc.binv_planted(n, pattern)
            # a WHOLE chain: exactly the indices congruent to t modulo the lane count
            assert sorted(planted) == [i for i in range(t, n, nt)] and not any(planted.values())
        ends = pc.binv_planted(n, "chain_ends_zero")
        idx = sorted(ends)
        assert idx[0] == ends_t and idx[-1] % nt == ends_t and idx[-1] + nt >= n and not any(ends.values())
        mixed = pc.binv_planted(n, "one_and_rm1")
        assert set(mixed.values()) <= {1, R_MOD - 1} and (n == 1 or set(mixed.values()) == {1, R_MOD - 1})
        if n <= pc.BINV_PYTHON_MAX:
            for case in (c for c in pc.binv_cases() if c.n == n):
                vals = pc.from_mont(case.make())
                zeros = {i for i, v in enumerate(vals) if v == 0}
                if case.pattern == "none":
                    assert not zeros
                elif case.pattern == "all_zero":
                    assert len(zeros) == n
                elif case.pattern == "one_nonzero":
                    assert len(zeros) == n - 1
                else:
                    planted = pc.binv_planted(n, case.pattern)
                    assert zeros == {i for i, v in planted.items() if v == 0}
                    assert all(vals[i] == v for i, v in planted.items())
        # the windows hold every structural position
        for pattern in pc.BINV_PATTERNS:
            spans = pc.windows(n, pc.binv_window_positions(n, pattern))
            covered = lambda p: any(lo <= p < hi for lo, hi in spans)
            assert all(covered(p) for p in (0, n - 1, min(nt, n - 1), min(255, n - 1)))
            assert all(0 <= lo < hi <= n for lo, hi in spans)


def test_other_claims():
    # the 32768-slice: one evaluation more than a launch takes, two or three distinct polynomials, distinct points
    many, three = pc.horner_batches()
    assert len(many.slots) == pc.EVAL_BATCH_SLICE + 1 == len(many.points) == len(set(many.points)) and many.n == 5
    assert set(many.slots) == {0, 1, 2} and len(many.polys) == 3
    assert three.n == 2 * pc.HORNER_BLOCK + 1 and three.points == [0, 1, R_MOD - 1]
    assert all(b.n <= pc.HOST_TWIN_MAX for b in pc.horner_twin_batches())
    # lincomb: 0, 1, r - 1 among the coefficients of every slice that exists
    for count in pc.LINCOMB_COUNTS:
        polys, coeffs = pc.lincomb_inputs(count)
        assert len(polys) == len(coeffs) == count
        for j0 in range(0, count, pc.LINCOMB_MAX):
            if count - j0 >= 4:
                assert {0, 1, R_MOD - 1} & set(coeffs[j0:j0 + pc.LINCOMB_MAX])
    # the root of unity is one, of that order
    assert pow(pc.ROOT_2_28, 1 << 28, R_MOD) == 1 and pow(pc.ROOT_2_28, 1 << 27, R_MOD) == R_MOD - 1
    assert sorted(pc.dp_generators()) == ["one", "random", "rm1", "root_2_28", "zero"]
    assert pc.distribute_powers_reference([5, 6, 7], 0) == [5, 0, 0]
    # permutation: the planted rows make their factor zero, and only those rows
    for n in pc.PERM_SIZES:
        for coeffs in pc.PERM_COEFFS:
            c = pc.perm_case(n, coeffs)
            assert (c.beta == 0) == (coeffs == "beta_zero") and (c.gamma == 0) == (coeffs == "gamma_zero")
            assert {0, 1, 65535} <= set(int(x) for x in c.map_col) or n < 5
            assert {0, n - 1} <= set(int(x) for x in c.map_row) or n < 5
            sigma = pc.sigma_reference(c.map_col, c.map_row, pc.DELTA, c.omega)
            num, den = pc.perm_terms_reference(None, None, c.values[0], sigma, c.beta, c.gamma, c.delta_pows[0], c.omega, True)
            assert [i for i, v in enumerate(num) if v == 0] == [c.num_zero_row]
            num2, den2 = pc.perm_terms_reference(num, den, c.values[1], sigma, c.beta, c.gamma, c.delta_pows[1], c.omega, False)
            # (with beta = 0 numerator and denominator factor are the same gamma + value: the first call's row is zero in both)
            first_den = [c.num_zero_row] if coeffs == "beta_zero" else []
            assert [i for i, v in enumerate(den) if v == 0] == first_den
            assert [i for i, v in enumerate(den2) if v == 0] == sorted(set(first_den + [c.den_zero_row]))
            second_num = [c.den_zero_row] if coeffs == "beta_zero" else []
            assert [i for i, v in enumerate(num2) if v == 0] == sorted(set(second_num + [c.num_zero_row]))   # a zero stays one
    # rotations as C reduces them
    assert [pc.c_rem(a, 7) for a in (7, -7, 10, -15, (1 << 31) - 1, -(1 << 31))] == [0, 0, 3, -1, 1, -2]
    assert pc.rot_index(0, -15, 7) == 6 and pc.rot_index(6, 10, 7) == 2
    for size in pc.ROT_SIZES:
        assert all(abs(r) >= size for r in pc.rotations(size))
    assert pc.vanishing_shapes() == [(64, 1), (64, 2), (64, 64), (64, 64), (64, 128), (1000, 1), (1000, 2), (1000, 64), (1000, 1024), (1000, 2048)]
    # max_scalar_bits: the late value is in the ninth pass of a capped grid and decides its column's answer
    buffers, slots, want = pc.maxbits_case()
    n = pc.MAXBITS_ROWS_N
    assert min((n + pc.MAXBITS_ROWS - 1) // pc.MAXBITS_ROWS, pc.MAXBITS_GRID) == pc.MAXBITS_GRID
    (late, value), = buffers[0]["planted"].items()
    assert late >= pc.MAXBITS_GRID * pc.MAXBITS_ROWS and late // (pc.MAXBITS_GRID * 256) == pc.MAXBITS_ROWS // 256 < n / (pc.MAXBITS_GRID * 256)
    assert value.bit_length() == 200 and buffers[0]["background"].bit_length() == 10
    assert len(slots) == pc.MAXBITS_COLS + 1 and set(slots) == {0, 1, 2} and slots[pc.MAXBITS_COLS] == 0
    assert want == [(200, 0, 253)[s] for s in slots]
    col = pc.maxbits_column(buffers[0], n)
    assert pc.raw_ints(col[late:late + 1]) == [value] and max(pc.raw_ints(col[:late][-4096:])) == 0x3FF


# ---------------------------------------------------------------------------------------------- against the oracle
def test_references_equal_the_oracle_on_the_small_cases(oracle):
    lib = oracle.lib
    sz, vp = ctypes.c_size_t, ctypes.c_void_p
    lib.oracle_distribute_powers.argtypes, lib.oracle_distribute_powers.restype = [vp, sz, vp], None
    # Kate division
    for c in pc.scan_cases():
        if c.mode != "kate" or c.L > pc.HOST_TWIN_MAX:
            continue
        a, b = c.make()
        q = np.zeros((c.L, 4), dtype=np.uint64)
        lib.oracle_kate_division(_ptr(a), c.L + 1, _ptr(pc.fr(b)), _ptr(q))
        assert pc.from_mont(q) == pc.scan_reference(c, a, b), c.name
    # batch inversion
    for c in pc.binv_cases():
        if c.n > pc.BINV_PYTHON_MAX:
            continue
        a = c.make()
        got = a.copy()
        lib.oracle_batch_invert(_ptr(got), c.n)
        assert pc.from_mont(got) == pc.batch_invert_reference(pc.from_mont(a)), c.name
    # Horner
    many, three = pc.horner_batches()
    for batch, js in ((many, list(range(0, len(many.slots), 997)) + [pc.EVAL_BATCH_SLICE - 1, pc.EVAL_BATCH_SLICE]), (three, [0, 1, 2])):
        polys = [pc.to_mont(p) for p in batch.polys]
        for j in js:
            out = np.zeros(4, dtype=np.uint64)
            lib.oracle_eval_polynomial(_ptr(polys[batch.slots[j]]), batch.n, _ptr(pc.fr(batch.points[j])), _ptr(out))
            assert pc.from_mont(out)[0] == pc.horner(batch.polys[batch.slots[j]], batch.points[j])
    # distribute_powers
    for n in pc.DP_SIZES:
        if n > 2 * pc.DP_BLOCK + 1:
            continue
        a = pc.rand_limbs(8450 + n, n)
        for name, g in pc.dp_generators().items():
            got = a.copy()
            lib.oracle_distribute_powers(_ptr(got), n, _ptr(pc.fr(g)))
            assert pc.from_mont(got) == pc.distribute_powers_reference(pc.from_mont(a), g), (n, name)
    # eval_op: every op on the edge cross product, and the rotations
    lv, rv = pc.edge_operands()
    l, r = pc.to_mont(lv), pc.to_mont(rv)
    for op in pc.OPS.values():
        for cv in pc.EDGE_VALUES:
            got = oracle.eval_op(op, l, r if op in pc.OPS_NEED_R else None, 0, 0, pc.fr(cv))   # (l also gives the size)
            assert pc.from_mont(got) == pc.eval_op_reference(op, lv, rv, 0, 0, len(lv), cv), (op, cv)
    for size in pc.ROT_SIZES + (1,):
        lv, rv = pc.rand_ints(8900 + size, size), pc.rand_ints(8901 + size, size)
        l, r = pc.to_mont(lv), pc.to_mont(rv)
        rots = pc.rotations(size)
        for k, rot in enumerate(rots):
            other = rots[(k + 1) % len(rots)]
            got = oracle.eval_op(pc.OPS["SUB"], l, r, rot, other, None)
            assert pc.from_mont(got) == pc.eval_op_reference(pc.OPS["SUB"], lv, rv, rot, other, size, 0), (size, rot)
