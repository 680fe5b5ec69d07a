"""The cases of tests/test_gpu_poly_kernels.py: the elementwise and scan kernels of csrc/poly.hip and csrc/scan.hip at the sizes
and values their structure is made of, with the expected values in Python integers.  No GPU, no torch, no oracle.

Random data at round sizes exercises none of what these kernels consist of: per-lane chains, per-workgroup blocks, recursion
levels, launch slices and multipliers applied by position.  Every size below is derived from the structural constants of the
sources (tests/test_poly_cases_host.py reads them back from scan.hip, poly.hip and batchinv.hpp, so a retune fails there instead
of silently moving a boundary away from its test), and every case that promises a property ("this zero is a block's last
element") carries it as a `claim` that the host test checks.

Values cross the library boundary in Montgomery form, (n, 4) uint64 limbs; the references work on canonical Python integers.
  from_mont / to_mont / fr                 the conversions (bytes-based: a million elements a second)
  rand_limbs                               reproducible stored-form values straight from numpy, for the large cases
  kate_reference, prefix_product_reference, prefix_sum_reference, batch_invert_reference, horner, lincomb_reference,
  distribute_powers_reference, sigma_reference, perm_terms_reference, eval_op_reference, c_rem, windows
"""
from collections import namedtuple

import numpy as np

R_MOD = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001
MONT_R = 1 << 256
R_INV = pow(MONT_R, -1, R_MOD)
ROOT_2_28 = 0x03DDB9F5166D18B798865EA93DD31F743215CF6DD39329C8D34F1ED960C37C9C   # a primitive 2^28-th root of unity
DELTA = 0x09226B6E22C6F0CA64EC26AAD4C86E715B5F898E5E963F25870E56BBE533E9A2

# ------------------------------------------------------------------------------------------ the structural constants
SC_ITEMS, SC_LANES = 4, 256                 # scan.hip: items per lane; lanes per workgroup
SC_BLOCK = SC_ITEMS * SC_LANES              # scan.hip: elements per workgroup = per recursion level
HORNER_BLOCK = 4096                         # poly.hip eval_poly_block: coefficients folded by one workgroup
EVAL_BATCH_SLICE = 32768                    # poly.hip eval_polynomial_batch_launch: evaluations per launch
BINV_CHUNK_MAX, BINV_CHUNK_MIN = 64, 8      # batchinv.hpp batch_invert_threads: chain lengths
BINV_FILL, BINV_FLOOR = 65536, 256          # ... lanes that fill the chip; the one-workgroup floor
LINCOMB_MAX = 8                             # poly.hip: inputs per launch
DP_ITEMS = 8                                # poly.hip k_distribute_powers: strided elements per lane
DP_BLOCK = 256 * DP_ITEMS
PT_ITEMS = 32                               # poly.hip k_perm_terms
PT_BLOCK = 256 * PT_ITEMS
MAXBITS_COLS, MAXBITS_GRID, MAXBITS_ROWS = 16, 256, 2048   # poly.hip max_scalar_bits_launch: columns per launch, grid cap, rows
                                                           # per workgroup below the cap

SCAN_SMALL = (1, 2, 3, SC_ITEMS, SC_ITEMS + 1, SC_BLOCK - 1, SC_BLOCK, SC_BLOCK + 1, 2 * SC_BLOCK, 2 * SC_BLOCK + 1)
SCAN_LARGE = (SC_BLOCK * SC_BLOCK, SC_BLOCK * SC_BLOCK + 1)    # level 2 is exactly one block; a third level exists
SCAN_LENGTHS = SCAN_SMALL + SCAN_LARGE
HOST_TWIN_MAX = 2 * SC_BLOCK + 1            # the host-vector twins run on the boundary sizes up to here

BINV_SIZES = (1, BINV_FLOOR - 1, BINV_FLOOR, BINV_FLOOR + 1, (BINV_FLOOR - 1) * BINV_CHUNK_MIN, (BINV_FLOOR - 1) * BINV_CHUNK_MIN + 1,
              BINV_FLOOR * BINV_CHUNK_MIN + 1, 2 * BINV_CHUNK_MIN * BINV_FILL - 1, 2 * BINV_CHUNK_MIN * BINV_FILL,
              4 * BINV_CHUNK_MIN * BINV_FILL, BINV_CHUNK_MAX * BINV_FILL)
BINV_PYTHON_MAX = 1 << 12                   # above: the oracle at every element, Python integers on windows

LINCOMB_COUNTS = (0, 1, LINCOMB_MAX, LINCOMB_MAX + 1, 2 * LINCOMB_MAX, 2 * LINCOMB_MAX + 1)
LINCOMB_SIZE = 257
DP_SIZES = (1, 255, 256, 257, DP_BLOCK - 1, DP_BLOCK, DP_BLOCK + 1, 2 * DP_BLOCK + 1, (1 << 20) + 1)
PERM_SIZES = (1, 255, 256, 257, PT_BLOCK - 1, PT_BLOCK, PT_BLOCK + 1, PT_BLOCK + 257)
EDGE_VALUES = (0, 1, 2, R_MOD - 2, R_MOD - 1, (R_MOD + 1) // 2)
WIDEN_SIZES = (1, 127, 128, 129)
MAXBITS_ROWS_N = MAXBITS_GRID * MAXBITS_ROWS + 257   # 524288 + 257: past what the capped grid covers in its first 8 passes
MAXBITS_SLOTS = MAXBITS_COLS + 1
WINDOW = 40

OPS = dict(MUL_C=0, SUM_C=1, SUM=2, MUL=3, SUB=4, LCTHETA=5, LCBETA=6, ADDGAMMA=7, CONSTANT=8)   # include/halo2_hip.h H2_OP_*


# ------------------------------------------------------------------------------------------ conversions
def raw_ints(a):
    """(n, 4) uint64 limbs -> the integers they spell, no reduction"""
    buf = np.ascontiguousarray(a, dtype="<u8").tobytes()
    return [int.from_bytes(buf[i:i + 32], "little") for i in range(0, len(buf), 32)]


def raw_limbs(vals):
    """integers < 2^256 -> (n, 4) uint64"""
    if not len(vals):
        return np.zeros((0, 4), dtype=np.uint64)
    return np.frombuffer(b"".join(v.to_bytes(32, "little") for v in vals), dtype="<u8").reshape(-1, 4).astype(np.uint64)


def from_mont(a):
    return [v * R_INV % R_MOD for v in raw_ints(a)]


def to_mont(vals):
    return raw_limbs([v * MONT_R % R_MOD for v in vals])


def fr(v):
    return to_mont([v % R_MOD])[0].copy()


def rand_limbs(seed, n):
    """n stored-form field elements (every integer below r is the Montgomery form of some element): uniform limbs, the top one
    reduced below r's top limb, so that the value is below r whatever the others hold"""
    a = np.random.default_rng(seed).integers(0, 1 << 64, size=(n, 4), dtype=np.uint64)
    a[:, 3] %= np.uint64(R_MOD >> 192)
    return a


def rand_ints(seed, n):
    """n canonical values; zero is not among them in any seed used here (checked by the host test where it matters)"""
    return from_mont(rand_limbs(seed, n))


def windows(n, positions, width=WINDOW):
    """sorted, disjoint [lo, hi) ranges of `width` elements (clipped to [0, n)) that contain every position"""
    spans = sorted((max(0, min(p, n - 1) - width // 2), min(n, max(0, min(p, n - 1) - width // 2) + width)) for p in positions)
    out = []
    for lo, hi in spans:
        if out and lo <= out[-1][1]:
            out[-1] = (out[-1][0], max(out[-1][1], hi))
        else:
            out.append((lo, hi))
    return out


# ------------------------------------------------------------------------------------------ the references
def kate_reference(a, b):
    """q = a / (X - b) without remainder: q[n-2] = a[n-1], q[i] = a[i+1] + b q[i+1]  (arithmetic.rs:754-773)"""
    q, nxt = [0] * (len(a) - 1), 0
    for i in range(len(a) - 2, -1, -1):
        nxt = (a[i + 1] + b * nxt) % R_MOD
        q[i] = nxt
    return q


def prefix_product_reference(f, init):
    """z[0] = init, z[i] = z[i-1] f[i-1]: len(f) + 1 values"""
    z = [init % R_MOD]
    for v in f:
        z.append(z[-1] * v % R_MOD)
    return z


def prefix_sum_reference(f, init):
    z = [init % R_MOD]
    for v in f:
        z.append((z[-1] + v) % R_MOD)
    return z


def batch_invert_reference(a):
    """every non-zero element replaced by its inverse, zeros kept (ff::BatchInvert)"""
    return [pow(v, -1, R_MOD) if v else 0 for v in a]


def horner(poly, x):
    acc = 0
    for c in reversed(poly):
        acc = (acc * x + c) % R_MOD
    return acc


def lincomb_reference(polys, coeffs, size):
    return [sum(c * p[i] for c, p in zip(coeffs, polys)) % R_MOD for i in range(size)]


def distribute_powers_reference(a, g):
    """a[i] g^i, with g^0 = 1 for g = 0 too"""
    out, w = [], 1
    for v in a:
        out.append(v * w % R_MOD)
        w = w * g % R_MOD
    return out


def sigma_reference(map_col, map_row, delta, omega):
    return [pow(delta, int(c), R_MOD) * pow(omega, int(r), R_MOD) % R_MOD for c, r in zip(map_col, map_row)]


def perm_terms_reference(num, den, value, sigma, beta, gamma, delta_pow, omega, first):
    """(num, den) after one h2_dev_permutation_terms call  (permutation/prover.rs:89-128)"""
    out_n, out_d, w = [], [], 1
    for i, v in enumerate(value):
        nu = (delta_pow * w % R_MOD * beta + gamma + v) % R_MOD
        de = (beta * sigma[i] + gamma + v) % R_MOD
        out_n.append(nu if first else nu * num[i] % R_MOD)
        out_d.append(de if first else de * den[i] % R_MOD)
        w = w * omega % R_MOD
    return out_n, out_d


def c_rem(a, b):
    """a % b as C computes it: truncated towards zero, the sign of a"""
    q = abs(a) % abs(b)
    return -q if a < 0 else q


def rot_index(i, rot, size):
    """the element a rotated operand reads at i: the rotation reduced as C's `%` does, then (i + rot) mod size"""
    return (i + c_rem(rot, size)) % size


def eval_op_reference(op, l, r, l_rot, r_rot, size, c):
    out = []
    for i in range(size):
        lv = l[rot_index(i, l_rot, size)] if l is not None else 0
        rv = r[rot_index(i, r_rot, size)] if r is not None else 0
        out.append({
            OPS["MUL_C"]: lv * c, OPS["SUM_C"]: lv + c, OPS["SUM"]: lv + rv, OPS["MUL"]: lv * rv, OPS["SUB"]: lv - rv,
            OPS["LCTHETA"]: lv * c + rv, OPS["LCBETA"]: (lv + c) * rv, OPS["ADDGAMMA"]: lv + c, OPS["CONSTANT"]: c,
        }[op] % R_MOD)
    return out


OPS_NEED_L = frozenset(OPS.values()) - {OPS["CONSTANT"]}
OPS_NEED_R = frozenset(OPS[k] for k in ("SUM", "MUL", "SUB", "LCTHETA", "LCBETA"))


# ------------------------------------------------------------------------------------------ scans
# mode: "kate" (a: L + 1 coefficients, b; q: L), "product" / "sum" (f: L values, init; z: L + 1).  make() -> (stored-form array,
# scalar as a canonical int).  claim: None or (kind, position): the host test checks it.
ScanCase = namedtuple("ScanCase", "name mode L make claim")


def scan_blocks(L):
    """workgroups per recursion level of a scan over L elements"""
    out, c = [], L
    while True:
        c = (c + SC_BLOCK - 1) // SC_BLOCK
        out.append(c)
        if c == 1:
            return out


def _scalar(kind, seed):
    if kind == "random":
        return rand_ints(seed, 1)[0]
    return {"zero": 0, "one": 1, "rm1": R_MOD - 1}[kind]


def _kate_make(L, inp, bkind, seed):
    def make():
        n = L + 1
        if inp == "random":
            a = rand_limbs(seed, n)
        else:
            a = np.zeros((n, 4), dtype=np.uint64)
            if inp == "monomial":
                a[n - 1] = fr(1)
        return a, _scalar(bkind, seed + 1)
    return make


def _scan_make(L, inp, ikind, seed, zero_at=None):
    def make():
        if inp == "random":
            f = rand_limbs(seed, L)
        elif inp == "constant":
            f = np.tile(rand_limbs(seed, 1), (L, 1))
        elif inp == "ones":
            f = np.tile(fr(1), (L, 1))
        else:
            assert inp == "rm1"
            f = np.tile(fr(R_MOD - 1), (L, 1))
        if zero_at is not None:
            f[zero_at] = 0
        return f, _scalar(ikind, seed + 1)
    return make


# the classes of position a single zero factor can have
def zero_positions(L):
    """{class: index into the L factors} for the classes that exist at this length"""
    lane = 5 if L > SC_ITEMS * 6 else 0
    want = {
        "inside_lane": SC_ITEMS * lane + 1,           # neither first nor last of a lane's four
        "lane_last": SC_ITEMS * lane + SC_ITEMS - 1,
        "block_last": SC_BLOCK - 1,
        "block1_first": SC_BLOCK,
        "level2_block_last": SC_BLOCK * SC_BLOCK - 1,  # the last element whose block aggregate lies in level-2 block 0
        "level2_block1_first": SC_BLOCK * SC_BLOCK,
        "last": L - 1,
    }
    return {k: p for k, p in want.items() if p < L}


def position_class_holds(kind, p, L):
    """the restatement of what zero_positions promises, from the kernel's index arithmetic: lane t of block B scans elements
    B * SC_BLOCK + SC_ITEMS * t + k, k < SC_ITEMS"""
    k, blk = p % SC_ITEMS, p // SC_BLOCK
    return {
        "inside_lane": 0 < k < SC_ITEMS - 1,
        "lane_last": k == SC_ITEMS - 1 and p % SC_BLOCK != SC_BLOCK - 1,
        "block_last": p % SC_BLOCK == SC_BLOCK - 1 and blk == 0,
        "block1_first": p % SC_BLOCK == 0 and blk == 1,
        "level2_block_last": p % SC_BLOCK == SC_BLOCK - 1 and blk % SC_BLOCK == SC_BLOCK - 1 and blk // SC_BLOCK == 0,
        "level2_block1_first": p % SC_BLOCK == 0 and blk % SC_BLOCK == 0 and blk // SC_BLOCK == 1,
        "last": p == L - 1,
    }[kind]


def scan_cases():
    out, seed = [], 1000
    for L in SCAN_LENGTHS:
        large = L in SCAN_LARGE
        # Kate division
        combos = [(i, b) for i in ("random", "zero", "monomial") for b in ("zero", "one", "rm1", "random")]
        if large:   # every b against random data; the monomial (each positional multiplier by itself) and zero once
            combos = [("random", b) for b in ("zero", "one", "rm1", "random")] + [("monomial", "random"), ("zero", "random")]
        for inp, b in combos:
            seed += 2
            out.append(ScanCase("kate-%d-%s-b_%s" % (L, inp, b), "kate", L, _kate_make(L, inp, b, seed), None))
        # prefix product
        combos = [(i, z) for i in ("random", "constant", "ones") for z in ("zero", "one", "random")]
        if large:
            combos = [("random", "random"), ("constant", "one"), ("ones", "random"), ("random", "zero")]
        for inp, init in combos:
            seed += 2
            out.append(ScanCase("product-%d-%s-init_%s" % (L, inp, init), "product", L, _scan_make(L, inp, init, seed), None))
        for kind, p in zero_positions(L).items():
            if large and kind in ("inside_lane", "lane_last"):
                continue
            seed += 2
            out.append(ScanCase("product-%d-zero_%s" % (L, kind), "product", L, _scan_make(L, "random", "random", seed, zero_at=p),
                                (kind, p)))
        # prefix sum
        for inp, init in (("random", "random"), ("random", "zero"), ("rm1", "random"), ("ones", "zero")):
            seed += 2
            out.append(ScanCase("sum-%d-%s-init_%s" % (L, inp, init), "sum", L, _scan_make(L, inp, init, seed), None))
    return out


def scan_reference(case, arr, scalar):
    vals = from_mont(arr)
    return {"kate": kate_reference, "product": prefix_product_reference, "sum": prefix_sum_reference}[case.mode](vals, scalar)


# ------------------------------------------------------------------------------------------ batch inversion
def batch_invert_threads(n):
    """batchinv.hpp::batch_invert_threads"""
    chunk = BINV_CHUNK_MAX
    while chunk > BINV_CHUNK_MIN and n // chunk < BINV_FILL:
        chunk //= 2
    nthreads = (n + chunk - 1) // chunk
    if nthreads < BINV_FLOOR:
        nthreads = n if n < BINV_FLOOR else BINV_FLOOR
    return nthreads


def chain(n, t):
    """the elements lane t of k_batch_invert walks: t, t + nthreads, ..."""
    return range(t, n, batch_invert_threads(n))


BINV_PATTERNS = ("none", "all_zero", "one_nonzero", "chain_zero_first_wg", "chain_zero_last_wg", "chain_ends_zero", "one_and_rm1")
BinvCase = namedtuple("BinvCase", "name n pattern make")


def binv_lanes(n):
    """the lanes the patterns plant into: (a lane of the first workgroup, the last active lane, the lane whose chain ends are zeroed)"""
    nt = batch_invert_threads(n)
    return min(3, nt - 1), nt - 1, min(1, nt - 1)


def binv_planted(n, pattern):
    """the indices a pattern sets, {index: canonical value}; all_zero / one_nonzero are described by the index they keep"""
    first_t, last_t, ends_t = binv_lanes(n)
    if pattern == "chain_zero_first_wg":
        return {i: 0 for i in chain(n, first_t)}
    if pattern == "chain_zero_last_wg":
        return {i: 0 for i in chain(n, last_t)}
    if pattern == "chain_ends_zero":
        c = chain(n, ends_t)
        return {c[0]: 0, c[-1]: 0}
    if pattern == "one_and_rm1":
        c = chain(n, first_t)
        planted = {i: (1 if k % 2 == 0 else R_MOD - 1) for k, i in enumerate(c)}
        planted[n - 1] = R_MOD - 1
        planted[0] = 1
        return planted
    return {}


_base = {}


def _binv_base(n):
    if n not in _base:
        _base.clear()                       # one large array at a time
        _base[n] = rand_limbs(7000 + n % 9973, n)
    return _base[n]


def _binv_make(n, pattern):
    def make():
        if pattern == "all_zero":
            return np.zeros((n, 4), dtype=np.uint64)
        if pattern == "one_nonzero":
            a = np.zeros((n, 4), dtype=np.uint64)
            a[n // 2] = rand_limbs(77, 1)[0]
            return a
        a = _binv_base(n).copy()
        planted = binv_planted(n, pattern)
        if planted:
            idx = sorted(planted)
            a[idx] = to_mont([planted[i] for i in idx])
        return a
    return make


def binv_cases():
    return [BinvCase("binv-%d-%s" % (n, p), n, p, _binv_make(n, p)) for n in BINV_SIZES for p in BINV_PATTERNS]


def binv_window_positions(n, pattern):
    """every structural position of a case: the ends, the workgroup and lane-stride edges, the planted elements"""
    nt = batch_invert_threads(n)
    pos = [0, n - 1, n // 2, BINV_FLOOR - 1, BINV_FLOOR, nt - 1, nt, 2 * nt - 1, 2 * nt, n - nt, (n - 1) // nt * nt]
    planted = sorted(binv_planted(n, pattern))
    pos += planted[:2] + planted[-2:] + planted[len(planted) // 2:len(planted) // 2 + 1]
    return [p for p in pos if 0 <= p < n]


# ------------------------------------------------------------------------------------------ Horner
HornerBatch = namedtuple("HornerBatch", "name n polys slots points")   # polys: canonical coefficient lists; slots[j]: polynomial
                                                                       # of evaluation j; points[j]: canonical


def horner_batches():
    count = EVAL_BATCH_SLICE + 1
    pts = rand_ints(8100, count)
    pts[:3] = [0, 1, R_MOD - 1]
    pts[EVAL_BATCH_SLICE - 1], pts[EVAL_BATCH_SLICE] = 2, R_MOD - 2       # either side of the slice edge
    many = HornerBatch("batch-%d-n5" % count, 5, [rand_ints(8000 + j, 5) for j in range(3)],
                       [(j * 7 + j // EVAL_BATCH_SLICE) % 3 for j in range(count)], pts)
    n = 2 * HORNER_BLOCK + 1
    three = HornerBatch("batch-3-n%d" % n, n, [rand_ints(8010 + j, n) for j in range(3)], [0, 1, 2], [0, 1, R_MOD - 1])
    return [many, three]


def horner_twin_batches():
    """the host-vector twin's sizes: up to HOST_TWIN_MAX coefficients"""
    out = []
    for n, count in ((1, 3), (BINV_FLOOR + 1, 3), (HOST_TWIN_MAX, 2)):
        out.append(HornerBatch("twin-%d-n%d" % (count, n), n, [rand_ints(8020 + n % 89 + j, n) for j in range(count)],
                               list(range(count)), ([0, R_MOD - 1] + rand_ints(8030, 1))[:count] if count == 3 else rand_ints(8031, 2)))
    return out


# ------------------------------------------------------------------------------------------ lincomb
def lincomb_inputs(count):
    """(polys, coeffs) as canonical lists: coefficients 0, 1, r - 1 among random ones, placed so that every slice of
    LINCOMB_MAX inputs has one of them"""
    polys = [rand_ints(8200 + j, LINCOMB_SIZE) for j in range(count)]
    coeffs = rand_ints(8300 + count, count) if count else []
    for j, v in ((0, R_MOD - 1), (3, 0), (LINCOMB_MAX - 1, 1), (LINCOMB_MAX, R_MOD - 1), (2 * LINCOMB_MAX - 1, 0), (2 * LINCOMB_MAX, 1)):
        if j < count:
            coeffs[j] = v
    if count == 1:
        coeffs[0] = rand_ints(8299, 1)[0]
    return polys, coeffs


# ------------------------------------------------------------------------------------------ distribute_powers
def dp_generators():
    return {"zero": 0, "one": 1, "rm1": R_MOD - 1, "root_2_28": ROOT_2_28, "random": rand_ints(8400, 1)[0]}


# ------------------------------------------------------------------------------------------ permutation sigma and terms
PermCase = namedtuple("PermCase", "name n map_col map_row omega beta gamma delta_pows values num_zero_row den_zero_row")


def perm_case(n, coeffs):
    """one sigma column and two h2_dev_permutation_terms calls (first, multiplying) over it.  Row num_zero_row of the FIRST call's
    value makes the numerator factor zero, row den_zero_row of the SECOND call's value the denominator factor."""
    rng = np.random.default_rng(8500 + n)
    map_col = rng.integers(0, 5, size=n).astype(np.uint32)
    map_row = rng.integers(0, n, size=n).astype(np.uint32)
    for k, (c, r) in enumerate(((0, 0), (1, n - 1), (65535, 0), (65535, n - 1), (0, n - 1))):
        if k < n:
            map_col[(k * 97) % n], map_row[(k * 97) % n] = c, r
    omega = rand_ints(8600, 1)[0]
    beta, gamma = rand_ints(8601 + n, 2)
    if coeffs == "beta_zero":
        beta = 0
    elif coeffs == "gamma_zero":
        gamma = 0
    delta_pows = [pow(DELTA, 3, R_MOD), pow(DELTA, 4, R_MOD)]
    values = [rand_ints(8700 + n % 101 + j, n) for j in range(2)]
    sigma = sigma_reference(map_col, map_row, DELTA, omega)
    num_zero_row, den_zero_row = n - 1, (n // 2 if n > 1 else 0)
    values[0][num_zero_row] = -(delta_pows[0] * beta * pow(omega, num_zero_row, R_MOD) + gamma) % R_MOD
    values[1][den_zero_row] = -(beta * sigma[den_zero_row] + gamma) % R_MOD
    return PermCase("perm-%d-%s" % (n, coeffs), n, map_col, map_row, omega, beta, gamma, delta_pows, values, num_zero_row, den_zero_row)


PERM_COEFFS = ("random", "beta_zero", "gamma_zero")

# ------------------------------------------------------------------------------------------ eval_op
ROT_SIZES = (7, 257)


def rotations(size):
    return (size, -size, size + 3, -(2 * size + 1), (1 << 31) - 1, -(1 << 31))


def edge_operands():
    """(l, r): the cross product of EDGE_VALUES with itself, element i = (l[i], r[i])"""
    pairs = [(a, b) for a in EDGE_VALUES for b in EDGE_VALUES]
    return [a for a, _ in pairs], [b for _, b in pairs]


# ------------------------------------------------------------------------------------------ divide_by_vanishing, widen, max bits
def vanishing_shapes():
    """(size, t_len): t_len a power of two as the launcher requires; 1000 is no multiple of 256 and no power of two, so `size`
    and `2 size` are taken as the powers of two above it"""
    out = []
    for size, full in ((64, 64), (1000, 1024)):
        out += [(size, t) for t in (1, 2, 64, full, 2 * full)]
    return out


def widen_values(n):
    v = [int(x) for x in np.random.default_rng(8800 + n).integers(0, 1 << 64, size=n, dtype=np.uint64)]
    v[0] = (1 << 64) - 1
    if n > 2:
        v[n // 2], v[n - 1] = 0, (1 << 64) - 1
    return v


def maxbits_case():
    """(buffers, slots, want): three CANONICAL columns of MAXBITS_ROWS_N rows as {row: value} over a small background, the buffer
    of each of the 17 slots, and the expected bit lengths.  Buffer 0's only large value sits in a row that the capped grid
    reaches in its ninth grid-stride pass and no earlier; buffer 1 is all zero; buffer 2's sits in the last row."""
    n = MAXBITS_ROWS_N
    late = MAXBITS_GRID * MAXBITS_ROWS + 5
    buffers = [
        {"background": 0x3FF, "planted": {late: (1 << 199) | 1}},
        {"background": 0, "planted": {}},
        {"background": 0xFFFF, "planted": {n - 1: 1 << 252, 0: 1 << 64}},
    ]
    slots = [(0, 1, 2)[j % 3] for j in range(MAXBITS_SLOTS)]
    slots[MAXBITS_COLS] = 0                       # the slot of the second launch looks at the late value too
    bits = [max([b["background"]] + list(b["planted"].values())).bit_length() for b in buffers]
    return buffers, slots, [bits[s] for s in slots]


def maxbits_column(buf, n):
    """the canonical (n, 4) column of a maxbits_case buffer: background * (row % 2) and the planted rows"""
    a = np.zeros((n, 4), dtype=np.uint64)
    a[1::2, 0] = buf["background"]
    for row, v in buf["planted"].items():
        a[row] = raw_limbs([v])[0]
    return a
