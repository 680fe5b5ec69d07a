"""Cases and the big-integer reference for the rational (`Assigned`) cells: out = num * den^-1 mod r, 0 for a zero
denominator (tests/test_cpu_assigned_boundary.py, tests/test_gpu_assigned.py).  Nothing here needs a device."""
import numpy as np

R_MOD = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001
MONT_R = (1 << 256) % R_MOD
CANONICAL, MONTGOMERY, COMPACT = 0, 1, 2          # H2_ASSIGNED_FORM_*
NONE = 0xFFFFFFFF
MASK64 = (1 << 64) - 1


def reference(num, den):
    """the resolved cells of integer columns: num * den^-1 mod r, 0 where den = 0 (`Assigned::evaluate`)"""
    return [(u * pow(d, -1, R_MOD)) % R_MOD if d % R_MOD else 0 for u, d in zip(num, den)]


def reference_sparse(num, den, rows):
    """... of a sparse column: den[j] belongs to row rows[j], every other row is num"""
    out = [u % R_MOD for u in num]
    for r, v in zip(rows, reference([num[r] for r in rows], den)):
        out[r] = v
    return out


def zero_report(den, rows=None):
    """(the number of zero denominators, the first row that has one or NONE): what the status of a column must say"""
    at = [j if rows is None else int(rows[j]) for j, d in enumerate(den) if d % R_MOD == 0]
    return len(at), (min(at) if at else NONE)


def limbs(values):
    """integers below 2^256 -> an (n, 4) u64 column"""
    out = np.zeros((len(values), 4), dtype=np.uint64)
    for i, v in enumerate(values):
        out[i] = [(v >> (64 * j)) & MASK64 for j in range(4)]
    return out


def ints(column):
    """an (n, 4) u64 column (or a compact 1-D one) -> integers"""
    a = np.asarray(column, dtype=np.uint64)
    if a.ndim == 1:
        return [int(v) for v in a]
    return [int(r[0]) | (int(r[1]) << 64) | (int(r[2]) << 128) | (int(r[3]) << 192) for r in a]


def encode(values, form):
    """integers (below 2^64 for COMPACT) -> the host array of a column in `form`"""
    if form == COMPACT:
        assert all(0 <= v <= MASK64 for v in values)
        return np.array(values, dtype=np.uint64).reshape(-1)
    if form == MONTGOMERY:
        return limbs([(v * MONT_R) % R_MOD for v in values])
    return limbs([v % R_MOD for v in values])


def decode(column, form):
    """the integers a downloaded out column in `form` (CANONICAL or MONTGOMERY) stands for"""
    vals = ints(column)
    if form == MONTGOMERY:
        r_inv = pow(MONT_R, -1, R_MOD)
        return [(v * r_inv) % R_MOD for v in vals]
    return vals


def chain_lanes(count):
    """the lanes a batch inversion of `count` elements runs (batch_invert_threads, csrc/batchinv.hpp): lane t owns the
    elements t, t + lanes, t + 2 lanes, ...; lanes [256 w, 256 w + 256) make workgroup w.  Switches: 8 elements a lane
    below 2^20, 16 below 2^21, 32 below 2^22, 64 from there; one workgroup up to 2048 elements."""
    chunk = 64
    while chunk > 8 and count // chunk < 65536:
        chunk //= 2
    lanes = -(-count // chunk)
    if lanes < 256:
        lanes = min(count, 256)
    return lanes


def random_field(rng, size, small=False):
    """`size` seeded integers: below 2^64 with `small` (what a compact column can hold), else anywhere below r"""
    if small:
        return [int(v) for v in rng.integers(1, 1 << 63, size=size, dtype=np.uint64)]
    words = rng.integers(0, 1 << 63, size=(size, 5), dtype=np.uint64)
    return [(sum(int(w) << (62 * i) for i, w in enumerate(row)) % (R_MOD - 1)) + 1 for row in words]


PATTERNS = ("uniform", "ones", "zeros", "chain ends", "lane", "workgroup", "r-1", "num zero")


def pattern(name, n, seed, small=False):
    """-> (num, den) integer columns of n rows; `small`: every value fits a compact cell (r - 1 then becomes 2^64 - 1)"""
    rng = np.random.Generator(np.random.PCG64(seed))
    num, den = random_field(rng, n, small), random_field(rng, n, small)
    lanes = chain_lanes(n)
    if name == "ones":
        den = [1] * n
    elif name == "zeros":
        den = [0] * n
    elif name == "chain ends":           # the first and the last element of the chains of two lanes, and of the column
        for lane in {0, min(3, lanes - 1), lanes - 1}:
            own = list(range(lane, n, lanes))
            den[own[0]] = den[own[-1]] = 0
        den[n - 1] = 0
    elif name == "lane":                 # every element of one lane's chain
        for j in range(min(5, lanes - 1), n, lanes):
            den[j] = 0
    elif name == "workgroup":            # every element of every lane of the second workgroup (of the only one when lanes <= 256)
        first = 256 if lanes > 256 else 0
        for j in range(n):
            if first <= j % lanes < first + 256:
                den[j] = 0
    elif name == "r-1":
        den = [MASK64 if small else R_MOD - 1] * n
    elif name == "num zero":
        num = [0] * n
    return num, den


# ---- the is-zero circuit -------------------------------------------------------------------------------------------------

def is_zero_circuit(inverse_columns=1):
    """advice v, inv (x inverse_columns: the same gadget side by side), z; fixed selector q:
        q v z = 0        q (z - (1 - v inv)) = 0
    v and z take part in the permutation (a copy constraint ties two rows of each)"""
    from halo2_gpu_specific_amd.circuit import Constant, ConstraintSystem

    cs = ConstraintSystem("is-zero-%d" % inverse_columns)
    q = cs.fixed_column()
    gadgets = []
    for _ in range(inverse_columns):
        v, inv, z = cs.advice_column(), cs.advice_column(), cs.advice_column()
        fq = cs.query_fixed(q)
        av, ai, az = cs.query_advice(v), cs.query_advice(inv), cs.query_advice(z)
        cs.create_gate("is zero", [fq * av * az, fq * (az - (Constant(1) - av * ai))])
        gadgets.append((v, inv, z))
    cs.enable_equality(gadgets[0][0])
    cs.enable_equality(gadgets[0][2])
    return cs


def is_zero_witness(k, seed, inverse_columns=1, blinding=5, zeros=True):
    """-> dict: the witness of is_zero_circuit at 2^k rows in every form the tests hand to the prover.
      "resolved"  canonical (n, 4) host columns, every fraction resolved by big integers (the twin)
      "dense"     the inv columns as Rational(1, v) over (n, 4) columns -- Rational(1, 0) where v = 0
      "compact"   ... over compact 1-D columns (v is below 2^64)
      "sparse"    ... with denominators for the rows where v != 0 only (num = 1 there and 0 elsewhere)
      "fixed" / "fixed_resolved": the selector as a fraction c / c on the usable rows, and resolved
      "copies", "zero_rows" (the rows of the first gadget where v = 0), "n"
    """
    from halo2_gpu_specific_amd.prover import Rational

    n = 1 << k
    usable = n - (blinding + 1)
    rng = np.random.Generator(np.random.PCG64(seed))
    out = {"n": n, "resolved": [], "dense": [], "compact": [], "sparse": []}
    for g in range(inverse_columns):
        v = np.zeros(n, dtype=np.uint64)
        v[:usable] = rng.integers(1, 1 << 62, size=usable, dtype=np.uint64)
        if zeros:
            v[rng.integers(2, usable, size=max(usable // 7, 1))] = 0
        v[1] = v[0]                                                   # the copy constraint (v, 0) = (v, 1)
        vi = [int(x) for x in v]
        inv = [pow(x, -1, R_MOD) if x else 0 for x in vi]
        z = [0 if x else 1 for x in vi[:usable]] + [0] * (n - usable)
        if g == 0:
            out["zero_rows"] = [i for i in range(usable) if vi[i] == 0]
        wide_v, wide_z = limbs(vi), limbs(z)
        ones = np.ones(n, dtype=np.uint64)
        rows = np.array([i for i in range(n) if vi[i]], dtype=np.uint32)
        sparse_num = np.zeros(n, dtype=np.uint64)
        sparse_num[rows] = 1
        out["resolved"] += [wide_v, limbs(inv), wide_z]
        out["dense"] += [wide_v, Rational(limbs([1] * n), wide_v), wide_z]
        out["compact"] += [v.copy(), Rational(ones, v.copy()), np.array(z, dtype=np.uint64)]
        out["sparse"] += [wide_v, Rational(sparse_num, limbs([vi[i] for i in rows]), rows), wide_z]
    c = [int(x) for x in rng.integers(2, 1 << 62, size=n, dtype=np.uint64)]
    sel = [1] * usable + [0] * (n - usable)
    out["fixed_resolved"] = [limbs(sel)]
    out["fixed"] = [Rational(limbs([s * x for s, x in zip(sel, c)]), limbs(c))]
    # (left column position, left row, right column position, right row): v is position 0, z position 1
    out["copies"] = np.array([[0, 0, 0, 1], [1, 0, 1, 1]], dtype=np.int64)
    return out
