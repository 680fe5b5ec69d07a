"""Copy-constraint sets for the permutation mapping (prover.permutation_mapping on the host, permutation_mapping_device /
csrc/permmap.hip on the device), shared by tests/test_perm_mapping_cases_host.py and tests/test_gpu_perm_mapping.py.
Every generator returns (ncols, n, copies): copies an (m, 4) int64 array of (left column position, left row, right column
position, right row).  CASES are the sizes the device tests run; SMALL_CASES are cases 1-9 with n <= 2^10, small enough
for the big-integer twin (ref_plonk.permutation_mapping, pure Python)."""
import numpy as np


def sort_tile():
    """T: the (label, cell) pairs one workgroup of the device's radix sort ranks"""
    from halo2_gpu_specific_amd.prover import PERM_MAPPING_SORT_TILE

    return PERM_MAPPING_SORT_TILE


def _rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def _arr(rows):
    return np.array(rows, dtype=np.int64).reshape(-1, 4)


def _cells_to_copies(n, left, right):
    """cell ids (column position * n + row) -> copies"""
    left, right = np.asarray(left, dtype=np.int64), np.asarray(right, dtype=np.int64)
    return np.stack([left // n, left % n, right // n, right % n], axis=1)


def no_copies():
    return 2, 8, _arr([])


def self_copy():
    return 2, 8, _arr([(1, 3, 1, 3)])


def twice_and_reversed():
    return 2, 8, _arr([(0, 1, 1, 2), (0, 1, 1, 2), (1, 2, 0, 1)])


def three_column_cycle():
    """one cycle through the first and the last cell of the table"""
    ncols, n = 3, 8
    return ncols, n, _arr([(0, 0, 1, 4), (ncols - 1, n - 1, 1, 4), (1, 4, 0, 0)])


def chain(k, order):
    """cell i of column 1 copied to cell i + 1, over the whole column: one cycle of n cells"""
    n = 1 << k
    i = np.arange(n - 1, dtype=np.int64)
    if order == "descending":
        i = i[::-1]
    elif order == "shuffled":
        i = _rng(5).permutation(i)
    one = np.ones_like(i)
    return 2, n, np.stack([one, i, one, i + 1], axis=1)


def star(k, leaves):
    """cell (1, 5) copied to `leaves` random cells (with repeats, the centre itself possibly among them)"""
    ncols, n = 3, 1 << k
    to = _rng(6).integers(0, ncols * n, size=leaves)
    return ncols, n, _cells_to_copies(n, np.full(leaves, n + 5), to)


def pairs(k):
    """every cell of two columns in exactly one pair: 2^k disjoint pairs"""
    n = 1 << k
    p = _rng(7).permutation(2 * n)
    return 2, n, _cells_to_copies(n, p[:n], p[n:])


def random_copies(m, seed=8, ncols=3, k=10):
    n = 1 << k
    r = _rng(seed + m)
    return ncols, n, _cells_to_copies(n, r.integers(0, ncols * n, size=m), r.integers(0, ncols * n, size=m))


def touched(count):
    """copies that touch exactly `count` distinct cells: disjoint pairs, and one self-copy when the count is odd"""
    ncols, n = 5, 1 << 10
    assert count <= ncols * n
    p = _rng(9).permutation(ncols * n)[:count]
    half = count // 2
    left, right = list(p[:half]), list(p[half:2 * half])
    if count % 2:
        left.append(p[-1])
        right.append(p[-1])
    return ncols, n, _cells_to_copies(n, left, right)


def wide_labels():
    """5 columns of 2^22 rows: the labels of the last two columns need more than 24 bits, so every one of the four radix
    passes carries non-zero digits.  2^16 random copies confined to those columns, and one chain of 2^12 there."""
    ncols, k = 5, 22
    n = 1 << k
    r = _rng(10)
    lo, hi = (ncols - 2) * n, ncols * n
    left, right = r.integers(lo, hi, size=1 << 16), r.integers(lo, hi, size=1 << 16)
    start = (ncols - 1) * n + 12345
    i = start + r.permutation(1 << 12)
    return ncols, n, _cells_to_copies(n, np.concatenate([left, i]), np.concatenate([right, i + 1]))


N_RANDOM = 3 << 10                          # the cells of random_copies
CASES = {
    "none": no_copies,
    "self-copy": self_copy,
    "twice-and-reversed": twice_and_reversed,
    "three-column-cycle": three_column_cycle,
    "chain-ascending": lambda: chain(16, "ascending"),
    "chain-descending": lambda: chain(16, "descending"),
    "chain-shuffled": lambda: chain(16, "shuffled"),
    "star": lambda: star(13, 1 << 14),
    "pairs": lambda: pairs(15),
    "random-1": lambda: random_copies(1),
    "random-7": lambda: random_copies(7),
    "random-N/2": lambda: random_copies(N_RANDOM // 2),
    "random-2N": lambda: random_copies(2 * N_RANDOM),
    "touched-T-1": lambda: touched(sort_tile() - 1),
    "touched-T": lambda: touched(sort_tile()),
    "touched-T+1": lambda: touched(sort_tile() + 1),
    "wide-labels": wide_labels,
}
SMALL_CASES = dict(CASES)
del SMALL_CASES["wide-labels"]
SMALL_CASES.update({
    "chain-ascending": lambda: chain(10, "ascending"),
    "chain-descending": lambda: chain(10, "descending"),
    "chain-shuffled": lambda: chain(10, "shuffled"),
    "star": lambda: star(10, 1 << 11),
    "pairs": lambda: pairs(10),
})
