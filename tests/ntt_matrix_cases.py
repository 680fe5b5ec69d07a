"""The NTT test matrix (tests/test_gpu_ntt_matrix.py): which transforms are run, and what each one has to give.

Nothing here needs a GPU.  The enumeration asks the library's own h2_ntt_shape for the width of the first pass (the paddings
are placed around it) and for the kernel every pass of a case runs, so a CPU test can assert that the matrix still reaches
every kernel after a change of ntt_split or pass_shape (tests/test_cpu_boundary.py).

The expected values come in two layers, both bit for bit:
 (a) the whole output vector from the oracle's FFT (oracle.best_fft on 8 threads) over an input prepared on the CPU --
     zero padding, the pre3 scale of coeff_to_extended, the g^i of a coset transform -- and scaled on the CPU afterwards
     (divisor, the post3 of extended_to_coeff, g^-i), with the oracle's elementwise products only;
 (b) without the oracle's FFT: eight entries of that vector -- 0, 1, n/2, n - 1 and four seeded ones -- against the
     definition X[i] = post(i) * sum_j x'_j w^(ij), by Horner over the live inputs: Python integers up to 2^16 inputs, the
     oracle's Horner (oracle_eval_polynomial, in chunks on 8 threads) above.  The post factor is a Python integer always.
     A delta input has its whole expected vector in closed form, c w^(jk) post(k): that vector is what the device is
     compared with (and, up to 2^18, it is compared with the oracle's FFT as well).
"""
import ctypes
import random
import zlib
from collections import namedtuple

import numpy as np

from h2util import R_MOD, fr_mont

ROOT_W = 0x03DDB9F5166D18B798865EA93DD31F743215CF6DD39329C8D34F1ED960C37C9C  # of order 2^28
ORACLE_THREADS = 8

# h2_ntt_shape's kernel ids (H2_NTT_KERNEL_* in include/halo2_hip.h): one per launch of ntt_run_chunk
KERNELS = (
    "k_ntt_pass8<true>",
    "k_ntt_pass8<false>",
    "k_ntt_pass<true, true>",
    "k_ntt_pass<true, false>",
    "k_ntt_pass<false>",
)
ALL_KERNELS = frozenset(range(len(KERNELS)))
# the common pass (middle and last), the radix-4 kernel (a first pass of another width or with padding to skip; the 9-bit
# last pass), and below 2^18 the radix-2 kernel: every kernel runs with no knob set
DEFAULT_KERNELS = ALL_KERNELS

SHAPE_FIELDS = ("bits", "log_c", "threads", "radix4", "fixed", "zskip", "kernel")

OPS = ("ntt", "intt", "coeff_to_extended", "extended_to_coeff", "coset_ntt", "coset_intt")
# where the entry point allows both, source == destination and source != destination
PLACES = {
    "ntt": ("in",), "intt": ("in",), "coeff_to_extended": ("out", "in"), "extended_to_coeff": ("in",),
    "coset_ntt": ("out", "in"), "coset_intt": ("in",),
}
INPUTS = ("random", "zero", "rm1", "alt", "delta1", "delta_last", "delta_seeded")

FULL_SIZES = (9, 10, 16, 17, 18, 19, 20, 21)
# 2^22: every entry point and every padding, three of the seven inputs; 2^23 and 2^24: the rows that change kernel there.
# Thinned for time, the largest sizes first: the oracle's FFTs are most of this module's wall clock, and every kernel id of
# these sizes is also reached at 2^19 .. 2^21 with the full product.
FEWER_INPUTS_SIZES = (22,)
THIN_SIZES = (23, 24)
THIN_OPS = ("ntt", "intt", "coeff_to_extended", "coset_ntt", "coset_intt")
THIN_INPUTS = ("random", "rm1", "delta_seeded")
MATRIX_SIZES = FULL_SIZES + FEWER_INPUTS_SIZES + THIN_SIZES
BATCH_SIZES = (18, 20)
BATCH_COUNTS = (1, 2, 16, 17)
BATCH_OPS = ("ntt_batch", "intt_batch", "coset_ntt_batch", "coeff_to_extended_batch")

# one child process per setting (each knob is read once per process)
KNOBS = ("H2_NTT_NINE", "H2_NTT_NO_ZSKIP", "H2_NTT_LAST_TABLE", "H2_NTT_LAST_TABLE_MAX_LOG", "H2_NTT_TABLE_BUDGET")
KNOB_SETTINGS = (
    {"H2_NTT_NINE": "0"},
    {"H2_NTT_NO_ZSKIP": "1"},
    {"H2_NTT_LAST_TABLE": "0"},
)
CHILD_SIZES = (17, 18, 19, 20)
CHILD_INPUTS = ("random", "rm1")

Case = namedtuple("Case", "op z inp arbitrary")


# ------------------------------------------------------------------ the library's plan of a transform
def ntt_shape(L, log_n, in_log):
    """h2_ntt_shape as a list of dicts, one per pass"""
    out = np.zeros((8, len(SHAPE_FIELDS)), dtype=np.uint32)
    count = ctypes.c_size_t()
    rc = L.h2_ntt_shape(log_n, in_log, out.ctypes.data, len(out), ctypes.byref(count))
    assert rc == 0, ("h2_ntt_shape", log_n, in_log, rc)
    return [dict(zip(SHAPE_FIELDS, (int(v) for v in row))) for row in out[: count.value]]


def kernel_ids(L, log_n, z=0):
    return frozenset(p["kernel"] for p in ntt_shape(L, log_n, log_n - z))


def first_width(L, log_n):
    return ntt_shape(L, log_n, log_n)[0]["bits"]


def paddings(L, log_n):
    """z = extended_k - k: none, the small ones, around the first pass's width B (z >= B leaves one live row and no stage in
    the first pass) and down to a single coefficient"""
    B = first_width(L, log_n)
    out = []
    for z in (0, 1, 2, 3, B - 1, B, B + 1, log_n - 1, log_n):
        if 0 <= z <= log_n and z not in out:
            out.append(z)
    return out


def matrix_cases(L, log_n):
    """the single-vector rows of one size"""
    thin = log_n in THIN_SIZES
    inputs = INPUTS if log_n in FULL_SIZES else THIN_INPUTS
    B = first_width(L, log_n)
    cases = []
    for op in (THIN_OPS if thin else OPS):
        zs = ([1, 2, 3, B] if thin else paddings(L, log_n)) if op == "coeff_to_extended" else [0]
        for zi, z in enumerate(zs):
            for ii, inp in enumerate(inputs):
                # pre3 / post3 constants that are NOT zeta and zeta^2 in half the rows: a swapped pair cannot cancel
                arbitrary = (zi % 2 == 1) if op == "coeff_to_extended" else (op == "extended_to_coeff" and ii % 2 == 1)
                cases.append(Case(op, z, inp, arbitrary))
    return cases


def child_cases(L, log_n):
    """the thinned rows every knob setting runs"""
    B = first_width(L, log_n)
    cases = []
    for op in OPS:
        zs = sorted({0, 1, B}) if op == "coeff_to_extended" else [0]
        for zi, z in enumerate(zs):
            for inp in CHILD_INPUTS:
                cases.append(Case(op, z, inp, zi % 2 == 1 or op == "extended_to_coeff"))
    return cases


def batch_paddings(L, log_n):
    B = first_width(L, log_n)
    return [z for z in (1, 3, B) if z in paddings(L, log_n)]


def matrix_kernel_ids(L):
    """kernel id -> the (log_n, z) of the matrix that reach it under this process's knobs"""
    reach = {}
    for log_n in MATRIX_SIZES:
        for z in sorted({c.z for c in matrix_cases(L, log_n)}):
            for k in kernel_ids(L, log_n, z):
                reach.setdefault(k, []).append((log_n, z))
    return reach


# ------------------------------------------------------------------ expected values
OP_MUL_C, OP_MUL = 0, 3  # oracle_eval_op


def _mont_ints(a):
    """(n, 4) uint64 rows -> Python integers (the Montgomery residues as they are)"""
    raw = np.ascontiguousarray(a, dtype="<u8").tobytes()
    return [int.from_bytes(raw[i : i + 32], "little") for i in range(0, len(raw), 32)]


def _mont_int(row):
    return _mont_ints(np.asarray(row).reshape(1, 4))[0]


class Reference:
    """expected outputs of the six transforms at one size"""

    def __init__(self, oracle, log_n):
        self.o, self.log_n, self.n = oracle, log_n, 1 << log_n
        self.w = pow(ROOT_W, 1 << (28 - log_n), R_MOD)
        self.w_inv = pow(self.w, -1, R_MOD)
        self.d = pow(self.n, -1, R_MOD)
        self.g = 7 * pow(ROOT_W, 5, R_MOD) % R_MOD  # a coset generator: no power of w
        self.g_inv = pow(self.g, -1, R_MOD)
        dom, _ = oracle.domain(3, 4)
        one = _mont_int(fr_mont(1))
        self.zeta = (_mont_int(dom.fr("g_coset")) * pow(one, -1, R_MOD) % R_MOD,
                     _mont_int(dom.fr("g_coset_inv")) * pow(one, -1, R_MOD) % R_MOD)
        self.arbitrary = (0x1F3C5A79B2D4E6F8091A2B3C4D5E6F708192A3B4C5D6E7F8091A2B3C4D5E6F71 % R_MOD,
                          0x2A4C6E8091B3D5F7192B3D4F5A6C7E8091A3B5C7D9EBFD0F21436587A9CBED0F % R_MOD)
        self._powers, self._inputs = {}, {}
        lib = oracle.lib
        lib.oracle_eval_polynomial_par.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_int,
                                                   ctypes.c_void_p]
        lib.oracle_eval_polynomial_par.restype = None

    # ---- building blocks: the oracle's elementwise products
    def powers(self, base):
        """base^i, i < n, by doubling (log n elementwise products by a constant)"""
        if base not in self._powers:
            out = np.empty((self.n, 4), dtype=np.uint64)
            out[0] = fr_mont(1)
            m = 1
            while m < self.n:
                out[m : 2 * m] = self.o.eval_op(OP_MUL_C, np.ascontiguousarray(out[:m]), None, 0, 0, fr_mont(pow(base, m, R_MOD)))
                m *= 2
            while len(self._powers) >= 6:
                self._powers.pop(next(iter(self._powers)))  # the oldest
            self._powers[base] = out
        return self._powers[base]

    def scale(self, a, c):
        self.o.lib.oracle_poly_scale(a.ctypes.data, fr_mont(c).ctypes.data, len(a), ORACLE_THREADS)

    def zeta_scale(self, a, pair, into_coset):
        """a[i] *= pair[0] (i % 3 == 1), pair[1] (i % 3 == 2) into the coset, the other way round out of it"""
        g, gi = fr_mont(pair[0]), fr_mont(pair[1])
        self.o.lib.oracle_distribute_powers_zeta(a.ctypes.data, len(a), g.ctypes.data, gi.ctypes.data, 1 if into_coset else 0,
                                                 ORACLE_THREADS)

    # ---- inputs
    def delta_position(self, inp, in_len):
        if inp == "delta1":
            return min(1, in_len - 1)
        if inp == "delta_last":
            return in_len - 1
        if inp == "delta_seeded":
            return random.Random(0xD17A + 31 * self.log_n + in_len).randrange(in_len)
        return None

    def raw_input(self, inp, in_len):
        key = (inp, in_len)
        if key not in self._inputs:
            if inp == "random":
                x = self.o.random_fr(0x9000 + 64 * self.log_n + in_len.bit_length(), in_len)
            else:
                x = np.zeros((in_len, 4), dtype=np.uint64)
                if inp == "rm1":
                    x[:] = fr_mont(R_MOD - 1)
                elif inp == "alt":
                    x[1::2] = fr_mont(R_MOD - 1)
                elif inp != "zero":
                    x[self.delta_position(inp, in_len)] = fr_mont(1)
            self._inputs[key] = x
        return self._inputs[key]

    # ---- one case
    def constants(self, case):
        return self.arbitrary if case.arbitrary else self.zeta

    def spec(self, case):
        """(the number of live inputs, the root of the transform)"""
        root = self.w if case.op in ("ntt", "coeff_to_extended", "coset_ntt") else self.w_inv
        return self.n >> case.z, root

    def post_int(self, case, i):
        if case.op == "intt":
            return self.d
        if case.op == "extended_to_coeff":
            a, b = self.constants(case)  # (g_coset, g_coset_inv) as passed: y[i] *= d {1, g_coset_inv, g_coset}[i % 3]
            return self.d * (1, b, a)[i % 3] % R_MOD
        if case.op == "coset_intt":
            return self.d * pow(self.g_inv, i, R_MOD) % R_MOD
        return 1

    def post_vec(self, case, a):
        if case.op == "coset_intt":
            a = self.o.eval_op(OP_MUL, a, self.powers(self.g_inv), 0, 0, None)
        if case.op in ("intt", "extended_to_coeff", "coset_intt"):
            self.scale(a, self.d)
        if case.op == "extended_to_coeff":
            self.zeta_scale(a, self.constants(case), into_coset=False)
        return a

    def prepared(self, case, x):
        if case.op == "coeff_to_extended":
            a = x.copy()
            self.zeta_scale(a, self.constants(case), into_coset=True)
            return a
        if case.op == "coset_ntt":
            return self.o.eval_op(OP_MUL, x, self.powers(self.g), 0, 0, None)
        return x

    def sample_indices(self, case):
        n = self.n
        rng = random.Random(zlib.crc32(repr((self.log_n,) + tuple(case)).encode()))
        return sorted({0, 1 % n, n // 2, n - 1} | {rng.randrange(n) for _ in range(4)})

    def horner(self, prepared, ints, point):
        """sum_j x'_j point^j as a Montgomery residue"""
        if ints is not None:
            acc = 0
            for c in reversed(ints):
                acc = (acc * point + c) % R_MOD
            return acc
        out = np.zeros(4, dtype=np.uint64)
        self.o.lib.oracle_eval_polynomial_par(prepared.ctypes.data, len(prepared), fr_mont(point).ctypes.data, ORACLE_THREADS,
                                              out.ctypes.data)
        return _mont_int(out)

    def expected(self, case):
        """(the raw input of in_len elements, the expected output of n elements); layer (b) is asserted on the way"""
        in_len, root = self.spec(case)
        x = self.raw_input(case.inp, in_len)
        if case.inp == "zero":
            return x, np.zeros((self.n, 4), dtype=np.uint64)
        prepared = np.ascontiguousarray(self.prepared(case, x))
        j = self.delta_position(case.inp, in_len)
        want = None
        if j is None or self.log_n <= 18:
            padded = np.zeros((self.n, 4), dtype=np.uint64)
            padded[:in_len] = prepared
            want = self.post_vec(case, self.o.best_fft(padded, fr_mont(root), self.log_n, threads=ORACLE_THREADS))
        if j is not None:
            # X[k] = c (w^j)^k: one table of powers, scaled
            closed = self.powers(pow(root, j, R_MOD)).copy()
            self.o.lib.oracle_poly_scale(closed.ctypes.data, np.ascontiguousarray(prepared[j]).ctypes.data, self.n, ORACLE_THREADS)
            closed = self.post_vec(case, closed)
            assert want is None or np.array_equal(want, closed), ("the oracle's FFT differs from the closed form", self.log_n, case)
            want = closed
            ints = None
            cj = _mont_int(prepared[j])
        else:
            ints = _mont_ints(prepared) if in_len <= (1 << 16) else None
        for i in self.sample_indices(case):
            point = pow(root, i, R_MOD)
            h = cj * pow(point, j, R_MOD) % R_MOD if j is not None else self.horner(prepared, ints, point)
            assert _mont_int(want[i]) == h * self.post_int(case, i) % R_MOD, ("expected vector differs from the definition",
                                                                            self.log_n, case, i)
        return x, want
