"""One adapter per h2_dev_* entry point for the stream-contract tests (tests/test_gpu_stream_contract.py on the device,
tests/test_stream_cases_host.py without one).  Nothing here needs a GPU.

An Adapter knows how to BUILD a case from a seed -- numpy inputs, host-side parameters, and the expected outputs from the
references the suite already has -- and how to CALL its entry point on a table of addresses.  The same `call` runs against
libhalo2_hip.so over device tensors and against HostLib (below: tests/oracle_prover.py's OracleLib, the C oracle behind the
entry points' signatures, over host memory), and that second run is where most expected outputs come from.  The host test
pins them to the definitions in Python integers at a reduced size.

Two builds of one adapter from different seeds have the same shapes, table lengths and vector sizes (Case.signature) and
different contents: every value a case holds is a valid input at any position of the other, so a test that mixes two of them
up -- a decoy left in the inputs, two streams sharing a scratch block -- can compute wrong VALUES and nothing else.

  Case      inputs    name -> array: what the device tensors hold when the call is made
            like      name -> (shape, dtype): tensors the call only writes
            scratch   name -> bytes(L): caller-owned device scratch, contents irrelevant
            dims      name -> int: sizes (equal for every seed)
            p         name -> array / bytes: parameters passed through host memory (they differ by seed)
            expect    name -> array: the tensors named by Adapter.outputs after the call
            host      name -> array: what the call returns through host pointers
  Adapter   name, entry (the h2_dev_* symbol), waits, outputs, build(seed, size), call(L, stream, ptr, case) -> (rc, host
            results), normalise (for outputs whose bytes are not determined: unordered records, a Jacobian point)
`waits`: the header lists the entry point among those that return only after the caller's stream has drained.
"""
import ctypes
import random

import numpy as np

import hash_table_cases as H
from check_records import CIRCUIT, H2_CHECK_GATE, SENTINEL, SLACK
from evalh_cases import COLUMN_TABLES, oracle_evaluate_h, random_case
from h2util import Oracle, Q_MOD, R_MOD, fr_mont, to_mont
from halo2_gpu_specific_amd import evaluation as ev
from oracle_prover import OracleLib

ROOT_OF_UNITY = 0x03DDB9F5166D18B798865EA93DD31F743215CF6DD39329C8D34F1ED960C37C9C
DELTA = 0x09226B6E22C6F0CA64EC26AAD4C86E715B5F898E5E963F25870E56BBE533E9A2
OP_MUL, OP_LCTHETA = 3, 5          # h2_dev_eval_op
_vp = ctypes.c_void_p


def _at(a):
    return a.ctypes.data


class Case:
    def __init__(self, inputs=None, like=None, scratch=None, dims=None, p=None):
        self.inputs, self.like, self.scratch = inputs or {}, like or {}, scratch or {}
        self.dims, self.p = dims or {}, p or {}
        self.expect, self.host = {}, {}
        self.keep = []               # whatever a call must keep alive (descriptors)
        self.host_words = {}         # _host_words

    def signature(self):
        """everything about the case that sizes memory or bounds an index: equal for every seed"""
        sig = {"in." + k: (v.shape, str(v.dtype)) for k, v in self.inputs.items()}
        sig.update({"like." + k: (tuple(s), str(np.dtype(d))) for k, (s, d) in self.like.items()})
        sig.update({"dim." + k: v for k, v in self.dims.items()})
        sig.update({"p." + k: (np.shape(v), str(np.asarray(v).dtype)) if not isinstance(v, bytes) else len(v) for k, v in self.p.items()})
        sig.update({"expect." + k: (v.shape, str(v.dtype)) for k, v in self.expect.items()})
        sig.update({"host." + k: (np.shape(v), str(np.asarray(v).dtype)) for k, v in self.host.items()})
        sig["scratch"] = sorted(self.scratch)
        return sig


class Adapter:
    def __init__(self, name, entry, build, call, outputs, waits=False, size=None, small=None, normalise=None, expect=None):
        self.name, self.entry, self.waits, self.outputs = name, entry, waits, tuple(outputs)
        self._build, self.call, self.size, self.small = build, call, size, small
        self.normalised = normalise is not None
        self.normalise = normalise or (lambda case, out: out)
        self._expect = expect          # (case) -> fills case.expect / case.host; default: the call on HostLib

    def build(self, seed, size=None):
        case = self._build(seed, self.size if size is None else size)
        if self._expect:
            self._expect(case)
        else:
            rc, host, out = run_on_host(self, host_lib(), case)
            assert rc == 0, (self.name, rc)
            case.expect, case.host = out, host
        for a in list(case.inputs.values()) + list(case.expect.values()):
            a.setflags(write=False)
        return case


def run_on_host(adapter, L, case):
    """the adapter's call over host copies of the case's tensors -> (rc, host results, the output tensors)"""
    bufs = {k: np.array(v, order="C") for k, v in case.inputs.items()}
    bufs.update({k: np.zeros(s, dtype=d) for k, (s, d) in case.like.items()})
    bufs.update({k: np.zeros(max(int(f(L)), 8), dtype=np.uint8) for k, f in case.scratch.items()})
    rc, host = adapter.call(L, None, {k: _at(v) for k, v in bufs.items()}, case)
    return rc, host, {k: bufs[k] for k in adapter.outputs}


# ---------------------------------------------------------------------------------------------- the host twin
class HostLib(OracleLib):
    """OracleLib with the entry points the host prover never calls, each over the suite's own reference"""

    def h2_dev_widen_u64(self, src, n, dst, stream):
        a = np.ctypeslib.as_array(ctypes.cast(src, ctypes.POINTER(ctypes.c_uint64)), (n,))
        d = np.ctypeslib.as_array(ctypes.cast(dst, ctypes.POINTER(ctypes.c_uint64)), (n, 4))
        d[:] = 0
        d[:, 0] = a
        return 0

    def h2_dev_points_compress(self, pts, n, out, stream):
        self.O.oracle_points_compress(pts, n, out)
        return 0

    def h2_dev_points_decompress(self, raw, n, out, stream):
        return 1 if self.O.oracle_points_decompress(raw, n, out) else 0

    def h2_dev_g1_mul_each(self, pts, scalars, n, out, stream):
        jac = np.zeros(12, dtype=np.uint64)
        for i in range(n):
            self.O.oracle_g1_mul(pts + 64 * i, scalars + 32 * i, _at(jac))
            self.O.oracle_g1_to_affine(_at(jac), out + 64 * i)
        return 0


_host_lib = []


def host_lib():
    if not _host_lib:
        _host_lib.append(HostLib(threads=8))
    return _host_lib[0]


def _oracle():
    return Oracle.get()


def _scalar(rng):
    return fr_mont(rng.randrange(1, R_MOD))


def _omega(k):
    return pow(ROOT_OF_UNITY, 1 << (28 - k), R_MOD)


# ---------------------------------------------------------------------------------------------- scans and evaluations
def _kate_build(seed, n):
    rng = random.Random(seed)
    return Case(inputs={"a": _oracle().random_fr(1000 + seed, n)}, like={"q": ((n - 1, 4), np.uint64)}, dims={"n": n},
                p={"b": _scalar(rng)})


def _kate_call(L, stream, ptr, c):
    return L.h2_dev_kate_division(ptr["a"], c.dims["n"], _at(c.p["b"]), ptr["q"], stream), {}


def _scan_build(seed, n):
    rng = random.Random(seed)
    return Case(inputs={"f": _oracle().random_fr(1100 + seed, n - 1)}, like={"z": ((n, 4), np.uint64)}, dims={"n": n},
                p={"init": _scalar(rng)})


def _scan_call(entry):
    def call(L, stream, ptr, c):
        return getattr(L, entry)(ptr["f"], c.dims["n"], _at(c.p["init"]), ptr["z"], stream), {}
    return call


def _evalp_build(seed, n):
    rng = random.Random(seed)
    return Case(inputs={"poly": _oracle().random_fr(1200 + seed, n)}, dims={"n": n}, p={"point": _scalar(rng)})


def _host_words(L, case, words):
    """`words` zeroed u64 for a call to write a host result into: page-locked memory where L can allocate it (once per case and
    library) -- a copy into such memory is a DMA the stream runs in its turn, so nothing but the entry point's own wait makes
    the value final by the time the call returns -- and ordinary memory otherwise"""
    key = (id(L), words)
    if key not in case.host_words:
        if hasattr(L, "h2_host_alloc_pinned"):
            p = _vp()
            assert L.h2_host_alloc_pinned(8 * words, ctypes.byref(p)) == 0
            case.host_words[key] = np.ctypeslib.as_array(ctypes.cast(p, ctypes.POINTER(ctypes.c_uint64)), (words,))
        else:
            case.host_words[key] = np.zeros(words, dtype=np.uint64)
    out = case.host_words[key]
    out[:] = 0
    return out


def _evalp_call(L, stream, ptr, c):
    out = _host_words(L, c, 4)
    rc = L.h2_dev_eval_polynomial(ptr["poly"], c.dims["n"], _at(c.p["point"]), _at(out), stream)
    return rc, {"value": out.copy()}                           # (as it is when the call returns)


EVALP_BATCH = 3


def _evalpb_build(seed, n):
    o = _oracle()
    return Case(inputs={"poly%d" % j: o.random_fr(1300 + 10 * seed + j, n) for j in range(EVALP_BATCH)}, dims={"n": n},
                p={"points": o.random_fr(1390 + seed, EVALP_BATCH)})


def _evalpb_call(L, stream, ptr, c):
    out = _host_words(L, c, 4 * EVALP_BATCH)
    ptrs = (_vp * EVALP_BATCH)(*[ptr["poly%d" % j] for j in range(EVALP_BATCH)])
    rc = L.h2_dev_eval_polynomial_batch(ptrs, EVALP_BATCH, c.dims["n"], _at(c.p["points"]), _at(out), stream)
    return rc, {"values": out.copy().reshape(EVALP_BATCH, 4)}


def _binv_build(seed, n):
    a = _oracle().random_fr(1400 + seed, n)
    a[seed % 7::7] = 0                                          # zeros stay zero
    return Case(inputs={"a": a}, scratch={"tmp": lambda L: 32 * n}, dims={"n": n})


def _binv_call(L, stream, ptr, c):
    return L.h2_dev_batch_invert(ptr["a"], ptr["tmp"], c.dims["n"], stream), {}


LINCOMB_COUNT = 11


def _lincomb_build(seed, size):
    o = _oracle()
    return Case(inputs={"p%d" % j: o.random_fr(1500 + 20 * seed + j, size) for j in range(LINCOMB_COUNT)},
                like={"res": ((size, 4), np.uint64)}, dims={"size": size}, p={"coeffs": o.random_fr(1590 + seed, LINCOMB_COUNT)})


def _lincomb_call(L, stream, ptr, c):
    ptrs = (_vp * LINCOMB_COUNT)(*[ptr["p%d" % j] for j in range(LINCOMB_COUNT)])
    return L.h2_dev_lincomb(ptr["res"], ptrs, _at(c.p["coeffs"]), LINCOMB_COUNT, c.dims["size"], stream), {}


def _evalop_build(seed, size):
    o, rng = _oracle(), random.Random(seed)
    return Case(inputs={"l": o.random_fr(1600 + seed, size), "r": o.random_fr(1650 + seed, size)},
                like={"res": ((size, 4), np.uint64)}, dims={"size": size}, p={"c": _scalar(rng)})


def _evalop_call(L, stream, ptr, c):
    """res = l[i + 1] * r[i - 2] (rotated, out of place), then l = l * c + r in place"""
    size = c.dims["size"]
    rc = L.h2_dev_eval_op(OP_MUL, ptr["res"], ptr["l"], ptr["r"], 1, -2, size, None, stream)
    return rc or L.h2_dev_eval_op(OP_LCTHETA, ptr["l"], ptr["l"], ptr["r"], 0, 0, size, _at(c.p["c"]), stream), {}


VANISH_J, VANISH_K = 3, 10


def _vanish_build(seed, _):
    d, t = _oracle().domain(VANISH_J, VANISH_K)
    size = 1 << d.extended_k
    return Case(inputs={"a": _oracle().random_fr(1700 + seed, size), "t": t}, dims={"size": size, "t_len": len(t)})


def _vanish_call(L, stream, ptr, c):
    return L.h2_dev_divide_by_vanishing_poly(ptr["a"], c.dims["size"], ptr["t"], c.dims["t_len"], stream), {}


def _mont_build(seed, n):
    return Case(inputs={"a": _oracle().random_fr(1800 + seed, n)}, dims={"n": n})     # (any residue below r is both forms)


def _mont_call(entry):
    def call(L, stream, ptr, c):
        return getattr(L, entry)(ptr["a"], c.dims["n"], stream), {}
    return call


def _widen_build(seed, n):
    src = np.random.default_rng(seed).integers(0, 1 << 63, size=n, dtype=np.uint64) * np.uint64(2) + np.uint64(seed & 1)
    return Case(inputs={"src": src}, like={"dst": ((n, 4), np.uint64)}, dims={"n": n})


def _widen_call(L, stream, ptr, c):
    return L.h2_dev_widen_u64(ptr["src"], c.dims["n"], ptr["dst"], stream), {}


def _powers_build(seed, n):
    return Case(inputs={"a": _oracle().random_fr(1900 + seed, n)}, dims={"n": n}, p={"g": _scalar(random.Random(seed))})


def _powers_call(L, stream, ptr, c):
    return L.h2_dev_distribute_powers(ptr["a"], c.dims["n"], _at(c.p["g"]), stream), {}


PERM_COLUMNS = 5


def _sigma_build(seed, n):
    rng = np.random.default_rng(seed)
    return Case(inputs={"map_col": rng.integers(0, PERM_COLUMNS, size=n, dtype=np.uint32),
                        "map_row": rng.integers(0, n, size=n, dtype=np.uint32)},
                like={"sigma": ((n, 4), np.uint64)}, dims={"n": n},
                p={"delta": fr_mont(DELTA), "omega": _scalar(random.Random(seed))})


def _sigma_call(L, stream, ptr, c):
    return L.h2_dev_permutation_sigma(ptr["sigma"], ptr["map_col"], ptr["map_row"], c.dims["n"], _at(c.p["delta"]),
                                      _at(c.p["omega"]), stream), {}


def _terms_build(seed, n):
    o, rng = _oracle(), random.Random(seed)
    return Case(inputs={name: o.random_fr(2000 + 10 * seed + j, n) for j, name in enumerate(("num", "den", "value", "sigma"))},
                dims={"n": n}, p={"beta": _scalar(rng), "gamma": _scalar(rng), "delta_pow": fr_mont(pow(DELTA, 3, R_MOD)),
                                  "omega": _scalar(rng)})


def _terms_call(L, stream, ptr, c):
    """first = 0: the products are multiplied INTO num / den, so what they held is an input"""
    p = c.p
    return L.h2_dev_permutation_terms(ptr["num"], ptr["den"], ptr["value"], ptr["sigma"], c.dims["n"], _at(p["beta"]),
                                      _at(p["gamma"]), _at(p["delta_pow"]), _at(p["omega"]), 0, stream), {}


def _random_build(seed, n):
    return Case(like={"out": ((n, 4), np.uint64)}, dims={"n": n}, p={"key": bytes(random.Random(seed).randrange(256) for _ in range(32))})


def _random_call(L, stream, ptr, c):
    return L.h2_dev_random_fr(c.p["key"], c.dims["n"], ptr["out"], stream), {}


MAX_BITS_COLUMNS = 3


def _maxbits_build(seed, n):
    rng = np.random.default_rng(seed)
    cols = {}
    for j, bits in enumerate(((17 + 5 * seed) % 64 + 1, 64 + (29 * seed) % 64, 130 + (53 * seed) % 120)):
        a = rng.integers(0, 1 << 62, size=(n, 4), dtype=np.uint64)
        limb, top = divmod(bits - 1, 64)
        a[:, limb] &= np.uint64((1 << top) - 1)
        a[:, limb + 1:] = 0
        a[(7 * n) // 11, limb] |= np.uint64(1 << top)          # one value with the top bit set
        cols["c%d" % j] = a
    return Case(inputs=cols, scratch={"words": lambda L: 32 * MAX_BITS_COLUMNS}, dims={"n": n})


def _maxbits_call(L, stream, ptr, c):
    out = (ctypes.c_uint32 * MAX_BITS_COLUMNS)()
    ptrs = (_vp * MAX_BITS_COLUMNS)(*[ptr["c%d" % j] for j in range(MAX_BITS_COLUMNS)])
    rc = L.h2_dev_max_scalar_bits(ptrs, MAX_BITS_COLUMNS, c.dims["n"], ptr["words"], out, stream)
    return rc, {"bits": np.array(list(out), dtype=np.uint32)}


# ---------------------------------------------------------------------------------------------- points
def _points(seed, n):
    pts = _oracle().random_g1(seed, n)
    pts[(3 * seed) % n] = 0                                      # the identity
    return pts


def _compress_build(seed, n):
    return Case(inputs={"points": _points(2100 + seed, n)}, like={"bytes": ((n, 32), np.uint8)}, dims={"n": n})


def _compress_call(L, stream, ptr, c):
    return L.h2_dev_points_compress(ptr["points"], c.dims["n"], ptr["bytes"], stream), {}


def _decompress_build(seed, n):
    return Case(inputs={"bytes": _oracle().points_compress(_points(2200 + seed, n))}, like={"points": ((n, 8), np.uint64)},
                dims={"n": n})                                  # valid encodings only


def _decompress_call(L, stream, ptr, c):
    return L.h2_dev_points_decompress(ptr["bytes"], c.dims["n"], ptr["points"], stream), {}


def _msm_build(seed, n):
    return Case(inputs={"scalars": _oracle().random_fr(2300 + seed, n), "bases": _oracle().random_g1(2350 + seed, n)},
                scratch={"scratch": lambda L: L.h2_msm_scratch_bytes(n, 254)}, dims={"n": n})


def _msm_call(L, stream, ptr, c):
    out = np.zeros(12, dtype=np.uint64)
    n = c.dims["n"]
    rc = L.h2_dev_msm(ptr["scalars"], ptr["bases"], n, 254, ptr["scratch"], int(L.h2_msm_scratch_bytes(n, 254)), _at(out), stream)
    return rc, {"point": out}


def _msm_normalise(case, out):
    """a Jacobian point has many forms: compare the affine one"""
    return {k: (_oracle().to_affine(v) if k == "point" else v) for k, v in out.items()}


def _muleach_build(seed, n):
    scalars = _oracle().random_fr(2400 + seed, n)
    scalars[(5 * seed + 1) % n] = 0
    scalars[(5 * seed + 2) % n] = fr_mont(R_MOD - 1)
    return Case(inputs={"points": _points(2450 + seed, n), "scalars": scalars}, like={"out": ((n, 8), np.uint64)}, dims={"n": n})


def _muleach_call(L, stream, ptr, c):
    return L.h2_dev_g1_mul_each(ptr["points"], ptr["scalars"], c.dims["n"], ptr["out"], stream), {}


# ---------------------------------------------------------------------------------------------- transforms
def _ntt_build(seed, k):
    return Case(inputs={"a": _oracle().random_fr(2500 + seed, 1 << k)}, scratch={"tmp": lambda L: 32 << k}, dims={"k": k},
                p={"omega": fr_mont(_omega(k))})


def _ntt_call(L, stream, ptr, c):
    return L.h2_dev_ntt(ptr["a"], ptr["tmp"], _at(c.p["omega"]), c.dims["k"], stream), {}


def _coset_build(seed, k):
    g = random.Random(seed).randrange(2, R_MOD)
    return Case(inputs={"coeffs": _oracle().random_fr(2600 + seed, 1 << k)}, like={"out": ((1 << k, 4), np.uint64)},
                scratch={"tmp": lambda L: 32 << k}, dims={"k": k}, p={"g": fr_mont(g), "omega": fr_mont(_omega(k))})


def _coset_call(L, stream, ptr, c):
    return L.h2_dev_coset_ntt(ptr["coeffs"], ptr["out"], ptr["tmp"], c.dims["k"], _at(c.p["g"]), _at(c.p["omega"]), stream), {}


def _coset_inv_build(seed, k):
    g = random.Random(seed).randrange(2, R_MOD)
    return Case(inputs={"a": _oracle().random_fr(2700 + seed, 1 << k)}, scratch={"tmp": lambda L: 32 << k}, dims={"k": k},
                p={"g_inv": fr_mont(pow(g, -1, R_MOD)), "omega_inv": fr_mont(pow(_omega(k), -1, R_MOD)),
                   "divisor": fr_mont(pow(1 << k, -1, R_MOD))})


def _coset_inv_call(L, stream, ptr, c):
    p = c.p
    return L.h2_dev_coset_intt(ptr["a"], ptr["tmp"], c.dims["k"], _at(p["g_inv"]), _at(p["omega_inv"]), _at(p["divisor"]), stream), {}


# ---------------------------------------------------------------------------------------------- evaluate_h
def _evalh_columns(kw):
    """the descriptor's column vectors by name, in a fixed order"""
    cols = {"%s%d" % (t, i): a for t in COLUMN_TABLES for i, a in enumerate(kw[t])}
    cols.update({name: kw[name] for name in ("l0", "l_last", "l_active_row")})
    return cols


def _evalh_kw(kw, at):
    """kw with every column replaced by at(name)"""
    out = dict(kw)
    for t in COLUMN_TABLES:
        out[t] = [at("%s%d" % (t, i)) for i in range(len(kw[t]))]
    for name in ("l0", "l_last", "l_active_row"):
        out[name] = at(name)
    return out


def _evalh_build(flags):
    def build(seed, size):
        k, ek = size
        kw = random_case(seed, k, ek, _oracle(), n_calcs=40)
        case = Case(inputs=_evalh_columns(kw), like={"values": ((1 << ek, 4), np.uint64)}, dims={"k": k, "extended_k": ek, "flags": flags})
        case.kw = kw
        return case
    return build


def _evalh_expect(case):
    b = ev.Builder().build(**case.kw)
    case.expect = {"values": oracle_evaluate_h(_oracle(), b)}


def _evalh_call(L, stream, ptr, c):
    b = ev.Builder().build(**_evalh_kw(c.kw, lambda name: ptr[name]), flags=c.dims["flags"])
    c.keep.append(b)
    return L.h2_dev_evaluate_h(ctypes.byref(b.desc), ptr["values"], stream), {}


# ---------------------------------------------------------------------------------------------- check_gates
GATE_PARTS = 3


def _elements(rng, n):
    """(n, 4) stored forms: any value below 2^253 is one"""
    a = rng.integers(0, 1 << 63, size=(n, 4), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=(n, 4), dtype=np.uint64)
    a[:, 3] >>= np.uint64(11)
    return a


def _gates_build(seed, k):
    """the three gate polynomials of tests/test_gpu_check_kernels.py (zero-ness decided by limb comparison alone):
         part 0  advice0 - fixed0      part 1  advice1[row + 1] * fixed1      part 2  (advice0 - fixed0) * advice2
    over the rows where `values` is non-zero (about 60 % of them), which h2_dev_check_nonzero_rows lists first"""
    n = 1 << k
    rng = np.random.default_rng(3000 + seed)
    fixed0 = _elements(rng, n)
    advice0 = fixed0.copy()
    differ = rng.random(n) < 0.3
    advice0[np.arange(n), rng.integers(0, 4, size=n)] ^= np.where(differ, np.uint64(1) << rng.integers(0, 52, size=n).astype(np.uint64), np.uint64(0))
    advice1, fixed1, advice2 = _elements(rng, n), _elements(rng, n), _elements(rng, n)
    advice1[rng.random(n) < 0.2] = 0
    fixed1[rng.random(n) < 0.7] = 0
    advice2[rng.random(n) < 0.5] = 0
    values = _elements(rng, n)
    values[rng.random(n) < 0.4] = 0
    cap = GATE_PARTS * n
    case = Case(inputs={"values": values, "fixed0": fixed0, "fixed1": fixed1, "advice0": advice0, "advice1": advice1, "advice2": advice2,
                        "records": _empty_records(cap), "row_count": np.zeros(1, dtype=np.uint64)},     # (both counts are the caller's to zero)
                like={"rows": ((n + 8,), np.uint32)}, dims={"k": k, "cap": cap})
    return case


def _empty_records(cap):
    """tests/check_records.py's block: [u64 count = 0, 8 B pad][(cap + SLACK) x 16 B of SENTINEL], as u32 words"""
    blob = np.full(4 + 4 * (cap + SLACK), SENTINEL, dtype=np.uint32)
    blob[:4] = 0
    return blob


def gate_failures(case):
    """(part, row) of every failing gate polynomial at a listed row, by numpy limb comparison"""
    i = case.inputs
    part0 = (i["advice0"] != i["fixed0"]).any(axis=1)
    part1 = np.roll(i["advice1"].any(axis=1), -1) & i["fixed1"].any(axis=1)
    part2 = part0 & i["advice2"].any(axis=1)
    listed = i["values"].any(axis=1)
    return sorted((part, int(r)) for part, fail in enumerate((part0, part1, part2)) for r in np.flatnonzero(fail & listed))


def _gates_expect(case):
    want = gate_failures(case)
    blob = _empty_records(case.dims["cap"])
    blob[0] = len(want)
    recs = blob[4:].reshape(-1, 4)
    for j, (part, row) in enumerate(want):
        recs[j] = (H2_CHECK_GATE | CIRCUIT << 8, part, 0, row)
    case.expect = {"records": blob}


def _gates_desc(ptr, k):
    zero = [0, 0, 0, 0]
    return ev.Builder().build(
        k=k, extended_k=k, blinding_factors=0, chunk_len=1, constants=np.zeros((0, 4), dtype=np.uint64), rotations=[0, 1],
        calculations=[ev.calc(ev.CALC_SUB, ev.vs(ev.VS_ADVICE, 0, 0), ev.vs(ev.VS_FIXED, 0, 0)),
                      ev.calc(ev.CALC_MUL, ev.vs(ev.VS_ADVICE, 1, 1), ev.vs(ev.VS_FIXED, 1, 0)),
                      ev.calc(ev.CALC_MUL, ev.vs(ev.VS_INTERMEDIATE, 0), ev.vs(ev.VS_ADVICE, 2, 0))],
        value_parts=[ev.vs(ev.VS_INTERMEDIATE, j) for j in range(GATE_PARTS)],
        fixed=[ptr["fixed0"], ptr["fixed1"]], advice=[ptr["advice0"], ptr["advice1"], ptr["advice2"]], instance=[],
        y=zero, beta=zero, gamma=zero, theta=zero, delta=zero, zeta=zero, extended_omega=zero)


def _gates_call(L, stream, ptr, c):
    k = c.dims["k"]
    b = _gates_desc(ptr, k)
    c.keep.append(b)
    rc = L.h2_dev_check_nonzero_rows(ptr["values"], 1 << k, ptr["rows"], ptr["row_count"], stream)
    return rc or L.h2_dev_check_gates(ctypes.byref(b.desc), ptr["rows"], ptr["row_count"], CIRCUIT, ptr["records"], ptr["records"] + 16,
                                      c.dims["cap"], stream), {}


def _gates_normalise(case, out):
    """the records arrive in no particular order: the count, the records sorted, and the untouched tail"""
    if "records" not in out:
        return out
    blob = np.asarray(out["records"]).view(np.uint32)
    total = int(blob[:2].copy().view(np.uint64)[0])
    recs = blob[4:].reshape(-1, 4)
    kept = min(total, len(recs))
    body = recs[:kept]
    body = body[np.lexsort((body[:, 3], body[:, 2], body[:, 1], body[:, 0]))]
    return {"records": np.concatenate([blob[:4], body.reshape(-1), recs[kept:].reshape(-1)])}


# ---------------------------------------------------------------------------------------------- logup, permutation mapping
LOGUP_INPUTS = 3


def _logup_build(seed, size):
    usable, n = size
    rng = np.random.default_rng(3100 + seed)
    table = _oracle().random_fr(3100 + seed, n)
    for _ in range(max(1, usable // 8)):                       # duplicated table values: credited to their lowest row
        table[rng.integers(0, usable)] = table[rng.integers(0, usable)]
    table[usable:] = table[0]
    inputs = {"table": table}
    for j in range(LOGUP_INPUTS):
        idx = np.where(rng.random(n) < 0.7, rng.integers(0, usable, size=n), 3)                # row 3 is hot
        inputs["in%d" % j] = table[idx].copy()
    return Case(inputs=inputs, like={"m": ((n, 4), np.uint64)}, scratch={"scratch": lambda L: L.h2_logup_scratch_bytes(n)},
                dims={"usable": usable, "n": n})


def _logup_expect(case):
    i, usable, n = case.inputs, case.dims["usable"], case.dims["n"]
    m, misses = H.multiplicities(i["table"], [i["in%d" % j] for j in range(LOGUP_INPUTS)], usable, n)
    assert misses == 0
    case.expect = {"m": to_mont(m)}


def _logup_call(L, stream, ptr, c):
    ptrs = (_vp * LOGUP_INPUTS)(*[ptr["in%d" % j] for j in range(LOGUP_INPUTS)])
    n = c.dims["n"]
    return L.h2_dev_logup_multiplicity(ptr["table"], ptrs, LOGUP_INPUTS, c.dims["usable"], n, ptr["m"], ptr["scratch"],
                                       int(L.h2_logup_scratch_bytes(n)), stream), {}


PERMMAP_COPIES = 3 << 9            # perm_mapping_cases.py's "random-N/2"


def _permmap_build(seed, _):
    from perm_mapping_cases import random_copies

    ncols, n, copies = random_copies(PERMMAP_COPIES, seed=8 + 1000 * (seed - 1))          # seed 1 is the named case itself
    case = Case(inputs={"copies": np.ascontiguousarray(copies, dtype=np.uint32)},
                like={"map_col": ((ncols * n,), np.uint32), "map_row": ((ncols * n,), np.uint32), "status": ((2,), np.uint32)},
                scratch={"scratch": lambda L: L.h2_permutation_mapping_scratch_bytes(ncols, n, PERMMAP_COPIES)},
                dims={"ncols": ncols, "n": n, "copies": PERMMAP_COPIES})
    return case


def _permmap_expect(case):
    from halo2_gpu_specific_amd import prover

    d = case.dims
    map_col, map_row = prover.permutation_mapping(d["ncols"], d["n"], case.inputs["copies"].astype(np.int64))
    case.expect = {"map_col": np.ascontiguousarray(map_col, dtype=np.uint32).reshape(-1),
                   "map_row": np.ascontiguousarray(map_row, dtype=np.uint32).reshape(-1),
                   "status": np.array([0, 0xFFFFFFFF], dtype=np.uint32)}


def _permmap_call(L, stream, ptr, c):
    d = c.dims
    nbytes = int(L.h2_permutation_mapping_scratch_bytes(d["ncols"], d["n"], d["copies"]))
    return L.h2_dev_permutation_mapping(ptr["copies"], d["copies"], d["ncols"], d["n"], ptr["map_col"], ptr["map_row"], ptr["status"],
                                        ptr["scratch"], nbytes, stream), {}


# ---------------------------------------------------------------------------------------------- the table
SCAN_N = (1 << 20) + 3              # three levels of the blocked scan (1024 elements per workgroup)
ADAPTERS = [
    Adapter("kate_division", "h2_dev_kate_division", _kate_build, _kate_call, ["q"], size=SCAN_N, small=1029),
    Adapter("prefix_product", "h2_dev_prefix_product", _scan_build, _scan_call("h2_dev_prefix_product"), ["z"], waits=True,
            size=SCAN_N, small=1029),
    Adapter("prefix_sum", "h2_dev_prefix_sum", _scan_build, _scan_call("h2_dev_prefix_sum"), ["z"], waits=True, size=SCAN_N, small=1029),
    Adapter("eval_polynomial", "h2_dev_eval_polynomial", _evalp_build, _evalp_call, [], waits=True, size=4097, small=67),
    Adapter("eval_polynomial_batch", "h2_dev_eval_polynomial_batch", _evalpb_build, _evalpb_call, [], waits=True, size=4097, small=67),
    Adapter("batch_invert", "h2_dev_batch_invert", _binv_build, _binv_call, ["a"], size=70001, small=53),
    Adapter("lincomb", "h2_dev_lincomb", _lincomb_build, _lincomb_call, ["res"], size=5000, small=19),
    Adapter("eval_op", "h2_dev_eval_op", _evalop_build, _evalop_call, ["res", "l"], size=5001, small=19),
    Adapter("divide_by_vanishing_poly", "h2_dev_divide_by_vanishing_poly", _vanish_build, _vanish_call, ["a"]),
    Adapter("batch_mont", "h2_dev_batch_mont", _mont_build, _mont_call("h2_dev_batch_mont"), ["a"], size=5003, small=19),
    Adapter("batch_unmont", "h2_dev_batch_unmont", _mont_build, _mont_call("h2_dev_batch_unmont"), ["a"], size=5003, small=19),
    Adapter("widen_u64", "h2_dev_widen_u64", _widen_build, _widen_call, ["dst"], size=5003, small=19),
    Adapter("distribute_powers", "h2_dev_distribute_powers", _powers_build, _powers_call, ["a"], size=70001, small=53),
    Adapter("permutation_sigma", "h2_dev_permutation_sigma", _sigma_build, _sigma_call, ["sigma"], size=2049, small=37),
    Adapter("permutation_terms", "h2_dev_permutation_terms", _terms_build, _terms_call, ["num", "den"], size=2049, small=37),
    Adapter("random_fr", "h2_dev_random_fr", _random_build, _random_call, ["out"], size=1000, small=5),
    Adapter("max_scalar_bits", "h2_dev_max_scalar_bits", _maxbits_build, _maxbits_call, [], waits=True, size=70001, small=53),
    Adapter("points_compress", "h2_dev_points_compress", _compress_build, _compress_call, ["bytes"], size=1000, small=9),
    Adapter("points_decompress", "h2_dev_points_decompress", _decompress_build, _decompress_call, ["points"], waits=True,
            size=1000, small=9),
    Adapter("ntt", "h2_dev_ntt", _ntt_build, _ntt_call, ["a"], size=13, small=4),
    Adapter("coset_ntt", "h2_dev_coset_ntt", _coset_build, _coset_call, ["out"], size=13, small=4),
    Adapter("coset_intt", "h2_dev_coset_intt", _coset_inv_build, _coset_inv_call, ["a"], size=13, small=4),
    Adapter("msm", "h2_dev_msm", _msm_build, _msm_call, [], waits=True, size=4099, small=9, normalise=_msm_normalise),
    Adapter("g1_mul_each", "h2_dev_g1_mul_each", _muleach_build, _muleach_call, ["out"], size=257, small=5),
    Adapter("evaluate_h_generated", "h2_dev_evaluate_h", _evalh_build(0), _evalh_call, ["values"], size=(10, 12), small=(2, 3),
            expect=_evalh_expect),
    Adapter("evaluate_h_interpreter", "h2_dev_evaluate_h", _evalh_build(ev.EVALH_INTERPRET), _evalh_call, ["values"], size=(10, 12),
            small=(2, 3), expect=_evalh_expect),
    Adapter("check_gates", "h2_dev_check_gates", _gates_build, _gates_call, ["records"], size=17, small=6, normalise=_gates_normalise,
            expect=_gates_expect),
    Adapter("logup_multiplicity", "h2_dev_logup_multiplicity", _logup_build, _logup_call, ["m"], waits=True, size=(4090, 4096),
            small=(250, 256), expect=_logup_expect),          # (its status is whether a value was missing: the header's "Synchronous")
    Adapter("permutation_mapping", "h2_dev_permutation_mapping", _permmap_build, _permmap_call, ["map_col", "map_row", "status"],
            expect=_permmap_expect),
]
BY_NAME = {a.name: a for a in ADAPTERS}
_built = {}


def built(name, seed, small=False):
    """the adapter's case for `seed` at its full (or reduced) size: built once, read-only"""
    key = (name, seed, small)
    if key not in _built:
        a = BY_NAME[name]
        _built[key] = a.build(seed, a.small if small else None)
    return _built[key]


# The issue's table also lists h2_dev_range_check_complete, h2_dev_values_eval and h2_dev_assigned_resolve: their arguments are
# tables of structures (plans, leaves, per-column forms) whose cases live inside tests of their own; they have no adapter.
