"""CPU-only checks of the rational-cell resolution's C boundary and Python intake: the two entries are exported with the
header's arity, bad arguments come back as H2_ERR_INVALID with h2_last_error naming the entry and the argument, without a
device; `Rational` refuses bad shapes and rows on the host; a witness without a Rational goes through untouched."""
import ctypes
import os
import re

import numpy as np
import pytest

import halo2_gpu_specific_amd as h2
from halo2_gpu_specific_amd._lib import SYMBOLS
from h2util import ROOT

H2_ERR_INVALID = 1
ENTRIES = ("h2_dev_assigned_resolve", "h2_assigned_resolve")


def header():
    text = open(os.path.join(ROOT, "include", "halo2_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


@pytest.mark.parametrize("name", ENTRIES)
def test_declared_exported_and_bound_with_the_headers_arity(name):
    m = re.search(r"\b%s\s*\(([^)]*)\)\s*;" % name, header())
    assert m, "%s is not declared in include/halo2_hip.h" % name
    arity = len([a for a in m.group(1).split(",") if a.strip()])
    assert hasattr(h2.lib(), name)
    assert name in SYMBOLS and len(SYMBOLS[name][1]) == arity


def test_header_constants_match_the_python_layer_and_the_range_check_forms():
    from halo2_gpu_specific_amd import prover

    text = header()
    for name, value in (("H2_ASSIGNED_FORM_CANONICAL", prover.ASSIGNED_FORM_CANONICAL), ("H2_ASSIGNED_FORM_MONTGOMERY", prover.ASSIGNED_FORM_MONTGOMERY),
                        ("H2_ASSIGNED_FORM_COMPACT", prover.ASSIGNED_FORM_COMPACT), ("H2_ASSIGNED_OK", prover.ASSIGNED_OK),
                        ("H2_ASSIGNED_BAD_ROWS", prover.ASSIGNED_BAD_ROWS)):
        assert re.search(r"\b%s = %d\b" % (name, value), text), name
    assert re.search(r"#define H2_ASSIGNED_STATUS_WORDS %d\b" % prover.ASSIGNED_STATUS_WORDS, text)
    assert (prover.ASSIGNED_FORM_CANONICAL, prover.ASSIGNED_FORM_MONTGOMERY, prover.ASSIGNED_FORM_COMPACT) == (
        prover.RC_FORM_CANONICAL, prover.RC_FORM_MONTGOMERY, prover.RC_FORM_COMPACT)


class Call:
    """one well-formed call of three columns (dense 32-byte, dense compact, sparse) on made-up, never dereferenced
    addresses; a case spoils one argument.  `entry`: the device form or the host twin (no stream argument)."""
    N = 256

    def __init__(self, entry):
        u32 = lambda *v: (ctypes.c_uint32 * len(v))(*v)      # noqa: E731
        self.entry = entry
        self.num = (ctypes.c_void_p * 3)(0x100000, 0x110000, 0x120000)
        self.den = (ctypes.c_void_p * 3)(0x200000, 0x210000, 0x220000)
        self.rows = (ctypes.c_void_p * 3)(None, None, 0x300000)
        self.out = (ctypes.c_void_p * 3)(0x400000, 0x410000, 0x420000)
        self.nforms, self.dforms = u32(0, 2, 1), u32(1, 2, 0)
        self.counts = (ctypes.c_uint64 * 3)(0, 0, 100)
        self.cols, self.n, self.out_form, self.status = 3, self.N, 1, 0x500000

    def run(self):
        args = [self.num, self.nforms, self.den, self.dforms, self.rows, self.counts, self.out, self.cols, self.n, self.out_form,
                self.status]
        if self.entry == "h2_dev_assigned_resolve":
            args.append(None)
        return getattr(h2.lib(), self.entry)(*args)


def spoil(**kw):
    def make(entry):
        c = Call(entry)
        for name, value in kw.items():
            setattr(c, name, value)
        return c
    return make


def element(name, index, value):
    def make(entry):
        c = Call(entry)
        getattr(c, name)[index] = value
        return c
    return make


def elements(*changes):
    def make(entry):
        c = Call(entry)
        for name, index, value in changes:
            getattr(c, name)[index] = value
        return c
    return make


N32 = Call.N * 32
CASES = [
    ("null num", spoil(num=None), "num is null"),
    ("null num forms", spoil(nforms=None), "num_forms"),
    ("null den", spoil(den=None), "den is null"),
    ("null den forms", spoil(dforms=None), "den_forms"),
    ("null counts with rows", spoil(counts=None), "counts"),
    ("null out", spoil(out=None), "out is null"),
    ("null status", spoil(status=None), "status is null"),
    ("null num column", element("num", 1, None), "num holds a null"),
    ("null den column", element("den", 0, None), "den holds a null"),
    ("null den column of a sparse column with rows", element("den", 2, None), "den holds a null"),
    ("null out column", element("out", 2, None), "out holds a null"),
    ("unknown num form", element("nforms", 0, 3), "num_forms"),
    ("unknown den form", element("dforms", 2, 9), "den_forms"),
    ("unknown out form", spoil(out_form=2), "out_form"),
    ("n zero", spoil(n=0), "n is zero"),
    ("count above n", element("counts", 2, Call.N + 1), "counts"),
    ("misaligned num", element("num", 0, 0x100004), "misaligned"),
    ("misaligned compact den", element("den", 1, 0x210004), "misaligned"),
    ("misaligned out", element("out", 1, 0x410004), "misaligned"),
    ("misaligned rows", element("rows", 2, 0x300002), "rows array is misaligned"),
    ("out is num", element("out", 0, 0x100000), "overlaps a num"),
    ("out reaches into the num of another column", element("out", 0, 0x110000 - N32 + 32), "overlaps a num"),
    ("out starts inside a den", element("out", 2, 0x200000 + N32 - 32), "overlaps a den"),
    ("out inside the compact den", element("out", 1, 0x210000 + Call.N * 8 - 16), "overlaps a den"),
]
DEVICE_ONLY = [
    ("32-byte cells at 8 bytes", element("den", 0, 0x200008), "misaligned"),
]


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("what,make,needle", CASES, ids=[c[0] for c in CASES])
def test_bad_arguments_are_refused_without_a_device(entry, what, make, needle):
    L = h2.lib()
    assert make(entry).run() == H2_ERR_INVALID, what
    message = L.h2_last_error().decode()
    assert message.startswith(entry + ": ") and needle in message, message


@pytest.mark.parametrize("what,make,needle", DEVICE_ONLY, ids=[c[0] for c in DEVICE_ONLY])
def test_device_columns_need_16_byte_alignment(what, make, needle):
    L = h2.lib()
    assert make("h2_dev_assigned_resolve").run() == H2_ERR_INVALID
    message = L.h2_last_error().decode()
    assert message.startswith("h2_dev_assigned_resolve: ") and needle in message, message


def test_what_is_allowed():
    """no column at all does nothing, successfully, whatever else is passed; a sparse column without a listed row needs no
    denominators; an out column just past a den is no overlap (both only reach validation's end on a machine without a
    device, where the call itself then fails -- never as H2_ERR_INVALID)"""
    L = h2.lib()
    for entry in ENTRIES:
        assert spoil(cols=0, num=None, den=None, out=None, status=None, n=0)(entry).run() == 0
    if L.h2_device_count() > 0:
        return
    for entry in ENTRIES:
        assert elements(("counts", 2, 0), ("den", 2, None))(entry).run() != H2_ERR_INVALID
        assert element("out", 2, 0x200000 + N32)(entry).run() != H2_ERR_INVALID


@pytest.mark.parametrize("entry", ENTRIES)
def test_resolution_without_a_device_is_an_error_not_a_fallback(entry):
    """a well-formed call reaches the device: without one it fails loudly (on the made-up addresses above it is not run
    where there is one)"""
    L = h2.lib()
    if L.h2_device_count() > 0:
        pytest.skip("a GPU is visible")
    assert Call(entry).run() not in (0, H2_ERR_INVALID)
    assert L.h2_last_error()


def test_rational_refuses_bad_shapes_and_rows_without_a_device():
    from halo2_gpu_specific_amd.prover import Rational

    n = 16
    wide, compact = np.zeros((n, 4), dtype=np.uint64), np.zeros(n, dtype=np.uint64)
    for num, den in ((wide, wide), (wide, compact), (compact, wide), (compact, compact)):
        r = Rational(num, den)
        assert r.n == n and r.rows is None
    r = Rational(wide, compact[:3], rows=[0, 7, 15])
    assert r.rows.dtype == np.uint32 and list(r.rows) == [0, 7, 15]
    assert Rational(compact, wide[:0], rows=[]).rows.size == 0
    bad = [
        (np.zeros((n, 3), dtype=np.uint64), wide, None, "num is an"),
        (np.zeros((n, 4), dtype=np.int32), wide, None, "num is an"),
        (np.zeros((2, n, 4), dtype=np.uint64), wide, None, "num is an"),
        (wide, np.zeros((n, 2), dtype=np.uint64), None, "den is an"),
        (wide, [1.5] * n, None, "den is an"),
        (wide, wide[:n - 1], None, "den has 15 entries for 16 rows"),
        (wide[:0], wide[:0], None, "at least one row"),
        (wide, compact[:3], [0, 7], "den has 3 entries for 2 listed rows"),
        (wide, compact[:3], [0, 7, 7], "strictly increasing"),
        (wide, compact[:3], [7, 3, 9], "strictly increasing"),
        (wide, compact[:3], [0, 7, n], "below n"),
        (wide, compact[:3], [-1, 7, 9], "below n"),
        (wide, compact[:3], [[0, 7, 9]], "1-D array"),
        (wide, compact[:3], [0.0, 7.0, 9.0], "1-D array"),
    ]
    for num, den, rows, needle in bad:
        with pytest.raises(ValueError, match=needle):
            Rational(num, den, rows)


def test_a_rational_without_a_device_is_an_error():
    from halo2_gpu_specific_amd import witness
    from assigned_cases import is_zero_circuit, is_zero_witness

    cs = is_zero_circuit()
    w = is_zero_witness(6, 1, blinding=cs.blinding_factors())
    with pytest.raises(ValueError, match="resolved on a device"):
        witness._witness_sets(cs, w["n"], w["dense"], (), False, None)


def test_witness_without_a_rational_goes_through_untouched():
    """the caller's arrays themselves come back, unwritten, and nothing asks the device for anything (the one handed in here
    has no attribute to touch)"""
    from halo2_gpu_specific_amd import witness
    from assigned_cases import is_zero_circuit, is_zero_witness

    cs = is_zero_circuit()
    w = is_zero_witness(6, 1, blinding=cs.blinding_factors())
    adv = w["resolved"] + []
    before = [a.copy() for a in adv]
    for kw in ({}, {"device": object()}, {"device": object(), "strict_rationals": True}):
        sets, inst = witness._witness_sets(cs, w["n"], adv, (), False, None, **kw)
        assert len(sets) == 1 and inst == [[]]
        assert all(a is b for a, b in zip(sets[0], adv))
    two, _ = witness._witness_sets(cs, w["n"], [adv, adv], [(), ()], False, None, device=object())
    assert all(a is b for s in two for a, b in zip(s, adv))
    assert all(np.array_equal(a, b) for a, b in zip(adv, before))


def test_the_reference_and_the_case_builders_agree_with_themselves():
    """the big-integer reference on cells whose answer is known, and the witness builders against the circuit's gates"""
    import assigned_cases as A

    r = A.R_MOD
    assert A.reference([6, 5, 0, 7, r - 1], [3, 0, 9, 1, r - 1]) == [2, 0, 0, 7, 1]
    assert A.reference_sparse([6, 5, 4, 3], [3, 3], [0, 3]) == [2, 5, 4, 1]
    assert A.zero_report([1, 0, 2, 0]) == (2, 1) and A.zero_report([0, 4], rows=[5, 9]) == (1, 5) and A.zero_report([3]) == (0, A.NONE)
    for form in (A.CANONICAL, A.MONTGOMERY):
        vals = [0, 1, r - 1, 12345678901234567890123]
        assert A.decode(A.encode(vals, form), form) == vals
    assert [A.chain_lanes(c) for c in (1, 255, 256, 2047, 2048, 2049, 6149, (1 << 20) - 1, 1 << 20)] == [
        1, 255, 256, 256, 256, 257, 769, 131072, 65536]
    cs = A.is_zero_circuit()
    w = A.is_zero_witness(6, 3, blinding=cs.blinding_factors())
    v, inv, z = (A.ints(c) for c in w["resolved"])
    usable = w["n"] - cs.blinding_factors() - 1
    assert w["zero_rows"] and all((v[i] * z[i]) % r == 0 and (z[i] - (1 - v[i] * inv[i])) % r == 0 for i in range(usable))
    dense, sparse = w["dense"][1], w["sparse"][1]
    assert A.reference(A.ints(dense.num), A.ints(dense.den)) == inv
    assert A.reference_sparse(A.ints(sparse.num), A.ints(sparse.den), sparse.rows) == inv
    assert A.reference(A.ints(w["fixed"][0].num), A.ints(w["fixed"][0].den)) == A.ints(w["fixed_resolved"][0])
