"""CPU-only checks of the range-check completion's C boundary: the two entries are exported with the header's arity, and
bad arguments come back as H2_ERR_INVALID with h2_last_error naming the argument, without a device."""
import ctypes
import os
import re

import numpy as np
import pytest

import halo2_gpu_specific_amd as h2
from halo2_gpu_specific_amd._lib import SYMBOLS
from h2util import ROOT

H2_ERR_INVALID = 1
UNKNOWN = (1 << 64) - 1


def header():
    text = open(os.path.join(ROOT, "include", "halo2_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


@pytest.mark.parametrize("name", ["h2_range_check_scratch_bytes", "h2_dev_range_check_complete"])
def test_declared_exported_and_bound_with_the_headers_arity(name):
    m = re.search(r"\b%s\s*\(([^)]*)\)\s*;" % name, header())
    assert m, "%s is not declared in include/halo2_hip.h" % name
    arity = len([a for a in m.group(1).split(",") if a.strip()])
    assert hasattr(h2.lib(), name)
    assert name in SYMBOLS and len(SYMBOLS[name][1]) == arity


def test_header_constants_match_the_python_layer():
    from halo2_gpu_specific_amd import prover

    text = header()
    for name, value in (("H2_RANGE_CHECK_FORM_CANONICAL", prover.RC_FORM_CANONICAL), ("H2_RANGE_CHECK_FORM_MONTGOMERY", prover.RC_FORM_MONTGOMERY),
                        ("H2_RANGE_CHECK_FORM_COMPACT", prover.RC_FORM_COMPACT), ("H2_RANGE_CHECK_OK", prover.RC_OK),
                        ("H2_RANGE_CHECK_NO_FIT", prover.RC_NO_FIT), ("H2_RANGE_CHECK_IN_USE", prover.RC_IN_USE),
                        ("H2_RANGE_CHECK_OUT_OF_RANGE", prover.RC_OUT_OF_RANGE), ("H2_RANGE_CHECK_UNSUPPORTED", prover.RC_UNSUPPORTED)):
        assert re.search(r"\b%s = %d\b" % (name, value), text), name
    assert re.search(r"#define H2_RANGE_CHECK_STATUS_WORDS %d\b" % prover.RC_STATUS_WORDS, text)


def test_scratch_bytes():
    L = h2.lib()
    u64 = lambda *v: (ctypes.c_uint64 * len(v))(*v)          # noqa: E731
    base = L.h2_range_check_scratch_bytes(u64(5), u64(5), 0)
    one = L.h2_range_check_scratch_bytes(u64(0), u64(0xFFFF), 1)
    assert one - base >= (0x10000 + 1) * 4                   # the bins and the end sentinel
    # pairs add up; a width past the cap (the call reports UNSUPPORTED for it) and a null array take nothing
    assert L.h2_range_check_scratch_bytes(u64(0, 3), u64(0xFFFF, 40), 2) > one
    assert L.h2_range_check_scratch_bytes(u64(0, 0), u64(0xFFFF, 1 << 24), 2) == one
    assert L.h2_range_check_scratch_bytes(None, None, 3) == base


class Call:
    """one well-formed call on made-up (never dereferenced) device addresses; a case spoils one argument"""

    def __init__(self):
        u64 = lambda *v: (ctypes.c_uint64 * len(v))(*v)      # noqa: E731
        u32 = lambda *v: (ctypes.c_uint32 * len(v))(*v)      # noqa: E731
        self.origins = (ctypes.c_void_p * 2)(0x10000, 0x30000)
        self.companions = (ctypes.c_void_p * 2)(0x20000, 0x40000)
        self.oforms, self.cforms = u32(0, 2), u32(1, 0)
        self.vmin, self.vmax, self.step, self.first = u64(0, 3), u64(61, 40), u64(4, 1), u64(UNKNOWN, 7)
        self.pairs, self.usable, self.n = 2, 250, 256
        self.status, self.scratch = 0x50000, 0x60000
        self.scratch_bytes = h2.lib().h2_range_check_scratch_bytes(self.vmin, self.vmax, 2)

    def run(self):
        return h2.lib().h2_dev_range_check_complete(self.origins, self.companions, self.oforms, self.cforms, self.vmin, self.vmax,
                                                    self.step, self.first, self.pairs, self.usable, self.n, self.status,
                                                    self.scratch, self.scratch_bytes, None)


def spoil(**kw):
    c = Call()
    for name, value in kw.items():
        setattr(c, name, value)
    return c


def element(name, index, value):
    c = Call()
    getattr(c, name)[index] = value
    return c


CASES = [
    ("null origins", lambda: spoil(origins=None), "d_origins"),
    ("null companions", lambda: spoil(companions=None), "d_companions"),
    ("null origin forms", lambda: spoil(oforms=None), "origin_forms"),
    ("null companion forms", lambda: spoil(cforms=None), "companion_forms"),
    ("null vmin", lambda: spoil(vmin=None), "vmin"),
    ("null vmax", lambda: spoil(vmax=None), "vmax"),
    ("null step", lambda: spoil(step=None), "step"),
    ("null status", lambda: spoil(status=None), "d_status"),
    ("null scratch", lambda: spoil(scratch=None), "d_scratch"),
    ("null column", lambda: element("origins", 1, None), "d_origins"),
    ("null companion column", lambda: element("companions", 0, None), "d_companions"),
    ("n not a power of two", lambda: spoil(n=255, usable=250), "power of two"),
    ("n zero", lambda: spoil(n=0, usable=0), "power of two"),
    ("usable beyond n", lambda: spoil(usable=257), "usable_rows"),
    ("vmin above vmax", lambda: element("vmin", 1, 41), "vmin exceeds vmax"),
    ("step zero", lambda: element("step", 0, 0), "step"),
    ("unknown origin form", lambda: element("oforms", 0, 3), "origin_forms"),
    ("unknown companion form", lambda: element("cforms", 1, 7), "companion_forms"),
    ("misaligned column", lambda: element("origins", 0, 0x10008), "misaligned"),
    ("scratch too small", lambda: spoil(scratch_bytes=64), "scratch"),
]


@pytest.mark.parametrize("what,make,needle", CASES, ids=[c[0] for c in CASES])
def test_bad_arguments_are_refused_without_a_device(what, make, needle):
    L = h2.lib()
    assert make().run() == H2_ERR_INVALID, what
    message = L.h2_last_error().decode() if isinstance(L.h2_last_error(), bytes) else str(L.h2_last_error())
    assert message.startswith("h2_dev_range_check_complete: ") and needle in message, message


def test_device_completion_without_a_device_is_an_error_not_a_fallback():
    """a well-formed call reaches the device: without one it fails loudly (on the made-up addresses above it is not run
    where there is one)"""
    L = h2.lib()
    if L.h2_device_count() > 0:
        pytest.skip("a GPU is visible")
    assert Call().run() not in (0, H2_ERR_INVALID)
    assert L.h2_last_error()


def test_host_path_is_untouched_without_a_device():
    """host columns of canonical integers keep the host path and its in-place semantics (a guard against a regression: this
    holds before the device path exists too, so it is no evidence of it)"""
    from halo2_gpu_specific_amd import circuits, prover, witness

    cs = circuits.range_check(0, 61, 4)
    adv, _, _ = circuits.range_check_synthesize(8, vmax=61, count=100)
    n = 1 << 8
    want = [a.copy() for a in adv]
    prover.complete_range_check_witness(cs, n, want)
    sets, _ = witness._witness_sets(cs, n, adv, (), False, None)
    assert sets[0][0] is adv[0] and all(np.array_equal(a, b) for a, b in zip(adv, want))
    with pytest.raises(ValueError, match="needs canonical advice columns"):
        witness._witness_sets(cs, n, adv, (), True, None)          # no device given: nothing to complete Montgomery columns on


def test_opt_in_leaves_a_wide_range_of_host_columns_to_the_host():
    """a range of 2^24 values or more is past the device's cap: under `range_checks_on_device` host columns are completed by
    the host path, on copies (the device handed in here has no attribute to touch)"""
    from halo2_gpu_specific_amd import circuits, prover, witness

    import types

    vmax, step = (1 << 24) + 5, 1 << 20                              # 18 planted values
    # (what the completion reads of a ConstraintSystem; a gate for such a step is a product of 2^20 factors)
    cs = types.SimpleNamespace(range_checks=[(0, 1, 0, vmax, step)], blinding_factors=lambda: 5)
    adv, _, _ = circuits.range_check_synthesize(8, vmax=vmax, count=100)
    n = 1 << 8
    before = [a.copy() for a in adv]
    want = [a.copy() for a in adv]
    prover.complete_range_check_witness(cs, n, want)
    sets, _ = witness._witness_sets(cs, n, adv, (), False, None, device=object(), range_checks_on_device=True)
    assert all(np.array_equal(a, b) for a, b in zip(adv, before)), "the caller's columns were written"
    assert all(np.array_equal(a, b) for a, b in zip(sets[0], want))
