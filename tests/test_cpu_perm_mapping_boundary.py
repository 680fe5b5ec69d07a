"""CPU-only checks of the permutation mapping's C boundary: the entries are exported with the header's arity, the header's
constants are the Python layer's, and bad arguments come back as H2_ERR_INVALID with h2_last_error naming the argument,
without a device."""
import os
import re

import pytest

import halo2_gpu_specific_amd as h2
from halo2_gpu_specific_amd._lib import SYMBOLS
from h2util import ROOT

H2_ERR_INVALID = 1
ENTRIES = ["h2_permutation_mapping_scratch_bytes", "h2_dev_permutation_mapping", "h2_dev_permutation_mapping_phases"]


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


def test_header_constants_match_the_python_layer():
    from halo2_gpu_specific_amd import prover

    text = header()
    for name, value in (("H2_PERM_MAPPING_OK", prover.PM_OK), ("H2_PERM_MAPPING_OUT_OF_BOUNDS", prover.PM_OUT_OF_BOUNDS),
                        ("H2_PERM_MAPPING_INTERNAL", prover.PM_INTERNAL)):
        assert re.search(r"\b%s = %d\b" % (name, value), text), name
    assert re.search(r"#define H2_PERM_MAPPING_STATUS_WORDS %d\b" % prover.PM_STATUS_WORDS, text)
    assert re.search(r"#define H2_PERM_MAPPING_SORT_TILE %d\b" % prover.PERM_MAPPING_SORT_TILE, text)


def test_scratch_bytes():
    size = h2.lib().h2_permutation_mapping_scratch_bytes
    base = size(4, 1 << 10, 0)
    assert base >= 4 * (4 << 10)                                         # one u32 per cell at the least
    assert size(4, 1 << 10, 100) > base                                  # grows with the copies ...
    assert size(4, 1 << 10, 1000) > size(4, 1 << 10, 100)
    assert size(4, 1 << 10, 1 << 40) == size(4, 1 << 10, 1 << 41)        # ... up to one entry per cell
    assert size(8, 1 << 10, 100) > size(4, 1 << 10, 100)                 # and with the cells
    assert size(4, 1 << 12, 100) > size(4, 1 << 10, 100)
    assert size(0, 8, 1) == size(8, 0, 1) == size(1 << 16, 1 << 16, 1) == 0    # sizes the call refuses


class Call:
    """one well-formed call on made-up (never dereferenced) device addresses; a case spoils one argument"""

    def __init__(self):
        self.copies, self.count, self.ncols, self.n = 0x10000, 100, 3, 1 << 10
        self.map_col, self.map_row, self.status, self.scratch = 0x20000, 0x30000, 0x40000, 0x50000
        self.scratch_bytes = None

    def run(self):
        L = h2.lib()
        nbytes = self.scratch_bytes
        if nbytes is None:
            nbytes = L.h2_permutation_mapping_scratch_bytes(self.ncols, self.n, self.count)
        return L.h2_dev_permutation_mapping(self.copies, self.count, self.ncols, self.n, self.map_col, self.map_row, self.status,
                                            self.scratch, nbytes, None)


def spoil(**kw):
    c = Call()
    for name, value in kw.items():
        setattr(c, name, value)
    return c


CASES = [
    ("null map_col", lambda: spoil(map_col=None), "d_map_col"),
    ("null map_row", lambda: spoil(map_row=None), "d_map_row"),
    ("null status", lambda: spoil(status=None), "d_status"),
    ("null scratch", lambda: spoil(scratch=None), "d_scratch"),
    ("null copies with copies > 0", lambda: spoil(copies=None), "d_copies"),
    ("no columns", lambda: spoil(ncols=0, scratch_bytes=1 << 30), "n_columns"),
    ("no rows", lambda: spoil(n=0, scratch_bytes=1 << 30), "n is zero"),
    ("2^32 cells", lambda: spoil(ncols=1 << 10, n=1 << 22, scratch_bytes=1 << 40), "2^32"),
    ("2^32 cells past a size_t product", lambda: spoil(ncols=1 << 40, n=1 << 40, scratch_bytes=1 << 40), "2^32"),
    ("misaligned copies", lambda: spoil(copies=0x10004), "misaligned"),
    ("scratch too small", lambda: spoil(scratch_bytes=64), "scratch"),
    ("scratch one byte short", lambda: spoil(scratch_bytes=h2.lib().h2_permutation_mapping_scratch_bytes(3, 1 << 10, 100) - 1),
     "scratch"),
]


@pytest.mark.parametrize("what,make,needle", CASES, ids=[c[0] for c in CASES])
def test_bad_arguments_are_refused_without_a_device(what, make, needle):
    L = h2.lib()
    assert make().run() == H2_ERR_INVALID, what
    message = L.h2_last_error().decode()
    assert message.startswith("h2_dev_permutation_mapping: ") and needle in message, message


def test_the_timed_entry_refuses_the_same_arguments():
    L = h2.lib()
    c = Call()
    nbytes = L.h2_permutation_mapping_scratch_bytes(c.ncols, c.n, c.count)
    assert L.h2_dev_permutation_mapping_phases(c.copies, c.count, c.ncols, c.n, None, c.map_row, c.status, c.scratch, nbytes,
                                               None, None) == H2_ERR_INVALID
    assert b"d_map_col" in L.h2_last_error()


def test_a_well_formed_call_without_a_device_is_an_error_not_a_fallback():
    """(not run where there is a device: the addresses above are made up)"""
    L = h2.lib()
    if L.h2_device_count() > 0:
        pytest.skip("a GPU is visible")
    assert Call().run() not in (0, H2_ERR_INVALID)
    assert L.h2_last_error()


def test_scipy_is_named_by_the_host_function_alone():
    """the package's only use of scipy is inside prover.permutation_mapping, which keygen calls only off the default route
    (tests/test_gpu_perm_mapping.py runs keygen with scipy made unimportable)"""
    import inspect

    from halo2_gpu_specific_amd import prover

    package = os.path.dirname(inspect.getsourcefile(prover))
    lines = [(name, line) for name in sorted(os.listdir(package)) if name.endswith(".py")
             for line in open(os.path.join(package, name)) if re.search(r"\bimport\b", line) and "scipy" in line]
    inside = [line for line in inspect.getsource(prover.permutation_mapping).splitlines(True) if "scipy" in line]
    assert lines and [line for _, line in lines] == inside
