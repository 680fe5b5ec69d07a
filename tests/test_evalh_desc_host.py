"""h2_evalh_desc stated once (csrc/evalh_desc.hpp) without a GPU: tests/evalh_desc_host.cpp is built with g++ alone -- the header
includes no HIP header -- plainly and once more under AddressSanitizer / UndefinedBehaviorSanitizer, and asked for

  1. the two derived counts;
  2. the walk over the column slots of one hand-made descriptor (an empty instance table behind a null pointer, a null
     l_active_row, one address named three times) in the documented order;
  3. evalh_column at every slot, one past every table and at the null single;
  4. evalh_remap: every non-null slot mapped once, null left null, the original untouched, everything else copied;
  5. every validity rule at one offending value, with the message the entry points have always given, and the boundary
     values that are sound, in each of the three forms.
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "halo2-gpu-specific_amd", "csrc")
FLAGS = ["-O1", "-std=c++17", "-Wall", "-Werror"]
SANITIZE = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]

# tests/evalh_desc_host.cpp's descriptor: (table, its slots) in evgen::Table's order
TABLES = [
    ("fixed", [0x10000, 0x10100]),
    ("advice", [0x20000, 0x20100, 0x20000]),
    ("instance", []),
    ("perm_z", [0x40000, 0x40100]),
    ("perm_sigma", [0x50000, 0x20000, 0x50200]),
    ("lookup_z", [0x60000, 0x60100, 0x60200, 0x60300]),
    ("lookup_m", [0x70000, 0x70100]),
    ("shuffle_z", [0x80000]),
    ("l0", [0x90000]),
    ("l_last", [0xA0000]),
    ("l_active_row", [0]),
]
WALK = [(t, i, p) for t, (_, slots) in enumerate(TABLES) for i, p in enumerate(slots)]


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def exe(request, tmp_path_factory):
    out = str(tmp_path_factory.mktemp("evalh_desc_host") / "evalh_desc_host")
    extra = SANITIZE if request.param == "sanitized" else []
    cmd = ["g++", *FLAGS, *extra, "-I", CSRC, os.path.join(ROOT, "tests", "evalh_desc_host.cpp"), "-o", out]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=240)
    assert res.returncode == 0, res.stderr[-4000:]
    return out


def ask(exe, cmd, lines=()):
    res = subprocess.run([exe, cmd], input="".join(ln + "\n" for ln in lines), capture_output=True, text=True, timeout=120)
    assert res.returncode == 0 and not res.stderr, (cmd, res.returncode, res.stderr[-3000:])
    return res.stdout.splitlines()


def slots(lines):
    return [(int(t), int(i), int(p, 16)) for t, i, p in (ln.split() for ln in lines)]


def test_the_descriptor_header_includes_no_hip_header():
    text = open(os.path.join(CSRC, "evalh_desc.hpp")).read()
    includes = [ln.split()[1] for ln in text.splitlines() if ln.startswith("#include")]
    assert includes and all(i.startswith("<") or i in ('"evalh_gen.hpp"', '"../../include/halo2_hip.h"') for i in includes), includes
    assert not [i for i in includes if "hip/" in i], includes
    gen = open(os.path.join(CSRC, "evalh_gen.hpp")).read()      # what it includes in turn
    assert not [ln for ln in gen.splitlines() if ln.startswith("#include") and ("hip/" in ln or "common.hpp" in ln)]


def test_the_derived_counts(exe):
    assert ask(exe, "counts") == ["4 10"]


def test_the_walk_visits_every_slot_in_the_documented_order(exe):
    assert len(WALK) == 2 + 3 + 0 + 2 + 3 + 4 + 2 + 1 + 3
    assert [name for name, _ in TABLES] == ["fixed", "advice", "instance", "perm_z", "perm_sigma", "lookup_z", "lookup_m", "shuffle_z",
                                            "l0", "l_last", "l_active_row"]
    assert slots(ask(exe, "walk")) == WALK


def test_column_agrees_with_the_walk_and_is_null_outside(exe):
    want = []
    for t, (_, ps) in enumerate(TABLES):
        want += [(t, i, p) for i, p in enumerate(ps)] + [(t, len(ps), 0)]      # one past the table: null
    assert slots(ask(exe, "column")) == want
    assert (10, 0, 0) in want                                                   # the null single


def test_remap_maps_each_non_null_slot_once_and_leaves_the_rest(exe):
    out = ask(exe, "remap")
    n = len(WALK)
    assert len(out) == 2 * n + 1
    assert slots(out[:n]) == [(t, i, p + 8 if p else 0) for t, i, p in WALK]
    non_null = sum(1 for _, _, p in WALK if p)
    assert out[n] == "calls=%d original_unchanged=1 others_equal=1" % non_null and non_null == n - 1
    assert slots(out[n + 1:]) == WALK


DEV = "h2_evaluate_h: "
ROW_RANGE = "entry: a row range is for the device entry point (h2_dev_evaluate_h)"
RULES = {   # mutation -> message (None: sound); a dict where the forms differ
    "null": "entry: null argument",
    "ek_below_k": "entry: bad k / extended_k",
    "ek_29": "entry: bad k / extended_k",
    "chunk_len_0": DEV + "chunk_len must be non-zero when permutation sets are present",
    "reserved": DEV + "`reserved` must be NULL (round 4's caller-supplied kernel slot: the library generates the program's kernels itself "
                      "now, see h2_evalh_prepare)",
    "row_outside": DEV + "row range outside the domain",
    "perm_index": DEV + "permutation column index out of range",
    "row_range": {"device": None, "host": ROW_RANGE, "coeff": ROW_RANGE},
    "sound": None,
    "ek_equals_k": None,
    "ek_28": None,
    "row_end_exact": {"device": None, "host": ROW_RANGE, "coeff": ROW_RANGE},
    "row_count_0": None,
}


def test_every_validity_rule_in_every_form(exe):
    asked = [(form, m) for form in ("device", "host", "coeff") for m in RULES]
    out = ask(exe, "validate", ["%s %s" % fm for fm in asked])
    assert len(out) == len(asked)
    for (form, m), got in zip(asked, out):
        want = RULES[m][form] if isinstance(RULES[m], dict) else RULES[m]
        assert got == (want or "ok"), (form, m, got)
