"""The sort without a GPU: the host twin h2_sort_permutation against the definition (tests/sort_cases.py) on every size and
key set the device is tested on, the argument refusals by name, the header against SYMBOLS, Value.argsort / sort / sort_by on
the host backend, SortedAccessLog through the host assembly against a pure-Python construction, and csrc/sort_plan.cpp with
csrc/sort_host.cpp under the address and undefined-behaviour sanitizers as a stand-alone program (the plan's candidate
positions, tiles and scratch layout are checked there)."""
import os
import random
import re
import subprocess

import numpy as np
import pytest

import halo2_gpu_specific_amd as h2
import sort_cases as sc
import values_cases as vc
from halo2_gpu_specific_amd import circuits_frontend as fe, prover, values as V
from halo2_gpu_specific_amd._lib import SYMBOLS
from halo2_gpu_specific_amd.values import Value
from sort_cases import R_MOD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "halo2-gpu-specific_amd", "csrc")
CAPS = V.sort_limits()
TILE = CAPS["tile"]


# -- the twin against the definition -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", sc.sizes(TILE))
def test_twin_matches_the_definition(n):
    L = h2.lib()
    for case in sc.cases(n, TILE):
        sc.check(case, lambda keys, forms, bits: sc.run_host(L, keys, forms, bits))
    if n == 257:                                                             # 8-byte indices hold the same rows
        case = sc.cases(n, TILE)[-2]
        assert sc.run_host(L, case.keys, case.forms[0], case.bits, 8)[0] == sc.oracle(case.keys)


def test_twin_on_the_sentinels_and_a_broken_promise():
    L = h2.lib()
    sc.check(sc.sentinel_case(), lambda keys, forms, bits: sc.run_host(L, keys, forms, bits))
    rng = random.Random(3)
    keys = [[rng.randrange(1 << 12) for _ in range(500)], [rng.randrange(1 << 20) for _ in range(500)]]
    keys[1][321] = keys[1][400] = 1 << 20                                     # the lowest breaking row is named, with its key
    keys[0][400] = 1 << 12
    for forms in ((sc.CANONICAL, sc.MONTGOMERY), (sc.COMPACT, sc.COMPACT)):
        perm, status = sc.run_host(L, keys, forms, (12, 20))
        assert status[:3] == [sc.OUT_OF_RANGE, 321, 1] and sorted(perm) == list(range(500))
    perm, status = sc.run_host(L, keys, (sc.CANONICAL, sc.CANONICAL), (13, 21))
    assert status[0] == sc.OK and perm == sc.oracle(keys)
    # a promise of 9 bits ends inside byte 1: bit 9 breaks it although the byte is a candidate
    perm, status = sc.run_host(L, [[5, 1 << 9, 3]], (sc.CANONICAL,), (9,))
    assert status[:3] == [sc.OUT_OF_RANGE, 1, 0]


def test_scratch_bytes_are_monotone():
    L = h2.lib()
    for keys in range(1, CAPS["max_keys"] + 1):
        sizes = [L.h2_sort_scratch_bytes(n, keys) for n in (0, 1, TILE - 1, TILE, TILE + 1, 3 * TILE + 77, 1 << 22)]
        assert sizes == sorted(sizes) and sizes[0] > 0
        assert keys == 1 or L.h2_sort_scratch_bytes(TILE, keys) > L.h2_sort_scratch_bytes(TILE, keys - 1)
    assert L.h2_sort_scratch_bytes(8, 0) == 0 and L.h2_sort_scratch_bytes(8, CAPS["max_keys"] + 1) == 0
    assert L.h2_sort_scratch_bytes(1 << 32, 1) == 0


# -- refusals --------------------------------------------------------------------------------------------------------------------
def test_entry_points_refuse_bad_arguments_by_name():
    L = h2.lib()
    cells = sc.encode([3, 1, 2], sc.CANONICAL)
    keys = np.array([cells.ctypes.data], dtype=np.uint64)
    forms, bits = np.zeros(1, dtype=np.uint32), np.zeros(1, dtype=np.uint32)
    perm, status = np.zeros(3, dtype=np.uint64), np.zeros(4, dtype=np.uint32)
    good = dict(keys=keys.ctypes.data, forms=forms.ctypes.data, bits=bits.ctypes.data, num_keys=1, n=3, perm=perm.ctypes.data,
                width=4, status=status.ctypes.data)

    def refused(what, **change):
        a = dict(good, **change)
        rc = L.h2_sort_permutation(a["keys"], a["forms"], a["bits"], a["num_keys"], a["n"], a["perm"], a["width"], a["status"])
        message = L.h2_last_error().decode()
        assert rc == 1 and message == "h2_sort_permutation: " + what, (rc, message)
        # the device entry refuses the same before it looks for a device (there is none here)
        rc = L.h2_dev_sort_permutation(a["keys"], a["forms"], a["bits"], a["num_keys"], a["n"], a["perm"], a["width"], a["status"],
                                       a.get("scratch", cells.ctypes.data), a.get("scratch_bytes", 1 << 30), None)
        message = L.h2_last_error().decode()
        assert rc == 1 and message.startswith("h2_dev_sort_permutation: "), (rc, message)
        return message[len("h2_dev_sort_permutation: "):]

    assert refused("keys is null", keys=None) == "d_keys is null"
    assert refused("forms is null", forms=None) == "forms is null"
    assert refused("bits is null", bits=None) == "bits is null"
    assert refused("perm is null", perm=None) == "d_perm is null"
    assert refused("status is null", status=None) == "d_status is null"
    assert refused("num_keys is 0 (1 .. 4)", num_keys=0).startswith("num_keys")
    assert refused("num_keys is 5 (1 .. 4)", num_keys=5).startswith("num_keys")
    assert refused("n is 2^32 or more", n=1 << 32) == "n is 2^32 or more"
    assert refused("perm_width is 3 (4 or 8)", width=3) == "perm_width is 3 (4 or 8)"
    null_key = np.zeros(1, dtype=np.uint64)
    assert refused("keys[0] is null", keys=null_key.ctypes.data) == "keys[0] is null"
    forms[0] = 3
    assert refused("forms[0] is 3 (H2_ASSIGNED_FORM_*)").startswith("forms[0]")
    forms[0], bits[0] = sc.CANONICAL, 255
    assert refused("bits[0] is above 254") == "bits[0] is above 254"
    forms[0], bits[0] = sc.COMPACT, 65
    assert refused("bits[0] is above 64") == "bits[0] is above 64"
    forms[0], bits[0] = sc.CANONICAL, 0
    # the device entry alone: its scratch
    a = good
    for scratch, size, what in ((None, 1 << 30, "d_scratch is null"), (cells.ctypes.data, 64, "scratch too small (h2_sort_scratch_bytes)")):
        rc = L.h2_dev_sort_permutation(a["keys"], a["forms"], a["bits"], 1, 3, a["perm"], 4, a["status"], scratch, size, None)
        assert rc == 1 and L.h2_last_error().decode() == "h2_dev_sort_permutation: " + what
    assert L.h2_sort(None, 5) == 1 and L.h2_last_error().decode() == "h2_sort: null argument"
    assert L.h2_sort_limits(None) == 1
    # n = 0 is a no-op that reports OK, whatever the keys point at
    status[:] = 9
    assert L.h2_sort_permutation(null_key.ctypes.data, forms.ctypes.data, bits.ctypes.data, 1, 0, None, 4, status.ctypes.data) == 0
    assert list(status) == [0, 0xFFFFFFFF, 0xFFFFFFFF, 0]


def test_header_symbols_and_caps_agree():
    text = open(os.path.join(ROOT, "include", "halo2_hip.h")).read()
    plain = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    L = h2.lib()
    names = ("h2_sort_limits", "h2_sort_scratch_bytes", "h2_dev_sort_permutation", "h2_sort_permutation", "h2_sort")
    for name in names:
        declared = re.search(r"\b%s\s*\(([^)]*)\)" % name, plain)
        assert declared and name in SYMBOLS and hasattr(L, name), name
        assert len(declared.group(1).split(",")) == len(SYMBOLS[name][1]), name
    assert sorted(n for n in SYMBOLS if "sort" in n and "msm" not in n) == sorted(names)
    body = re.search(r"typedef struct \{([^}]*)\} h2_sort_caps;", plain).group(1)
    assert [name for _, name in re.findall(r"(\w+)\s+(\w+);", body)] == list(V.SORT_CAPS.names) and V.SORT_CAPS.itemsize == 16
    assert re.search(r"H2_SORT_OK = %d, H2_SORT_OUT_OF_RANGE = %d" % (V.SORT_OK, V.SORT_OUT_OF_RANGE), plain)
    assert re.search(r"#define H2_SORT_STATUS_WORDS %d\b" % CAPS["status_words"], plain) and CAPS["status_words"] == V.SORT_STATUS_WORDS
    assert re.search(r"#define H2_SORT_TILE %d\b" % TILE, plain) and re.search(r"#define H2_SORT_MAX_KEYS %d\b" % CAPS["max_keys"], plain)
    assert CAPS["max_keys"] >= 4 and TILE % 256 == 0
    assert (V.FORM_CANONICAL, V.FORM_MONTGOMERY, V.FORM_COMPACT) == (sc.CANONICAL, sc.MONTGOMERY, sc.COMPACT)
    srcs = open(os.path.join(CSRC, "Makefile")).read()
    assert " sort.hip " in srcs and " sort.hpp " in srcs and "sort_plan.o" in srcs and "sort_host.o" in srcs


# -- Value on the host backend -------------------------------------------------------------------------------------------------
def sorts(fn):
    before = (V.HOST.values_sorts, V.HOST.values_launches)
    out = fn()
    return out, V.HOST.values_sorts - before[0], V.HOST.values_launches - before[1]


def test_value_argsort_sort_and_sort_by():
    rng = random.Random(11)
    n = 700
    A = [rng.randrange(R_MOD) for _ in range(n)]
    B = [rng.randrange(5) for _ in range(n)]
    C = [rng.randrange(1 << 40) for _ in range(n)]
    a, b, c = Value.from_ints(None, A), Value.from_u64(None, B), Value.from_limbs(None, sc.encode(C, sc.MONTGOMERY), montgomery=True)
    # whole leaves go as they stand, in whatever form: one sort, no launch
    perm, count, launches = sorts(lambda: a.argsort().to_ints())
    assert perm == sc.oracle([A]) and (count, launches) == (1, 1)              # (the one launch widens the compact result for to_ints)
    perm, count, launches = sorts(lambda: Value.argsort([b, c], bits=[3, 40]).to_ints())
    assert perm == sc.oracle([B, C]) and (count, launches) == (1, 1)
    assert Value.argsort(b).to_ints() == sc.oracle([B]) and Value.argsort([b]).to_ints() == sc.oracle([B])
    # an expression is evaluated first (one launch for both keys), then sorted
    perm, count, launches = sorts(lambda: Value.argsort([b * 2, a + 1]).tensor())
    assert count == 1 and launches == 2
    assert V.limbs_to_ints(perm) == sc.oracle([[2 * v for v in B], [(v + 1) % R_MOD for v in A]])
    # sort: one argsort, one take; the take of a whole leaf costs no launch
    (got, count, launches) = sorts(lambda: a.sort().tensor(montgomery=False))
    assert V.limbs_to_ints(got) == sorted(A) and count == 1
    assert c.sort(bits=40).to_ints() == sorted(C) and b.sort().to_ints() == sorted(B)
    # sort_by: ONE argsort however many payloads, and no bounds check of its own permutation
    order = sc.oracle([B, C])
    (x, y, z), count, launches = sorts(lambda: Value.materialize(Value.sort_by([b, c], [a, b, c * 3], bits=[3, None])))
    assert count == 1
    assert V.limbs_to_ints(x) == [A[i] for i in order] and V.limbs_to_ints(y) == [B[i] for i in order]
    assert V.limbs_to_ints(z) == [3 * C[i] % R_MOD for i in order]
    # views of a sorted Value, and a sort of a view
    assert a.sort()[10:20].to_ints() == sorted(A)[10:20] and a[::3].sort().to_ints() == sorted(A[::3])
    assert Value.from_ints(None, []).argsort().to_ints() == [] and Value.from_ints(None, [9]).sort().to_ints() == [9]


def test_unknown_in_gives_unknown_out():
    u, a = Value.unknown(6), Value.from_ints(None, [5, 4, 3, 2, 1, 0])
    for v in (u.argsort(), u.sort(), Value.argsort([a, u]), Value.argsort([u, a], bits=[3, 3]), a.take(u.argsort())):
        assert not v.known and len(v) == 6
    assert all(not v.known and len(v) == 6 for v in Value.sort_by([u], [a, a]))
    assert all(not v.known for v in Value.sort_by([a], [u])) and Value.sort_by([a], [a, u])[0].to_ints() == [0, 1, 2, 3, 4, 5]
    with pytest.raises(ValueError, match="different lengths"):
        Value.argsort([a, a[:3]])
    with pytest.raises(ValueError, match="one promise"):
        Value.argsort([a], bits=[1, 2])
    with pytest.raises(ValueError, match="one promise"):
        a.argsort(bits=255)


def test_a_broken_promise_names_key_row_and_value():
    A = [3, 9, 1 << 20, 7, (1 << 20) + 5]
    B = [1, 2, 3, 4, 1 << 9]
    a, b = Value.from_ints(None, A), Value.from_u64(None, B)
    with pytest.raises(ValueError, match=r"argsort: key 0 at row 2 is 1048576, which is not below 2\^20"):
        a.argsort(bits=20).to_ints()
    with pytest.raises(ValueError, match=r"argsort: key 1 at row 4 is 512, which is not below 2\^9"):
        Value.argsort([a, b], bits=[21, 9]).to_ints()
    m = Value.from_limbs(None, sc.encode(A, sc.MONTGOMERY), montgomery=True)
    with pytest.raises(ValueError, match=r"argsort: key 0 at row 2 is 1048576, which is not below 2\^20"):
        m.sort(bits=20).to_ints()
    assert a.argsort(bits=21).to_ints() == [0, 3, 1, 2, 4]


# -- the circuit -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k, addr_bits, height", ((8, 4, None), (9, 7, 200), (7, 1, 33)))
def test_sorted_access_log_through_the_host_assembly(k, addr_bits, height):
    circuit = fe.SortedAccessLog(k, addr_bits, height)
    H = circuit.height
    cs, fixed, copies = prover.synthesize_keygen(None, circuit, k)
    assert not any(v.known for v in circuit.without_witnesses().columns())
    assert (cs.num_advice, cs.num_fixed) == (11, 3) and cs.degree() == 4 and len(copies) == 0
    before = V.HOST.values_sorts
    advice, first = prover.synthesize_witness(None, circuit, cs, k, resident=False)
    assert V.HOST.values_sorts == before + 1
    want = sc.sorted_access_log_columns(circuit)
    for column, values in zip(advice, want):
        assert vc.ints(column[:len(values)]) == values and not column[len(values):].any()
    assert first == {i: H if i < 8 else H - 1 for i in range(11)}
    # the relations on plain integers: the order is strict, d fits the table, a read returns the value before it
    a, t, v, w, A, T, Vs, W, inv, s, d = want
    assert all((A[i], T[i]) < (A[i + 1], T[i + 1]) and d[i] < (1 << circuit.table_bits) for i in range(H - 1))
    assert all(not s[i] or W[i + 1] or Vs[i + 1] == Vs[i] for i in range(H - 1))
    assert vc.ints(fixed[0]) == [1] * H + [0] * ((1 << k) - H) and vc.ints(fixed[1]) == [1] * (H - 1) + [0] * ((1 << k) - H + 1)
    assert vc.ints(fixed[2])[:1 << circuit.table_bits] == list(range(1 << circuit.table_bits))
    with pytest.raises(ValueError, match="SortedAccessLog"):
        fe.SortedAccessLog(k, addr_bits=k)


# -- the host code under the sanitizers ----------------------------------------------------------------------------------------
def test_sort_host_under_the_sanitizers(tmp_path):
    """a stand-alone program: nothing is preloaded into Python"""
    exe = tmp_path / "sort_host_main"
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    cmd = ["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-g", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(rocm, "include"), "-I", CSRC,
           os.path.join(ROOT, "tests", "sort_host_main.cpp"), os.path.join(CSRC, "sort_plan.cpp"), os.path.join(CSRC, "sort_host.cpp"),
           "-o", str(exe)]
    built = subprocess.run(cmd, capture_output=True, text=True, timeout=240)
    assert built.returncode == 0, built.stderr[-4000:]
    ran = subprocess.run([str(exe), "300"], capture_output=True, text=True, timeout=120)
    assert ran.returncode == 0 and not ran.stderr and ran.stdout.split()[0] == "ok", (ran.returncode, ran.stdout[-500:], ran.stderr[-3000:])
    # the plan file alone has no HIP in it
    plan = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", os.path.join(CSRC, "sort_plan.cpp")],
                          capture_output=True, text=True, timeout=120)
    assert plan.returncode == 0, plan.stderr[-2000:]
