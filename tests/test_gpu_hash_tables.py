"""The open-addressing hash tables of csrc/logup.hip (k_logup_build / k_logup_count / k_logup_emit) and csrc/check.hip
(k_check_lookup, k_check_shuffle_count / _report) on the adversarial inputs of tests/hash_table_cases.py -- wrapped and merged
clusters, misses that walk a whole cluster, far duplicates, waves of 1, 2, 3 and 5 hot values, padded tables, keys one limb
apart -- against dict / Counter references.  Every assertion is bit-exact.  tests/test_hash_table_cases_host.py shows on the CPU
that each case is what it is named; test_slot_table_is_the_named_cluster pins the hash twin those claims rest on to the device."""
import ctypes

import numpy as np
import pytest
import torch

import halo2_gpu_specific_amd as h2
import hash_table_cases as H
from check_records import CIRCUIT, H2_CHECK_LOOKUP, H2_CHECK_SHUFFLE, Records, dev, dev_u32, host, host_u32
from h2util import from_mont

pytestmark = pytest.mark.gpu

MAX_N = 2048


@pytest.fixture(scope="module")
def scratch():
    L = h2.lib()
    nbytes = max(L.h2_logup_scratch_bytes(MAX_N), L.h2_check_scratch_bytes(MAX_N))
    return torch.empty(nbytes, dtype=torch.uint8, device="cuda"), nbytes


_on_device = {}


def _case_on_device(name):
    """(case, table, inputs, HOST array of the inputs' device pointers), uploaded once"""
    if name not in _on_device:
        c = H.case(name)
        assert c.n <= MAX_N
        d_in = [dev(a) for a in c.inputs]
        _on_device[name] = (c, dev(c.table), d_in, (ctypes.c_void_p * len(d_in))(*[t.data_ptr() for t in d_in]))
    return _on_device[name]


def _garbage(n):
    return dev(np.full((n, 4), 0x1111111111111111, dtype=np.uint64))


def _assert_rc(L, rc, misses):
    if misses:
        assert rc == 1 and b"logup: %d input value(s) are missing from the table" % misses in L.h2_last_error()
    else:
        assert rc == 0, L.h2_last_error()


@pytest.mark.parametrize("name", H.NAMES)
def test_multiplicities(scratch, name):
    L = h2.lib()
    c, d_table, d_in, ptrs = _case_on_device(name)
    want, misses = H.multiplicities(c.table, c.inputs, c.usable, c.n)
    d_m = _garbage(c.n)                                  # rows past usable must be WRITTEN zero
    rc = L.h2_dev_logup_multiplicity(d_table.data_ptr(), ptrs, len(d_in), c.usable, c.n, d_m.data_ptr(), scratch[0].data_ptr(),
                                     scratch[1], None)
    _assert_rc(L, rc, misses)
    assert from_mont(host(d_m)) == want


@pytest.mark.parametrize("name", H.NAMES)
def test_row_range_counts(scratch, name):
    """h2_dev_logup_counts over three row ranges -- the cuts fall inside the input rows of a cluster, the second range ends
    before usable, the third runs past it -- each against the reference for its rows; then the sum through h2_dev_logup_emit"""
    L = h2.lib()
    c, d_table, d_in, ptrs = _case_on_device(name)
    want, misses = H.multiplicities(c.table, c.inputs, c.usable, c.n)
    cut = c.usable // 3 + 1
    total = np.zeros(c.n + 1, dtype=np.uint64)
    for lo, hi in ((0, cut), (cut, c.usable - 3), (c.usable - 3, c.n)):
        part = torch.full((c.n + 1,), 0x77, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        assert L.h2_dev_logup_counts(d_table.data_ptr(), ptrs, len(d_in), c.usable, c.n, lo, hi, part.data_ptr(),
                                     scratch[0].data_ptr(), scratch[1], None) == 0, L.h2_last_error()
        got = host_u32(part)
        want_part, miss_part = H.multiplicities(c.table, c.inputs, c.usable, c.n, rows=(lo, hi))
        assert [int(x) for x in got[:c.n]] == want_part and int(got[c.n]) == miss_part, (lo, hi)
        total += got
    assert [int(x) for x in total[:c.n]] == want and int(total[c.n]) == misses
    d_counts = dev_u32(total.astype(np.uint32))
    d_m = _garbage(c.n)
    assert L.h2_dev_logup_emit(d_counts.data_ptr(), c.usable, c.n, d_m.data_ptr(), None) == 0
    assert from_mont(host(d_m)) == want


@pytest.mark.parametrize("name", ["hot_waves", "padding", "full_cluster_miss"])
def test_largest_multiplicity_bits(scratch, name):
    L = h2.lib()
    c, d_table, d_in, ptrs = _case_on_device(name)
    want, misses = H.multiplicities(c.table, c.inputs, c.usable, c.n)
    bits = ctypes.c_uint32(99)
    d_m = _garbage(c.n)
    rc = L.h2_dev_logup_multiplicity_bits(d_table.data_ptr(), ptrs, len(d_in), c.usable, c.n, d_m.data_ptr(), scratch[0].data_ptr(),
                                          scratch[1], ctypes.byref(bits), None)
    _assert_rc(L, rc, misses)
    assert bits.value == max(want).bit_length() and bits.value > 2
    assert from_mont(host(d_m)) == want


@pytest.mark.parametrize("name", ["wrap", "capacity_step", "adjacent_homes"])
def test_slot_table_is_the_named_cluster(scratch, name):
    """The cases are real on the device: h2_dev_logup_multiplicity leaves the slot table in the first `cap` u32 of the
    caller's scratch (logup_multiplicity_launch: slots, then the counters).  Its occupied slots are exactly the cluster the
    case is named for under the Python twin of key_hash -- 62, 63, 0..29 for `wrap` -- and each holds the lowest row of a
    distinct table value.  (If that scratch layout changes, this is the one assertion to update.)"""
    L = h2.lib()
    c, d_table, d_in, ptrs = _case_on_device(name)
    cap = H.table_capacity(c.usable)
    d_m = _garbage(c.n)
    assert L.h2_dev_logup_multiplicity(d_table.data_ptr(), ptrs, len(d_in), c.usable, c.n, d_m.data_ptr(), scratch[0].data_ptr(),
                                       scratch[1], None) == 0, L.h2_last_error()
    slots = [int(s) for s in host_u32(scratch[0][:4 * cap])]
    occupied = [s for s in range(cap) if slots[s] != 0xFFFFFFFF]
    assert occupied == sorted(c.claim["occupied"]) == sorted(H.occupied_slots(c.table[:c.usable], cap))
    first = {}
    for i, key in enumerate(H.keys_of(c.table[:c.usable])):
        first.setdefault(key, i)
    assert sorted(slots[s] for s in occupied) == sorted(first.values())


# ------------------------------------------------------------------------------------------------ h2_dev_check_lookup
TAGS = (0 << 16 | 0, 0 << 16 | 1, 1 << 16 | 0)
LOOKUP_INDEX = 5


def _planted(c):
    """three input columns of the case with absent values at: row 0, row usable - 1, a row >= usable (not reported), rows held
    by two inputs (only the first reports) and every row of one whole wave (all usable rows when there are fewer than 128).
    The absent values probe the case's cluster first where it has one."""
    u = c.usable
    home = min(c.claim["homes"]) if "homes" in c.claim else None
    absent = H.absent_values(c, 4, home=home)
    ins = [c.inputs[j % len(c.inputs)].copy() for j in range(3)]
    ins[0][0] = absent[0]
    ins[2][u - 1] = absent[1]
    ins[0][u] = absent[0]
    ins[1][c.n - 1] = absent[2]
    if u >= 128:
        ins[1][64:128] = absent[2]
        ins[1][np.arange(64, 128, 3)] = absent[3]
        shared = ((70, (0, 1)), (200, (1, 2)), (u - 2, (0, 2)))
    else:
        ins[2][:u] = absent[2]
        shared = ((7, (0, 1)), (9, (1,)), (u - 1, (0, 2)))
    for row, cols in shared:
        for j in cols:
            ins[j][row] = absent[1]
    return ins


@pytest.mark.parametrize("name", ["wrap", "adjacent_homes", "padding"])
def test_check_lookup_reports_the_first_missing_input_of_a_row(scratch, name):
    L = h2.lib()
    c, d_table, _, _ = _case_on_device(name)
    ins = _planted(c)
    want = H.lookup_failures(c.table, ins, TAGS, c.usable, index=LOOKUP_INDEX)
    rows = [r for _, _, r in want]
    assert 0 in rows and c.usable - 1 in rows and len(set(rows)) == len(rows) >= 32 and max(rows) < c.usable
    assert {t for _, t, _ in want} == set(TAGS)
    d_in = [dev(a) for a in ins]
    ptrs = (ctypes.c_void_p * 3)(*[t.data_ptr() for t in d_in])
    rec = Records(c.usable + 50)
    assert L.h2_dev_check_lookup(d_table.data_ptr(), ptrs, (ctypes.c_uint32 * 3)(*TAGS), 3, c.usable, c.n, LOOKUP_INDEX, CIRCUIT,
                                 scratch[0].data_ptr(), scratch[1], *rec.out, None) == 0, L.h2_last_error()
    assert rec.check(want, H2_CHECK_LOOKUP | CIRCUIT << 8) == want


# ------------------------------------------------------------------------------------------------ h2_dev_check_shuffle
GROUP, UNIT = 4, 2
SHUFFLE_SHAPES = {250: (256, 1020, 200, 65), 32: (64, 126, 20, 17)}     # usable: n, home slot, repeats, hot rows
SHUFFLE_KINDS = ("permuted", "all_equal", "swapped", "shuffle_only", "hot_wave")


def _shuffle_columns(kind, usable):
    """Both columns from range-table keys that all probe ONE slot near the end of the shuffle table (its capacity is
    table_capacity(2 usable)): the table's clusters wrap as the lookup's do.  Rows >= usable differ between the sides."""
    n, home, repeats, hot = SHUFFLE_SHAPES[usable]
    cap = H.table_capacity(2 * usable)
    vals = H.small_by_home(cap)[home]
    keys = H.small_keys()[vals[:12]]
    assert cap - home < 12                                  # the cluster of the distinct keys runs past the last slot
    rng = np.random.default_rng(usable)
    idx = np.concatenate([np.full(repeats, 0), rng.integers(1, 9, size=usable - repeats)])    # one value `repeats` times
    if kind == "all_equal":
        idx[:] = 3
    if kind == "hot_wave":                                  # `hot` rows of key 9: a whole wave and its neighbour (usable 250)
        idx = np.where(idx == 9, 1, idx)
        first = 64 if usable >= 128 else 8
        idx[first:first + hot] = 9
    inp = idx[rng.permutation(usable)] if kind != "hot_wave" else idx
    shf = inp[rng.permutation(usable)].copy()
    if kind in ("swapped", "hot_wave"):                     # one occurrence of a value becomes another value of the input
        frm, to = (0, 5) if kind == "swapped" else (9, 2)
        shf[np.nonzero(shf == frm)[0][0]] = to
    if kind == "shuffle_only":                              # ... or a value the input does not have
        shf[np.nonzero(shf == 0)[0][0]] = 10
    a = np.concatenate([keys[inp], np.repeat(keys[11][None], n - usable, axis=0)])
    b = np.concatenate([keys[shf], np.repeat(keys[4][None], n - usable, axis=0)])
    return a, b, n, inp


@pytest.mark.parametrize("usable", sorted(SHUFFLE_SHAPES))
@pytest.mark.parametrize("kind", SHUFFLE_KINDS)
def test_check_shuffle_reports_the_rows_counted_differently(scratch, kind, usable):
    L = h2.lib()
    a, b, n, inp = _shuffle_columns(kind, usable)
    rows = H.shuffle_failures(a, b, usable)
    hot = SHUFFLE_SHAPES[usable][3]
    expect = {"permuted": [], "all_equal": [], "swapped": [r for r in range(usable) if inp[r] in (0, 5)],
              "shuffle_only": [r for r in range(usable) if inp[r] == 0],
              "hot_wave": [r for r in range(usable) if inp[r] in (9, 2)]}[kind]
    assert rows == expect
    if kind == "hot_wave":
        assert sum(1 for r in range(usable) if inp[r] == 9) == hot and hot in (17, 65)
    want = [(GROUP, UNIT, r) for r in rows]
    d_a, d_b = dev(a), dev(b)
    rec = Records(usable + 10)
    assert L.h2_dev_check_shuffle(d_a.data_ptr(), d_b.data_ptr(), usable, n, GROUP, UNIT, CIRCUIT, scratch[0].data_ptr(),
                                  scratch[1], *rec.out, None) == 0, L.h2_last_error()
    assert rec.check(want, H2_CHECK_SHUFFLE | CIRCUIT << 8) == want
