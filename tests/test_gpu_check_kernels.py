"""Direct calls of the h2_dev_check_* entry points (csrc/check.hip, append.hpp) on the device: the record append at every wave
pattern and around a full buffer, the non-zero row compaction, the gate interpreter's grid-stride loop on its second trip
(k = 17, more than 65 536 listed rows) and the copy check with mappings that leave the columns.  References are Python loops and
numpy limb comparisons; every assertion is bit-exact."""
import ctypes

import numpy as np
import pytest
import torch

import halo2_gpu_specific_amd as h2
import hash_table_cases as H
from check_records import (CIRCUIT, H2_CHECK_COPY, H2_CHECK_GATE, H2_CHECK_LOOKUP, SENTINEL, Records, dev, dev_u32, host_u32)
from halo2_gpu_specific_amd import evaluation as ev

pytestmark = pytest.mark.gpu

MAX_N = 1024
LOOKUP_INDEX, TAG = 2, 1 << 16 | 3


@pytest.fixture(scope="module")
def scratch():
    nbytes = h2.lib().h2_check_scratch_bytes(MAX_N)
    return torch.empty(nbytes, dtype=torch.uint8, device="cuda"), nbytes


# ------------------------------------------------------------------------------------------------ the record append
_table = {}


def _lookup_table():
    """the `padding` table (usable = 1000 of 1024 rows: 16 waves, the last one of 40 usable lanes), on the device once"""
    if not _table:
        c = H.case("padding")
        _table.update(c=c, d=dev(c.table), absent=H.absent_values(c, 1)[0])
    return _table["c"], _table["d"], _table["absent"]


def _failing_column(rows):
    """one input column of the table's own values with an absent value at `rows`"""
    c, _, absent = _lookup_table()
    col = c.inputs[0].copy()
    col[list(rows)] = absent
    return col


def _run_lookup(scratch, col, rec):
    c, d_table, _ = _lookup_table()
    d_col = dev(col)
    ptrs = (ctypes.c_void_p * 1)(d_col.data_ptr())
    L = h2.lib()
    assert L.h2_dev_check_lookup(d_table.data_ptr(), ptrs, (ctypes.c_uint32 * 1)(TAG), 1, c.usable, c.n, LOOKUP_INDEX, CIRCUIT,
                                 scratch[0].data_ptr(), scratch[1], *rec.out, None) == 0, L.h2_last_error()


LOOKUP_KIND = H2_CHECK_LOOKUP | CIRCUIT << 8
# the failing lanes of a wave (rows w * 64 + lane); rows 1000 .. 1023 are past usable and never reported
WAVE_PATTERNS = {
    "whole_wave": list(range(128, 192)),
    "lane_0": [320],
    "lane_63": [383],
    "lanes_31_32": [5 * 64 + 31, 5 * 64 + 32],
    "none": [],
    "partial_last_wave": list(range(960, 1024)),
    "partial_last_wave_lane_39": [999, 1000],
    "every_pattern": list(range(64)) + [64] + [191] + [4 * 64 + 31, 4 * 64 + 32] + list(range(970, 1024, 3)) + [999],
}


@pytest.mark.parametrize("pattern", sorted(WAVE_PATTERNS))
def test_record_append_by_wave_pattern(scratch, pattern):
    c, _, _ = _lookup_table()
    rows = WAVE_PATTERNS[pattern]
    want = [(LOOKUP_INDEX, TAG, r) for r in sorted(set(rows)) if r < c.usable]
    assert len(want) == {"whole_wave": 64, "lane_0": 1, "lane_63": 1, "lanes_31_32": 2, "none": 0, "partial_last_wave": 40,
                         "partial_last_wave_lane_39": 1, "every_pattern": 64 + 1 + 1 + 2 + 11}[pattern]
    rec = Records(len(want) + 3)
    _run_lookup(scratch, _failing_column(rows), rec)
    assert rec.check(want, LOOKUP_KIND) == want


def _three_hundred():
    rows = sorted(int(r) for r in np.random.default_rng(300).permutation(1000)[:300])
    return rows, [(LOOKUP_INDEX, TAG, r) for r in rows]


@pytest.mark.parametrize("cap", [0, 1, 63, 64, 65, 299, 300, 307])
def test_record_append_around_a_full_buffer(scratch, cap):
    """300 failures into a buffer of `cap` records: the count is exact, the first min(cap, 300) slots hold distinct real
    failures (all of them, once cap allows) and nothing is written behind them"""
    rows, want = _three_hundred()
    rec = Records(cap)
    _run_lookup(scratch, _failing_column(rows), rec)
    rec.check(want, LOOKUP_KIND)


@pytest.mark.parametrize("cap", [700, 450, 300])
def test_record_append_continues_after_an_earlier_call(scratch, cap):
    """the count is the caller's to zero: a second call on the same block appends behind the first call's records"""
    rows, want = _three_hundred()
    rec = Records(cap)
    col = _failing_column(rows)
    _run_lookup(scratch, col, rec)
    first = rec.check(want, LOOKUP_KIND)
    assert first == want
    _, before = rec.read()
    _run_lookup(scratch, col, rec)
    total, after = rec.read()
    assert total == 600
    assert (after[:300] == before[:300]).all()                       # no earlier record is overwritten
    kept = min(cap, 600) - 300
    second = [tuple(int(x) for x in r) for r in after[300:300 + kept]]
    assert all(r[0] == LOOKUP_KIND for r in second)
    assert len({r[1:] for r in second}) == kept and {r[1:] for r in second} <= set(want)
    if cap >= 600:
        assert sorted(r[1:] for r in second) == want
    assert (after[300 + kept:] == SENTINEL).all()


# ------------------------------------------------------------------------------------------------ h2_dev_check_nonzero_rows
@pytest.mark.parametrize("usable,n", [(0, 64), (1, 64), (64, 64), (250, 256), (1000, 1024)])
def test_nonzero_rows(usable, n):
    """non-zeros at rows 0, 63, 64, usable - 1, one full wave and past usable; a value may be non-zero in one limb only"""
    L = h2.lib()
    values = np.zeros((n, 4), dtype=np.uint64)
    marks = [0, 63, 64, usable - 1, usable, n - 1, 300, 301, 555] + list(range(128, 192))
    for j, r in enumerate(r for r in marks if 0 <= r < n):
        values[r, (j // 2) % 4] = np.uint64(1) << np.uint64((j % 2) * 32 + j % 31)      # one bit of one 32-bit limb
    want = [r for r in range(usable) if values[r].any()]
    assert set(want) == {r for r in marks if 0 <= r < usable} and (usable == n or values[usable:].any())
    d_values = dev(values)
    d_rows = dev_u32(np.full(max(usable, 1) + 8, SENTINEL, dtype=np.uint32))
    d_count = torch.zeros(1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    assert L.h2_dev_check_nonzero_rows(d_values.data_ptr(), usable, d_rows.data_ptr(), d_count.data_ptr(), None) == 0
    got = host_u32(d_rows)
    assert int(d_count.cpu()[0]) == len(want)
    assert sorted(int(r) for r in got[:len(want)]) == want           # (the list is in no particular order)
    assert (got[len(want):] == SENTINEL).all()


# ------------------------------------------------------------------------------------------------ h2_dev_check_gates
GATE_K = 17


def _random_elements(rng, n):
    """(n, 4) canonical stored forms: any value below 2^253 is one"""
    a = rng.integers(0, 1 << 63, size=(n, 4), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=(n, 4), dtype=np.uint64)
    a[:, 3] >>= np.uint64(11)
    return a


_gates = {}


def _gate_program():
    """Three gate polynomials over n = 2^17 rows whose zero-ness numpy decides by limb comparison alone:
         part 0   advice0 - fixed0                  zero where the two columns hold the same limbs
         part 1   advice1[row + 1] * fixed1         zero where either factor is zero; the rotation wraps at row n - 1
         part 2   (advice0 - fixed0) * advice2      the intermediate of part 0, read a second time
    -> (builder, columns kept alive, fail[3][n] booleans)"""
    if _gates:
        return _gates["b"], _gates["fail"]
    n = 1 << GATE_K
    rng = np.random.default_rng(GATE_K)
    fixed0 = _random_elements(rng, n)
    advice0 = fixed0.copy()
    differ = rng.random(n) < 0.3
    limb = rng.integers(0, 4, size=n)
    advice0[np.arange(n), limb] ^= np.where(differ, np.uint64(1) << rng.integers(0, 52, size=n).astype(np.uint64), np.uint64(0))
    advice1 = _random_elements(rng, n)
    advice1[rng.random(n) < 0.2] = 0
    fixed1 = _random_elements(rng, n)
    fixed1[rng.random(n) < 0.7] = 0
    advice2 = _random_elements(rng, n)
    advice2[rng.random(n) < 0.5] = 0
    # the wrap: row n - 1 reads advice1[0]; row n - 2 reads a zero at advice1[n - 1]
    advice1[0], fixed1[n - 1] = _random_elements(rng, 1)[0], _random_elements(rng, 1)[0]
    advice1[n - 1], fixed1[n - 2] = 0, _random_elements(rng, 1)[0]
    differ[0], advice0[0] = False, fixed0[0]
    part0 = (advice0 != fixed0).any(axis=1)
    assert (part0 == differ).all()
    part1 = np.roll(advice1.any(axis=1), -1) & fixed1.any(axis=1)
    part2 = part0 & advice2.any(axis=1)
    assert part1[n - 1] and not part1[n - 2]
    fail = np.stack([part0, part1, part2])
    assert len({tuple(f) for f in fail.T[:4096]}) == 6              # every combination the three parts allow (2 implies 0)
    cols = [dev(a) for a in (fixed0, fixed1, advice0, advice1, advice2)]
    zero = [0, 0, 0, 0]
    b = ev.Builder().build(
        k=GATE_K, extended_k=GATE_K, blinding_factors=0, chunk_len=1, constants=np.zeros((0, 4), dtype=np.uint64),
        rotations=[0, 1],
        calculations=[ev.calc(ev.CALC_SUB, ev.vs(ev.VS_ADVICE, 0, 0), ev.vs(ev.VS_FIXED, 0, 0)),
                      ev.calc(ev.CALC_MUL, ev.vs(ev.VS_ADVICE, 1, 1), ev.vs(ev.VS_FIXED, 1, 0)),
                      ev.calc(ev.CALC_MUL, ev.vs(ev.VS_INTERMEDIATE, 0), ev.vs(ev.VS_ADVICE, 2, 0))],
        value_parts=[ev.vs(ev.VS_INTERMEDIATE, 0), ev.vs(ev.VS_INTERMEDIATE, 1), ev.vs(ev.VS_INTERMEDIATE, 2)],
        fixed=[t.data_ptr() for t in cols[:2]], advice=[t.data_ptr() for t in cols[2:]], instance=[],
        y=zero, beta=zero, gamma=zero, theta=zero, delta=zero, zeta=zero, extended_omega=zero)
    b.keep.append(cols)
    _gates.update(b=b, fail=fail)
    return b, fail


# 65 536 lanes take the listed rows 65 536 at a time (256 workgroups of 256): 65 536 + 64 + 37 rows make every lane of two
# waves and 37 lanes of a third take a second trip
@pytest.mark.parametrize("listed", [65536 + 64 + 37, 65536, 1, 0])
def test_gate_rows_over_a_list_longer_than_the_grid(listed):
    L = h2.lib()
    b, fail = _gate_program()
    n = 1 << GATE_K
    rows = np.random.default_rng(listed).permutation(n)[:max(listed, 1)].astype(np.uint32)
    if listed == 1:
        rows[0] = n - 1                                              # the rotation's wrap
    d_rows = dev_u32(rows)
    d_listed = torch.tensor([listed], dtype=torch.int64, device="cuda")
    f = fail[:, rows[:listed].astype(np.int64)]                      # (3, listed)
    part, at = np.nonzero(f)
    want = np.stack([part.astype(np.uint32), rows[:listed][at]], axis=1) if listed else np.zeros((0, 2), dtype=np.uint32)
    want = want[np.lexsort((want[:, 1], want[:, 0]))]
    assert listed < 2 or len(want) > listed // 2
    rec = Records(len(want) + 5)
    torch.cuda.synchronize()
    assert L.h2_dev_check_gates(ctypes.byref(b.desc), d_rows.data_ptr(), d_listed.data_ptr(), CIRCUIT, *rec.out, None) == 0, \
        L.h2_last_error()
    total, recs = rec.read()
    assert total == len(want)
    got = recs[:total]
    assert (got[:, 0] == (H2_CHECK_GATE | CIRCUIT << 8)).all() and (got[:, 2] == 0).all()
    got = got[:, [1, 3]]
    got = got[np.lexsort((got[:, 1], got[:, 0]))]
    assert np.array_equal(got, want)
    assert (recs[total:] == SENTINEL).all()


# ------------------------------------------------------------------------------------------------ h2_dev_check_copies
def _copies(cols, map_col, map_row):
    """-> sorted (column, 0, row) of the cells whose mapped cell differs or lies outside the columns, by a Python loop"""
    n_columns, n = len(cols), len(cols[0])
    keys = [H.keys_of(c) for c in cols]
    out = []
    for c in range(n_columns):
        for r in range(n):
            mc, mr = int(map_col[c * n + r]), int(map_row[c * n + r])
            if mc >= n_columns or mr >= n or keys[c][r] != keys[mc][mr]:
                out.append((c, 0, r))
    return out


def _run_copies(cols, map_col, map_row, cap):
    L = h2.lib()
    n_columns, n = len(cols), len(cols[0])
    d_cols = [dev(c) for c in cols]
    d_ptrs = torch.tensor([t.data_ptr() for t in d_cols], dtype=torch.int64).cuda()
    d_mc, d_mr = dev_u32(map_col), dev_u32(map_row)
    rec = Records(cap)
    torch.cuda.synchronize()
    assert L.h2_dev_check_copies(d_ptrs.data_ptr(), n_columns, d_mc.data_ptr(), d_mr.data_ptr(), n, CIRCUIT, *rec.out, None) == 0, \
        L.h2_last_error()
    return rec


def test_copies_over_three_columns_of_a_hundred_rows():
    """n_columns n = 300 cells, not a multiple of the workgroup: the identity over unequal columns, 3-cycles across the
    columns, and mapping entries that leave the columns (a failure of their cell, never a read out of bounds)"""
    n_columns, n = 3, 100
    keys = H.small_keys()
    cols = [keys[1000 * c + 1:1000 * c + 1 + n].copy() for c in range(n_columns)]
    map_col = np.repeat(np.arange(n_columns, dtype=np.uint32), n)
    map_row = np.tile(np.arange(n, dtype=np.uint32), n_columns)
    assert _copies(cols, map_col, map_row) == []
    _run_copies(cols, map_col, map_row, 4).check([], H2_CHECK_COPY | CIRCUIT << 8)

    def cycle(cells):
        for (c, r), (mc, mr) in zip(cells, cells[1:] + cells[:1]):
            map_col[c * n + r], map_row[c * n + r] = mc, mr

    # (0, 10) -> (1, 20) -> (2, 30) -> (0, 10): the first two hold one value, the third another
    cycle([(0, 10), (1, 20), (2, 30)])
    cols[1][20] = cols[0][10]
    # a cycle of equal cells through the last row and the last cell: no record
    cycle([(0, 99), (2, 99), (1, 0)])
    cols[2][99] = cols[1][0] = cols[0][99]
    want = _copies(cols, map_col, map_row)
    assert want == [(1, 0, 20), (2, 0, 30)]
    _run_copies(cols, map_col, map_row, 8).check(want, H2_CHECK_COPY | CIRCUIT << 8)
    # entries outside the columns: column == n_columns, row == n, all ones -- at the first cell, inside and at the last cell
    for (c, r), (mc, mr) in {(0, 50): (n_columns, 50), (1, 60): (1, n), (2, 98): (0xFFFFFFFF, 0xFFFFFFFF), (0, 0): (0xFFFFFFFF, 0),
                             (1, 99): (1, 0xFFFFFFFF), (2, 97): (n_columns, n)}.items():
        map_col[c * n + r], map_row[c * n + r] = mc, mr
    want = _copies(cols, map_col, map_row)
    assert want == [(0, 0, 0), (0, 0, 50), (1, 0, 20), (1, 0, 60), (1, 0, 99), (2, 0, 30), (2, 0, 97), (2, 0, 98)]
    _run_copies(cols, map_col, map_row, 16).check(want, H2_CHECK_COPY | CIRCUIT << 8)
    _run_copies(cols, map_col, map_row, 5).check(want, H2_CHECK_COPY | CIRCUIT << 8)
