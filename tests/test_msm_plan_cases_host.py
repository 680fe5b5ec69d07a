"""tests/msm_plan_cases.py without a GPU: the ctypes mirror of h2_msm_launch_info against the header, the two host references
against the oracle and against each other's premises, and the well-formedness of the rows of tests/test_gpu_msm_plans.py."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np

import halo2_gpu_specific_amd as h2
from h2util import R_MOD, ROOT, arr_to_points, to_mont

import msm_plan_cases as mc


def test_launch_info_mirrors_the_header(tmp_path):
    """field names, order and types of h2_msm_launch_info, and its size as a C compiler lays it out"""
    header = open(os.path.join(ROOT, "include", "halo2_hip.h")).read()
    body = re.search(r"typedef struct \{((?:(?!typedef struct).)*?)\} h2_msm_launch_info;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for ctype, names in re.findall(r"(uint32_t|uint64_t)\s+([^;]+);", body):
        fields += [(n.strip(), ctypes.c_uint32 if ctype == "uint32_t" else ctypes.c_uint64) for n in names.split(",")]
    assert fields == list(mc.LaunchInfo._fields_)
    for name, count in mc.L_ENUM_COUNTS.items():
        assert re.search(r"\b%s\s*=\s*%d\b" % (name, count), header), name
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "halo2_hip.h"\nint main(void) { printf("%zu %zu\\n", '
                   'sizeof(h2_msm_launch_info), offsetof(h2_msm_launch_info, hot_mask)); return 0; }\n')
    exe = tmp_path / "size"
    subprocess.check_call(["cc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    size, off = map(int, subprocess.check_output([str(exe)]).split())
    assert (size, off) == (ctypes.sizeof(mc.LaunchInfo), mc.LaunchInfo.hot_mask.offset)


def test_no_launch_no_record():
    L = h2.lib()
    assert L.h2_msm_last_launches(None, 0) == 0
    buf = (mc.LaunchInfo * 1)()
    assert L.h2_msm_last_launches(buf, 1) == 0
    out = np.zeros(12, dtype=np.uint64)
    assert L.h2_msm(None, None, 0, 254, out.ctypes.data) == 0 and L.h2_msm_last_launches(None, 0) == 0


def test_int_msm_equals_the_oracle(oracle):
    """the Python-integer sum and the oracle's best_multiexp share no code and agree -- over the pinned points (identity,
    P + P, P - P) and every distribution"""
    n = 48
    pts = mc.build_points(oracle, 5, n)
    assert arr_to_points(pts)[5] == (0, 0) and arr_to_points(pts)[10] == arr_to_points(pts)[11]
    (x12, y12), (x13, y13) = arr_to_points(pts)[12:14]
    assert x12 == x13 and (y12 + y13) % mc.Q_MOD == 0 and y12
    for dist in ("uniform", "one", "dominant", "sparse", "three", "five", "zero_one_minus_one", "digit_extremes"):
        vals = mc.build_scalars(dist, n, 254, 9, mc.digit_widths(254, W=64))
        want = arr_to_points(oracle.to_affine(oracle.best_multiexp(to_mont(vals), pts, threads=2)))[0]
        assert mc.int_msm(vals, arr_to_points(pts)) == want, dist


def _fake_record(form, c, wfull, W, bits, R=1, range_shift=31, hot=0, block_sums=0, cols=0):
    rec = dict.fromkeys([k for k, _ in mc.LaunchInfo._fields_], 0)
    rec.update(form=form, c=c, wfull=wfull, W=W, max_bits=bits, R=R, range_shift=range_shift, nb=1 << (c - 1), hot_on=hot,
               block_sums=block_sums, cols=cols, Wc=W + 1)
    return rec


def test_recode_gives_back_the_scalars():
    """the (bucket, entry) pairs of recode(), decoded again: sum over a row's entries of +-(bucket + 1) 2^(window offset) is
    its scalar; the dominant value's rows sit in bucket 0 of the extra window, whole blocks as one entry; digit extremes
    produce nothing but the two extreme digits"""
    n, bits, W = 600, 254, 37
    widths = mc.digit_widths(bits, W=W)
    c, wfull = widths[0], sum(1 for w in widths if w == widths[0])
    offs = [sum(widths[:w]) for w in range(W)]
    assert sum(widths) == bits + 1 and set(widths) <= {c, c - 1}
    for dist in ("uniform", "dominant", "digit_extremes", "zero_one_minus_one"):
        vals = mc.build_scalars(dist, n, bits, 3, widths)
        hot = mc.sampled_hot(vals)
        rec = _fake_record(0, c, wfull, W, bits, hot=1 if hot is not None else 0, block_sums=1 if hot is not None else 0)
        pairs = mc.recode([vals], rec)
        total = [0] * n
        blocks = 0
        for e in pairs:
            bucket, entry = int(e) >> 32, int(e) & 0xFFFFFFFF
            w, b = divmod(bucket, rec["nb"])
            idx, neg = entry & 0x7FFFFFFF, entry >> 31
            if w == W:
                assert b == 0 and not neg
                if idx >= mc.BLOCK_INDEX0:
                    blocks += 1
                    for i in range((idx - mc.BLOCK_INDEX0) * 256, (idx - mc.BLOCK_INDEX0 + 1) * 256):
                        total[i] += hot
                else:
                    total[idx] += hot
                continue
            if dist == "digit_extremes" and w < W - 1:
                assert (b + 1, neg) in ((1 << (widths[w] - 1), 0), ((1 << (widths[w] - 1)) - 1, 1)), (w, b, neg)
            total[idx] += (-1 if neg else 1) * (b + 1) << offs[w]
        assert total == vals, dist
        assert (blocks > 0) == (dist == "dominant")
    # over a table: every digit in window 0, entry = level * table_n + row; row ranges: window (i >> shift) * W + w
    vals = mc.build_scalars("uniform", 300, 254, 4, mc.digit_widths(254, digits=32))
    rec = _fake_record(1, 8, 31, 32, 254)
    pairs = mc.recode([vals], rec, table_n=1000)
    assert all(int(e) >> 32 < 128 for e in pairs) and {(int(e) & 0x7FFFFFFF) // 1000 for e in pairs} == set(range(32))
    vals = mc.build_scalars("uniform", 5000, 8, 4, [9])
    pairs = mc.recode([vals], _fake_record(0, 9, 1, 1, 8, R=3, range_shift=11))
    assert all((int(e) >> 32) // 256 == (int(e) & 0x7FFFFFFF) >> 11 for e in pairs)


def test_rows_are_well_formed():
    rows = mc.WINDOWED_ROWS + mc.TABLE_ROWS + mc.FUSED_ROWS
    assert len({r.name for r in rows}) == len(rows)
    fields = {k for k, _ in mc.LaunchInfo._fields_} | {"launches", "scratch_slices", "hot_mask_bit", "staged", "RG>1", "R>1"}
    names = [c[0] for c in mc.CHILDREN]
    assert len(set(names)) == len(names)
    for r in rows + [r for c in mc.CHILDREN for r in c[2]]:
        assert set(r.expect) <= fields, r.name
        assert r.classes <= mc.DEFAULT_CLASSES, r.name
        assert r.n <= (1 << 17) + 8
        assert (r.kind == "single") == isinstance(r.dist, str), r.name
        assert not r.digits or r.lo + r.n <= r.table_n
    for form in ("w ", "t ", "f "):   # a row for the Python-integer sum in every form
        assert any(r.name.startswith(form) and r.n <= mc.INT_CHECK_MAX_N for r in rows), form
    for _, env, _, must in mc.CHILDREN:
        assert set(env) <= set(mc.KNOBS) and must
    assert not mc.DEFAULT_BRANCHES & mc.KNOB_ONLY_BRANCHES
    assert mc.KNOB_ONLY_BRANCHES <= set().union(*[c[3] for c in mc.CHILDREN])


def test_scratch_classes_on_a_made_up_launch():
    """partials per bucket, the heavy count and the classes, from starts and pbase written by hand (log_s = 3)"""
    rec = _fake_record(0, 3, 1, 2, 5)
    rec.update(np=2, nbt=8, log_s=3, lo_bits=2, hi_bits=0, skew_threshold=4096, stage_cap=0, hot_partition=mc.NO_PARTITION)
    # bucket 0: 8 * 33 entries = 33 partials (mid); 1: 3 entries; 2: empty; 3: 8 * 513 (heavy); 4: 8 * 16385 (capped); 5..7: one each
    sizes = [264, 3, 0, 4104, 131080, 1, 1, 1]
    starts = np.cumsum([0] + sizes).astype(np.uint32)
    pbase = np.array([0, starts[4], starts[8]], dtype=np.uint32)
    got = mc.scratch_classes(rec, pbase, starts, 3)
    assert got == {"serial", "mid", "heavy", "heavy_capped", "empty_run", "skewed"}, got
    import pytest

    with pytest.raises(AssertionError):
        mc.scratch_classes(rec, pbase, starts, 2)


def test_check_sort_names_what_is_wrong():
    """a sorted list built from the recoding passes; with one entry lost from the end of a partition (what a broken copy-out
    of a staged partition leaves), one sign flipped or one digit moved to the next bucket it fails and names the bucket"""
    import pytest

    n, bits, D = 512, 254, 32
    vals = mc.build_scalars("uniform", n, bits, 11, mc.digit_widths(bits, digits=D))
    rec = _fake_record(1, 8, 31, 32, bits)
    rec.update(nbt=128, np=1, lo_bits=7)
    pairs = mc.recode([vals], rec, table_n=n)
    bucket = (pairs >> np.uint64(32)).astype(np.int64)
    starts = np.concatenate([[0], np.cumsum(np.bincount(bucket, minlength=128))]).astype(np.uint32)
    entries = (pairs & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    rng = np.random.default_rng(1)
    for b in range(128):   # (the device's order inside a bucket is whatever the atomics gave)
        rng.shuffle(entries[starts[b]:starts[b + 1]])
    mc.check_sort(rec, starts, entries, pairs)
    lost = entries.copy()
    lost[-1] = 0
    with pytest.raises(AssertionError, match="bucket 127"):
        mc.check_sort(rec, starts, lost, pairs)
    flipped = entries.copy()
    flipped[starts[40]] ^= mc.SIGN_BIT
    with pytest.raises(AssertionError, match="bucket 40"):
        mc.check_sort(rec, starts, flipped, pairs)
    moved = starts.copy()
    moved[41] -= 1      # the last entry of bucket 40 counted into bucket 41
    with pytest.raises(AssertionError, match="bucket 40 holds"):
        mc.check_sort(rec, moved, entries, pairs)
