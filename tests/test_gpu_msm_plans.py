"""Every branch of the MSM launcher (csrc/msm_plan.cpp msm_plan_launch, csrc/msm_kernels.hip msm_enqueue) at small pinned shapes,
with evidence that it ran.

One planned launch picks a form (windowed, shifted-base table, fused group), a partition (k_partition<2048>, <16384>, the
two-level k_part_a / k_part_b), a k_bucket_sort path per partition (plain, staged in LDS, skewed, the dominant value's
short cut), k_acc_slice<4> or <5>, k_finish or k_finish_lane with four classes of bucket behind it, and k_reduce or the bit
planes.  Part of that depends on the sampled scalars, so it cannot be told from the sizes: the launcher records what it
handed its kernels (h2_msm_last_launches) and the rows of tests/msm_plan_cases.py are laid over the record's space.

Every row (tests/msm_plan_worker.py) is compared, as an affine point, with the oracle's best_multiexp; rows of n <= 256 -- at
least one per form -- also with sum s_i P_i in Python integers (msm_plan_cases.int_msm).  Then the evidence:
  (a) the record shows the values the row exists for (Row.expect);
  (b) single-launch rows: pbase, starts and heavy[0] are read back from the scratch; heavy[0] is the number of buckets with
      more than FINISH_SERIAL partials, and the row populated the classes it names (a skewed partition, one with more bins
      than SKEW_ROUNDS, a staged partition, a mid / heavy / capped-heavy bucket, a bucket ending inside a slice in front of
      an empty one);
  (c) single-launch rows of n <= 2^15: the scalars' digits, recoded in Python integers by the rule k_digits documents, give
      every bucket's size and its (row or table index, sign) entries as a set: `starts` and `sorted` are exactly that;
  (d) the branches of this process's rows are every branch default knobs reach at these sizes, and every knob child (one
      fresh process per setting, one after another, compared with the oracle inside the child) reports the branch it is for;
  (e) every row's launch records, but for the scratch address, equal tests/golden/msm_launch_records.json, recorded on an
      MI355X before the launcher was split into plan and enqueue (the children compare theirs in the child).

Rows (msm_plan_cases.WINDOWED_ROWS / TABLE_ROWS / FUSED_ROWS / CHILDREN; DESIGN.md's MSM section lists them with the wall
clock).  Distributions: uniform, one value, 7/8 one value over whole 256-row blocks and ragged runs, 1/16 non-zero, three
and five neighbouring values, {0, 1, r - 1}, digit extremes (every digit 2^(cw-1) or 2^(cw-1) + 1 with the carry).  Points:
random, one identity, two equal, P and -P in one bucket.

The cap of heavy_parts at HEAVY_SPLIT changes something only from 256 * 64 + 1 = 16385 partials on (16129 .. 16384 give 64
parts with or without it), which at the shortest slices default knobs choose (log_s = 3) is one slice more than 2^17 rows of
one value: that row has n = 2^17 + 8, the largest of the module; with H2_MSM_SLICE_LOG=1 a child has it at 2^15 + 2.

What default knobs do not reach below n = 2^17, and why (each is reached by a child instead):
  * k_finish_lane: nbt >= 2^19.  Windowed, nbt = Wt * 2^(c-1) with c <= 12 and Wt <= 65 below 2^17 rows: < 2^18.  Over a
    table it takes c >= 20, i.e. D <= 13 digits, and table_pays asks D n + 10 * 2^(c-1) < W n + 10 Wt nb of the windowed
    shape: (20 - 13) * 2^17 = 0.9 M against 10 * 2^19 = 5.2 M -- such a table pays from 2^20 rows.  H2_MSM_TABLE_FORCE=1 (it
    skips table_pays) and H2_MSM_FINISH_LANE_LOG=0 reach it.
  * k_partition<16384> over every key array: a table with hi_bits > 10 that is not two-level, and two-level is every table
    with 8 <= hi_bits <= 14: H2_MSM_TWO_LEVEL=0 only.
  * k_reduce over a table's window: the planes are on for every power-of-two qm with nb >= 4 qm, and a table has nb >= 128
    and qm a power of two by default: H2_MSM_REDUCE_PLANES=0 or H2_MSM_REDUCE_QM=3 only.
  * the lo_bits growth loops: windowed / fused, Wt << (c - 1 - 8) > 16384 needs c = 17 with more than 64 windows
    (H2_MSM_WINDOW=17, fused); over a table c - 1 - 8 > 13 is D <= 11 or 12 digits (2^22, 2^23 buckets: H2_MSM_TABLE_FORCE=1).
  * k_acc_slice<5>: H2_MSM_ACC_WAVES=5 only.
  * a fused group without the dominant-value slot (Wc = W) needs a bound of one or two windows that still spreads over 16
    partitions: not 16 bits below 2^17 rows (two windows of 9 bits: one partition each) but 23 bits from 11137 rows on
    (two windows of 12 bits); that row is in FUSED_ROWS.
"""
import os
import subprocess
import sys
import threading
import time

import pytest

import halo2_gpu_specific_amd as h2
from h2util import ROOT

import msm_plan_cases as mc

pytestmark = pytest.mark.gpu

SEEN = {}          # row name -> (branches, classes) of the rows that passed in this process
# the slowest child measured on an MI355X host with 16 CPUs (MSM section), times four, rounded up to 10 s
CHILD_TIMEOUT = 20
_RUNNER = []


@pytest.fixture(scope="module")
def runner(oracle):
    from msm_plan_worker import Runner

    if not _RUNNER:
        _RUNNER.append(Runner(oracle))
    yield _RUNNER[0]
    _RUNNER[0].forget()


def _ids(rows):
    return [r.name for r in rows]


def _run(runner, row):
    import msm_plan_worker  # noqa: F401

    recs, found = runner.run(row)
    mc.check_golden(None, row, recs)
    SEEN[row.name] = (set().union(*[mc.branches(r) for r in recs]), found)
    print(row.name, "->", sorted(SEEN[row.name][0]), sorted(found))


@pytest.mark.parametrize("row", mc.WINDOWED_ROWS, ids=_ids(mc.WINDOWED_ROWS))
def test_windowed(runner, row):
    """the windowed form: bounds of one, two and many windows, row ranges, the dominant value's window on both sides of
    MID_MAX and above the cap of heavy_parts, the skewed sort; one pipeline batch"""
    _run(runner, row)


@pytest.mark.parametrize("row", mc.TABLE_ROWS, ids=_ids(mc.TABLE_ROWS))
def test_table(runner, row):
    """over a shifted-base table: one partition and several, staged and not, the two-level partition with and without the
    dominant value's array, block sums and a view off a block boundary"""
    _run(runner, row)


@pytest.mark.parametrize("row", mc.FUSED_ROWS, ids=_ids(mc.FUSED_ROWS))
def test_fused(runner, row):
    """fused groups: with the dominant-value slot, 64 + 2 columns, and without the slot"""
    _run(runner, row)


def test_the_record_is_per_call_and_per_thread(runner):
    """the list holds the last call's launches only, a zero-length MSM leaves it empty, a count above `cap` is reported and
    `cap` respected, and another thread sees none of it"""
    L = runner.L
    runner.run(mc.FUSED_ROWS[2])                    # 64 + 2 columns: two launches
    assert L.h2_msm_last_launches(None, 0) == 2
    buf = (mc.LaunchInfo * 2)()
    buf[1].form = 77
    assert L.h2_msm_last_launches(buf, 1) == 2 and buf[0].cols == 64 and buf[1].form == 77
    assert L.h2_msm_last_launches(buf, 2) == 2 and buf[1].cols == 2 and buf[1].form == 2
    other = []
    t = threading.Thread(target=lambda: other.append(L.h2_msm_last_launches(None, 0)))
    t.start()
    t.join()
    assert other == [0]
    runner.run(mc.WINDOWED_ROWS[0])
    assert L.h2_msm_last_launches(None, 0) == 1
    import numpy as np

    out = np.zeros(12, dtype=np.uint64)
    assert L.h2_dev_msm(None, None, 0, 254, None, 0, out.ctypes.data, None) == 0
    assert L.h2_msm_last_launches(None, 0) == 0


@pytest.mark.timeout(len(mc.CHILDREN) * CHILD_TIMEOUT + 60)
def test_coverage_and_knob_children():
    """(d): this process's rows reached every default branch and class; then every knob setting in a child process of its
    own, one after another -- a child that fails, times out or dies by a signal ends the test there"""
    rows = mc.WINDOWED_ROWS + mc.TABLE_ROWS + mc.FUSED_ROWS
    missing = [r.name for r in rows if r.name not in SEEN]
    assert not missing, "the coverage is over the rows of the whole module: these did not pass: %s" % missing
    seen_branches = set().union(*[SEEN[r.name][0] for r in rows])
    seen_classes = set().union(*[SEEN[r.name][1] for r in rows])
    never = sorted((mc.DEFAULT_BRANCHES - seen_branches) | {"class:" + c for c in mc.DEFAULT_CLASSES - seen_classes})
    assert not never, "no row of this process reaches %s" % never
    for names, prefix in ((mc.FORMS, "form:"), (mc.PARTS, "part:"), (mc.FINISH, "finish:"), (mc.REDUCE, "reduce:")):
        for name in names:   # every value of the record's enumerations is somebody's: a default row's or a child's
            assert prefix + name in mc.DEFAULT_BRANCHES | mc.KNOB_ONLY_BRANCHES
    beyond = sorted(seen_branches & mc.KNOB_ONLY_BRANCHES)
    assert not beyond, "default knobs reach %s: move it to DEFAULT_BRANCHES and correct the module docstring" % beyond
    script = os.path.join(ROOT, "tests", "msm_plan_worker.py")
    reported = set()
    for name, knobs, _, must in mc.CHILDREN:
        env = {k: v for k, v in os.environ.items() if k not in mc.KNOBS}
        env.update(knobs)
        t0 = time.time()
        res = subprocess.run([sys.executable, script, name], env=env, capture_output=True, text=True, timeout=CHILD_TIMEOUT, cwd=ROOT)
        assert res.returncode == 0 and "CHILD OK" in res.stdout, (name, knobs, res.returncode, res.stdout[-3000:], res.stderr[-3000:])
        line = [ln for ln in res.stdout.splitlines() if ln.startswith("BRANCHES ")][-1]
        got = set(line.split()[1:])
        print("%s %s: %.1f s -> %s" % (name, knobs, time.time() - t0, sorted(got)))
        assert must <= got, "child %s does not report %s" % (name, sorted(must - got))
        reported |= got
    assert mc.KNOB_ONLY_BRANCHES <= reported, "no child reaches %s" % sorted(mc.KNOB_ONLY_BRANCHES - reported)
