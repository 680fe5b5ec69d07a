"""The MSM plan (csrc/msm_plan.hpp, msm_plan.cpp) without a GPU: tests/msm_plan_host.cpp is built with g++ alone -- the plan
includes no HIP header -- and asked for

  1. every launch record of tests/golden/msm_launch_records.json (recorded on an MI355X by golden/gen_msm_launch_records.py).
     The program is given the call's inputs and what only the device could know -- the chosen form, whether the samples
     showed a dominant value (hot_on / hot_mask) and whether its blocks' sums were tabulated -- and every other field of the
     record has to come out of the plan: the shape, partition, finish, reduce, stage_cap, skew_threshold, hot_partition,
     acc_waves, the planes, every offset and the total.  Rows recorded under knobs run under that environment.  The size of
     every fused group is fused_group_limit's;
  2. tests/golden/msm_scratch_sizes.json (the grid of gen_msm_scratch_sizes.py) from the plan alone;
  3. each parsing rule of the H2_MSM_* variables at an unset, a valid and an invalid value.
"""
import json
import os
import subprocess

import pytest

import msm_plan_cases as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "halo2-gpu-specific_amd", "csrc")
FLAGS = ["-O1", "-std=c++17", "-Wall", "-Werror"]


def build(exe, extra=()):
    cmd = ["g++", *FLAGS, *extra, "-I", CSRC, os.path.join(ROOT, "tests", "msm_plan_host.cpp"), os.path.join(CSRC, "msm_plan.cpp"), "-o", str(exe)]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=240)
    assert res.returncode == 0, res.stderr[-4000:]
    return str(exe)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return build(tmp_path_factory.mktemp("msm_plan_host") / "msm_plan_host")


def ask(exe, cmd, lines=(), knobs=None):
    env = {k: v for k, v in os.environ.items() if not k.startswith("H2_MSM_")}
    env.update(knobs or {})
    res = subprocess.run([exe, cmd], input="".join(ln + "\n" for ln in lines), env=env, capture_output=True, text=True, timeout=120)
    assert res.returncode == 0 and not res.stderr, (cmd, knobs, res.returncode, res.stderr[-3000:])
    return res.stdout.splitlines()


def test_the_plan_includes_no_hip_header():
    for name in ("msm_plan.hpp", "msm_plan.cpp"):
        text = open(os.path.join(CSRC, name)).read()
        includes = [ln.split()[1] for ln in text.splitlines() if ln.startswith("#include")]
        assert all(i.startswith("<") or i in ('"msm_plan.hpp"', '"../../include/halo2_hip.h"') for i in includes), includes
        assert not [i for i in includes if "hip/" in i], includes
    for name in ("msm.hip", "msm_kernels.hip", "msm_table.hip", "msm_kernels.hpp", "msm_table.hpp", "msm.hpp", "msm_plan.hpp"):
        assert "getenv" not in open(os.path.join(CSRC, name)).read(), "%s reads the environment: msm_knobs() is the one reader" % name


def check_records(exe, entries):
    by_knobs = {}
    for e in entries:
        by_knobs.setdefault(json.dumps(e["knobs"], sort_keys=True), []).append(e)
    checked = 0
    for knobs, group in by_knobs.items():
        recs = [(e, r) for e in group for r in e["launches"]]
        lines = []
        for e, r in recs:
            assert r["max_bits"] in e["bits"], "a launch's bound is one of its call's"
            # the windowed form of a row over a table (table_pays said no) knows nothing of the table
            digits, table_n = (e["digits"], e["table_n"]) if r["form"] == 1 else (0, 0)
            lines.append("%d %d %d %d %d %d %d %d %d" % (r["form"], e["n"], r["max_bits"], r["cols"], digits, table_n, r["hot_on"], r["hot_mask"],
                                                         r["block_sums"]))
        out = ask(exe, "records", lines, json.loads(knobs))
        assert len(out) == len(recs)
        for (e, r), line in zip(recs, out):
            vals = [int(v) for v in line.split()]
            got, limit = dict(zip(mc.RECORD_FIELDS, vals)), vals[-1]
            assert len(vals) == len(mc.RECORD_FIELDS) + 1
            diff = {k: (got[k], r[k]) for k in mc.RECORD_FIELDS if got[k] != r[k]}
            assert not diff, "row '%s' %s: the plan differs from the record (plan, record): %s" % (e["name"], e["knobs"], diff)
            checked += 1
        for e in group:   # the columns of a batch fuse in groups of fused_group_limit
            sizes = [r["cols"] for r in e["launches"] if r["form"] == 2]
            if sizes:
                limit = int(out[[i for i, (e2, r) in enumerate(recs) if e2 is e][0]].split()[-1])
                count = len(e["columns"])
                assert sizes == [min(limit, count - m0) for m0 in range(0, count, limit) if count - m0 >= 2], (e["name"], sizes, limit)
    return checked


def test_the_plan_gives_every_recorded_launch(exe):
    entries = list(mc.golden_records().values())
    rows = mc.WINDOWED_ROWS + mc.TABLE_ROWS + mc.FUSED_ROWS
    want = {(None, r.name) for r in rows} | {(name, r.name) for name, _, child_rows, _ in mc.CHILDREN for r in child_rows}
    assert set(mc.golden_records()) == want, "the recorded rows are not msm_plan_cases' rows: record again"
    for name, knobs, _, _ in mc.CHILDREN:
        assert all(e["knobs"] == knobs for e in entries if e["child"] == name)
    assert check_records(exe, entries) == sum(len(e["launches"]) for e in entries) >= len(want)


def sizes_from_plan(exe):
    with open(os.path.join(ROOT, "tests", "golden", "msm_scratch_sizes.json")) as f:
        doc = json.load(f)
    lines = ["%d %d %s" % (n, bits, " ".join(map(str, doc["count"]))) for n in doc["n"] for bits in doc["max_bits"]]
    out = ask(exe, "sizes", lines)
    got = []
    for (n, bits), line in zip(((n, b) for n in doc["n"] for b in doc["max_bits"]), out):
        v = [int(x) for x in line.split()]
        got.append([n, bits, v[0], v[1], v[2], v[3], v[4:]])
    return got, doc["rows"]


def test_the_plan_gives_the_recorded_scratch_sizes(exe):
    got, want = sizes_from_plan(exe)
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g == w, "plan %s, recorded %s" % (g, w)


DEFAULTS = dict(slice_log=0, window=0, reduce_qm=0, table_lo=0, fuse_log=22, fuse_log_present=0, lanes=2, no_table=0, no_hot=0, no_fuse=0,
                table_force=0, table_min_n=1 << 15, table_digits=0, reduce_wgs=256, plane_wgs=192, reduce_planes=1, two_level=1,
                two_level_min_hi=8, sort_stage=1, acc_waves=4, finish_lane_from=1 << 19)
# variable -> (a valid value, what it sets), (an invalid or odd value, what that sets)
RULES = {
    "SLICE_LOG": (("10", dict(slice_log=10)), ("11", {})),
    "WINDOW": (("18", dict(window=18)), ("1", {})),
    "REDUCE_QM": (("64", dict(reduce_qm=64)), ("0", {})),
    "TABLE_LO": (("4", dict(table_lo=4)), ("13", {})),
    "FUSE_LOG": (("10", dict(fuse_log=10, fuse_log_present=1)), ("29", dict(fuse_log_present=1))),   # present, valid or not
    "LANES": (("4", dict(lanes=4)), ("5", {})),
    "NO_TABLE": (("1", dict(no_table=1)), ("yes", {})),             # on when the first character is 1
    "NO_HOT": (("1x", dict(no_hot=1)), ("0", {})),
    "NO_FUSE": (("1", dict(no_fuse=1)), ("0", dict(no_fuse=1))),     # on when present
    "TABLE_FORCE": (("1", dict(table_force=1)), ("", dict(table_force=1))),
    "TABLE_MIN_N": (("1", dict(table_min_n=1)), ("x", dict(table_min_n=0))),   # atoll of anything
    "TABLE_DIGITS": (("11", dict(table_digits=11)), ("33", {})),
    "REDUCE_WGS": (("64", dict(reduce_wgs=64)), ("-3", dict(reduce_wgs=1))),   # max(1, atoi)
    "PLANE_WGS": (("512", dict(plane_wgs=512)), ("x", dict(plane_wgs=1))),
    "REDUCE_PLANES": (("0", dict(reduce_planes=0)), ("2", {})),      # off only when set and atoi == 0
    "TWO_LEVEL": (("0", dict(two_level=0)), ("1", {})),
    "SORT_STAGE": (("x", dict(sort_stage=0)), ("1", {})),            # (atoi of a word is 0)
    "TWO_LEVEL_MIN_HI": (("2", dict(two_level_min_hi=2)), ("x", dict(two_level_min_hi=0))),   # atoi
    "ACC_WAVES": (("5", dict(acc_waves=5)), ("6", {})),              # 5 when atoi == 5, else 4
    "FINISH_LANE_LOG": (("0", dict(finish_lane_from=1)), ("x", dict(finish_lane_from=1))),    # 1 << atoi
}


def parsed(exe, knobs):
    (line,) = ask(exe, "knobs", knobs=knobs)
    return {k: int(v) for k, v in (kv.split("=") for kv in line.split())}


def test_every_parsing_rule(exe):
    assert {"H2_MSM_" + k for k in RULES} == set(mc.KNOBS) and len(RULES) == 20
    assert parsed(exe, {}) == DEFAULTS
    for name, cases in RULES.items():
        for value, changed in cases:
            assert parsed(exe, {"H2_MSM_" + name: value}) == dict(DEFAULTS, **changed), (name, value)

