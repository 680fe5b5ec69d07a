"""The rows of tests/test_gpu_msm_plans.py: what is run, what each row has to show, and the references it is compared with.

Nothing here needs a GPU.  A row is one call of h2_dev_msm, h2_dev_msm_batch or h2_dev_msm_batch_ex; `expect` names the values
of its launch record (h2_msm_last_launches) the row exists for and `classes` the scratch-derived classes (scratch_classes) it
has to populate.  Three references, none of which shares code with another:
  * the oracle's best_multiexp (every row, by the worker);
  * int_msm: sum s_i P_i in Python integers, affine arithmetic over F_q and double-and-add (rows of n <= 256);
  * recode: the signed digits of every scalar by the rule k_digits documents, as (bucket, reference | sign) pairs, against
    the sorted list the device left in the scratch (single-launch rows of n <= 2^15).
"""
import collections
import ctypes
import json
import os
import random

import numpy as np

from h2util import Q_MOD, R_MOD

FORMS = ("windowed", "table", "fused")             # H2_MSM_FORM_*
PARTS = ("2048", "16384", "two_level")             # H2_MSM_PART_*
FINISH = ("quads", "lanes")                        # H2_MSM_FINISH_*
REDUCE = ("groups", "planes")                      # H2_MSM_REDUCE_*
L_ENUM_COUNTS = {"H2_MSM_FORM_COUNT": 3, "H2_MSM_PART_COUNT": 3, "H2_MSM_FINISH_COUNT": 2, "H2_MSM_REDUCE_COUNT": 2}

FINISH_SERIAL, MID_MAX, HEAVY_SPLIT, SKEW_ROUNDS = 32, 512, 64, 4   # csrc/msm_plan.hpp, csrc/msm_kernels.hip
SIGN_BIT, BLOCK_INDEX0, BLOCK_ROWS, NO_PARTITION = 0x80000000, 0x40000000, 256, 0xFFFFFFFF
HOT_SAMPLES, HOT_MIN = 64, 16
SORT_CHECK_MAX_N = 1 << 15   # (2^13 would do for the digits; the skewed sort needs 2^15 rows to happen at all)
INT_CHECK_MAX_N = 256

_U32 = ("form max_bits c wfull W Wt Wk R range_shift cols Wc nb nbt lo_bits hi_bits np log_s qm RG planes chunks plane_seg "
        "plane_l two_level a_bits hot_on block_sums partition hot_partitioned stage_cap skew_threshold hot_partition finish "
        "acc_waves reduce").split()
_U64 = "hot_mask n entries scratch off_keys off_sorted off_pbase off_starts off_heavy off_buckets total".split()


class LaunchInfo(ctypes.Structure):
    """h2_msm_launch_info (include/halo2_hip.h)"""
    _fields_ = [(k, ctypes.c_uint32) for k in _U32] + [(k, ctypes.c_uint64) for k in _U64]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


def last_launches(L):
    """the records of this thread's last MSM call, as dicts"""
    count = L.h2_msm_last_launches(None, 0)
    buf = (LaunchInfo * max(count, 1))()
    assert L.h2_msm_last_launches(ctypes.addressof(buf), count) == count
    return [buf[i].as_dict() for i in range(count)]


RECORD_FIELDS = [k for k in _U32 + _U64 if k != "scratch"]   # what of a record is a function of the call's inputs
GOLDEN_RECORDS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "msm_launch_records.json")
_GOLDEN = {}


def golden_records():
    """tests/golden/msm_launch_records.json (golden/gen_msm_launch_records.py, recorded on an MI355X):
    (child's name or None, row name) -> the row's inputs, knobs and launch records"""
    if not _GOLDEN:
        with open(GOLDEN_RECORDS) as f:
            rows = json.load(f)["rows"]
        _GOLDEN.update({(e["child"], e["name"]): e for e in rows})
        assert len(_GOLDEN) == len(rows), "two recorded rows share a name"
    return _GOLDEN


def check_golden(child, row, recs):
    """the launches of one row are the recorded ones, field by field (all but the scratch address)"""
    want = golden_records()[(child, row.name)]["launches"]
    got = [{k: r[k] for k in RECORD_FIELDS} for r in recs]
    assert len(got) == len(want), "%d launches, %d recorded" % (len(got), len(want))
    for i, (g, w) in enumerate(zip(got, want)):
        diff = {k: (g[k], w[k]) for k in RECORD_FIELDS if g[k] != w[k]}
        assert not diff, "launch %d differs from the recorded one (got, recorded): %s" % (i, diff)


def branches(rec):
    """the launcher's choices one record shows, as names (what the coverage test counts)"""
    out = {"form:" + FORMS[rec["form"]], "part:" + PARTS[rec["partition"]], "finish:" + FINISH[rec["finish"]],
           "reduce:" + REDUCE[rec["reduce"]], "acc:%d" % rec["acc_waves"], "RG>1" if rec["RG"] > 1 else "RG=1",
           "stage_cap" if rec["stage_cap"] else "no_stage_cap"}
    if rec["R"] > 1:
        out.add("R>1")
    if rec["hot_on"]:
        out.add("hot:" + FORMS[rec["form"]])
    if rec["block_sums"]:
        out.add("block_sums")
    if rec["hot_partitioned"]:
        out.add("hot_partitioned")
    if rec["two_level"]:
        out.add("a_bits:%d" % rec["a_bits"])
    if rec["form"] == 1 and rec["reduce"] == 0:
        out.add("table_k_reduce")
    if rec["form"] == 2:
        out.add("fused_hot_slot" if rec["Wc"] > rec["W"] else "fused_no_hot_slot")
    if rec["lo_bits"] > 8:
        out.add("lo_grown:" + FORMS[rec["form"]])
    if rec["lo_bits"] < 8 and rec["lo_bits"] == rec["c"] - 1:
        out.add("lo=c-1")
    return out


# every value of the record's enumerations and every extra that default knobs reach within the sizes of this module
# (n <= 2^17); what they do not reach is listed, with the arithmetic, in test_gpu_msm_plans.py's docstring
DEFAULT_BRANCHES = {
    "form:windowed", "form:table", "form:fused", "part:2048", "part:two_level", "finish:quads", "reduce:groups", "reduce:planes",
    "acc:4", "RG=1", "RG>1", "stage_cap", "no_stage_cap", "R>1", "hot:windowed", "hot:table", "hot:fused", "block_sums",
    "hot_partitioned", "fused_hot_slot", "fused_no_hot_slot", "lo=c-1",
}
DEFAULT_CLASSES = {"skewed", "skew_fallback", "staged", "serial", "mid", "heavy", "heavy_capped", "empty_run"}
KNOB_ONLY_BRANCHES = {"part:16384", "finish:lanes", "acc:5", "table_k_reduce", "lo_grown:table", "lo_grown:fused"}

Row = collections.namedtuple("Row", "name kind n bits dist digits table_n lo expect classes env")


def row(name, n, bits, dist, kind="single", digits=0, table_n=None, lo=0, expect=None, classes=(), env=None):
    """dist: a builder's name (single) or a list of them, one per column (batch, batch_ex); digits: the base table the row
    runs over (0: none) of table_n >= lo + n points, the row's bases starting at point `lo`"""
    return Row(name, kind, n, bits, dist, digits, table_n or (n if digits else None), lo, dict(expect or {}), frozenset(classes),
               dict(env or {}))


WINDOWED_ROWS = [
    row("w n=64 1 bit", 64, 1, "uniform", expect={"form": "windowed", "c": 2, "W": 1, "nb": 2, "lo_bits": 1, "np": 1, "RG>1": False}),
    row("w n=64 8 bits", 64, 8, "uniform", expect={"form": "windowed", "c": 5, "W": 2, "nb": 16, "lo_bits": 4, "np": 2}),
    row("w n=64 254 bits", 64, 254, "uniform", expect={"form": "windowed", "c": 4, "W": 64, "nb": 8, "lo_bits": 3, "np": 64}),
    row("w n=64 254 bits {0,1,r-1}", 64, 254, "zero_one_minus_one", expect={"form": "windowed", "W": 64}),
    row("w n=64 254 bits digit extremes", 64, 254, "digit_extremes", expect={"form": "windowed", "W": 64, "hot_on": 0}),
    row("w n=1000 254 bits", 1000, 254, "uniform", expect={"form": "windowed", "c": 7, "W": 37, "partition": "2048", "finish": "quads",
                                                           "reduce": "groups", "acc_waves": 4, "staged": False}, classes={"serial"}),
    row("w n=1000 digit extremes", 1000, 254, "digit_extremes", expect={"form": "windowed", "c": 7, "hot_on": 0}),
    row("w n=1000 sparse", 1000, 254, "sparse", expect={"form": "windowed", "hot_on": 0}, classes={"empty_run"}),
    row("w n=4096 254 bits", 4096, 254, "uniform", expect={"form": "windowed", "c": 9, "W": 29, "hi_bits": 0, "hot_on": 0}),
    row("w n=8192 64 bits", 8192, 64, "uniform", expect={"form": "windowed", "c": 11, "W": 6, "hi_bits": 2, "RG>1": True, "RG": 2}),
    row("w n=2^15 1 bit", 1 << 15, 1, "uniform", expect={"form": "windowed", "R>1": True, "R": 16, "W": 1}),
    row("w n=2^15 8 bits", 1 << 15, 8, "uniform", expect={"form": "windowed", "R>1": True, "R": 16, "W": 1}),
    row("w n=2^15 16 bits", 1 << 15, 16, "uniform", expect={"form": "windowed", "R>1": True, "R": 16, "W": 2}),
    row("w n=2^15+4321 8 bits", (1 << 15) + 4321, 8, "uniform", expect={"form": "windowed", "R>1": True, "R": 10}),
    row("w n=2^15 254 bits", 1 << 15, 254, "uniform", expect={"form": "windowed", "W": 22, "R>1": False, "RG>1": True}),
    row("w n=2^15 three values", 1 << 15, 254, "three", expect={"form": "windowed", "W": 22}, classes={"skewed", "heavy"}),
    row("w n=2^15 five values", 1 << 15, 254, "five", expect={"form": "windowed", "W": 22, "hot_on": 0},
        classes={"skewed", "skew_fallback", "heavy"}),
    row("w n=4096 one value", 4096, 254, "one", expect={"form": "windowed", "hot_on": 1, "log_s": 3, "block_sums": 0}),
    row("w n=4088 one value", 4088, 254, "one", expect={"form": "windowed", "hot_on": 1, "log_s": 3}, classes={"mid"}),
    row("w n=4104 one value", 4104, 254, "one", expect={"form": "windowed", "hot_on": 1, "log_s": 3}, classes={"heavy"}),
    row("w n=4096 7/8 one value", 4096, 254, "dominant", expect={"form": "windowed", "hot_on": 1}, classes={"mid"}),
    # heavy_parts = min(ceil(partials / 256), HEAVY_SPLIT): the cap changes something from 256 * 64 + 1 partials on, i.e. one
    # slice more than 2^17 rows of one value fill at log_s = 3 (2^17 rows are 16384 partials: 64 parts with or without it)
    row("w n=2^17+8 one value", (1 << 17) + 8, 254, "one", expect={"form": "windowed", "hot_on": 1, "log_s": 3}, classes={"heavy_capped"}),
    row("w n=2^17 7/8 one value", 1 << 17, 254, "dominant", expect={"form": "windowed", "hot_on": 1, "log_s": 3}, classes={"heavy"}),
    # one or two windows: plan_decide switches the dominant window off though every sample agrees (16 bits are three windows
    # of 6 bits up to n = 1365 and two of 9 from there on)
    row("w n=2048 16 bits one value", 2048, 16, "one", expect={"form": "windowed", "W": 2, "hot_on": 0}, classes={"mid"}),
    row("ex 6 columns n=1000", 1000, 254, ["uniform", "one", "sparse", "dominant", "five", "uniform"], kind="batch_ex",
        expect={"form": "windowed", "launches": 6, "scratch_slices": 2}),
]

# Over a table.  Whether a call takes the table form is table_pays' decision: D n + 10 * 2^(c-1) against the windowed
# W n + 10 Wt nb.  A table of 16 digits (2^15 buckets) pays from n = 2^15, one of 15 digits (2^16 buckets: the two-level
# partition) too; with a dominant value only an eighth of the rows count and 15 digits pay from 2^17.
TABLE_ROWS = [
    row("t n=200 D=32", 200, 254, "uniform", digits=32, expect={"form": "table", "c": 8, "nb": 128, "lo_bits": 7, "hi_bits": 0, "np": 1,
                                                                "reduce": "planes", "staged": False}),
    row("t n=512 D=32", 512, 254, "uniform", digits=32, expect={"form": "table", "c": 8, "np": 1, "staged": True, "partition": "2048"},
        classes={"staged"}),
    row("t n=512 D=32 7/8 one value", 512, 254, "dominant", digits=32, expect={"form": "table", "hot_on": 1, "block_sums": 1, "staged": True},
        classes={"staged"}),
    row("t n=512 D=32 64 bits", 512, 64, "uniform", digits=32, expect={"form": "table", "W": 9}),
    row("t n=512 D=32 digit extremes", 512, 254, "digit_extremes", digits=32, expect={"form": "table", "hot_on": 0}),
    row("t n=900 D=27", 900, 254, "uniform", digits=27, expect={"form": "table", "c": 10, "hi_bits": 1, "staged": True}, classes={"staged"}),
    row("t n=1000 D=32", 1000, 254, "uniform", digits=32, expect={"form": "table", "staged": False}),
    row("t n=1000 of 2000 D=32 off a block", 1000, 254, "dominant", digits=32, table_n=2000, lo=1000,
        expect={"form": "table", "hot_on": 1, "block_sums": 0}),
    row("t n=8192 D=20", 8192, 254, "uniform", digits=20, expect={"form": "table", "c": 13, "hi_bits": 4, "staged": True, "reduce": "planes"},
        classes={"staged"}),
    row("t n=2^15 D=16", 1 << 15, 254, "uniform", digits=16, expect={"form": "table", "c": 16, "hi_bits": 7, "partition": "2048", "planes": 14,
                                                                     "RG": 64}),
    # a partition is skewed above 4x the average: a bucket that holds all n rows of one digit needs np > 4 D
    row("t n=2^15 D=16 three values", 1 << 15, 254, "three", digits=16, expect={"form": "table"}, classes={"skewed"}),
    row("t n=2^15 D=16 five values", 1 << 15, 254, "five", digits=16, expect={"form": "table", "hot_on": 0}, classes={"skewed", "skew_fallback"}),
    row("t n=2^15 D=15", 1 << 15, 254, "uniform", digits=15, expect={"form": "table", "c": 17, "hi_bits": 8, "partition": "two_level",
                                                                     "a_bits": 4, "finish": "quads"}),
    row("t n=2^17 D=15 7/8 one value", 1 << 17, 254, "dominant", digits=15,
        expect={"form": "table", "partition": "two_level", "hot_on": 1, "hot_partitioned": 1, "block_sums": 1}),
]

_SEVEN = ["uniform", "one", "dominant", "sparse", "three", "five", "zero_one_minus_one"]
FUSED_ROWS = [
    row("f 7 x n=256", 256, 254, _SEVEN, kind="batch", expect={"form": "fused", "cols": 7, "Wc": 44, "hot_on": 1}),
    row("f 7 x n=5000", 5000, 254, _SEVEN, kind="batch", expect={"form": "fused", "cols": 7, "Wc": 30, "hot_on": 1}),
    row("f 66 x n=300", 300, 254, ["dominant" if j in (0, 63, 64, 65) else "uniform" for j in range(66)], kind="batch",
        expect={"form": "fused", "launches": 2, "cols": 64, "hot_mask_bit": 63}),
    # a bound of one or two windows is fused only when a column still spreads over 16 partitions (fused_group_limit):
    # W << (c - 1 - 8) >= 16 with W = 2 is c = 12, i.e. 24 bits in two windows, which the cost model picks over three
    # windows of 8 bits from 2 (n + 3 * 2^11) < 3 (n + 3 * 2^7), n > 11136
    row("f 5 x n=12288 23 bits", 12288, 23, ["uniform"] * 4 + ["one"], kind="batch",
        expect={"form": "fused", "cols": 5, "W": 2, "Wc": 2, "hot_on": 0}),
]


# ---------------------------------------------------------------- knob children (one process each; see the test module)
_FORCE = {"H2_MSM_TABLE_FORCE": "1"}
KNOBS = ("H2_MSM_ACC_WAVES", "H2_MSM_TWO_LEVEL", "H2_MSM_REDUCE_PLANES", "H2_MSM_SORT_STAGE", "H2_MSM_FINISH_LANE_LOG", "H2_MSM_SLICE_LOG",
         "H2_MSM_REDUCE_QM", "H2_MSM_WINDOW", "H2_MSM_TABLE_LO", "H2_MSM_LANES", "H2_MSM_NO_FUSE", "H2_MSM_TWO_LEVEL_MIN_HI", "H2_MSM_NO_HOT",
         "H2_MSM_TABLE_FORCE", "H2_MSM_TABLE_MIN_N", "H2_MSM_NO_TABLE", "H2_MSM_TABLE_DIGITS", "H2_MSM_REDUCE_WGS", "H2_MSM_PLANE_WGS",
         "H2_MSM_FUSE_LOG")


def _t(n, D, dist="uniform", bits=254, **kw):
    return row("t n=%d D=%d %s %d bits" % (n, D, dist, bits), n, bits, dist, digits=D, **kw)


_W4096 = row("w n=4096 254 bits", 4096, 254, "uniform", expect={"form": "windowed"})
_W8192 = row("w n=8192 64 bits", 8192, 64, "uniform", expect={"form": "windowed", "RG>1": True})
_F7 = row("f 7 x n=256", 256, 254, _SEVEN, kind="batch", expect={"form": "fused"})
_EX6 = row("ex 6 columns n=1000, four lanes", 1000, 254, ["uniform", "one", "sparse", "dominant", "five", "uniform"], kind="batch_ex",
           expect={"form": "windowed", "launches": 6, "scratch_slices": 4})

# (name, environment, rows, the branches the child has to report)
CHILDREN = [
    # the wide tables at a size that keeps the rows small: 2^19 .. 2^23 buckets pay by themselves only from 2^20 rows on
    ("table_force", _FORCE, [
        _t(4096, 16, expect={"form": "table", "c": 16, "hi_bits": 7, "partition": "2048", "planes": 14, "RG": 64}),
        _t(4096, 13, expect={"form": "table", "c": 20, "hi_bits": 11, "partition": "two_level", "a_bits": 5, "finish": "lanes"}),
        _t(4096, 13, "dominant", expect={"form": "table", "partition": "two_level", "hot_on": 1, "hot_partitioned": 1, "block_sums": 1}),
        _t(4096, 13, bits=64, expect={"form": "table", "W": 4}),
        _t(4096, 12, expect={"form": "table", "c": 22, "hi_bits": 13}),
        _t(4096, 11, expect={"form": "table", "c": 24, "lo_bits": 10, "hi_bits": 13, "finish": "lanes"}),
        _t(8192, 13, "three", expect={"form": "table"}, classes={"skewed"}),
        _t(8192, 13, "five", expect={"form": "table", "hot_on": 0}, classes={"skewed", "skew_fallback"}),
        row("t n=1000 of 5096 D=13 off a block", 1000, 254, "dominant", digits=13, table_n=5096, lo=1000,
            expect={"form": "table", "hot_on": 1, "block_sums": 0, "hot_partitioned": 1}),
    ], {"part:two_level", "finish:lanes", "lo_grown:table", "hot_partitioned", "a_bits:5"}),
    ("acc_waves_5", {"H2_MSM_ACC_WAVES": "5"}, [_W4096, _t(512, 32, expect={"form": "table"}), _F7,
                                                row("w n=4104 one value", 4104, 254, "one", classes={"heavy"})], {"acc:5"}),
    ("two_level_0", dict(_FORCE, H2_MSM_TWO_LEVEL="0"), [
        _t(4096, 13, expect={"partition": "16384", "two_level": 0}), _t(4096, 12, expect={"partition": "16384"}),
        _t(4096, 13, "dominant", expect={"partition": "16384", "hot_on": 1, "hot_partitioned": 0})], {"part:16384"}),
    ("reduce_planes_0", dict(_FORCE, H2_MSM_REDUCE_PLANES="0"), [
        _t(4096, 16, expect={"reduce": "groups", "RG": 64}), _t(4096, 11, expect={"reduce": "groups", "RG": 1024}),
        _t(512, 32, "dominant", expect={"reduce": "groups", "RG": 1, "hot_on": 1})], {"table_k_reduce", "RG>1"}),
    ("sort_stage_0", {"H2_MSM_SORT_STAGE": "0"}, [_t(512, 32, expect={"staged": False}), _t(900, 27, expect={"staged": False}),
                                                  _t(8192, 20, expect={"staged": False})], {"no_stage_cap"}),
    ("finish_lane_log_0", {"H2_MSM_FINISH_LANE_LOG": "0"}, [
        row("w n=1000 254 bits", 1000, 254, "uniform", expect={"finish": "lanes"}),
        row("w n=4104 one value", 4104, 254, "one", expect={"finish": "lanes"}, classes={"heavy"}),
        row("w n=4088 one value", 4088, 254, "one", expect={"finish": "lanes"}, classes={"mid"}),
        _t(512, 32, expect={"finish": "lanes"}), _F7], {"finish:lanes"}),
    ("slice_log_1", {"H2_MSM_SLICE_LOG": "1", "H2_MSM_NO_HOT": "1"}, [
        row("w n=2^15+2 one value, no dominant window", (1 << 15) + 2, 254, "one", expect={"log_s": 1, "hot_on": 0},
            classes={"heavy_capped"})],
     {"form:windowed"}),
    ("slice_log_10", {"H2_MSM_SLICE_LOG": "10"}, [
        row("w n=4096 254 bits", 4096, 254, "uniform", expect={"log_s": 10}),
        row("w n=1000 sparse", 1000, 254, "sparse", expect={"log_s": 10}, classes={"empty_run"}),
        _t(512, 32, expect={"log_s": 10})], {"form:windowed", "form:table"}),
    ("reduce_qm_3", {"H2_MSM_REDUCE_QM": "3"}, [
        row("w n=4096 254 bits", 4096, 254, "uniform", expect={"qm": 3}), _W8192,
        _t(512, 32, expect={"qm": 3, "reduce": "groups"}), _t(8192, 20, expect={"qm": 3, "reduce": "groups", "RG>1": True})],
     {"table_k_reduce"}),
    ("reduce_qm_64", {"H2_MSM_REDUCE_QM": "64"}, [
        row("w n=8192 64 bits", 8192, 64, "uniform", expect={"qm": 64, "RG>1": False}),
        _t(8192, 20, expect={"qm": 64, "reduce": "planes"}), _F7], {"reduce:planes"}),
    ("window_17", {"H2_MSM_WINDOW": "17"}, [
        row("f 5 x n=4096", 4096, 254, ["uniform", "dominant", "sparse", "three", "uniform"], kind="batch",
            expect={"form": "fused", "Wt": 80, "lo_bits": 9}),
        row("w n=4096 254 bits", 4096, 254, "uniform", expect={"c": 17, "W": 15, "RG>1": True})], {"lo_grown:fused"}),
    ("table_lo_4", {"H2_MSM_TABLE_LO": "4"}, [
        _t(512, 32, expect={"lo_bits": 4, "hi_bits": 3}),
        _t(8192, 20, expect={"lo_bits": 4, "hi_bits": 8, "partition": "two_level", "a_bits": 4}),
        _t(8192, 20, "dominant", expect={"lo_bits": 4, "hot_on": 1, "hot_partitioned": 1})], {"part:two_level"}),
    ("table_lo_12", {"H2_MSM_TABLE_LO": "12"}, [
        _t(8192, 20, expect={"lo_bits": 12, "hi_bits": 0}), _t(8192, 20, "five", expect={"lo_bits": 12})], {"lo_grown:table"}),
    ("lanes_4", {"H2_MSM_LANES": "4"}, [_EX6], {"form:windowed"}),
    ("no_fuse", {"H2_MSM_NO_FUSE": "1"}, [
        row("7 x n=256, not fused", 256, 254, _SEVEN, kind="batch", expect={"form": "windowed", "launches": 7})], {"form:windowed"}),
    ("two_level_min_hi_2", {"H2_MSM_TWO_LEVEL_MIN_HI": "2"}, [
        _t(8192, 20, expect={"partition": "two_level", "hi_bits": 4, "a_bits": 2}),
        _t(8192, 20, "dominant", expect={"partition": "two_level", "a_bits": 2, "hot_on": 1, "hot_partitioned": 1})], {"a_bits:2"}),
]


# ---------------------------------------------------------------- scalars and points
def digit_widths(bits, W=None, digits=0):
    """(widths of the windows, low to high): the balanced cut of bits + 1 bits into W windows, or of 255 bits into a
    table's `digits`"""
    T, W = (255, digits) if digits else (bits + 1, W)
    base, rem = divmod(T, W)
    return [base + 1 if w < (rem or W) and rem else base for w in range(W)]


def build_scalars(dist, n, bits, seed, widths):
    """canonical scalars (Python integers below min(2^bits, r)) of the named distribution; rows 10 / 11 and 12 / 13 agree"""
    rnd = random.Random(seed)
    bound = min(1 << bits, R_MOD)

    def rand():
        return rnd.randrange(1, bound)

    hot = rand()
    if dist == "uniform":
        vals = [rand() for _ in range(n)]
    elif dist == "one":
        vals = [hot] * n
    elif dist == "dominant":
        # 7/8 one value: whole 256-row blocks of it and ragged runs (a hole every 1301 rows in the second half)
        vals = [hot if i >= n // 8 and not (i >= n // 2 and i % 1301 == 1300) else rand() for i in range(n)]
    elif dist == "sparse":
        vals = [rand() if i % 16 == 3 else 0 for i in range(n)]
    elif dist in ("three", "five"):
        # neighbours: they share every digit but the lowest, whose buckets share one sort partition
        k = 3 if dist == "three" else 5
        base = min(hot, bound - k)
        vals = [base + (i * 7 + i // 64) % k for i in range(n)]
    elif dist == "zero_one_minus_one":
        vals = [(0, 1, bound - 1)[(i + i // 5) % 3] for i in range(n)]
    elif dist == "digit_extremes":
        # every window's digit (with the carry that reaches it) is exactly 2^(cw-1), the largest positive digit, or
        # 2^(cw-1) + 1, the first negative one, which carries; the top window holds nothing but the carry
        vals = []
        for i in range(n):
            v, off, carry = 0, 0, 0
            for cw in widths[:-1]:
                negative = (i >> 0) & 1 if i < 2 else rnd.randrange(2)
                raw = (1 << (cw - 1)) + negative - carry
                if raw >= 1 << cw:
                    raw, negative = raw - 1, 0
                v |= raw << off
                off += cw
                carry = negative
            vals.append(v)
    else:
        raise AssertionError(dist)
    if n > 13:
        vals[11], vals[13] = vals[10], vals[12]
    assert all(0 <= v < bound for v in vals), dist
    return vals


def build_points(oracle, seed, n):
    """random points; 5 is the identity, 10 and 11 are equal, 13 = -12 (with equal scalars: P + P and P - P in one bucket)"""
    pts = oracle.random_g1(seed, n)
    if n > 13:
        pts[5] = 0
        pts[11] = pts[10]
        pts[13] = pts[12]
        y = sum(int(pts[12][4 + k]) << (64 * k) for k in range(4))      # Montgomery form: -y R = q - y R
        pts[13][4:] = [((Q_MOD - y) >> (64 * k)) & (2**64 - 1) for k in range(4)]
    return pts


# ---------------------------------------------------------------- reference: Python integers
def _add(P, Q):
    if P is None:
        return Q
    if Q is None:
        return P
    (x1, y1), (x2, y2) = P, Q
    if x1 == x2:
        if (y1 + y2) % Q_MOD == 0:
            return None
        lam = 3 * x1 * x1 * pow(2 * y1, -1, Q_MOD) % Q_MOD
    else:
        lam = (y2 - y1) * pow(x2 - x1, -1, Q_MOD) % Q_MOD
    x3 = (lam * lam - x1 - x2) % Q_MOD
    return x3, (lam * (x1 - x3) - y1) % Q_MOD


def int_msm(vals, points):
    """sum s_i P_i: points as (x, y) integers ((0, 0): the identity); rows of one scalar are added first, then one
    double-and-add over the canonical scalar per distinct value"""
    groups = {}
    for s, p in zip(vals, points):
        if s:
            groups[s] = _add(groups.get(s), None if p == (0, 0) else p)
    total = None
    for s, P in groups.items():
        acc = None
        for bit in range(s.bit_length() - 1, -1, -1):
            acc = _add(acc, acc)
            if (s >> bit) & 1:
                acc = _add(acc, P)
        total = _add(total, acc)
    return total or (0, 0)


# ---------------------------------------------------------------- reference: the digits and where they go
def sampled_hot(vals):
    """detect_hot over k_sample's 64 rows: the most frequent non-zero sampled value when it fills >= 16 of them"""
    n = len(vals)
    s = [vals[(t * 0x9E3779B1 + 0x7F4A7C15) % n] for t in range(HOT_SAMPLES)]
    best, value = 0, None
    for v in s:
        if v and s.count(v) > best:
            best, value = s.count(v), v
    return value if best >= HOT_MIN else None


def recode(columns, rec, table_n=0):
    """the (global bucket, reference | sign) pairs k_digits + the sort leave for these columns (one: single MSM) under
    record `rec`, as one sorted array of bucket << 32 | entry"""
    c, wfull, W, nb, R = rec["c"], rec["wfull"], rec["W"], rec["nb"], rec["R"]
    table, fused = rec["form"] == 1, rec["form"] == 2
    mask = (1 << rec["max_bits"]) - 1
    out = []
    for j, vals in enumerate(columns):
        n = len(vals)
        hot = None
        if (rec["hot_mask"] >> j) & 1 if fused else rec["hot_on"]:
            hot = sampled_hot(vals)
            assert hot is not None, "the record has a dominant value where the 64 samples show none"
        w0 = j * rec["Wc"] if fused else 0
        hot_bucket = (nb if table else (w0 + R * W) * nb)
        whole = set()
        if hot is not None and rec["block_sums"]:
            whole = {k for k in range(n // BLOCK_ROWS) if all(v == hot for v in vals[k * BLOCK_ROWS:(k + 1) * BLOCK_ROWS])}
        for i, full in enumerate(vals):
            if hot is not None and full == hot:
                if i // BLOCK_ROWS in whole:
                    if i % BLOCK_ROWS == 0:
                        out.append(hot_bucket << 32 | (BLOCK_INDEX0 + i // BLOCK_ROWS))
                else:
                    out.append(hot_bucket << 32 | i)
                continue
            v, carry = full & mask, 0
            vw0 = w0 + (i >> rec["range_shift"]) * W
            for w in range(W):
                cw = c - (1 if w >= wfull else 0)
                raw = (v & ((1 << cw) - 1)) + carry
                v >>= cw
                neg = raw > 1 << (cw - 1)
                mag = (1 << cw) - raw if neg else raw
                carry = 1 if neg else 0
                if mag:
                    bucket = (0 if table else (vw0 + w) * nb) + mag - 1
                    out.append(bucket << 32 | ((w * table_n if table else 0) + i) | (SIGN_BIT if neg else 0))
            assert v == 0 and carry == 0, "the bound leaves a carry out of the top window"
    return np.sort(np.array(out, dtype=np.uint64))


def check_sort(rec, starts, sorted_entries, expected):
    """starts[0 .. nbt], sorted[0 .. starts[nbt]) of the device against recode()'s pairs"""
    nbt = rec["nbt"]
    starts = starts.astype(np.int64)
    assert (np.diff(starts) >= 0).all(), "starts decreases at bucket %d" % int(np.nonzero(np.diff(starts) < 0)[0][0])
    assert starts[0] == 0, "starts[0] = %d" % starts[0]
    assert starts[nbt] == len(expected), "starts[nbt] = %d, the scalars have %d non-zero digits" % (starts[nbt], len(expected))
    want_hist = np.bincount((expected >> np.uint64(32)).astype(np.int64), minlength=nbt)
    got_hist = np.diff(starts)
    bad = np.nonzero(want_hist != got_hist)[0]
    assert len(bad) == 0, "bucket %d holds %d entries, the digits put %d there (%d buckets differ)" % (
        bad[0], got_hist[bad[0]], want_hist[bad[0]], len(bad))
    bucket_of = np.repeat(np.arange(nbt, dtype=np.uint64), got_hist)
    got = np.sort(bucket_of << np.uint64(32) | sorted_entries.astype(np.uint64))
    bad = np.nonzero(got != expected)[0]
    if len(bad):
        b = int(got[bad[0]] >> np.uint64(32))
        raise AssertionError("bucket %d: the device has entry 0x%08x, the digits give 0x%08x (%d entries differ)" % (
            b, int(got[bad[0]]) & 0xFFFFFFFF, int(expected[bad[0]]) & 0xFFFFFFFF, len(bad)))


# ---------------------------------------------------------------- evidence from the scratch
def scratch_classes(rec, pbase, starts, heavy_count):
    """what the partitions and buckets of one launch populated (pbase[0 .. np], starts[0 .. nbt], heavy[0]); asserts the
    heavy list's length on the way"""
    out = set()
    np_, nbt, log_s, hi = rec["np"], rec["nbt"], rec["log_s"], rec["hi_bits"]
    sizes = np.diff(pbase.astype(np.int64))
    p = np.arange(np_)
    if rec["form"] == 2:
        w = p >> hi
        is_hot = ((p & ((1 << hi) - 1)) == 0) & (w % rec["Wc"] == rec["Wc"] - 1) & (rec["Wc"] > rec["W"])
        is_hot &= np.array([(rec["hot_mask"] >> int(col)) & 1 for col in w // rec["Wc"]], dtype=bool)
    else:
        is_hot = p == rec["hot_partition"]
    skewed = (sizes > rec["skew_threshold"]) & ~is_hot
    staged = (sizes > 0) & (sizes <= rec["stage_cap"]) & ~skewed & ~is_hot
    if skewed.any():
        out.add("skewed")
    if staged.any():
        out.add("staged")
    s = starts.astype(np.int64)
    e0, e1 = s[:nbt], s[1:nbt + 1]
    filled = e1 > e0
    partials = np.where(filled, ((e1 - 1) >> log_s) - (e0 >> log_s) + 1, 0)
    nbins = 1 << rec["lo_bits"]
    for q in np.nonzero(skewed)[0]:   # more distinct bins than SKEW_ROUNDS serves with one atomic each
        # partition q's buckets: window q >> hi, bins (q & mask) << lo ..; over a table the extra partition follows window 0
        first = (int(q) >> hi) * rec["nb"] + ((int(q) & ((1 << hi) - 1)) << rec["lo_bits"])
        if np.count_nonzero(filled[first:first + nbins]) > SKEW_ROUNDS:
            out.add("skew_fallback")
    assert heavy_count == np.count_nonzero(partials > FINISH_SERIAL), "heavy[0] = %d, %d buckets have more than %d partials" % (
        heavy_count, np.count_nonzero(partials > FINISH_SERIAL), FINISH_SERIAL)
    if ((partials > 0) & (partials <= FINISH_SERIAL)).any():
        out.add("serial")
    if ((partials > FINISH_SERIAL) & (partials <= MID_MAX)).any():
        out.add("mid")
    if ((partials > MID_MAX) & (partials <= 256 * HEAVY_SPLIT)).any():
        out.add("heavy")
    if (partials > 256 * HEAVY_SPLIT).any():     # ceil(partials / 256) > HEAVY_SPLIT: the cap of heavy_parts decides
        out.add("heavy_capped")
    # a bucket that ends inside a slice with an empty bucket behind it and entries after that: k_acc_slice's bisection
    total = s[nbt]
    ends_inside = filled & (e1 % (1 << log_s) != 0) & (e1 < total)
    next_empty = np.append(~filled[1:], False)
    if (ends_inside & next_empty).any():
        out.add("empty_run")
    return out
