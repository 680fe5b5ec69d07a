"""evaluate_h programs with an explicit SHAPE, for the branches of the generator (csrc/evalh_gen.cpp), of the plan cache
(csrc/evalh_plan.hip) and of the interpreter (csrc/evalh_interp.hip) that depend on how big a circuit is and not on its values.

tests/evalh_cases.random_case always has 2 + 3 + 1 columns, 5 rotations, 6 constants, 5 permutation columns in chunks of 2 and
at most 80 calculations: one stage, arguments read field by field, one compile.  `shaped_case` keeps the column DATA random
(oracle.random_fr) and puts the structure under control:
  * a gate is  selector (a fixed column) x a chain of ADD / SUB / MUL steps over `gate_width` (column, rotation) operands,
    then `consts_per_gate` steps with a constant; gate g takes operands g * gate_width ... of the advice + instance columns in
    turn, so the set of distinct columns the first n gates read is known in advance (`gate_columns`);
  * `wide_term` appends ONE value part that reads that many distinct columns (a term cannot be cut into stages);
  * the permutation argument covers the first `n_perm` of advice, fixed, instance columns in `chunk_len`-column sets.

SHAPES names one case per branch, each with the CLAIM of what it enters.  Every count below is derived from the generator's
structural constants; tests/test_evalh_shape_cases_host.py reads those constants back from evalh_gen.hpp / evalh_gen.cpp and
checks every claim through h2_evalh_source / h2_evalh_stage_args / h2_evalh_compile, so a retune fails there instead of
quietly moving a boundary away from its case."""
import random

import numpy as np

from evalh_cases import DELTA, ROOT, ZETA
from h2util import R_MOD, fr_mont, to_mont
from halo2_gpu_specific_amd import evaluation as ev

# ---- the structural constants (read back from the sources by the host test)
ARGS_FIXED_BYTES = 48        # evalh_gen.hpp: the fixed part of a stage's argument block
SCALAR_BYTES, POINTER_BYTES = 32, 8
ARGS_CUT_BYTES = 3072        # evalh_gen.cpp generate(): a stage whose block has passed this takes no further term
ARGS_MAX_BYTES = 4096        # ... and a block past this cannot be launched: the generator refuses the program
LDS_ARGS_DWORDS = 320        # Options::lds_args: more dwords of scalars + pointers than this are read through LDS
MAX_REGS = 256               # Options::max_regs: a stage compiled to more registers is rebuilt
CACHE_LDS_BIT = 0x80000000   # compile(): the layout word of a cache file whose program was rebuilt with its arguments in LDS
BLINDING = 5


def block_bytes(n_scalars, n_cols):
    return ARGS_FIXED_BYTES + SCALAR_BYTES * max(n_scalars, 1) + POINTER_BYTES * max(n_cols, 1)


def cols_past(limit_bytes, n_scalars):
    """the smallest number of column pointers whose block, with `n_scalars` scalars, exceeds `limit_bytes`"""
    return (limit_bytes - ARGS_FIXED_BYTES - SCALAR_BYTES * max(n_scalars, 1)) // POINTER_BYTES + 1


def _walk(n_fixed, n_advice, n_instance, order):
    tables = {"a": [(ev.VS_ADVICE, i) for i in range(n_advice)], "f": [(ev.VS_FIXED, i) for i in range(n_fixed)],
              "i": [(ev.VS_INSTANCE, i) for i in range(n_instance)]}
    return [c for t in order for c in tables[t]]


def gate_columns(n_gates, gate_width, *, n_fixed, n_advice, n_instance):
    """the distinct (kind, index) columns gates 0 .. n_gates - 1 read: their selectors and operands"""
    pool = _walk(n_fixed, n_advice, n_instance, "ai")
    seen = {(ev.VS_FIXED, g % n_fixed) for g in range(n_gates)}
    seen |= {pool[(g * gate_width + j) % len(pool)] for g in range(n_gates) for j in range(gate_width)}
    return seen


def shaped_case(seed, k, extended_k, oracle, *, n_fixed=2, n_advice=3, n_instance=1, n_perm=0, chunk_len=2, n_gates=4, gate_width=3,
                n_constants=6, rotations=(0, 1, -1), lookup_sets=(), n_shuffles=0, n_value_parts=None, consts_per_gate=1,
                wide_term=0):
    """-> the keyword dict of ev.Builder().build, like evalh_cases.random_case"""
    assert rotations[0] == 0 and n_constants >= 4 and n_fixed >= 1 and n_advice >= 1 and (n_gates == 0 or gate_width >= 2)
    rng = random.Random(seed)
    size = 1 << extended_k
    serial = [0]

    def column():
        serial[0] += 1
        return oracle.random_fr(seed * 4096 + serial[0], size)

    fixed, advice, instance = ([column() for _ in range(n)] for n in (n_fixed, n_advice, n_instance))
    constants = to_mont([0, 1, 2, R_MOD - 1] + [rng.randrange(R_MOD) for _ in range(n_constants - 4)])
    pool = _walk(n_fixed, n_advice, n_instance, "ai")
    calcs, gate_out, next_const = [], [], 0
    inter = lambda: ev.vs(ev.VS_INTERMEDIATE, len(calcs) - 1)  # noqa: E731
    for g in range(n_gates):
        for j in range(gate_width):
            kind, index = pool[(g * gate_width + j) % len(pool)]
            operand = ev.vs(kind, index, (g + j) % len(rotations))
            if j == 0:
                first = operand
            else:
                calcs.append(ev.calc(rng.choice([ev.CALC_ADD, ev.CALC_SUB, ev.CALC_MUL]), first if j == 1 else inter(), operand))
        for c in range(consts_per_gate):
            index = next_const % n_constants
            next_const += 1
            # (0, 1, 2 and -1 are only ever added: a product by 0 would take the whole gate out of the program)
            calcs.append(ev.calc(ev.CALC_MUL if index >= 4 and c % 2 else ev.CALC_ADD, inter(), ev.vs(ev.VS_CONSTANT, index)))
        calcs.append(ev.calc(ev.CALC_MUL, ev.vs(ev.VS_FIXED, g % n_fixed, 0), inter()))
        gate_out.append(inter())
    value_parts = gate_out if n_value_parts is None else gate_out[:n_value_parts]
    assert n_value_parts is None or len(value_parts) == n_value_parts
    if wide_term:
        every = _walk(n_fixed, n_advice, n_instance, "aif")
        assert 2 <= wide_term <= len(every)
        for j in range(1, wide_term):
            op = ev.CALC_MUL if j % 16 == 0 else rng.choice([ev.CALC_ADD, ev.CALC_SUB])
            calcs.append(ev.calc(op, ev.vs(*every[0], 0) if j == 1 else inter(), ev.vs(*every[j], 0)))
        value_parts = value_parts + [inter()]
    n_calcs = len(calcs)

    def rand_vs():
        kind = rng.choice([ev.VS_CONSTANT, ev.VS_FIXED, ev.VS_ADVICE, ev.VS_INSTANCE if n_instance else ev.VS_ADVICE] +
                          [ev.VS_INTERMEDIATE] * (3 if n_calcs else 0))
        if kind == ev.VS_CONSTANT:
            return ev.vs(kind, rng.randrange(n_constants))
        if kind == ev.VS_INTERMEDIATE:
            return ev.vs(kind, rng.randrange(n_calcs))
        n = {ev.VS_FIXED: n_fixed, ev.VS_ADVICE: n_advice, ev.VS_INSTANCE: n_instance}[kind]
        return ev.vs(kind, rng.randrange(n), rng.randrange(len(rotations)))

    def rand_calc():
        op = rng.choice([ev.CALC_ADD, ev.CALC_SUB, ev.CALC_MUL, ev.CALC_MUL, ev.CALC_NEGATE, ev.CALC_LC_CHALLENGE, ev.CALC_LC_THETA,
                         ev.CALC_ADD_CHALLENGE, ev.CALC_STORE])
        return ev.calc(op, rand_vs(), rand_vs(), rng.choice([0, 1]), rng.choice([0, 1, 2, 3, 5]))

    lookups = [(rand_calc(), [rand_calc() for _ in range(s)], [rand_calc() for _ in range(s)]) for s in lookup_sets]
    shuffles = [(rand_calc(), rand_calc()) for _ in range(n_shuffles)]
    any_of = {ev.VS_ADVICE: ev.ANY_ADVICE, ev.VS_FIXED: ev.ANY_FIXED, ev.VS_INSTANCE: ev.ANY_INSTANCE}
    perm_columns = [(any_of[kind], index) for kind, index in _walk(n_fixed, n_advice, n_instance, "afi")[:n_perm]]
    assert len(perm_columns) == n_perm and chunk_len >= 1
    n_sets = (n_perm + chunk_len - 1) // chunk_len
    ch = {name: fr_mont(rng.randrange(R_MOD)) for name in ("y", "beta", "gamma", "theta")}
    return dict(k=k, extended_k=extended_k, blinding_factors=BLINDING, chunk_len=chunk_len, constants=constants,
                rotations=list(rotations), calculations=calcs, value_parts=value_parts, lookups=lookups, shuffles=shuffles,
                fixed=fixed, advice=advice, instance=instance, l0=column(), l_last=column(), l_active_row=column(),
                perm_z=[column() for _ in range(n_sets)], perm_columns=perm_columns, perm_sigma=[column() for _ in range(n_perm)],
                lookup_z=[column() for _ in range(sum(lookup_sets))], lookup_m=[column() for _ in lookup_sets],
                shuffle_z=[column() for _ in range(n_shuffles)], delta=fr_mont(DELTA), zeta=fr_mont(ZETA),
                extended_omega=fr_mont(pow(ROOT, 1 << (28 - extended_k), R_MOD)), **ch)


def column_names(kw):
    """host address -> name of every vector of a case ("advice[7]", "perm_z[0]", "l0"): what the pointers of a stage's
    argument block (h2_evalh_stage_args) are looked up in"""
    names = {}
    for table in ("fixed", "advice", "instance", "perm_z", "perm_sigma", "lookup_z", "lookup_m", "shuffle_z"):
        for i, col in enumerate(kw[table]):
            names[col.ctypes.data] = "%s[%d]" % (table, i)
    for single in ("l0", "l_last", "l_active_row"):
        names[kw[single].ctypes.data] = single
    return names


def layout(kw):
    """What the generator makes of a case under the options of the environment, one dict per stage, read from the two things a
    stage consists of: its source (h2_evalh_source) and the argument block it would receive (h2_evalh_stage_args).  [] when the
    generator refuses the program."""
    import re

    b = ev.Builder().build(**kw)
    names = column_names(kw)
    size = 1 << kw["extended_k"]
    values = np.zeros((size, 4), dtype=np.uint64)
    stages = []
    while True:
        try:
            src = ev.generated_source(b, len(stages))
        except Exception:                                   # "no such stage": past the last one (or a refused program)
            return stages
        block = ev.stage_args(b, len(stages), values.ctypes.data, 0, 0, 0, size)
        n_scalars = int(re.search(r"Fr sc\[(\d+)\];", src).group(1))
        n_cols = int(re.search(r"const Fr\* cols\[(\d+)\];", src).group(1))
        pointers = np.frombuffer(block[ARGS_FIXED_BYTES + SCALAR_BYTES * n_scalars:], dtype=np.uint64)
        assert len(pointers) == n_cols and len(set(pointers.tolist())) == n_cols, "a vector passed twice"
        consts = re.search(r"__device__ Fr h2_consts\[(\d+)\]", src)
        lds, plain = "fp_load(sh_cols[" in src, "fp_load(a.cols[" in src
        assert lds != plain
        omega = "a.tw_lo" in src
        stages.append(dict(scalars=n_scalars, cols=n_cols, block=len(block), dwords=8 * n_scalars + 2 * n_cols, lds=lds,
                           accumulate="fp_add(fp_load(a.values + idx), " in src, omega=omega, omega_hi=omega and kw["extended_k"] > 12,
                           tables=sorted({names[int(p)].split("[")[0] for p in pointers}), consts=int(consts.group(1)) if consts else 0,
                           rotations=len(set(re.findall(r"const size_t (r[pm]\d+) =", src)))))


def build(name, oracle):
    """-> (keyword dict, claim) of SHAPES[name]"""
    args, claim = SHAPES[name]
    args = dict(args)
    return shaped_case(args.pop("seed"), args.pop("k"), args.pop("ek"), oracle, **args), claim


_cache = {}


def cached(name, oracle):
    """`build`, once per session: (keyword dict, claim, the oracle's evaluate_h).  The arrays are shared: leave them unchanged"""
    if name not in _cache:
        from evalh_cases import oracle_evaluate_h

        kw, claim = build(name, oracle)
        want = oracle_evaluate_h(oracle, ev.Builder().build(**kw))
        want.setflags(write=False)
        _cache[name] = (kw, claim, want)
    return _cache[name]


# ---------------------------------------------------------------------------------------------------------------- the shapes
# A claim is checked on the LAYOUT of the program at default options: one dict per stage with `scalars`, `cols`, `block` (bytes of
# the argument block), `dwords` (of scalars + pointers), `lds` (arguments read through LDS), `accumulate`, `omega`, `omega_hi` and
# `tables` (the column tables the stage reads).  `holds` is the branch, in terms of the constants above.
def _claim(enters, stages, holds, **more):
    return dict(enters=enters, stages=stages, holds=holds, **more)


_SMALL = dict(k=3, ek=4, n_fixed=2, n_advice=6, n_instance=1, n_gates=4, gate_width=3)
_one_plain_stage = lambda L: len(L) == 1 and not L[0]["lds"] and L[0]["block"] <= ARGS_CUT_BYTES  # noqa: E731
# gates over fresh columns until the pool wraps: 48 gates x 8 operands over n_advice + 1 columns, then the permutation's terms
_ARGS = dict(seed=1, n_fixed=4, n_instance=1, gate_width=8, n_gates=48, n_perm=3, chunk_len=2)
_ARGS_UNDER, _ARGS_OVER = 316, 326
_DEEP = dict(n_fixed=2, n_advice=10, n_instance=1, gate_width=10)
REGS_NATURAL_GATES = 50      # the smallest gate count of _DEEP whose default build is rebuilt on the register budget
_TERM = dict(k=3, ek=4, n_fixed=1, n_instance=1, n_gates=0)

SHAPES = {
    "args-under": (dict(_ARGS, k=4, ek=6, n_advice=_ARGS_UNDER), _claim(
        "one stage: the block stays within the cut, %d column pointers below it" % (_ARGS_OVER - _ARGS_UNDER), 1,
        lambda L: len(L) == 1 and ARGS_CUT_BYTES - POINTER_BYTES * (_ARGS_OVER - _ARGS_UNDER) < L[0]["block"] <= ARGS_CUT_BYTES)),
    "args-over": (dict(_ARGS, k=4, ek=6, n_advice=_ARGS_OVER), _claim(
        "two stages cut by the size of the argument block alone; the second accumulates", 2,
        lambda L: len(L) == 2 and ARGS_CUT_BYTES < L[0]["block"] <= ARGS_MAX_BYTES and L[1]["accumulate"] and not L[0]["accumulate"])),
    "lds-auto-under": (dict(seed=2, k=3, ek=4, n_fixed=2, n_advice=115, n_instance=1, gate_width=6, n_gates=24, n_perm=2, chunk_len=2),
                       _claim("scalars + pointers of exactly lds_args dwords: read from the kernel arguments", 1,
                              lambda L: len(L) == 1 and L[0]["dwords"] == LDS_ARGS_DWORDS and not L[0]["lds"])),
    "lds-auto-over": (dict(seed=2, k=3, ek=4, n_fixed=2, n_advice=116, n_instance=1, gate_width=6, n_gates=24, n_perm=2, chunk_len=2),
                      _claim("one column more than lds-auto-under: read through LDS without H2_JIT_LDS_ARGS", 1,
                             lambda L: len(L) == 1 and L[0]["dwords"] == LDS_ARGS_DWORDS + 2 and L[0]["lds"])),
    "wide": (dict(seed=3, k=3, ek=5, n_fixed=40, n_advice=300, n_instance=4, n_perm=200, chunk_len=3, n_gates=40, gate_width=9), _claim(
        "614 vectors, 400 calculations: five stages cut by size only, the permutation's products after the gates", 5,
        lambda L: len(L) == 5 and all(ARGS_CUT_BYTES < st["block"] <= ARGS_MAX_BYTES for st in L[:-1]) and all(st["lds"] for st in L)
        and "perm_sigma" not in L[0]["tables"] and all("perm_sigma" in st["tables"] and "fixed" not in st["tables"] for st in L[1:]))),
    "wide-omega": (dict(_ARGS, k=11, ek=13, n_advice=_ARGS_OVER), _claim(
        "args-over at 2^13 rows: the later stage takes extended_omega^idx from the two-level table", 2,
        lambda L: len(L) == 2 and L[1]["accumulate"] and L[1]["omega"] and L[1]["omega_hi"])),
    "term-at-limit": (dict(_TERM, seed=4, n_advice=cols_past(ARGS_CUT_BYTES, 1), wide_term=cols_past(ARGS_CUT_BYTES, 1)), _claim(
        "one term past the cut and within the limit: it cannot be split and runs as one generated stage", 1,
        lambda L: len(L) == 1 and ARGS_CUT_BYTES < block_bytes(1, L[0]["cols"]) and L[0]["block"] <= ARGS_MAX_BYTES)),
    "term-too-wide": (dict(_TERM, seed=4, n_advice=cols_past(ARGS_MAX_BYTES, 1), wide_term=cols_past(ARGS_MAX_BYTES, 1)), _claim(
        "one term whose pointers alone pass the limit: the generator refuses the program, the interpreter kernels run it", 0,
        lambda L: L == [], refused="a single term reads more columns than one kernel's arguments hold")),
    "regs-natural": (dict(_DEEP, seed=5, k=3, ek=4, n_gates=REGS_NATURAL_GATES), _claim(
        "a deep, narrow program: one stage as generated, rebuilt by compile() on the register budget with no option set", 1,
        lambda L: len(L) == 1 and L[0]["block"] <= ARGS_CUT_BYTES, rebuilt=True)),
    "regs-forced": (dict(seed=5, k=3, ek=4, n_fixed=2, n_advice=8, n_instance=1, n_gates=12, gate_width=8), _claim(
        "12 gates x 8 operands under H2_JIT_MAX_REGS=64: rebuilt until the attempts run out, accepted over the budget", 1,
        lambda L: len(L) == 1, rebuilt=True, env={"H2_JIT_MAX_REGS": "64"})),
    "deep-interp": (dict(_DEEP, seed=6, k=3, ek=4, n_gates=150), _claim(
        "1650 calculations: the interpreter's work space is 1650 x (lanes launched) x 32 bytes", 1,
        lambda L: len(L) == 1, interpreter_only=True)),
    # ---- permutation geometry (evalh_cases.random_case: always 5 columns in chunks of 2)
    "perm-chunk-1": (dict(_SMALL, seed=10, n_perm=4, chunk_len=1), _claim("every permutation column a set of its own", 1, _one_plain_stage)),
    "perm-one-set": (dict(_SMALL, seed=11, n_perm=3, chunk_len=5), _claim("chunk_len > n_perm: one short set", 1, _one_plain_stage)),
    "perm-exact-multiple": (dict(_SMALL, seed=12, n_perm=6, chunk_len=3), _claim("n_perm = 2 chunk_len: no short last set", 1, _one_plain_stage)),
    "perm-single-column": (dict(_SMALL, seed=13, n_perm=1, chunk_len=2), _claim("one permutation column", 1, _one_plain_stage)),
    "perm-long-set": (dict(_SMALL, seed=14, n_perm=9, chunk_len=9), _claim("one z set over nine columns (three sets' worth at chunk_len 3)", 1,
                                                                          _one_plain_stage)),
    # ---- argument counts
    "lookup-one-set": (dict(_SMALL, seed=20, lookup_sets=(1,)), _claim("one lookup with one input set", 1, _one_plain_stage)),
    "lookup-four-sets": (dict(_SMALL, seed=21, lookup_sets=(4,)), _claim("one lookup with four input sets", 1, _one_plain_stage)),
    "lookups-six": (dict(_SMALL, seed=22, lookup_sets=(1, 2, 1, 3, 1, 2)), _claim("six lookups", 1, _one_plain_stage)),
    "shuffles-five": (dict(_SMALL, seed=23, n_shuffles=5), _claim("five shuffles", 1, _one_plain_stage)),
    "parts-zero": (dict(_SMALL, seed=24, n_perm=3, n_value_parts=0), _claim("no value part: the fold starts at the permutation", 1, _one_plain_stage)),
    "parts-one": (dict(_SMALL, seed=25, n_perm=3, n_value_parts=1), _claim("one value part in front of the permutation", 1, _one_plain_stage)),
    "constants-300": (dict(_SMALL, seed=26, n_constants=300, n_gates=30, gate_width=4, consts_per_gate=10), _claim(
        "300 constants, every one read: the module's constant table, not kernel arguments", 1,
        lambda L: _one_plain_stage(L) and L[0]["consts"] >= 290)),
    # n = 16, 32 extended rows: +-(n - 1) reach almost once round, 19 rows scale to 38 > 32 and wrap
    "rotations-12": (dict(_SMALL, seed=27, k=4, ek=5, n_gates=10, rotations=(0, 1, -1, 2, -2, 3, -3, 7, -6, 15, -15, 19)), _claim(
        "12 distinct rotations, +-(n - 1) and one past the extended size among them", 1,
        lambda L: _one_plain_stage(L) and L[0]["rotations"] == 11)),
}
PERM_SHAPES = tuple(name for name in SHAPES if name.startswith("perm-"))
SMALL_SHAPES = tuple(name for name, (args, _) in SHAPES.items() if args.get("n_gates") in (4, 10, 30) and args["ek"] <= 5)
# every shape whose generated kernels run on the device at default options
GENERATED_SHAPES = tuple(name for name, (_, claim) in SHAPES.items()
                         if not claim.get("interpreter_only") and "refused" not in claim and name != "wide-omega")
