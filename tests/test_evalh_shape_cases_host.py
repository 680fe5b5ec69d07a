"""The shapes of tests/evalh_shape_cases.py checked without a GPU.

  * the structural constants the shapes are derived from are the ones in evalh_gen.hpp / evalh_gen.cpp;
  * every shape's CLAIM -- which branch of the generator it enters -- holds for the program the library generates: stage count,
    the argument block of every stage, where the arguments are read from, which stages accumulate;
  * every stage's generated source, compiled for the host and run (tests/test_evalh_host_exec._run_generated), gives the C
    oracle's evaluate_h bit for bit, and the C oracle gives the big-integer restatement's (python_evaluate_h) on these shapes;
  * the refused program is refused with the generator's sentence and leaves nothing in the cache directory;
  * the register-budget rebuild of compile() and its record on disk (tests/evalh_shapes_worker.py, a process of its own)."""
import os
import re
import subprocess
import sys
import time

import numpy as np
import pytest

import evalh_shape_cases as sc
from evalh_cases import python_evaluate_h
from h2util import from_mont
from halo2_gpu_specific_amd import evaluation as ev
from halo2_gpu_specific_amd._lib import lib
from test_evalh_host_exec import CSRC, _run_generated

HERE = os.path.dirname(os.path.abspath(__file__))
REFUSED = tuple(name for name, (_, claim) in sc.SHAPES.items() if "refused" in claim)
REBUILT = tuple(name for name, (_, claim) in sc.SHAPES.items() if claim.get("rebuilt"))


def _one(pattern, text):
    found = re.findall(pattern, text)
    assert len(found) == 1, (pattern, found)
    return found[0]


def test_constants_are_the_generators():
    hpp, cpp = (open(os.path.join(CSRC, name)).read() for name in ("evalh_gen.hpp", "evalh_gen.cpp"))
    assert int(_one(r"constexpr size_t ARGS_FIXED_BYTES = (\d+);", hpp)) == sc.ARGS_FIXED_BYTES
    assert int(_one(r"constexpr size_t ARGS_MAX_BYTES = (\d+);", hpp)) == sc.ARGS_MAX_BYTES
    assert int(_one(r"constexpr size_t ARGS_CUT_BYTES = (\d+);", hpp)) == sc.ARGS_CUT_BYTES
    assert int(_one(r"uint32_t lds_args = (\d+);", hpp)) == sc.LDS_ARGS_DWORDS
    assert int(_one(r"uint32_t max_regs = (\d+);", hpp)) == sc.MAX_REGS
    assert "max_cols" not in hpp + cpp                      # (could never fire: 440 pointers alone are past the cut)
    assert _one(r"return ARGS_FIXED_BYTES \+ (\d+) \* std::max<size_t>\(scalars\.size\(\), 1\) \+ (\d+) \* std::max<size_t>\(cols\.size\(\), 1\);",
                cpp) == (str(sc.SCALAR_BYTES), str(sc.POINTER_BYTES))
    assert _one(r"const size_t arg_dwords = (\d+) \* scalars\.size\(\) \+ (\d+) \* cols\.size\(\);", cpp) == (
        str(sc.SCALAR_BYTES // 4), str(sc.POINTER_BYTES // 4))
    assert _one(r"opt\.lds_args > 1 && arg_dwords (>=?) opt\.lds_args", cpp) == ">"
    assert _one(r"return e\.args_bytes\(\) (>=?) ARGS_CUT_BYTES;", cpp) == ">"
    assert _one(r"if \(emitters\[s\]\.args_bytes\(\) (>=?) ARGS_MAX_BYTES\) fail\(", cpp) == ">"
    assert _one(r"st\.vgprs \+ st\.agprs (>=?) opt\.max_regs", cpp) == ">"
    assert int(_one(r"opt_in\.lds_args != 1 \? (0x[0-9a-f]+)u : 0u", cpp), 16) == sc.CACHE_LDS_BIT
    assert _one(r"constexpr char CACHE_MAGIC\[6\] = \{'(\w)', '(\w)', '(\w)', '(\w)', '(\w)', '(\w)'\};", cpp) == tuple("H2EVG3")
    # the smallest single terms on either side of the limit, as SHAPES spells them
    assert sc.block_bytes(1, sc.cols_past(sc.ARGS_CUT_BYTES, 1)) == sc.ARGS_CUT_BYTES + sc.POINTER_BYTES
    assert sc.block_bytes(1, sc.cols_past(sc.ARGS_MAX_BYTES, 1)) == sc.ARGS_MAX_BYTES + sc.POINTER_BYTES


@pytest.mark.parametrize("name", list(sc.SHAPES))
def test_shape_enters_the_branch_it_claims(oracle, monkeypatch, tmp_path, name):
    monkeypatch.setenv("H2_JIT_CACHE", str(tmp_path / "cache"))
    kw, claim, _ = sc.cached(name, oracle)
    for key, value in claim.get("env", {}).items():
        monkeypatch.setenv(key, value)
    L = sc.layout(kw)
    print(name, [(st["scalars"], st["cols"], st["block"], st["lds"]) for st in L])
    assert len(L) == claim["stages"] and claim["holds"](L), (claim["enters"], L)
    for s, st in enumerate(L):
        assert st["block"] == sc.block_bytes(st["scalars"], st["cols"]) <= sc.ARGS_MAX_BYTES
        assert st["lds"] == (st["dwords"] > sc.LDS_ARGS_DWORDS) and st["accumulate"] == (s > 0)
    # every vector of the case that the program can reach is read by some stage, none twice in one stage (layout() checks that)
    if name in ("args-under", "args-over", "wide"):
        args = sc.SHAPES[name][0]
        gates = sc.gate_columns(args["n_gates"], args["gate_width"], **{key: args[key] for key in ("n_fixed", "n_advice", "n_instance")})
        perm = {(ev.VS_ADVICE, i) for i in range(min(args["n_perm"], args["n_advice"]))}
        n_sets = -(-args["n_perm"] // args["chunk_len"])
        distinct = len(gates | perm) + n_sets + args["n_perm"] + 3          # + z, sigma, l_0 / l_last / l_active_row
        union = set()
        b = ev.Builder().build(**kw)
        values = np.zeros((1 << kw["extended_k"], 4), dtype=np.uint64)
        for s, st in enumerate(L):
            block = ev.stage_args(b, s, values.ctypes.data, 0, 0, 0, len(values))
            union |= set(np.frombuffer(block[sc.ARGS_FIXED_BYTES + sc.SCALAR_BYTES * st["scalars"]:], dtype=np.uint64).tolist())
        assert len(union) == distinct


@pytest.mark.parametrize("name", REFUSED)
def test_refused_program_says_why_and_leaves_no_file(oracle, monkeypatch, tmp_path, name):
    cache = tmp_path / "cache"
    monkeypatch.setenv("H2_JIT_CACHE", str(cache))
    kw, claim, _ = sc.cached(name, oracle)
    b = ev.Builder().build(**kw)
    for call in (ev.generated_source, ev.compile_only):
        with pytest.raises(Exception, match=claim["refused"]):
            call(b)
        assert claim["refused"] in lib().h2_last_error().decode()
    assert not cache.exists() or os.listdir(cache) == []


HOST_SETTINGS = {"args-over": ({}, {"H2_JIT_FACTOR": "0"}, {"H2_JIT_LDS_ARGS": "1000000"}),
                 "wide": ({}, {"H2_JIT_FACTOR": "0"}, {"H2_JIT_LDS_ARGS": "1000000"})}


@pytest.mark.parametrize("name", [name for name in sc.SHAPES if name not in REFUSED])
def test_generated_source_of_the_shape_run_on_the_host_matches_the_oracle(oracle, monkeypatch, tmp_path, name):
    """at default options (the claim's environment, where it has one); args-over and wide also in the reference's fold order and
    with the LDS copy switched off, so that their wide stages read hundreds of pointers straight from the arguments"""
    monkeypatch.setenv("H2_JIT_CACHE", str(tmp_path / "cache"))
    kw, claim, want = sc.cached(name, oracle)
    b = ev.Builder().build(**kw)
    for i, further in enumerate(HOST_SETTINGS.get(name, ({},))):
        env = dict(claim.get("env", {}), **further)
        for key, value in env.items():
            monkeypatch.setenv(key, value)
        got, stages = _run_generated(tmp_path, b, kw, "%s_o%d" % (name.replace("-", "_"), i))
        # (another fold order moves the cuts: args-over without factors passes the cut at its last term only, and stays whole)
        assert stages == claim["stages"] if not further else stages >= (2 if name == "wide" else 1), env
        assert np.array_equal(got, want), (env, int(np.argmax((got != want).any(axis=1))))
        for key in env:
            monkeypatch.delenv(key)


@pytest.mark.parametrize("name", [name for name in sc.SHAPES if name != "wide-omega"])
def test_python_restatement_pins_the_oracle_on_the_shape(oracle, name):
    """the C oracle is what every other test compares with: on these shapes -- hundreds of columns, 200 permutation columns, six
    lookups, twelve rotations -- it has to be right itself.  (wide-omega is args-over at 2^13 rows: nothing new for the oracle)"""
    kw, _, want = sc.cached(name, oracle)
    assert from_mont(want) == python_evaluate_h(kw)


@pytest.mark.parametrize("name", [name for name in sc.GENERATED_SHAPES if name not in REBUILT])
def test_shape_compiles_to_the_stages_it_enumerates(oracle, monkeypatch, tmp_path, name):
    """h2_evalh_compile (hipRTC for gfx950, no device) of every shape the register budget leaves alone: the stages of the source
    enumeration, no scratch, within the register budget"""
    monkeypatch.setenv("H2_JIT_CACHE", str(tmp_path / "cache"))
    kw, claim, _ = sc.cached(name, oracle)
    t0 = time.time()
    info = ev.compile_only(ev.Builder().build(**kw))
    print("%s: %d stages, %d registers, %d products per row, %.1f s" % (
        name, info["stages"], info["max_registers"], info["products_per_row"], time.time() - t0))
    assert info["stages"] == claim["stages"] and info["scratch_bytes"] == 0 and info["max_registers"] <= sc.MAX_REGS, info
    assert len(os.listdir(tmp_path / "cache")) == 1


@pytest.mark.parametrize("name", REBUILT)
def test_register_budget_rebuild_and_its_disk_record(tmp_path, name):
    env = dict(os.environ, H2_JIT_CACHE=str(tmp_path / "cache"))
    r = subprocess.run([sys.executable, os.path.join(HERE, "evalh_shapes_worker.py"), "host-cache", name], env=env, capture_output=True,
                       text=True, timeout=900)
    print(r.stdout[-500:])
    assert r.returncode == 0 and "shapes worker ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
