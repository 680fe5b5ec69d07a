"""evaluate_h on the device at the shapes of tests/evalh_shape_cases.py: the branches that depend on how big a circuit is -- stages
cut by the size of the argument block, the automatic LDS copy of the arguments, a single term at the launch limit, the refused
program's fallback, the register-budget rebuild and its reload from disk, the interpreter on a deep program -- each entered by a
named case (tests/test_evalh_shape_cases_host.py checks that it is), every result compared bit for bit (np.array_equal) with the
CPU oracle's evaluate_h.

The refused program (term-too-wide): h2_evaluate_h computes it on the interpreter kernels and says so once per program on
stderr; h2_evalh_prepare is an ERROR that carries the generator's sentence -- a caller that prepares at keygen time hears that,
and why, this circuit has no generated kernels, instead of an info with zero stages that it would have to know to look at."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import evalh_shape_cases as sc
from evalh_cases import COLUMN_TABLES, oracle_evaluate_h
from halo2_gpu_specific_amd import evaluation as ev

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
REBUILT = tuple(name for name, (_, claim) in sc.SHAPES.items() if claim.get("rebuilt"))
# at most two further generator settings per shape: each costs a hipRTC build
FURTHER = dict({"wide": ({"H2_JIT_FACTOR": "0"}, {"H2_JIT_LDS_ARGS": "1000000"})}, **{name: ({"H2_JIT_MUL2": "0"},) for name in sc.PERM_SHAPES})


@pytest.mark.parametrize("name", [name for name in sc.GENERATED_SHAPES if name not in REBUILT] + ["wide-omega"])
def test_shape_on_the_interpreter_and_as_generated_kernels(oracle, monkeypatch, tmp_path, name):
    monkeypatch.setenv("H2_JIT_CACHE", str(tmp_path))
    kw, claim, want = sc.cached(name, oracle)
    b = ev.Builder().build(**kw)
    before = ev.generated_launches()
    assert np.array_equal(ev.evaluate_h(ev.Builder().build(**kw, flags=ev.EVALH_INTERPRET)), want)
    assert ev.generated_launches() == before, "H2_EVALH_INTERPRET must keep the interpreter kernels"
    for env in ({},) + FURTHER.get(name, ()):
        for key, value in env.items():
            monkeypatch.setenv(key, value)
        info = ev.prepare(b)
        print(name, env, info)
        assert info["scratch_bytes"] == 0 and info["max_registers"] <= sc.MAX_REGS, info
        assert info["stages"] == claim["stages"] if not env else info["stages"] >= (2 if name == "wide" else 1), info
        before = ev.generated_launches()
        assert np.array_equal(ev.evaluate_h(b), want), env
        assert ev.generated_launches() == before + info["stages"], "the generated kernels did not run"
        for key in env:
            monkeypatch.delenv(key)


def test_refused_program_runs_on_the_interpreter_with_one_warning(oracle, monkeypatch, tmp_path, capfd):
    monkeypatch.setenv("H2_JIT_CACHE", str(tmp_path))
    kw, claim, want = sc.cached("term-too-wide", oracle)
    b = ev.Builder().build(**kw)
    before = ev.generated_launches()
    capfd.readouterr()
    for _ in range(2):
        assert np.array_equal(ev.evaluate_h(b), want)
    assert ev.generated_launches() == before
    err = capfd.readouterr().err
    assert err.count("runs on the interpreter kernels") == 1 and err.count(claim["refused"]) == 1, err
    with pytest.raises(Exception, match="h2_evalh_prepare: no generated kernels for this program.*" + claim["refused"]):
        ev.prepare(b)
    assert capfd.readouterr().err == "" and os.listdir(tmp_path) == []


@pytest.mark.parametrize("name", REBUILT)
def test_rebuilt_stages_run_and_are_found_on_disk_by_a_fresh_process(oracle, monkeypatch, tmp_path, name):
    """compile()'s register-budget loop: the arguments through LDS, then stages of half the products, built again -- those code
    objects run here, and a process of its own (tests/evalh_shapes_worker.py) loads them from the file without compiling"""
    monkeypatch.setenv("H2_JIT_CACHE", str(tmp_path))
    kw, claim, want = sc.cached(name, oracle)
    assert np.array_equal(ev.evaluate_h(ev.Builder().build(**kw, flags=ev.EVALH_INTERPRET)), want)
    for key, value in claim.get("env", {}).items():
        monkeypatch.setenv(key, value)
    enumerated = len(sc.layout(kw))
    b = ev.Builder().build(**kw)
    info = ev.prepare(b)
    print(name, info)
    assert info["from_cache"] == 0 and info["stages"] > enumerated == claim["stages"] and info["scratch_bytes"] == 0, info
    before = ev.generated_launches()
    assert np.array_equal(ev.evaluate_h(b), want)
    assert ev.generated_launches() == before + info["stages"]
    assert len(os.listdir(tmp_path)) == 1
    r = subprocess.run([sys.executable, os.path.join(HERE, "evalh_shapes_worker.py"), "gpu-reload", name, str(info["stages"])],
                       env=dict(os.environ), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "shapes worker ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def _on_device(kw):
    """the case with every vector in device memory: (keyword dict of addresses, what keeps them alive)"""
    import torch

    dev = torch.device("cuda", 0)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).to(dev)  # noqa: E731
    tensors = {name: [up(c) for c in kw[name]] for name in COLUMN_TABLES}
    singles = {name: up(kw[name]) for name in ("l0", "l_last", "l_active_row")}
    dkw = dict(kw)
    for name in COLUMN_TABLES:
        dkw[name] = [t.data_ptr() for t in tensors[name]]
    for name in singles:
        dkw[name] = singles[name].data_ptr()
    return dkw, (tensors, singles)


def _check_ranges(dkw, want, flags, ranges):
    import torch

    import halo2_gpu_specific_amd as h2
    from halo2_gpu_specific_amd._lib import check

    size, sentinel = len(want), 0x5A5A5A5A5A5A5A5A
    for lo, cnt in ranges:
        b = ev.Builder().build(**dkw, flags=flags, row_begin=lo, row_count=cnt)
        out = torch.full((size, 4), sentinel, dtype=torch.int64, device=torch.device("cuda", 0))
        torch.cuda.synchronize()
        check(h2.lib().h2_dev_evaluate_h(ctypes.byref(b.desc), out.data_ptr(), None), "h2_dev_evaluate_h")
        torch.cuda.synchronize()
        got = out.cpu().numpy().view(np.uint64)
        lo_, hi = (lo, lo + cnt) if cnt else (0, size)
        assert np.array_equal(got[lo_:hi], want[lo_:hi]), (flags, lo, cnt)
        assert (np.concatenate([got[:lo_], got[hi:]]) == np.uint64(sentinel)).all(), ("rows outside the range were written", flags, lo, cnt)


@pytest.mark.parametrize("name", ["args-over", "wide"])
def test_row_ranges_of_stages_cut_by_size(oracle, monkeypatch, tmp_path, name):
    """row_begin / row_count on programs whose LATER stages exist because of the argument block: every stage after the first adds
    into `values` and must touch the rows asked for and no other -- at the start, a single row, across the wrap of the
    rotations, everything; the interpreter likewise"""
    monkeypatch.setenv("H2_JIT_CACHE", str(tmp_path))
    kw, claim, want = sc.cached(name, oracle)
    size = len(want)
    dkw, keep = _on_device(kw)
    ranges = ((0, size // 4), (size // 2 - 3, 1), (size - 5, 5), (7, size - 7), (0, 0))
    before = ev.generated_launches()
    _check_ranges(dkw, want, ev.EVALH_INTERPRET, ranges)
    assert ev.generated_launches() == before
    _check_ranges(dkw, want, 0, ranges)
    assert ev.generated_launches() == before + len(ranges) * claim["stages"]
    del keep


def test_coefficient_form_entry_points_on_stages_cut_by_size(oracle, monkeypatch, tmp_path):
    """h2_evaluate_h_coeff and h2_quotient_poly_coeff on args-over at j = 3, k = 5 (4 cosets of 32 rows): several hundred distinct
    host vectors, each uploaded once and transformed per coset, feed two stages per coset -- against the oracle's evaluate_h on
    the oracle's own extended cosets, its divide_by_vanishing_poly and extended_to_coeff"""
    import copy

    from halo2_gpu_specific_amd._lib import lib

    monkeypatch.setenv("H2_JIT_CACHE", str(tmp_path))
    j, k = 3, 5
    d, t = oracle.domain(j, k)
    args, claim = sc.SHAPES["args-over"]
    args = dict(args, k=k, ek=d.extended_k)
    kw = sc.shaped_case(args.pop("seed"), args.pop("k"), args.pop("ek"), oracle, **args)
    kw["zeta"], kw["extended_omega"] = d.fr("g_coset"), d.fr("extended_omega")
    n = 1 << k
    coeff, ext = copy.copy(kw), copy.copy(kw)
    for name in COLUMN_TABLES:
        coeff[name] = [np.ascontiguousarray(col[:n]) for col in kw[name]]
        ext[name] = [oracle.coeff_to_extended(col, d, threads=8) for col in coeff[name]]
    for name in ("l0", "l_last"):
        coeff[name] = np.ascontiguousarray(kw[name][:n])
        ext[name] = oracle.coeff_to_extended(coeff[name], d, threads=8)
    assert len(sc.layout(ext)) == claim["stages"]
    want = oracle_evaluate_h(oracle, ev.Builder().build(**ext))
    before = ev.generated_launches()
    assert np.array_equal(ev.evaluate_h_coeff(ev.Builder().build(**coeff)), want)
    assert ev.generated_launches() == before + claim["stages"] * (1 << (d.extended_k - k))
    divided = want.copy()
    oracle.lib.oracle_divide_by_vanishing_poly(divided.ctypes.data, len(divided), t.ctypes.data, len(t), 8)
    want_coeff = oracle.extended_to_coeff(divided, d, threads=8)
    b = ev.Builder().build(**coeff)
    out = np.empty((len(want_coeff), 4), dtype=np.uint64)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)                                  # noqa: E731
    scal = [d.fr(name) for name in ("g_coset", "g_coset_inv", "extended_omega_inv", "extended_ifft_divisor")]
    assert lib().h2_quotient_poly_coeff(ctypes.byref(b.desc), vp(t), len(t), *[vp(v) for v in scal], vp(out), len(out)) == 0
    assert np.array_equal(out, want_coeff)


def test_interpreter_on_a_deep_program(oracle):
    """1650 calculations on the interpreter kernels alone: the whole domain of 16 rows, and 300 rows -- two workgroups, the second
    partly idle -- out of 512.  k_evalh_expr keeps its intermediates as [calculation][lane]: the work space follows the lanes
    launched (16 MiB per calculation when every call launched 2^19 of them: 26 GiB for this program)"""
    kw, _, want = sc.cached("deep-interp", oracle)
    assert len(kw["calculations"]) >= 1500
    before = ev.generated_launches()
    assert np.array_equal(ev.evaluate_h(ev.Builder().build(**kw, flags=ev.EVALH_INTERPRET)), want)
    args = dict(sc.SHAPES["deep-interp"][0], k=7, ek=9)
    kw = sc.shaped_case(args.pop("seed"), args.pop("k"), args.pop("ek"), oracle, **args)
    want = oracle_evaluate_h(oracle, ev.Builder().build(**kw))
    dkw, keep = _on_device(kw)
    _check_ranges(dkw, want, ev.EVALH_INTERPRET, ((100, 300), (512 - 300, 300), (0, 0)))
    assert ev.generated_launches() == before
    del keep
