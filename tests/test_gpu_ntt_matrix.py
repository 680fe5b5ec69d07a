"""Every pass geometry, padding and scale of csrc/ntt.hip against the definition of the transform.

ntt_run_chunk picks one of five kernels per pass from the size and the arguments alone (ntt_split, pass_shape, the
position of the pass, the zero padding, the scale mode, the H2_NTT_* knobs).  The rows here are laid over that space rather
than along the lines a proof happens to take; tests/ntt_matrix_cases.py enumerates them and computes what each has to give --
(a) the whole vector from the oracle's FFT over a CPU-prepared input, (b) eight entries from the definition by Horner,
without the oracle's FFT.  Every comparison is bit for bit.

Rows (default knobs, this process), one test per size so that a failure names it:
  2^9, 2^10, 2^16, 2^17 and every size 2^18 .. 2^21 -- all six device entry points, in place and out of place where both
  exist; padding z = 0, 1, 2, 3, B - 1, B, B + 1, L - 1, L around the first pass's width B (h2_ntt_shape); inputs random,
  zero, all r - 1, alternating 0 / r - 1, delta at 1, at in_len - 1 and at a seeded position; from 2^18 with the last pass's
  twiddle table resident (two calls, both compared) and composed (h2_set_table_budget(0)); batches of 1, 2, 16 and 17 vectors
  at 2^18 and 2^20.  2^22: the same with three of the inputs; 2^23, 2^24: the rows that change kernel there
  (ntt_matrix_cases.THIN_*).  2^27: forward and inverse by layer (b) and the round trip.  Forty coset generators through
  one 2^18 plan (NttPlan::SCALE_TABS_MAX = 32).
Knobs: one child process per setting (tests/ntt_matrix_worker.py: three, the split without 9-bit passes, no padding skip,
no last-pass table), one after another, each compared with the oracle inside the child.

Coverage is asserted: the kernel ids h2_ntt_shape reports for the rows of this process alone are every kernel ntt_run_chunk
can launch.  An instantiation no row reaches fails here.

Wall clock on an MI355X host with 16 CPUs (the oracle's FFTs on 8 threads are most of it): see DESIGN.md 3.2; the cap is
240 s, and what is thinned for it is 2^22 and above.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import halo2_gpu_specific_amd as h2
from halo2_gpu_specific_amd._lib import check
from h2util import R_MOD, ROOT, fr_mont

import ntt_matrix_cases as mc
from ntt_matrix_worker import Runner, _vp

pytestmark = pytest.mark.gpu

SEEN = {}  # log_n (or a row's name) -> kernel ids of the rows that ran in this process
CHILD_TIMEOUT = 240
L_KERNEL_COUNT = 5  # H2_NTT_KERNEL_COUNT (include/halo2_hip.h)


def _restore(L):
    L.h2_set_table_budget(2**64 - 1)  # back to the default (H2_NTT_TABLE_BUDGET / 1/32 of memory)
    L.h2_release_plans()


@pytest.mark.parametrize("log_n", mc.MATRIX_SIZES)
def test_ntt_matrix(oracle, log_n):
    """all rows of one size (module docstring), both twiddle sources from 2^18; batches at 2^18 and 2^20"""
    L = h2.lib()
    r = Runner(oracle, log_n)
    cases = mc.matrix_cases(L, log_n)
    try:
        if log_n < 18:
            r.run_cases(cases)
        else:
            r.run_cases(cases, calls=2, tag=" (resident last-pass table)")
            if log_n in mc.BATCH_SIZES:
                for bop in mc.BATCH_OPS:
                    for z in (mc.batch_paddings(L, log_n) if bop == "coeff_to_extended_batch" else [0]):
                        for count in mc.BATCH_COUNTS:
                            r.run_batch(bop, count, z)
            check(L.h2_set_table_budget(0), "h2_set_table_budget")
            check(L.h2_release_plans(), "h2_release_plans")
            r.run_cases(cases, calls=1, tag=" (composed twiddles)")
            if log_n in mc.BATCH_SIZES:
                for bop in mc.BATCH_OPS:
                    for z in (mc.batch_paddings(L, log_n) if bop == "coeff_to_extended_batch" else [0]):
                        r.run_batch(bop, 17, z)
    finally:
        _restore(L)
    SEEN[log_n] = set(r.kernels)


def test_ntt_2p27_forward_and_inverse(oracle):
    """[3, 8, 8, 8] above the largest size that keeps a last-pass table: eight outputs of the forward transform and eight of
    the inverse against the definition (the oracle's Horner over all 2^27 inputs), and intt(ntt(x)) == x"""
    L = h2.lib()
    log_n = 27
    n = 1 << log_n
    r = Runner(oracle, log_n)
    ref = r.ref
    x = oracle.random_fr(0x2727, n)
    xd = r.upload(x)
    a = xd.clone()
    tmp = r.scratch().data_ptr()
    case = mc.Case("ntt", 0, "random", False)
    idx = ref.sample_indices(case)
    try:
        r.sync()
        check(L.h2_dev_ntt(a.data_ptr(), tmp, _vp(r.fr["w"]), log_n, None), "h2_dev_ntt")
        r.sync()
        got = a[idx].cpu().numpy().view(np.uint64)
        for row, i in zip(got, idx):
            assert mc._mont_int(row) == ref.horner(x, None, pow(ref.w, i, R_MOD)), ("ntt 2^27", i)
        fwd = a.cpu().numpy().view(np.uint64)
        check(L.h2_dev_intt(a.data_ptr(), tmp, _vp(r.fr["w_inv"]), _vp(r.fr["d"]), log_n, None), "h2_dev_intt")
        r.sync()
        assert torch.equal(a, xd), "intt(ntt(x)) != x at 2^27"
        for i in idx:  # the inverse on its own: x[i] = d sum_k X[k] w^(-ik)
            assert mc._mont_int(x[i]) == ref.horner(fwd, None, pow(ref.w_inv, i, R_MOD)) * ref.d % R_MOD, ("intt 2^27", i)
    finally:
        _restore(L)
    SEEN["2^27"] = set(mc.kernel_ids(L, log_n))


def test_forty_coset_generators_through_one_plan(oracle):
    """NttPlan::SCALE_TABS_MAX = 32 tables of g^i per plan, least recently used out first: forty generators through the
    2^18 plan, then the first again (evicted meanwhile, rebuilt), each against the oracle's FFT of x[i] g^i"""
    L = h2.lib()
    log_n = 18
    n = 1 << log_n
    r = Runner(oracle, log_n)
    ref = r.ref
    x = ref.raw_input("random", n)
    xd = r.upload(x)
    tmp = r.scratch().data_ptr()
    gens = [(3 + 2 * t) * pow(mc.ROOT_W, 7 + t, R_MOD) % R_MOD for t in range(40)]
    assert len(set(gens)) == 40
    try:
        for t, g in enumerate(gens + gens[:1]):
            ref._powers.clear()
            want = oracle.best_fft(oracle.eval_op(mc.OP_MUL, x, ref.powers(g), 0, 0, None), fr_mont(ref.w), log_n, threads=8)
            out = torch.full((n, 4), -1, dtype=torch.int64, device=r.dev)
            r.sync()
            check(L.h2_dev_coset_ntt(xd.data_ptr(), out.data_ptr(), tmp, log_n, _vp(fr_mont(g)), _vp(r.fr["w"]), None), "h2_dev_coset_ntt")
            r.sync()
            r.compare(out, r.upload(want), "coset generator %d of 40 (+ the first again)" % t)
    finally:
        _restore(L)
    SEEN["generators"] = set(mc.kernel_ids(L, log_n))


@pytest.mark.timeout(len(mc.KNOB_SETTINGS) * CHILD_TIMEOUT + 60)
def test_knob_settings_and_kernel_coverage():
    """every knob setting in a child process of its own, one after another (a child that fails, times out or dies by a signal
    ends the test there); before them the coverage: this process's rows alone reached every kernel the launcher can launch,
    and no child reports a kernel id outside the enumeration"""
    L = h2.lib()
    missing = [s for s in mc.MATRIX_SIZES if s not in SEEN]
    assert not missing, "the coverage is over the rows of the whole module: test_ntt_matrix did not pass at 2^%s" % missing
    default = set().union(*SEEN.values())
    never = sorted(mc.ALL_KERNELS - default)
    assert not never, "no row of this process reaches %s" % [mc.KERNELS[k] for k in never]
    assert default == set(mc.DEFAULT_KERNELS) == set(mc.ALL_KERNELS) == set(range(L_KERNEL_COUNT))
    assert set(mc.matrix_kernel_ids(L)) == default
    script = os.path.join(ROOT, "tests", "ntt_matrix_worker.py")
    for knobs in mc.KNOB_SETTINGS:
        env = {k: v for k, v in os.environ.items() if k not in mc.KNOBS}
        env.update(knobs)
        res = subprocess.run([sys.executable, script], env=env, capture_output=True, text=True, timeout=CHILD_TIMEOUT, cwd=ROOT)
        assert res.returncode == 0 and "CHILD OK" in res.stdout, (knobs, res.returncode, res.stdout[-2000:], res.stderr[-3000:])
        line = [ln for ln in res.stdout.splitlines() if ln.startswith("KERNELS ")][-1]
        ids = {int(v) for v in line.split()[1:]}
        print(knobs, "->", sorted(ids))
        assert ids <= default, (knobs, sorted(ids))
