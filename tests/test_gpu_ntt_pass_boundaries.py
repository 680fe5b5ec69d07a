"""What two NTT passes hand over (csrc/ntt_pass.hip, csrc/field.hpp): the last stage pair of a fixed pass before the last leaves
its results unreduced for the product that reads them, every store product ends as a canonical residue (fp_chunk_handover) so
that the pass behind it starts from bare sums, and the plain call -- one vector, whole length, no scale -- runs instantiations
of k_ntt_pass8 of its own (PLAIN, chosen in ntt_pass_launch: h2_ntt_shape's kernel ids do not move).  The bounds are
tests/test_ntt_pass_boundaries_host.py.  Only representatives change, never a residue: every output here is compared bit for
bit, with the inputs and expected vectors of tests/ntt_matrix_cases.py.

  2^19 (3, 8, 8) and 2^20 (4, 8, 8): a general first pass (the radix-4 kernel) that multiplies at its store and hands over
  canonical residues, then the plain middle pass (canonical first pair, loose last pair) and the plain last pass.
  Forward and inverse on random rows, the zero vector and all r - 1.  The calls that are not plain -- a padded one, a coset
  one, a batch of two vectors -- run the instantiations without PLAIN and the same store products.
  2^24 (8, 8, 8): the only size here whose first pass is the fixed kernel, k_ntt_pass8<true, true>: the random vector forward
  against the oracle's FFT (computed once), the round trip on the device, and the zero vector."""
import ctypes

import pytest
import torch

import halo2_gpu_specific_amd as h2
from halo2_gpu_specific_amd._lib import check
from h2util import fr_mont

import ntt_matrix_cases as mc
from ntt_matrix_worker import Runner

pytestmark = pytest.mark.gpu

PASS8_DP, PASS8, R4_DP = (mc.KERNELS.index(k) for k in ("k_ntt_pass8<true>", "k_ntt_pass8<false>", "k_ntt_pass<true, true>"))
# log_n -> (the passes' widths, the kernel id of each)
PLANS = {
    19: ([3, 8, 8], [R4_DP, PASS8_DP, PASS8]),
    20: ([4, 8, 8], [R4_DP, PASS8_DP, PASS8]),
    24: ([8, 8, 8], [PASS8_DP, PASS8_DP, PASS8]),
}


def _vp(a):
    return a.ctypes.data_as(ctypes.c_void_p)


@pytest.mark.parametrize("log_n", sorted(PLANS))
def test_the_sizes_run_the_kernels_the_docstring_names(log_n):
    passes = mc.ntt_shape(h2.lib(), log_n, log_n)
    assert ([p["bits"] for p in passes], [p["kernel"] for p in passes]) == PLANS[log_n]
    assert all(p["fixed"] == (p["bits"] == 8 and p["kernel"] in (PASS8_DP, PASS8)) for p in passes)


def test_a_padded_call_keeps_the_fixed_passes_behind_a_general_first_pass():
    for log_n in (19, 20):
        passes = mc.ntt_shape(h2.lib(), log_n, log_n - 1)
        assert passes[0]["zskip"] == 1 and [p["kernel"] for p in passes][1:] == [PASS8_DP, PASS8]


@pytest.fixture(scope="module", params=[19, 20])
def runner(request, oracle):
    return Runner(oracle, request.param)


@pytest.mark.parametrize("inp", ["random", "zero", "rm1"])
@pytest.mark.parametrize("op", ["ntt", "intt"])
def test_forward_and_inverse_bit_exact(runner, op, inp):
    runner.run_cases([mc.Case(op, 0, inp, False)])


@pytest.mark.parametrize("op,z", [("coeff_to_extended", 1), ("coset_ntt", 0), ("extended_to_coeff", 0)])
def test_the_calls_that_are_not_plain(runner, op, z):
    runner.run_cases([mc.Case(op, z, "random", False)])


@pytest.mark.parametrize("bop", ["ntt_batch", "intt_batch"])
def test_a_batch_of_two_vectors(runner, bop):
    runner.run_batch(bop, 2)


@pytest.fixture(scope="module")
def runner24(oracle):
    return Runner(oracle, 24)


def test_2p24_forward_against_the_oracle(oracle, runner24):
    r = runner24
    x = r.ref.raw_input("random", r.n)
    want = oracle.best_fft(x.copy(), fr_mont(r.ref.w), r.log_n, threads=mc.ORACLE_THREADS)
    buf = r.upload(x)
    r.sync()
    check(r.L.h2_dev_ntt(buf.data_ptr(), r.scratch().data_ptr(), _vp(r.fr["w"]), r.log_n, None), "h2_dev_ntt")
    r.sync()
    r.compare(buf, r.upload(want), "2^24 ntt random")


def test_2p24_round_trip_on_the_device(runner24):
    r = runner24
    x = r.upload(r.ref.raw_input("random", r.n))
    buf = x.clone()
    r.sync()
    check(r.L.h2_dev_ntt(buf.data_ptr(), r.scratch().data_ptr(), _vp(r.fr["w"]), r.log_n, None), "h2_dev_ntt")
    check(r.L.h2_dev_intt(buf.data_ptr(), r.scratch().data_ptr(), _vp(r.fr["w_inv"]), _vp(r.fr["d"]), r.log_n, None),
          "h2_dev_intt")
    r.sync()
    r.compare(buf, x, "2^24 intt(ntt(x))")


def test_2p24_the_zero_vector(runner24):
    r = runner24
    buf = torch.zeros((r.n, 4), dtype=torch.int64, device=r.dev)
    r.sync()
    check(r.L.h2_dev_ntt(buf.data_ptr(), r.scratch().data_ptr(), _vp(r.fr["w"]), r.log_n, None), "h2_dev_ntt")
    check(r.L.h2_dev_intt(buf.data_ptr(), r.scratch().data_ptr(), _vp(r.fr["w_inv"]), _vp(r.fr["d"]), r.log_n, None),
          "h2_dev_intt")
    r.sync()
    assert not bool(buf.any()), "the transforms of the zero vector are not zero"
