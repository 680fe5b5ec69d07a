"""The two ends of a tile of the fixed 8-bit pass (csrc/ntt_pass.hip, k_ntt_pass8): the loads at its head are issued before
the LDS copy of the twiddle table waits for its own, the last stage pair's first twiddle is requested before the barrier in
front of it, the store product of a first pass keeps the next table entry in flight, and the first stage pair skips the
reductions of operands that left a product (fp_lazy_first_pair, csrc/field.hpp).  None of it changes a value: every output
here is compared bit for bit, with the inputs and expected vectors of tests/ntt_matrix_cases.py.

  2^19 (passes 3, 8, 8): the smallest size at which both instantiations behind a first pass run -- the middle one loads
  operands the first pass multiplied at its store (tw_applied: no reduction, no product at the load), the last one loads
  after its own twiddle product.  Forward and inverse (in place: the only form those two entry points have), the coset and
  the extended forward transforms in place and out of place (the pre-scaled first pass is the general kernel here; the two
  fixed passes behind it are the same), five inputs each, and one batched call of two vectors each way.

  2^24 (8, 8, 8): the smallest size whose FIRST pass is the fixed kernel, k_ntt_pass8<true, true>: it loads the caller's
  data (the reductions stay) and multiplies at its store.  The all-(r - 1) vector and a random one forward against the
  oracle's FFT, and intt(ntt(x)) == x on the device for the whole vector.
"""
import ctypes

import pytest

import halo2_gpu_specific_amd as h2
from halo2_gpu_specific_amd._lib import check
from h2util import fr_mont

import ntt_matrix_cases as mc
from ntt_matrix_worker import Runner

pytestmark = pytest.mark.gpu

PASS8_DP, PASS8, R4_DP = (mc.KERNELS.index(k) for k in ("k_ntt_pass8<true>", "k_ntt_pass8<false>", "k_ntt_pass<true, true>"))
INPUTS = ("random", "zero", "rm1", "alt", "delta1")


def _vp(a):
    return a.ctypes.data_as(ctypes.c_void_p)


@pytest.mark.parametrize("log_n,bits,first", [(19, [3, 8, 8], R4_DP), (24, [8, 8, 8], PASS8_DP)])
def test_the_sizes_reach_the_three_instantiations(log_n, bits, first):
    passes = mc.ntt_shape(h2.lib(), log_n, log_n)
    assert [p["bits"] for p in passes] == bits
    assert [p["kernel"] for p in passes] == [first, PASS8_DP, PASS8]


@pytest.fixture(scope="module")
def runner19(oracle):
    return Runner(oracle, 19)


@pytest.mark.parametrize("inp", INPUTS)
@pytest.mark.parametrize("op", ["ntt", "intt", "coset_ntt", "coeff_to_extended"])
def test_2p19_forward_and_inverse_in_place_and_out_of_place(runner19, op, inp):
    """every place the entry point has (ntt_matrix_cases.PLACES): ntt and intt in place, the other two both ways"""
    runner19.run_cases([mc.Case(op, 0, inp, False)])


@pytest.mark.parametrize("bop", ["ntt_batch", "intt_batch"])
def test_2p19_a_batch_of_two_vectors(runner19, bop):
    runner19.run_batch(bop, 2)


@pytest.fixture(scope="module")
def runner24(oracle):
    return Runner(oracle, 24)


@pytest.mark.parametrize("inp", ["rm1", "random"])
def test_2p24_forward_against_the_oracle(oracle, runner24, inp):
    r = runner24
    x = r.ref.raw_input(inp, r.n)
    want = oracle.best_fft(x.copy(), fr_mont(r.ref.w), r.log_n, threads=mc.ORACLE_THREADS)
    buf = r.upload(x)
    r.sync()
    check(r.L.h2_dev_ntt(buf.data_ptr(), r.scratch().data_ptr(), _vp(r.fr["w"]), r.log_n, None), "h2_dev_ntt")
    r.sync()
    r.compare(buf, r.upload(want), "2^24 ntt " + inp)


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
