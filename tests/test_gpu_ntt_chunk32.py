"""The fixed 8-bit pass (csrc/ntt_pass.hip, k_ntt_pass8) multiplies by the twiddles that are the same for a whole wave -- the
one twiddle of its first stage pair, and all of the round of stages 2 and 3, whose twiddle index is the wave's index -- through
EIGHT-chunk entries (FpChunk<1>, the 8 KiB table tw_store's fourth form builds) read plane by plane into scalar registers
(fp_mul_chunk_planes, csrc/field.hpp; the schedule is tests/test_fp_mul_chunk32_host.py).  A product returns another
representative below p (1 + 2^-29) than the four-chunk one, never another residue: every output here is compared bit for
bit, with the inputs and expected vectors of tests/ntt_matrix_cases.py.

  2^19 (3, 8, 8) and 2^20 (4, 8, 8): the smallest plans with the fixed pass as middle and as last pass.  Forward and inverse
  on random canonical rows, the all-zero vector and all r - 1; one padded call (coeff_to_extended); one batched call of two
  vectors at 2^19.  Any full tile runs all four waves, hence every entry the scalar path reads and all four wave indices.
  2^24 (8, 8, 8): the only size here whose first pass is the fixed kernel with the next pass's twiddles at its store: one
  random forward transform against the oracle, and the round trip on the device."""
import ctypes

import pytest

import halo2_gpu_specific_amd as h2
from halo2_gpu_specific_amd._lib import check
from h2util import fr_mont

import ntt_matrix_cases as mc
from ntt_matrix_worker import Runner

pytestmark = pytest.mark.gpu

PASS8_DP, PASS8 = (mc.KERNELS.index(k) for k in ("k_ntt_pass8<true>", "k_ntt_pass8<false>"))


def _vp(a):
    return a.ctypes.data_as(ctypes.c_void_p)


@pytest.mark.parametrize("log_n,bits", [(19, [3, 8, 8]), (20, [4, 8, 8])])
def test_the_last_two_passes_are_the_fixed_kernel(log_n, bits):
    passes = mc.ntt_shape(h2.lib(), log_n, log_n)
    assert [p["bits"] for p in passes] == bits
    assert [p["kernel"] for p in passes[1:]] == [PASS8_DP, PASS8]
    assert passes[0]["kernel"] not in (PASS8_DP, PASS8)


_RUNNERS = {}


def _runner(oracle, log_n):
    """one Runner per size: its expected vectors are computed once and shared"""
    if log_n not in _RUNNERS:
        _RUNNERS[log_n] = Runner(oracle, log_n)
    return _RUNNERS[log_n]


@pytest.fixture(scope="module", params=[19, 20])
def runner(request, oracle):
    return _runner(oracle, request.param)


@pytest.mark.parametrize("inp", ["random", "zero", "rm1"])
@pytest.mark.parametrize("op", ["ntt", "intt"])
def test_forward_and_inverse_bit_exact(runner, op, inp):
    runner.run_cases([mc.Case(op, 0, inp, False)])


def test_a_padded_call(runner):
    runner.run_cases([mc.Case("coeff_to_extended", 1, "random", False)])


def test_2p19_a_batch_of_two_vectors(oracle):
    _runner(oracle, 19).run_batch("ntt_batch", 2)


def test_2p24_forward_against_the_oracle_and_back(oracle):
    r = Runner(oracle, 24)
    assert [p["kernel"] for p in mc.ntt_shape(r.L, 24, 24)] == [PASS8_DP, PASS8_DP, PASS8]
    x = r.ref.raw_input("random", r.n)
    want = oracle.best_fft(x.copy(), fr_mont(r.ref.w), r.log_n, threads=mc.ORACLE_THREADS)
    src = r.upload(x)
    buf = src.clone()
    r.sync()
    check(r.L.h2_dev_ntt(buf.data_ptr(), r.scratch().data_ptr(), _vp(r.fr["w"]), r.log_n, None), "h2_dev_ntt")
    r.sync()
    r.compare(buf, r.upload(want), "2^24 ntt random")
    check(r.L.h2_dev_intt(buf.data_ptr(), r.scratch().data_ptr(), _vp(r.fr["w_inv"]), _vp(r.fr["d"]), r.log_n, None),
          "h2_dev_intt")
    r.sync()
    r.compare(buf, src, "2^24 intt(ntt(x))")
