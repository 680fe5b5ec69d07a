"""The tabulated inter-pass twiddles of a middle pass are applied where the pass before it STORES (csrc/ntt_pass.hip: ST,
store_twiddle; the middle pass then loads finished operands), as chunk products.  Two kernels do that:

  the general first-pass kernel, k_ntt_pass<true, true>: 2^19 (passes 3, 8, 8) and 2^20 (4, 8, 8) are the smallest plans with a
  tabulated middle pass behind it.  Forward, inverse and round trip of four inputs -- a seeded random vector, every element
  r - 1, a single 1 at index 1, only the last element non-zero -- against the oracle's best_fft, element for element; one
  batched call of three vectors at 2^19; at 2^20 one zero-padded call with z = 1 and one with z = B (the first pass skips
  stages and still stores every row) and one coset call (the pre-scale at the load and the new product at the store of the
  same pass);

  the fixed first pass, k_ntt_pass8<true>: 2^24 (8, 8, 8) is the only size below 2^25 whose first pass it is.  One random
  vector forward against the oracle and back again on the device, and the unit vector at index 1 against the twiddle powers
  w^k (and w^-k / n) computed directly by doubling, without any FFT.

The oracle's 2^24 transform takes 1.9 s on 8 threads of an MI355X host (the test prints what it measured) and the device's,
host to host, 0.07 s.  With the oracle's inverse of the random vector as well the test took 4.9 s, so only the forward case is
compared with the oracle; the inverse at this size is covered by the round trip and by intt(e_1) against w^-k / n.
"""
import ctypes
import time

import numpy as np
import pytest

import halo2_gpu_specific_amd as h2
from halo2_gpu_specific_amd import arithmetic as ar
from halo2_gpu_specific_amd._lib import check
from h2util import R_MOD, fr_mont

import ntt_matrix_cases as mc
from ntt_matrix_worker import Runner
from test_gpu_ntt_chunk_twiddles import INPUTS, Expected  # the same inputs and oracle transforms, computed once per session

pytestmark = pytest.mark.gpu

PASS8_DP, PASS8, R4_DP = (mc.KERNELS.index(k) for k in ("k_ntt_pass8<true>", "k_ntt_pass8<false>", "k_ntt_pass<true, true>"))


@pytest.mark.parametrize("log_n,bits,first", [(19, [3, 8, 8], R4_DP), (20, [4, 8, 8], R4_DP), (24, [8, 8, 8], PASS8_DP)])
def test_the_plans_have_a_tabulated_middle_pass_behind_each_first_pass_kernel(log_n, bits, first):
    passes = mc.ntt_shape(h2.lib(), log_n, log_n)
    assert [p["bits"] for p in passes] == bits
    assert [p["kernel"] for p in passes] == [first, PASS8_DP, PASS8]
    if log_n == 20:  # the padded calls below: the first pass skips z stages in the general kernel
        for z in (1, 4):
            assert [(p["zskip"], p["kernel"]) for p in mc.ntt_shape(h2.lib(), log_n, log_n - z)] == [(z, R4_DP), (0, PASS8_DP), (0, PASS8)]


@pytest.mark.parametrize("kind", INPUTS)
@pytest.mark.parametrize("log_n", [19, 20])
def test_forward_inverse_and_round_trip_behind_the_general_first_pass(oracle, log_n, kind):
    e = Expected.get(oracle, log_n)
    x = e.x[kind]
    fwd = ar.best_fft(x.copy(), e.w, log_n)
    assert np.array_equal(fwd, e.fwd[kind]), "forward transform differs from the oracle"
    inv = ar.gpu_ifft(x.copy(), e.w_inv, log_n, e.d)
    assert np.array_equal(inv, e.inv[kind]), "inverse transform differs from the oracle"
    assert np.array_equal(ar.gpu_ifft(fwd, e.w_inv, log_n, e.d), x), "intt(ntt(x)) != x"


def test_three_vectors_in_one_batched_call(oracle):
    import torch

    log_n = 19
    n = 1 << log_n
    e = Expected.get(oracle, log_n)
    L = h2.lib()
    dev = torch.device("cuda", 0)
    kinds = ("random", "rm1", "last")
    bufs = [torch.from_numpy(e.x[k].copy().view(np.int64)).to(dev) for k in kinds]
    tmp = torch.empty((len(kinds) * n, 4), dtype=torch.int64, device=dev)
    ptrs = (ctypes.c_void_p * len(kinds))(*[b.data_ptr() for b in bufs])
    torch.cuda.synchronize()
    check(L.h2_dev_ntt_batch(ptrs, len(kinds), tmp.data_ptr(), e.w.ctypes.data_as(ctypes.c_void_p), log_n, None), "h2_dev_ntt_batch")
    check(L.h2_synchronize(), "h2_synchronize")
    for k, b in zip(kinds, bufs):
        assert np.array_equal(b.cpu().numpy().view(np.uint64), e.fwd[k]), "batched forward transform differs from the oracle: " + k
    check(L.h2_dev_intt_batch(ptrs, len(kinds), tmp.data_ptr(), e.w_inv.ctypes.data_as(ctypes.c_void_p),
                              e.d.ctypes.data_as(ctypes.c_void_p), log_n, None), "h2_dev_intt_batch")
    check(L.h2_synchronize(), "h2_synchronize")
    for k, b in zip(kinds, bufs):
        assert np.array_equal(b.cpu().numpy().view(np.uint64), e.x[k]), "batched intt(ntt(x)) != x: " + k


@pytest.fixture(scope="module")
def runner20(oracle):
    return Runner(oracle, 20)


@pytest.mark.parametrize("z", [1, 4])
def test_zero_padded_call(runner20, z):
    """coeff_to_extended of 2^(20 - z) coefficients: z = 1 and z = B, the matrix's zskip rows, against the oracle's FFT of the
    padded, pre-scaled vector (ntt_matrix_cases.Reference.expected, which also checks eight entries against the definition)"""
    assert z in (1, mc.first_width(h2.lib(), 20))
    runner20.run_cases([mc.Case("coeff_to_extended", z, "random", False)])


def test_coset_call(runner20):
    """x[i] g^i at the load and the next pass's twiddle at the store of the same first pass"""
    runner20.run_cases([mc.Case("coset_ntt", 0, "random", False), mc.Case("coset_ntt", 0, "rm1", False)])


def test_the_fixed_first_pass_at_2p24(oracle):
    log_n = 24
    n = 1 << log_n
    w = pow(mc.ROOT_W, 1 << (28 - log_n), R_MOD)
    w_inv, d = pow(w, -1, R_MOD), pow(n, -1, R_MOD)
    fw, fw_inv, fd = fr_mont(w), fr_mont(w_inv), fr_mont(d)

    x = oracle.random_fr(0x57A0 + log_n, n)
    t0 = time.perf_counter()
    want = oracle.best_fft(x.copy(), fw, log_n, threads=mc.ORACLE_THREADS)
    t1 = time.perf_counter()
    print("oracle best_fft 2^24 on %d threads: %.2f s" % (mc.ORACLE_THREADS, t1 - t0))
    got = ar.best_fft(x.copy(), fw, log_n)
    t2 = time.perf_counter()
    print("device best_fft 2^24, host to host: %.2f s" % (t2 - t1))
    assert np.array_equal(got, want), "forward transform differs from the oracle"
    del want
    assert np.array_equal(ar.gpu_ifft(got, fw_inv, log_n, fd), x), "intt(ntt(x)) != x"
    del x, got

    # e_1 -> w^k, and -> w^-k / n: the powers by doubling (24 elementwise products of the oracle), no FFT
    ref = mc.Reference(oracle, log_n)
    delta = np.zeros((n, 4), dtype=np.uint64)
    delta[1] = fr_mont(1)
    assert np.array_equal(ar.best_fft(delta.copy(), fw, log_n), ref.powers(w)), "ntt(e_1)[k] != w^k"
    inv = ref.powers(w_inv).copy()
    ref.scale(inv, d)
    assert np.array_equal(ar.gpu_ifft(delta, fw_inv, log_n, fd), inv), "intt(e_1)[k] != w^-k / n"
