"""The fixed 8-bit pass (k_ntt_pass8) multiplies by its butterfly twiddles through chunk tables (fp_mul_chunk, csrc/field.hpp).
2^19 (passes 3, 8, 8) and 2^20 (4, 8, 8) are the smallest transforms whose plans hold that pass in both its instantiations,
the middle one and the last: forward and inverse transforms of four inputs -- a seeded random vector, every element r - 1, a
single 1 at index 1 (every output a pure twiddle power) and a vector that is zero except for its last element -- against
the oracle's FFT, element for element, and back again; one batched call of three vectors at 2^19 (blockIdx.y)."""
import ctypes

import numpy as np
import pytest

import halo2_gpu_specific_amd as h2
from halo2_gpu_specific_amd import arithmetic as ar
from halo2_gpu_specific_amd._lib import check
from h2util import R_MOD, fr_mont

import ntt_matrix_cases as mc

pytestmark = pytest.mark.gpu

INPUTS = ("random", "rm1", "delta1", "last")
PASS8_DP, PASS8 = mc.KERNELS.index("k_ntt_pass8<true>"), mc.KERNELS.index("k_ntt_pass8<false>")


def _input(oracle, kind, log_n):
    n = 1 << log_n
    if kind == "random":
        return oracle.random_fr(0xC4A0 + log_n, n)
    x = np.zeros((n, 4), dtype=np.uint64)
    if kind == "rm1":
        x[:] = fr_mont(R_MOD - 1)
    elif kind == "delta1":
        x[1] = fr_mont(1)
    else:
        x[n - 1] = fr_mont(0x1234567 % R_MOD)
    return x


class Expected:
    """per size: the inputs with their forward and inverse transforms by the oracle, computed once"""
    _by_size = {}

    @classmethod
    def get(cls, oracle, log_n):
        if log_n not in cls._by_size:
            cls._by_size[log_n] = cls(oracle, log_n)
        return cls._by_size[log_n]

    def __init__(self, oracle, log_n):
        n = 1 << log_n
        w = pow(mc.ROOT_W, 1 << (28 - log_n), R_MOD)
        self.w, self.w_inv, self.d = fr_mont(w), fr_mont(pow(w, -1, R_MOD)), fr_mont(pow(n, -1, R_MOD))
        self.x, self.fwd, self.inv = {}, {}, {}
        for kind in INPUTS:
            x = _input(oracle, kind, log_n)
            self.x[kind] = x
            self.fwd[kind] = oracle.best_fft(x.copy(), self.w, log_n, threads=mc.ORACLE_THREADS)
            inv = oracle.best_fft(x.copy(), self.w_inv, log_n, threads=mc.ORACLE_THREADS)
            oracle.lib.oracle_poly_scale(inv.ctypes.data, self.d.ctypes.data, n, mc.ORACLE_THREADS)
            self.inv[kind] = inv
        for a in list(self.x.values()) + list(self.fwd.values()) + list(self.inv.values()):
            a.setflags(write=False)


@pytest.mark.parametrize("log_n,first", [(19, 3), (20, 4)])
def test_the_fixed_pass_runs_in_both_instantiations(log_n, first):
    passes = mc.ntt_shape(h2.lib(), log_n, log_n)
    assert [p["bits"] for p in passes] == [first, 8, 8]
    assert [p["kernel"] for p in passes[1:]] == [PASS8_DP, PASS8]
    assert all(p["fixed"] for p in passes[1:])


@pytest.mark.parametrize("kind", INPUTS)
@pytest.mark.parametrize("log_n", [19, 20])
def test_forward_and_inverse_against_the_oracle(oracle, log_n, kind):
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
    kinds = ("random", "rm1", "delta1")
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
