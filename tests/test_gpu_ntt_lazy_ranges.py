"""The fixed 8-bit pass (csrc/ntt_pass.hip, k_ntt_pass8) with two reductions of its lazy domain left out: the stage pairs with
twiddles take the row x2 as LDS holds it (below 4p) and multiply the difference taken the other way round, and the first
stage pair of a pass that loads the caller's data takes canonical residues with bare sums (fp_lazy_first_pair_canon,
csrc/field.hpp; the bounds are tests/test_ntt_lazy_ranges_host.py).  Only representatives below 4p change, never a residue:
every output here is compared bit for bit, with the inputs and expected vectors of tests/ntt_matrix_cases.py.

  2^16 (8, 8): a first and a last pass of eight bits -- below 2^18 both are the radix-2 kernel, which shares field.hpp's lazy
  domain (fp_lazy_sub is now one case of the subtraction with an offset) and none of the fixed pass's changes.
  2^19 (3, 8, 8): a middle and a last fixed pass behind a short first pass of the general kernel.
  2^20 (4, 8, 8).
Forward and inverse on random canonical rows, the all-zero vector and all r - 1 (the largest canonical operand in every
place), and one padded call (in_len = n / 2: coeff_to_extended, whose pre3 keeps the reductions of a first pair).

  2^24 (8, 8, 8): the smallest size whose first pass is the fixed kernel, i.e. the only one here that runs the canonical
  first pair.  tests/test_gpu_ntt_tile_ends.py has the random and the all-(r - 1) vector forward against the oracle and the
  round trip; the all-zero vector is added here (every bare sum at its lower end; its transform is zero, no oracle needed)."""
import ctypes

import pytest
import torch

import halo2_gpu_specific_amd as h2
from halo2_gpu_specific_amd._lib import check
from h2util import R_MOD, fr_mont

import ntt_matrix_cases as mc
from ntt_matrix_worker import Runner

pytestmark = pytest.mark.gpu

PASS8_DP, PASS8 = (mc.KERNELS.index(k) for k in ("k_ntt_pass8<true>", "k_ntt_pass8<false>"))
SIZES = {16: [8, 8], 19: [3, 8, 8], 20: [4, 8, 8], 24: [8, 8, 8]}
FIXED = {16: [], 19: [PASS8_DP, PASS8], 20: [PASS8_DP, PASS8], 24: [PASS8_DP, PASS8_DP, PASS8]}   # the fixed passes: the last ones


@pytest.mark.parametrize("log_n", sorted(SIZES))
def test_the_sizes_run_the_fixed_pass_where_the_docstring_says(log_n):
    passes = mc.ntt_shape(h2.lib(), log_n, log_n)
    assert [p["bits"] for p in passes] == SIZES[log_n]
    assert [p["kernel"] for p in passes][len(passes) - len(FIXED[log_n]):] == FIXED[log_n]
    assert PASS8_DP not in [p["kernel"] for p in passes][: len(passes) - len(FIXED[log_n])]


@pytest.fixture(scope="module", params=[16, 19, 20])
def runner(request, oracle):
    return Runner(oracle, request.param)


@pytest.mark.parametrize("inp", ["random", "zero", "rm1"])
@pytest.mark.parametrize("op", ["ntt", "intt"])
def test_forward_and_inverse_bit_exact(runner, op, inp):
    runner.run_cases([mc.Case(op, 0, inp, False)])


def test_a_padded_call(runner):
    runner.run_cases([mc.Case("coeff_to_extended", 1, "random", False)])


def test_2p24_the_canonical_first_pair_on_zeros():
    L, log_n = h2.lib(), 24
    dev = torch.device("cuda", 0)
    buf = torch.zeros((1 << log_n, 4), dtype=torch.int64, device=dev)
    tmp = torch.empty_like(buf)
    w = fr_mont(pow(mc.ROOT_W, 1 << (28 - log_n), R_MOD))
    torch.cuda.synchronize()
    check(L.h2_dev_ntt(buf.data_ptr(), tmp.data_ptr(), w.ctypes.data_as(ctypes.c_void_p), log_n, None), "h2_dev_ntt")
    check(L.h2_synchronize(), "h2_synchronize")
    torch.cuda.synchronize()
    assert not bool(buf.any()), "the transform of the zero vector is not zero"
