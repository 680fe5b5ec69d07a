"""The G1 NTT without a GPU: the definitional reference (tests/g1_ntt_reference.py) pinned to the oracle's setup -- which fixes
omega, the order and the n^-1 scale -- and the argument checks of h2_g1_ntt_scratch_bytes / h2_dev_g1_ntt."""
import ctypes

import numpy as np
import pytest

from g1_ntt_reference import dft_scalars, g1_dft, omega
from h2util import R_MOD, fr_mont

import halo2_gpu_specific_amd as h2

TRAPDOOR = 0x1D0C5F0A3B7E91C2A4D6F8091B2C3D4E5F60718293A4B5C6D7E8F9010203


def oracle_setup(oracle, k, s=TRAPDOOR):
    n = 1 << k
    g, gl = np.zeros((n, 8), dtype=np.uint64), np.zeros((n, 8), dtype=np.uint64)
    sm = fr_mont(s)
    oracle.lib.oracle_unsafe_setup(k, sm.ctypes.data, g.ctypes.data, gl.ctypes.data)
    return g, gl


def test_omega_is_the_domain_omega():
    from halo2_gpu_specific_amd import prover

    for k in (0, 1, 5, 12, 28):
        assert omega(k) == prover.Domain(k, 2).omega
        assert pow(omega(k), 1 << k, R_MOD) == 1
        if k:
            assert pow(omega(k), 1 << (k - 1), R_MOD) == R_MOD - 1


def test_inverse_and_forward_scalars_are_inverse_matrices():
    k = 3
    n = 1 << k
    inv, fwd = dft_scalars(k, True), dft_scalars(k, False)
    for i in range(n):
        for j in range(n):
            assert sum(fwd[i][t] * inv[t][j] for t in range(n)) % R_MOD == (1 if i == j else 0)


@pytest.mark.parametrize("k", [0, 1, 2, 3, 4, 6])
def test_reference_reproduces_the_setup_lagrange_basis(oracle, k):
    g, gl = oracle_setup(oracle, k)
    assert np.array_equal(g1_dft(oracle, g, k, inverse=True), gl)
    assert np.array_equal(g1_dft(oracle, gl, k, inverse=False), g)


def test_reference_identity_is_zeros(oracle):
    k = 2
    z = np.zeros((1 << k, 8), dtype=np.uint64)
    assert not g1_dft(oracle, z, k, inverse=True).any()
    assert not g1_dft(oracle, z, k, inverse=False).any()


def test_scratch_bytes():
    L = h2.lib()
    for k in (0, 1, 12, 22, 28):
        assert L.h2_g1_ntt_scratch_bytes(k) == 128 << k
    assert L.h2_g1_ntt_scratch_bytes(29) == 0


def test_g1_ntt_rejects_bad_arguments_without_a_device():
    L = h2.lib()
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.addressof(buf)
    INVALID = 1
    k = 4
    scratch = L.h2_g1_ntt_scratch_bytes(k)
    assert L.h2_dev_g1_ntt(p, p, 29, 1, p, 1 << 40, None) == INVALID               # log_n past the 2-adicity
    assert b"log_n" in L.h2_last_error()
    assert L.h2_dev_g1_ntt(p, p, 1 << 31, 0, p, 1 << 40, None) == INVALID
    assert L.h2_dev_g1_ntt(p, p, k, 2, p, scratch, None) == INVALID                # inverse not 0 or 1
    assert L.h2_dev_g1_ntt(p, p, k, -1, p, scratch, None) == INVALID
    assert b"inverse" in L.h2_last_error()
    assert L.h2_dev_g1_ntt(None, p, k, 1, p, scratch, None) == INVALID             # null pointers
    assert L.h2_dev_g1_ntt(p, None, k, 1, p, scratch, None) == INVALID
    assert L.h2_dev_g1_ntt(p, p, k, 0, None, scratch, None) == INVALID
    assert b"null" in L.h2_last_error()
    assert L.h2_dev_g1_ntt(p, p, k, 1, p, scratch - 1, None) == INVALID            # scratch too small
    assert L.h2_dev_g1_ntt(p, p, 0, 1, p, 127, None) == INVALID
    assert b"scratch" in L.h2_last_error()


def test_params_read_rejects_a_larger_k_before_reading_points(tmp_path):
    """k above the file's is refused from the header alone (no device is touched)"""
    import struct

    from halo2_gpu_specific_amd import formats

    path = tmp_path / "params.bin"
    path.write_bytes(struct.pack("<I", 5))
    with pytest.raises(ValueError):
        formats.params_read(None, str(path), k=6)
