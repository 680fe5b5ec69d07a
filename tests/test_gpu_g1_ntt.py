"""h2_dev_g1_ntt and what is built on it -- Params.from_powers, Params.downsize, formats.params_read(k=...) -- against the
oracle's setup, the definitional DFT of tests/g1_ntt_reference.py and proofs made with unsafe_setup's parameters."""
import gc

import numpy as np
import pytest

from g1_ntt_reference import g1_dft, g1_mul, g1_neg
from h2util import R_MOD
from test_g1_ntt_host import oracle_setup
from test_plonk_host import S_TRAPDOOR

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def device():
    from halo2_gpu_specific_amd import prover

    D = prover.Device()
    yield D
    gc.collect()          # the module's parameters (and their shifted-base tables) go with it


def ntt(D, pts, k, inverse, in_place=False):
    """h2_dev_g1_ntt of host points -> host points"""
    from halo2_gpu_specific_amd import prover

    t = D.upload(np.ascontiguousarray(pts, dtype=np.uint64))
    if in_place:
        torch = D.torch
        with torch.cuda.stream(D.tstream):
            scratch = torch.empty(D.L.h2_g1_ntt_scratch_bytes(k), dtype=torch.uint8, device=D.dev)
        prover.check(D.L.h2_dev_g1_ntt(t.data_ptr(), t.data_ptr(), k, int(inverse), scratch.data_ptr(), scratch.numel(),
                                       D.stream), "h2_dev_g1_ntt")
        out = t
    else:
        out = prover.g1_ntt(D, t, k, inverse)
    return D.download(out).reshape(-1, 8)


def generator():
    from h2util import points_to_arr

    return points_to_arr([(1, 2)])[0]


@pytest.mark.parametrize("k", [1, 2, 3, 5, 8, 12, 16])
def test_from_powers_equals_the_oracle_setup(device, oracle, k):
    from halo2_gpu_specific_amd import prover

    g, gl = oracle_setup(oracle, k)
    P = prover.Params.from_powers(device, k, g, tables=False)
    assert np.array_equal(device.download(P.g_lagrange).reshape(-1, 8), gl)
    assert np.array_equal(device.download(P.g).reshape(-1, 8), g)


@pytest.mark.parametrize("k", [18, 20, 22])
def test_large_transforms_against_unsafe_setup(device, k):
    from halo2_gpu_specific_amd import prover

    P = prover.Params.unsafe_setup(device, k, S_TRAPDOOR)
    torch = device.torch
    lag = prover.g1_ntt(device, P.g, k, inverse=True)
    back = prover.g1_ntt(device, P.g_lagrange, k, inverse=False)
    with torch.cuda.stream(device.tstream):
        assert torch.equal(lag, P.g_lagrange)
        assert torch.equal(back, P.g)
    del P, lag, back
    gc.collect()


@pytest.mark.parametrize("k", range(1, 9))
def test_random_points_against_the_definition(device, oracle, k):
    pts = oracle.random_g1(0x6E77 + k, 1 << k)
    for inverse in (True, False):
        assert np.array_equal(ntt(device, pts, k, inverse), g1_dft(oracle, pts, k, inverse)), ("inverse" if inverse else
                                                                                               "forward")


@pytest.mark.parametrize("k", [4, 7])
def test_exceptional_inputs(device, oracle, k):
    n = 1 << k
    G = generator()
    O = np.zeros(8, dtype=np.uint64)
    zeros = np.zeros((n, 8), dtype=np.uint64)
    # all identity
    for inverse in (True, False):
        assert not ntt(device, zeros, k, inverse).any()
    # a constant point: inverse [G, O, ...], forward [nG, O, ...] (stage 0 doubles and cancels)
    const = np.tile(G, (n, 1))
    want = zeros.copy()
    want[0] = G
    assert np.array_equal(ntt(device, const, k, True), want)
    want[0] = g1_mul(oracle, G, n)
    assert np.array_equal(ntt(device, const, k, False), want)
    # a delta: inverse every point [n^-1] G, forward every point G
    delta = zeros.copy()
    delta[0] = G
    assert np.array_equal(ntt(device, delta, k, True), np.tile(g1_mul(oracle, G, pow(n, -1, R_MOD)), (n, 1)))
    assert np.array_equal(ntt(device, delta, k, False), const)
    # a shifted delta's transform back to the delta: every stage meets A = w B or A = -w B with w != 1
    j0 = 3
    w = pow(0x03DDB9F5166D18B798865EA93DD31F743215CF6DD39329C8D34F1ED960C37C9C, 1 << (28 - k), R_MOD)
    wave = np.array([g1_mul(oracle, G, pow(w, i * j0, R_MOD)) for i in range(n)])
    shifted = zeros.copy()
    shifted[j0] = G
    assert np.array_equal(ntt(device, wave, k, True), shifted)
    # pairs P, -P that meet in one butterfly (j and j + n/2 share the first stage): cancellations and doublings
    rnd = oracle.random_g1(0xCA9CE1 + k, n // 2)
    pairs = np.concatenate([rnd, g1_neg(rnd)])
    for inverse in (True, False):
        assert np.array_equal(ntt(device, pairs, k, inverse), g1_dft(oracle, pairs, k, inverse))
    # identity points at random positions
    rng = np.random.default_rng(k)
    holes = oracle.random_g1(0x401E + k, n)
    holes[rng.random(n) < 0.4] = O
    for inverse in (True, False):
        assert np.array_equal(ntt(device, holes, k, inverse), g1_dft(oracle, holes, k, inverse))
    # d_out == d_in
    for inverse in (True, False):
        assert np.array_equal(ntt(device, holes, k, inverse, in_place=True), ntt(device, holes, k, inverse))


def test_one_point(device, oracle):
    G = generator()[None, :]
    for inverse in (True, False):
        assert np.array_equal(ntt(device, G, 0, inverse), G)
        assert np.array_equal(ntt(device, G, 0, inverse, in_place=True), G)
        assert not ntt(device, np.zeros((1, 8), dtype=np.uint64), 0, inverse).any()


def test_downsize_equals_unsafe_setup(device):
    from halo2_gpu_specific_amd import prover

    torch = device.torch
    big = prover.Params.unsafe_setup(device, 20, S_TRAPDOOR)
    assert big.downsize(device, 20) is big
    with torch.cuda.stream(device.tstream):
        g0, gl0 = big.g.clone(), big.g_lagrange.clone()
    for k in (8, 12, 16):
        small = big.downsize(device, k)
        ref = prover.Params.unsafe_setup(device, k, S_TRAPDOOR)
        assert small.k == k and small.n == 1 << k
        with torch.cuda.stream(device.tstream):
            assert torch.equal(small.g, ref.g)
            assert torch.equal(small.g_lagrange, ref.g_lagrange)
        # the child's g is an allocation of its own, not a view of the parent's
        assert small.g.untyped_storage().data_ptr() != big.g.untyped_storage().data_ptr()
        assert small.g.untyped_storage().nbytes() == 64 << k
    device.sync()
    with torch.cuda.stream(device.tstream):
        assert torch.equal(big.g, g0) and torch.equal(big.g_lagrange, gl0)
    with pytest.raises(ValueError):
        big.downsize(device, 21)


def test_proofs_with_downsized_params(device):
    from halo2_gpu_specific_amd import circuits, prover
    from halo2_gpu_specific_amd.rng import ProverRng

    k = 8
    direct = prover.Params.unsafe_setup(device, k, S_TRAPDOOR)
    derived = prover.Params.unsafe_setup(device, 12, S_TRAPDOOR).downsize(device, k)
    adv, fixed, copies = circuits.mini_plonk_synthesize(k)
    proofs = []
    for params in (direct, derived):
        pk = prover.keygen(device, params, circuits.mini_plonk(), fixed, copies)
        proofs.append((prover.create_proof_with_shplonk(device, params, pk, adv, ProverRng(5)),
                       prover.create_proof(device, params, pk, adv, ProverRng(6))))
    assert proofs[0] == proofs[1]


def test_params_read_prefix(device, tmp_path):
    from halo2_gpu_specific_amd import formats, prover

    torch = device.torch
    big = prover.Params.unsafe_setup(device, 16, S_TRAPDOOR)
    path = str(tmp_path / "params16.bin")
    extra = bytes(range(64)) + b"[s]G2"
    formats.params_write(device, big, path, extra)
    small, add = formats.params_read(device, path, k=12)
    ref = prover.Params.unsafe_setup(device, 12, S_TRAPDOOR)
    assert small.k == 12 and add == extra
    with torch.cuda.stream(device.tstream):
        assert torch.equal(small.g, ref.g) and torch.equal(small.g_lagrange, ref.g_lagrange)
    for k in (None, 16):
        whole, add = formats.params_read(device, path, k=k)
        assert whole.k == 16 and add == extra
        with torch.cuda.stream(device.tstream):
            assert torch.equal(whole.g, big.g) and torch.equal(whole.g_lagrange, big.g_lagrange)
    with pytest.raises(ValueError):
        formats.params_read(device, path, k=17)
    raw = open(path, "rb").read()
    for cut in (4 + 32 * 1000, 4 + 64 * (1 << 16) + 2, len(raw) - 1):      # inside g's prefix, in the length, in the data
        short = str(tmp_path / ("cut%d.bin" % cut))
        open(short, "wb").write(raw[:cut])
        with pytest.raises(IOError):
            formats.params_read(device, short, k=12)
