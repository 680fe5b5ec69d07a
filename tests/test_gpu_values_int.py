"""The integer half of Values on the device: the kernel's TO_INT, TO_FIELD, EXTRACT, LT, AND, OR and XOR (csrc/values.hip,
h2_dev_values_eval) against its host twin bit for bit and against Python integers (tests/values_int_cases.py) at every row
count around the wave and the workgroup and at one where every lane walks the grid-stride loop twice; the fuzz across the
kinds; the launch accounting of limbs, `strict` and `take` by a Value; LimbDecomposition through check_witness, a proof and
the verifier."""
import numpy as np
import pytest

import values_cases as vc
import values_int_cases as ic
from values_cases import R_MOD

pytestmark = pytest.mark.gpu

S_TRAPDOOR = 0x1D0C5F0A3B7E91C2A4D6F8091B2C3D4E5F60718293A4B5C6D7E8F9010203
SIZES = (1, 63, 64, 65, 255, 256, 257)


@pytest.fixture(scope="module")
def device():
    from halo2_gpu_specific_amd import prover

    return prover.Device()


@pytest.fixture(scope="module")
def caps():
    from halo2_gpu_specific_amd import values

    return values.limits()


def counted(device, fn):
    from halo2_gpu_specific_amd import values

    values._backend(device)
    before = device.values_launches
    out = fn()
    return out, device.values_launches - before


# -- the kernel against its twin and the integers --------------------------------------------------------------------------------
@pytest.mark.parametrize("m", SIZES)
def test_kernel_matches_the_host_twin_and_the_integers(device, m):
    for program in ic.programs(max(ic.SIZES)):
        got = vc.run_device(device, program, m)
        twin = vc.run_host(device.L, program, m)
        assert all(np.array_equal(g, t) for g, t in zip(got, twin)), program.name
        assert program.decode(got) == program.expected(m), program.name


def test_every_lane_walks_the_grid_stride_loop_twice_with_a_ragged_last_pass(device, caps):
    """EXTRACT, LT, XOR and both output forms in one launch of 2 * blocks * threads + 5 rows"""
    m = 2 * caps["blocks"] * caps["threads"] + 5
    program, want = ic.grid_stride_program(m)
    got = vc.run_device(device, program, m)
    twin = vc.run_host(device.L, program, m)
    assert all(np.array_equal(g, t) for g, t in zip(got, twin))
    half = caps["blocks"] * caps["threads"]
    for lo in (0, half - 40, 2 * half - 40, m - 40):
        rows = slice(lo, lo + 40)
        assert program.decode([g[rows] for g in got]) == want(rows)


@pytest.mark.parametrize("m", (1, 64, 257))
def test_fuzz_on_the_device_is_the_fuzz_on_the_host(device, m):
    """50 random expressions across the kinds: device tensors equal to the host backend's arrays bit for bit, and to the integers"""
    from halo2_gpu_specific_amd.values import Value

    upload = lambda a: device.upload(a, widen=False)                       # noqa: E731
    on_device, on_host = vc.fuzz_leaves(device, m, upload), vc.fuzz_leaves(None, m)
    leaf_ints = [x[4] for x in vc.fuzz_inputs(m)]
    for lo in range(0, 50, 4):
        seeds = range(lo, min(lo + 4, 50))
        dev = [ic.fuzz_expression(seed, on_device, leaf_ints) for seed in seeds]
        host = [ic.fuzz_expression(seed, on_host, leaf_ints) for seed in seeds]
        got = [device.download(t) for t in Value.materialize([v for v, _ in dev])]
        twin = Value.materialize([v for v, _ in host])
        for seed, g, t, (_, want) in zip(seeds, got, twin, dev):
            assert np.array_equal(g, t), seed
            assert vc.ints(g) == want, seed


# -- launch accounting ---------------------------------------------------------------------------------------------------------------
def test_limbs_strict_and_take_on_the_device(device, caps):
    import random

    from halo2_gpu_specific_amd.values import Value

    rng = random.Random(3)
    A, B = ([rng.randrange(R_MOD) for _ in range(300)] for _ in range(2))
    a, b = Value.from_ints(device, A), Value.from_ints(device, B)
    got, launches = counted(device, lambda: Value.materialize(a.limbs(8, 4)))
    assert launches == 1 and [vc.ints(device.download(g)) for g in got] == [[(v >> 8 * j) & 0xFF for v in A] for j in range(4)]
    got, launches = counted(device, lambda: Value.materialize((a * b).limbs(8, 32)))
    assert launches == -(-32 // caps["outputs"])
    assert [vc.ints(device.download(g)) for g in got] == [[(p * q % R_MOD >> 8 * j) & 0xFF for p, q in zip(A, B)] for j in range(32)]
    c = Value.from_u64(device, [v & vc.MASK64 for v in A])
    got, launches = counted(device, lambda: Value.materialize(c.limbs(16, 4)))
    assert launches == 1 and [vc.ints(device.download(g)) for g in got] == [[(v & vc.MASK64) >> 16 * j & 0xFFFF for v in A] for j in range(4)]
    # strict: the first row that does not fit is named; rows that fit come out
    small = [v % (1 << 32) for v in A]
    small[211] = 1 << 32
    with pytest.raises(ValueError, match="element 211 of the 300 does not fit 4 limbs of 8 bits"):
        Value.materialize(Value.from_ints(device, small).limbs(8, 4, strict=True))
    got, launches = counted(device, lambda: Value.materialize(a.low(32).limbs(8, 4, strict=True)))
    assert launches == 2 and [vc.ints(device.download(g)) for g in got] == [[(v % (1 << 32) >> 8 * j) & 0xFF for v in A] for j in range(4)]
    # take by a Value of integers: Python's indexing; an index out of range raises before the gather and the table is untouched
    T = [rng.randrange(R_MOD) for _ in range(256)]
    table = Value.from_ints(device, T)
    assert table.take(a.low(8)).to_ints() == [T[v & 0xFF] for v in A]
    assert (table.take(b.bits(100, 8)) + 1).to_ints() == [(T[(v >> 100) & 0xFF] + 1) % R_MOD for v in B]
    before = device.download(table.tensor()).copy()
    index = [v & 0xFF for v in A]
    index[123] = 256
    with pytest.raises(IndexError, match="index 256 at row 123 is out of range for 256 elements"):
        table.take(Value.from_ints(device, index)).to_ints()
    index[123], index[7] = 5, (1 << 64) + 3
    with pytest.raises(IndexError, match="index %d at row 7 is out of range" % ((1 << 64) + 3)):
        table.take(Value.from_ints(device, index)).to_ints()
    index[7] = 1 << 63                                                    # a negative 64-bit word on the device
    with pytest.raises(IndexError, match="at row 7"):
        table.take(Value.from_ints(device, index)).to_ints()
    assert np.array_equal(device.download(table.tensor()), before) and table.to_ints() == T


# -- LimbDecomposition ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", (9, 10))
def test_limb_decomposition_checks_proves_and_verifies(device, k):
    """cannot pass without the feature: this witness exists only as integer Values.  The proof's bytes are those of the same
    circuit over a witness computed on the host with numpy and Python integers"""
    from halo2_gpu_specific_amd import circuits_frontend as fe, prover, verifier
    from halo2_gpu_specific_amd.rng import ProverRng
    from halo2_gpu_specific_amd.values import Value

    circuit = fe.LimbDecomposition(k, device=device)
    H = circuit.height
    params = prover.Params.unsafe_setup(device, k, S_TRAPDOOR)
    cs, fixed, copies = prover.synthesize_keygen(device, circuit, k)
    pk = prover.keygen(device, params, cs, fixed, copies)
    advice, _ = prover.synthesize_witness(device, circuit, pk, k, resident=True)
    a, b = circuit.witness_inputs()
    p = [int(x) * int(y) % (1 << 32) for x, y in zip(a, b)]
    want = [[int(x) for x in a], [int(y) for y in b], p] + [[(v >> 8 * j) & 0xFF for v in p] for j in range(4)]
    for column, values in zip(advice, want):
        assert vc.ints(device.download(column)[:H]) == values
    assert prover.check_witness(device, pk, advice) == ([], 0)
    proof = prover.create_proof_with_shplonk(device, params, pk, [device.clone(c) for c in advice], ProverRng(5))
    vk = verifier.VerifyingKey.from_proving_key(pk)
    assert verifier.verify_proof_with_shplonk(device, verifier.ParamsVerifier.from_params(params), vk, proof)
    on_host = fe.LimbDecomposition(k, device=device, columns=[Value.from_ints(device, values) for values in want])
    advice_host, _ = prover.synthesize_witness(device, on_host, pk, k, resident=True)
    assert bytes(prover.create_proof_with_shplonk(device, params, pk, advice_host, ProverRng(5))) == bytes(proof)
    row = H - 3
    with device.torch.cuda.stream(device.tstream):
        advice[4][row, 0] ^= 1                                             # one limb
    failures, total = prover.check_witness(device, pk, advice)
    assert total >= 1 and any(f.gate_name == "p is the sum of its limbs" and f.row == row for f in failures)
