"""Values on the device: the fused evaluator's kernel (csrc/values.hip, h2_dev_values_eval) against its host twin bit for bit
and against Python integers (tests/values_cases.py: the hand programs and the seeded fuzz) at every row count around the wave
and the workgroup and at one where every lane walks the grid-stride loop twice; the slot cap; the launch accounting of staged
divisions; Values through the front end's two assemblies; ShuffleGatesValues against ShuffleGates, and at full height through
check_witness, a proof and the verifier."""
import random

import numpy as np
import pytest

import values_cases as vc
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
    before = (device.values_launches, device.values_inversions)
    out = fn()
    return out, device.values_launches - before[0], device.values_inversions - before[1]


# -- the kernel against its twin and the integers --------------------------------------------------------------------------------
@pytest.mark.parametrize("m", SIZES)
def test_kernel_matches_the_host_twin_and_the_integers(device, caps, m):
    for program in vc.programs(max(vc.SIZES)) + [vc.slot_cap_program(max(vc.SIZES), caps["slots"])]:
        got = vc.run_device(device, program, m)
        twin = vc.run_host(device.L, program, m)
        assert all(np.array_equal(g, t) for g, t in zip(got, twin)), program.name
        assert program.decode(got) == program.expected(m), program.name


def test_every_lane_walks_the_grid_stride_loop_twice_with_a_ragged_last_pass(device, caps):
    """a launch starts min(ceil(m / threads), blocks) workgroups: from 2 * blocks * threads rows on every lane takes two rows
    at least, and 5 more leave the last pass ragged"""
    m = 2 * caps["blocks"] * caps["threads"] + 5
    rng = np.random.Generator(np.random.PCG64(7))
    canonical = rng.integers(0, 1 << 64, size=(m + 3, 4), dtype=np.uint64)            # any 256-bit integers
    compact = rng.integers(0, 1 << 64, size=2 * m, dtype=np.uint64)
    leaves = [vc.Leaf(canonical, vc.CANONICAL, 3, 1), vc.Leaf(compact, vc.COMPACT, 1, 2)]
    ops = [(vc.MUL, 0, vc.LEAF | 0, vc.LEAF | 1, 0), (vc.ADD, 1, vc.SLOT | 0, vc.LEAF | 0, 0), (vc.SQR, 2, vc.SLOT | 1, 0, 0),
           (vc.SUB, 0, vc.SLOT | 2, vc.CONST | 0, 0)]
    program = vc.Program("long", leaves, [R_MOD - 5], ops, [(0, vc.CANONICAL), (1, vc.MONTGOMERY)])
    got = vc.run_device(device, program, m)
    twin = vc.run_host(device.L, program, m)
    assert all(np.array_equal(g, t) for g, t in zip(got, twin))
    # the twin against the integers where the passes meet and end (the whole range at small m is the test above)
    half = caps["blocks"] * caps["threads"]
    for lo in (0, half - 40, 2 * half - 40, m - 40):
        rows = slice(lo, lo + 40)
        x = [v % R_MOD for v in vc.ints(canonical[3:][rows])]
        y = [int(v) for v in compact[1::2][rows]]
        s = [(p * q + p) % R_MOD for p, q in zip(x, y)]
        assert vc.ints(got[0][rows]) == [(v * v + 5) % R_MOD for v in s]
        assert [v * vc.R_INV % R_MOD for v in vc.ints(got[1][rows])] == s


@pytest.mark.parametrize("m", SIZES)
def test_fuzz_on_the_device_is_the_fuzz_on_the_host(device, m):
    """300 random expressions: device tensors equal to the host backend's arrays bit for bit, and to the integers"""
    from halo2_gpu_specific_amd.values import Value

    upload = lambda a: device.upload(a, widen=False)                       # noqa: E731
    on_device, on_host = vc.fuzz_leaves(device, m, upload), vc.fuzz_leaves(None, m)
    leaf_ints = [x[4] for x in vc.fuzz_inputs(m)]
    for lo in range(0, 300, 4):
        seeds = range(lo, min(lo + 4, 300))
        dev = [vc.fuzz_expression(seed, on_device, leaf_ints) for seed in seeds]
        host = [vc.fuzz_expression(seed, on_host, leaf_ints) for seed in seeds]
        got = [device.download(t) for t in Value.materialize([v for v, _ in dev])]
        twin = Value.materialize([v for v, _ in host])
        for seed, g, t, (_, want) in zip(seeds, got, twin, dev):
            assert np.array_equal(g, t), seed
            assert vc.ints(g) == want, seed


def test_a_program_at_the_slot_cap_and_a_slot_read_long_after(device, caps):
    """every slot written by all four waves of a workgroup, 40 ops over slot 0, then every slot read again; three workgroups"""
    program = vc.slot_cap_program(700, caps["slots"])
    got = vc.run_device(device, program, 700)
    assert all(np.array_equal(g, t) for g, t in zip(got, vc.run_host(device.L, program, 700)))
    assert program.decode(got) == program.expected(700)


# -- launch accounting ---------------------------------------------------------------------------------------------------------------
def test_divisions_cost_one_launch_and_one_inversion_per_depth(device):
    from halo2_gpu_specific_amd.values import Value

    rng = random.Random(3)
    A, B, C = ([rng.randrange(R_MOD) for _ in range(300)] for _ in range(3))
    B[7] = 0
    a, b, c = (Value.from_ints(device, x) for x in (A, B, C))
    inv = lambda x: pow(x, -1, R_MOD) if x else 0                         # noqa: E731
    got, launches, inversions = counted(device, (a / b + b / c + c / a).to_ints)
    assert (launches, inversions) == (2, 1) and got == [(p * inv(q) + q * inv(s) + s * inv(p)) % R_MOD for p, q, s in zip(A, B, C)]
    got, launches, inversions = counted(device, (a / (b + c / a)).to_ints)
    assert (launches, inversions) == (3, 2) and got == [p * inv((q + s * inv(p)) % R_MOD) % R_MOD for p, q, s in zip(A, B, C)]
    # the form the batch inversion works in: x * x.invert() == 1, and 0 where x = 0; strict names the row
    assert (b * b.invert()).to_ints() == [int(q != 0) for q in B]
    with pytest.raises(ZeroDivisionError, match="element 7 of the 300"):
        b.invert(strict=True).to_ints()
    z = [3]
    for p in A:
        z.append(z[-1] * p % R_MOD)
    assert a.cumprod(3).to_ints() == z and a.cumsum(9).to_ints()[-1] == (9 + sum(A)) % R_MOD
    order = list(range(300))
    rng.shuffle(order)
    assert (a.take(order) - 1).to_ints() == [(A[i] - 1) % R_MOD for i in order]
    assert Value.concat([a[:5], b, c[::100]]).to_ints() == A[:5] + B + C[::100]
    assert a[1:299:7].tensor(montgomery=True).is_cuda and len(a[1:299:7].tensor()) == 43


# -- the front end -------------------------------------------------------------------------------------------------------------------
def products_circuit(a, b, count):
    from halo2_gpu_specific_amd import synthesis as syn
    from halo2_gpu_specific_amd.values import Value

    class Products(syn.Circuit):
        """c = a * b over `count` rows, then d = c[::2] + 1 computed from the assigned cells' own values"""
        planner = syn.V1
        cells = None

        def without_witnesses(self):
            return products_circuit(Value.unknown(count), Value.unknown(count), count)

        def configure(self, cs):
            return [cs.advice_column() for _ in range(4)]

        def synthesize(self, config, layouter):
            def body(region):
                ca = region.assign_advice(config[0], 0, a, count=count)
                cb = region.assign_advice(config[1], 0, b, count=count)
                cc = region.assign_advice(config[2], 0, ca.value() * cb.value())
                region.assign_advice(config[3], 1, cc[::2].value() + 1, stride=2)
                region.assign_advice(config[3], 3, 99)                  # a later overlapping assignment wins
                Products.cells = cc

            layouter.assign_region("products", body)

    return Products()


def test_values_through_both_assemblies(device):
    from halo2_gpu_specific_amd import prover
    from halo2_gpu_specific_amd.values import Value

    rng = random.Random(4)
    count, k = 300, 9
    A, B = ([rng.randrange(R_MOD) for _ in range(count)] for _ in range(2))
    circuit = products_circuit(Value.from_ints(device, A), Value.from_u64(device, [b & vc.MASK64 for b in B]), count)
    cs, fixed, copies = prover.synthesize_keygen(device, circuit, k)
    cs_none, _, copies_none = prover.synthesize_keygen(device, products_circuit(None, None, count), k)
    assert np.array_equal(copies, copies_none) and (cs.num_advice, cs.num_fixed) == (cs_none.num_advice, cs_none.num_fixed)
    resident, first = prover.synthesize_witness(device, circuit, cs, k, resident=True)
    host, host_first = prover.synthesize_witness(device, circuit, cs, k, resident=False)
    assert first == host_first and all(np.array_equal(device.download(r), h) for r, h in zip(resident, host))
    C = [p * (q & vc.MASK64) % R_MOD for p, q in zip(A, B)]
    assert vc.ints(host[2][:count]) == C
    want_d = [0] * (1 << k)
    want_d[1:count + 1:2] = [(c + 1) % R_MOD for c in C[::2]]
    want_d[3] = 99
    assert vc.ints(host[3]) == want_d
    cells = type(circuit).cells                                          # cells.value() round-trips and slices
    assert cells.value().to_ints() == C and cells[5:200:13].value().to_ints() == C[5:200:13] and cells[-1].value().to_ints() == [C[-1]]


def test_a_chip_over_cell_values_reproduces_simple_example(device):
    from halo2_gpu_specific_amd import circuits_frontend as fe, prover
    from halo2_gpu_specific_amd.values import Value

    class ValueChip(fe._Chip):
        """numbers are cells: the value travels with them (`AssignedCell::value()`)"""

        def load_private(self, layouter, value):
            return layouter.assign_region("load private", lambda region: region.assign_advice(self.config.advice[0], 0, value, count=1))

        def load_constant(self, layouter, constant):
            return layouter.assign_region("load constant", lambda region: region.assign_advice_from_constant(self.config.advice[0], 0, constant))

        def mul(self, layouter, a, b):
            def body(region):
                self.config.s_mul.enable(region, 0)
                fe._copy_advice(region, a, a.value(), self.config.advice[0], 0)
                fe._copy_advice(region, b, b.value(), self.config.advice[1], 0)
                return region.assign_advice(self.config.advice[0], 1, a.value() * b.value())

            return layouter.assign_region("mul", body)

        def expose_public(self, layouter, num, row):
            layouter.constrain_instance(num, self.config.instance, row)

    class SimpleExampleValues(fe.SimpleExample):
        def without_witnesses(self):
            return SimpleExampleValues(self.constant, Value.unknown(1), Value.unknown(1))

        def synthesize(self, config, layouter):
            chip = ValueChip(config)
            a = chip.load_private(layouter.namespace("load a"), self.a)
            b = chip.load_private(layouter.namespace("load b"), self.b)
            constant = chip.load_constant(layouter.namespace("load constant"), self.constant)
            ab = chip.mul(layouter.namespace("a * b"), a, b)
            absq = chip.mul(layouter.namespace("ab * ab"), ab, ab)
            c = chip.mul(layouter.namespace("constant * absq"), constant, absq)
            chip.expose_public(layouter.namespace("expose c"), c, 0)

    k = 4
    old = fe.SimpleExample()
    new = SimpleExampleValues(7, Value.from_u64(device, [2]), Value.from_ints(device, [3]))
    cs, fixed, copies = prover.synthesize_keygen(device, old, k)
    cs2, fixed2, copies2 = prover.synthesize_keygen(device, new, k)
    assert np.array_equal(copies, copies2) and all(np.array_equal(x, y) for x, y in zip(fixed, fixed2))
    advice, _ = prover.synthesize_witness(device, old, cs, k, resident=True, instances=old.public_inputs())
    advice2, _ = prover.synthesize_witness(device, new, cs2, k, resident=True, instances=old.public_inputs())
    assert all(np.array_equal(device.download(x), device.download(y)) for x, y in zip(advice, advice2))


# -- ShuffleGatesValues ----------------------------------------------------------------------------------------------------------------
def test_shuffle_gates_values_equals_shuffle_gates_cell_for_cell(device):
    """cannot pass without the feature: this witness exists only as Values"""
    from halo2_gpu_specific_amd import circuits_frontend as fe, prover

    k = 6
    old, new = fe.ShuffleGates(k), fe.ShuffleGatesValues(k, height=32, device=device)
    cs, fixed, copies = prover.synthesize_keygen(device, old, k)
    cs2, fixed2, copies2 = prover.synthesize_keygen(device, new, k)
    assert np.array_equal(copies, copies2) and all(np.array_equal(x, y) for x, y in zip(fixed, fixed2))
    advice, first = prover.synthesize_witness(device, old, cs, k, resident=True)
    (advice2, first2), launches, inversions = counted(device, lambda: prover.synthesize_witness(device, new, cs2, k, resident=True))
    assert first == first2 and (launches, inversions) == (3, 1)
    assert all(np.array_equal(device.download(x), device.download(y)) for x, y in zip(advice, advice2))


def test_shuffle_gates_values_at_full_height_checks_proves_and_verifies(device):
    from halo2_gpu_specific_amd import circuits_frontend as fe, prover, verifier
    from halo2_gpu_specific_amd.rng import ProverRng

    k = 10
    height = (1 << k) - 7                                                  # usable - 1
    circuit = fe.ShuffleGatesValues(k, height=height, device=device)
    params = prover.Params.unsafe_setup(device, k, S_TRAPDOOR)
    cs, fixed, copies = prover.synthesize_keygen(device, circuit, k)
    pk = prover.keygen(device, params, cs, fixed, copies)
    advice, _ = prover.synthesize_witness(device, circuit, pk, k, resident=True)
    assert circuit.columns()[-1][height].to_ints() == [1]
    assert vc.ints(device.download(advice[8])[height:height + 1]) == [1]
    assert prover.check_witness(device, pk, advice) == ([], 0)
    proof = prover.create_proof_with_shplonk(device, params, pk, [device.clone(c) for c in advice], ProverRng(5))
    assert verifier.verify_proof_with_shplonk(device, verifier.ParamsVerifier.from_params(params), verifier.VerifyingKey.from_proving_key(pk), proof)
    with device.torch.cuda.stream(device.tstream):
        advice[1][500, 0] ^= 1                                             # one original cell
    failures, total = prover.check_witness(device, pk, advice)
    assert total == 1 and failures[0].gate_name == "z should have valid transition" and failures[0].row == 500
