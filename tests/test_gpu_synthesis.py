"""The circuit front end on the device (synthesis.DeviceColumns over h2_dev_cells_place, csrc/place.hip).

The placement kernel against a sequential numpy placement, bit for bit: every count around the wave (64) and workgroup (256)
sizes, strides 1 .. 3, the three source forms, host and device-tensor sources, canonical and Montgomery output, segments that
end at row n - 1, thousands of one-cell segments in one launch, overlapping assignments (the later one wins), compact values
above 2^63 and canonical values just below the modulus.

Proofs: a circuit synthesised through the front end on the device proves to the same bytes as its hand-laid twin of
circuits.py, both multiopen schemes, and the project's verifier accepts them.  check_witness is silent on a synthesised
witness and names the row the planner gave an altered cell."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

S_TRAPDOOR = 0x1D0C5F0A3B7E91C2A4D6F8091B2C3D4E5F60718293A4B5C6D7E8F9010203
R_MOD = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001
MASK = (1 << 64) - 1
SENTINEL = 0x5A5A5A5A5A5A5A5A
COUNTS = (0, 1, 2, 63, 64, 65, 255, 256, 257, None)                      # None = as many as the stride lets into n rows
STRIDES = (1, 2, 3)


@pytest.fixture(scope="module")
def device():
    from halo2_gpu_specific_amd import prover

    return prover.Device()


@pytest.fixture(scope="module")
def setups(device):
    from halo2_gpu_specific_amd import prover, verifier

    made = {}

    def get(k):
        if k not in made:
            params = prover.Params.unsafe_setup(device, k, S_TRAPDOOR)
            made[k] = (params, verifier.ParamsVerifier.from_params(params))
        return made[k]

    return get


def limbs(v):
    return [(v >> (64 * j)) & MASK for j in range(4)]


def canonical_values(rng, count):
    """`count` field elements as (count, 4) u64: random ones, with r - 1, r - 2 and 2^64 among them"""
    vals = [int.from_bytes(rng.bytes(32), "little") % R_MOD for _ in range(count)]
    for at, special in zip(range(0, count, 7), (R_MOD - 1, R_MOD - 2, 1 << 64, 0)):
        vals[at] = special
    return np.array([limbs(v) for v in vals], dtype=np.uint64).reshape(count, 4)


def compact_values(rng, count):
    """`count` u64 values, 2^64 - 1, 2^63 and 2^63 + 1 among them"""
    vals = rng.integers(0, 1 << 64, size=count, dtype=np.uint64)
    for at, special in zip(range(0, count, 5), (MASK, 1 << 63, (1 << 63) + 1, 0)):
        vals[at] = special
    return vals


def to_montgomery(cells):
    out = np.empty_like(cells)
    for i, row in enumerate(cells):
        out[i] = limbs((sum(int(x) << (64 * j) for j, x in enumerate(row)) << 256) % R_MOD)
    return out


class Batch:
    """assignments for synthesis.DeviceColumns with the sequential numpy placement of the same cells next to them"""

    def __init__(self, device, columns, n, montgomery):
        from halo2_gpu_specific_amd import synthesis

        self.D, self.n, self.montgomery = device, n, montgomery
        self.dev = synthesis.DeviceColumns(device, columns, n, montgomery)
        with device.torch.cuda.stream(device.tstream):
            for t in self.dev.columns:                                   # whatever is not assigned must stay as it was
                t.fill_(SENTINEL)
        device.sync()
        self.want = np.full((columns, n, 4), SENTINEL, dtype=np.uint64)

    def place(self, column, row, stride, values, count=None, on_device=False):
        from halo2_gpu_specific_amd import synthesis

        if isinstance(values, int):
            cells = np.tile(np.array(limbs(values), dtype=np.uint64), (count, 1))
        else:
            cells = values if values.ndim == 2 else np.concatenate([values[:, None], np.zeros((len(values), 3), dtype=np.uint64)], axis=1)
            count = None
        if len(cells):
            self.want[column, row:row + (len(cells) - 1) * stride + 1:stride] = to_montgomery(cells) if self.montgomery else cells
        if on_device:
            values = self.D.torch.from_numpy(values.view(np.int64)).to(self.D.dev)
        self.dev.place(column, row, stride, synthesis._Values(values, count))

    def check(self, flushes=None):
        got = [self.D.download(t) for t in self.dev.finish()]
        if flushes is not None:
            assert self.dev.flushes == flushes
        for column, have in enumerate(got):
            bad = np.flatnonzero((have != self.want[column]).any(axis=1))
            assert len(bad) == 0, "column %d differs at rows %s" % (column, bad[:8])


@pytest.mark.parametrize("montgomery", [False, True], ids=["canonical", "montgomery"])
@pytest.mark.parametrize("log_n", [10, 12])
def test_placement_matches_sequential_numpy_placement(device, log_n, montgomery):
    """one launch: every count x stride x (canonical | compact) x (host | device source), and broadcast; one column each, the
    odd ones pushed down so that they end at row n - 1"""
    n = 1 << log_n
    rng = np.random.Generator(np.random.PCG64(100 + log_n))
    kinds = ("canonical", "canonical-device", "compact", "compact-device", "broadcast")
    cases = [(count, stride, kind) for count in COUNTS for stride in STRIDES for kind in kinds]
    batch = Batch(device, len(cases), n, montgomery)
    for column, (count, stride, kind) in enumerate(cases):
        fits = (n - 1) // stride + 1
        count = fits if count is None else count
        assert count <= fits
        row = n - 1 - (count - 1) * stride if column % 2 and count else 0
        if kind == "broadcast":
            batch.place(column, row, stride, int.from_bytes(rng.bytes(32), "little") % R_MOD if column % 3 else R_MOD - 1, count)
        else:
            values = canonical_values(rng, count) if kind.startswith("canonical") else compact_values(rng, count)
            batch.place(column, row, stride, values, on_device=kind.endswith("device"))
    batch.check(flushes=1)
    assert batch.dev.cells_placed == sum(int((batch.want[c] != SENTINEL).any(axis=1).sum()) for c in range(len(cases)))


def test_five_thousand_one_cell_segments_in_one_launch(device):
    n, columns = 1 << 12, 2
    rng = np.random.Generator(np.random.PCG64(7))
    batch = Batch(device, columns, n, False)
    for i, cell in enumerate(rng.permutation(columns * n)[:5000]):
        column, row = int(cell) // n, int(cell) % n
        if i % 3 == 0:
            batch.place(column, row, 1, int.from_bytes(rng.bytes(32), "little") % R_MOD, 1)
        elif i % 3 == 1:
            batch.place(column, row, 1, compact_values(rng, 1))
        else:
            batch.place(column, row, 1, canonical_values(rng, 1))
    batch.check(flushes=1)


def test_a_later_assignment_of_a_cell_wins(device):
    n = 1 << 10
    rng = np.random.Generator(np.random.PCG64(9))
    batch = Batch(device, 3, n, False)
    batch.place(0, 0, 1, compact_values(rng, 100))
    batch.place(1, 0, 2, compact_values(rng, 64))                        # rows 0, 2, ...: the odd rows below interleave
    batch.place(1, 1, 2, compact_values(rng, 64))
    batch.place(2, 5, 1, 11, 1)
    assert batch.dev.flushes == 0
    batch.place(0, 50, 1, canonical_values(rng, 100))                    # rows 50 .. 99 again: the queue goes out first
    assert batch.dev.flushes == 1
    batch.place(2, 5, 1, 12, 1)                                          # (2, 5) went out with that launch: nothing queued there
    assert batch.dev.flushes == 1
    batch.place(2, 0, 5, compact_values(rng, 3))                         # rows 0, 5, 10: over the queued single cell
    assert batch.dev.flushes == 2
    batch.place(0, 149, 3, 13, 4)                                        # rows 149, 152, ...: placed by launch 1, not queued
    assert batch.dev.flushes == 2
    batch.place(0, 150, 1, canonical_values(rng, 5))                     # row 152 is queued
    assert batch.dev.flushes == 3
    batch.check(flushes=4)


def test_bad_segments_are_refused_before_any_launch(device):
    from halo2_gpu_specific_amd import synthesis
    from halo2_gpu_specific_amd._lib import H2Error, check

    n = 1 << 10
    column, scratch = device.zeros(n), device.scratch(1 << 12)
    source = device.zeros(4)

    def call(first_row, stride, count, form=0, out=0, dst=None, src=None):
        segs = np.zeros(1, dtype=synthesis.PLACE_SEGMENT)
        segs[0] = (column.data_ptr() if dst is None else dst, source.data_ptr() if src is None else src, first_row, stride, count, form, 0)
        return device.L.h2_dev_cells_place(segs.ctypes.data, 1, n, out, scratch.data_ptr(), 1 << 12, device.stream)

    assert call(n - 4, 1, 4) == 0
    for bad in (dict(first_row=n - 3, stride=1, count=4), dict(first_row=0, stride=0, count=2), dict(first_row=n, stride=1, count=1),
                dict(first_row=1, stride=n // 2, count=3), dict(first_row=0, stride=1, count=1, form=3),
                dict(first_row=0, stride=1, count=1, out=2), dict(first_row=0, stride=1, count=1, dst=column.data_ptr() + 8),
                dict(first_row=0, stride=1, count=1, src=0)):
        assert call(**bad) != 0, bad
    device.sync()
    assert not device.download(column)[:n - 4].any()
    with pytest.raises(H2Error, match="stride"):
        check(call(0, 0, 2), "h2_dev_cells_place")


# ---- proofs through the front end ---------------------------------------------------------------------------------------------
def front_end_cases(k):
    from halo2_gpu_specific_amd import circuits, circuits_frontend as fe

    return {
        "mini_plonk": (fe.MiniPlonk(k), circuits.mini_plonk(), circuits.mini_plonk_synthesize(k), True),
        "lookup_api": (fe.LookupApi(), circuits.lookup_api(), circuits.lookup_api_synthesize(k), False),
        "shuffle_api_group": (fe.ShuffleApiGroup(), circuits.shuffle_api_group(), circuits.shuffle_api_group_synthesize(k), False),
        "range_check": (fe.RangeCheck(k, vmax=61, step=4, count=150), circuits.range_check(0, 61, 4),
                        circuits.range_check_synthesize(k, vmax=61, count=150), True),
    }


@pytest.mark.parametrize("name", ["mini_plonk", "lookup_api", "shuffle_api_group", "range_check"])
def test_front_end_proof_bytes_equal_the_hand_laid_circuits(device, setups, name):
    from halo2_gpu_specific_amd import prover, verifier
    from halo2_gpu_specific_amd.rng import ProverRng

    k = 8
    params, pv = setups(k)
    circuit, twin_cs, (twin_advice, twin_fixed, twin_copies), montgomery = front_end_cases(k)[name]
    assert type(circuit).planner is (prover.FlatFloorPlanner if name == "mini_plonk" else prover.V1)
    cs, fixed, copies = prover.synthesize_keygen(device, circuit, k, resident=True, montgomery=montgomery)
    assert all(device.torch.is_tensor(f) for f in fixed)
    pk = prover.keygen(device, params, cs, fixed, copies, fixed_montgomery=montgomery)
    twin_pk = prover.keygen(device, params, twin_cs, twin_fixed, twin_copies)
    assert pk.transcript_repr == twin_pk.transcript_repr and pk.fixed_commitments == twin_pk.fixed_commitments
    assert pk.perm_commitments == twin_pk.perm_commitments
    advice, first_unassigned = prover.synthesize_witness(device, circuit, pk, k, resident=True)
    assert all(device.torch.is_tensor(a) for a in advice)
    for seed, use_gwc in ((5, True), (6, False)):
        proof = prover.create_proof_ext(device, params, pk, advice, ProverRng(seed), use_gwc, first_unassigned=first_unassigned)
        want = prover.create_proof_ext(device, params, twin_pk, [a.copy() for a in twin_advice], ProverRng(seed), use_gwc)
        assert proof == want
        report = {}
        assert verifier.verify_proof_ext(device, pv, verifier.VerifyingKey.from_proving_key(pk), proof, (), use_gwc, report=report), report


def test_canonical_resident_fixed_columns_are_not_written_by_keygen(device, setups):
    from halo2_gpu_specific_amd import circuits_frontend as fe, prover

    k = 8
    params, _ = setups(k)
    cs, fixed, copies = prover.synthesize_keygen(device, fe.LookupApi(), k, resident=True)
    before = [device.download(f).copy() for f in fixed]
    _, host_fixed, _ = prover.synthesize_keygen(None, fe.LookupApi(), k)
    assert all(np.array_equal(a, b) for a, b in zip(before, host_fixed))
    pk = prover.keygen(device, params, cs, fixed, copies)
    assert all(np.array_equal(device.download(f), b) for f, b in zip(fixed, before))
    assert pk.fixed_commitments == prover.keygen(device, params, cs, host_fixed, copies).fixed_commitments


# ---- check_witness on a synthesised witness ----------------------------------------------------------------------------------
def two_region_circuit(device):
    from halo2_gpu_specific_amd import synthesis

    class TwoRegions(synthesis.Circuit):
        """q (a - b) = 0 on the rows of two regions over the same columns: V1 puts the taller one first.  b comes from a
        tensor torch made on the device."""
        planner = synthesis.V1

        def without_witnesses(self):
            return self

        def configure(self, cs):
            a, b, q = cs.advice_column(), cs.advice_column(), cs.fixed_column()
            cs.create_gate("equal", [cs.query_fixed(q) * (cs.query_advice(a) - cs.query_advice(b))])
            return a, b, q

        def synthesize(self, config, layouter):
            a, b, q = config

            def rows(first, count):
                def body(region):
                    values = np.arange(first, first + count, dtype=np.uint64)
                    region.assign_advice(a, 0, values)
                    resident = device.torch.arange(first, first + count, dtype=device.torch.int64, device=device.dev)
                    region.assign_advice(b, 0, resident)
                    region.assign_fixed(q, 0, 1, count=count)
                return body

            layouter.assign_region("short", rows(1000, 2))
            layouter.assign_region("tall", rows(2000, 5))

    return TwoRegions()


def test_check_witness_is_silent_then_names_the_planners_row(device, setups):
    from halo2_gpu_specific_amd import prover

    k = 6
    params, _ = setups(k)
    circuit = two_region_circuit(device)
    starts = prover.region_starts(circuit)
    assert starts == [5, 0]                                              # the tall region first, the short one below it
    cs, fixed, copies = prover.synthesize_keygen(device, circuit, k, resident=True)
    pk = prover.keygen(device, params, cs, fixed, copies)
    advice, first_unassigned = prover.synthesize_witness(device, circuit, pk, k, resident=True)
    assert first_unassigned == {0: 7, 1: 7}
    assert device.download(advice[1])[:7, 0].tolist() == [2000, 2001, 2002, 2003, 2004, 1000, 1001]
    assert prover.check_witness(device, pk, advice) == ([], 0)
    row = starts[0] + 1                                                  # offset 1 of the short region
    with device.torch.cuda.stream(device.tstream):
        advice[0][row, 0] += 1
    failures, total = prover.check_witness(device, pk, advice)
    assert total == 1 and failures == [prover.ConstraintNotSatisfied(0, "equal", 0, row, 0)]


def test_host_and_device_assemblies_agree(device):
    from halo2_gpu_specific_amd import circuits_frontend as fe, prover

    k = 8
    for circuit in (fe.Wide(k, 2), fe.ShuffleGates(k)):
        cs, fixed, copies = prover.synthesize_keygen(device, circuit, k, resident=True)
        _, host_fixed, host_copies = prover.synthesize_keygen(None, circuit, k)
        assert np.array_equal(copies, host_copies)
        assert all(np.array_equal(device.download(a), b) for a, b in zip(fixed, host_fixed))
        stats = {}
        advice, first = prover.synthesize_witness(device, circuit, cs, k, resident=True, stats=stats)
        host_advice, host_first = prover.synthesize_witness(device, circuit, cs, k, resident=False, alloc=device.pinned_columns)
        assert first == host_first and stats["flushes"] == 1
        assert all(np.array_equal(device.download(a), b) for a, b in zip(advice, host_advice))
