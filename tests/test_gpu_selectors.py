"""Selectors on the device (synthesis.DeviceSelectors over csrc/selectors.hip).

The three kernels against numpy, bit for bit: n below one bitmap word, one word, two, and 2^10 rows; 1, 2, 33 and 70 selectors;
strided segments across word boundaries, rows enabled twice, thousands of one-row segments in one launch, both output forms,
and a combination longer than one launch's member table.  The host and the device assembly give the same constraint system and
fixed columns.  A selector circuit proves to the bytes of its twin laid out by hand -- combination columns as plain fixed
columns under the substituted gates -- and of the big-integer prover of tests/ref_plonk.py; check_witness sees the compressed
system: silent on a good witness, it names gate, polynomial and row of a cell changed under an enabled selector, says nothing of
one changed where the selector is off, and reports the examples' wrong public input as permutation failures."""
import numpy as np
import pytest

import ref_plonk as rp
from test_plonk_host import S_TRAPDOOR

pytestmark = pytest.mark.gpu

R_MOD = rp.R
MASK = (1 << 64) - 1


@pytest.fixture(scope="module")
def device():
    from halo2_gpu_specific_amd import prover

    return prover.Device()


@pytest.fixture(scope="module")
def srs(device):
    """Params::unsafe_setup under the trapdoor the big-integer prover uses: these carry [s]G2 for the verifier"""
    from halo2_gpu_specific_amd import prover

    made = {}

    def get(k):
        if k not in made:
            made[k] = prover.Params.unsafe_setup(device, k, S_TRAPDOOR)
        return made[k]

    return get


def limbs(v):
    return [(v >> (64 * j)) & MASK for j in range(4)]


def montgomery(column):
    return np.array([limbs((int(v) << 256) % R_MOD) for v in column[:, 0]], dtype=np.uint64).reshape(len(column), 4)


def random_segments(rng, count, n, segments):
    """(selector, first_row, stride, rows) with every row below n: strides 1 .. 37 (37 and 33 step over word boundaries
    unevenly), single rows, and some segments repeated so that rows are enabled twice"""
    out = []
    for _ in range(segments):
        stride = int(rng.choice([1, 1, 2, 3, 31, 32, 33, 37]))
        first = int(rng.integers(0, n))
        rows = int(rng.integers(1, (n - 1 - first) // stride + 2))
        out.append((int(rng.integers(0, count)), first, stride, rows))
    return out + out[::3]


def assemblies(device, count, n, segments, montgomery_form=False):
    from halo2_gpu_specific_amd import synthesis

    host, dev = synthesis.HostSelectors(count, n), synthesis.DeviceSelectors(device, count, n, montgomery_form)
    for segment in segments:
        host.enable(*segment)
        dev.enable(*segment)
    return host, dev


def device_bitmaps(device, dev):
    dev.flush()
    with device.torch.cuda.stream(device.tstream):
        words = dev.bitmaps.cpu().numpy()
    return words.view("<u4").reshape(dev.count, dev.words)


def greedy_plan(host, max_degree, degree=2):
    """combinations of pairwise disjoint selectors, by the plan function itself over the numpy conflicts"""
    from halo2_gpu_specific_amd import circuit

    conflicts = host.conflicts()
    combinations, _ = circuit.compress_selectors_plan(
        [(i, degree if i % 5 else 0, set(np.flatnonzero(conflicts[i]).tolist())) for i in range(host.count)], max_degree)
    return combinations


@pytest.mark.parametrize("count", [1, 2, 33, 70])
@pytest.mark.parametrize("n", [16, 32, 64, 1 << 10])
def test_mark_conflicts_and_combine_match_numpy(device, n, count):
    rng = np.random.Generator(np.random.PCG64(1000 * count + n))
    segments = random_segments(rng, count, n, 2 * count + 3)
    if count > 1:                                     # two selectors that certainly share a row, the last row, and nothing else
        segments += [(0, n - 1, 1, 1), (count - 1, n - 1, 1, 1)]
    for form in (False, True):
        host, dev = assemblies(device, count, n, segments, form)
        assert np.array_equal(device_bitmaps(device, dev), host.bitmaps())
        assert dev.flushes == 1
        matrix = dev.conflicts()
        assert matrix.dtype == np.uint8 and np.array_equal(matrix, host.conflicts())
        assert np.array_equal(matrix, matrix.T) and not matrix.diagonal().any() and (count == 1 or matrix[0, count - 1] == 1)
        combinations = greedy_plan(host, 4)
        want = host.combine(combinations)
        got = [device.download(t) for t in dev.combine(combinations)]
        assert len(got) == len(want)
        for column, (have, expect) in enumerate(zip(got, want)):
            expect = montgomery(expect) if form else expect
            bad = np.flatnonzero((have != expect).any(axis=1))
            assert len(bad) == 0, "combination %d differs at rows %s" % (column, bad[:8])


def test_five_thousand_one_row_segments_in_one_launch(device):
    n, count = 1 << 10, 33
    rng = np.random.Generator(np.random.PCG64(5000))
    segments = [(int(s), int(r), 1, 1) for s, r in zip(rng.integers(0, count, 5000), rng.integers(0, n, 5000))]
    host, dev = assemblies(device, count, n, segments)
    assert np.array_equal(device_bitmaps(device, dev), host.bitmaps())
    assert dev.flushes == 1 and dev.rows_marked == 5000
    assert np.array_equal(dev.conflicts(), host.conflicts())


def test_a_combination_of_max_degree_minus_one_members(device):
    """degree-2 selectors on rows of their own under max_degree 20: d = 1, and the combination closes at d + len = 20, that is
    with 19 members -- more than one launch of the combine kernel takes (16): the column is written in two slices"""
    n, count, max_degree = 1 << 10, 24, 20
    segments = [(s, s, count, (n - 1 - s) // count + 1) for s in range(count)]          # selector s on the rows = s mod 24
    for form in (False, True):
        host, dev = assemblies(device, count, n, segments, form)
        assert not dev.conflicts().any()
        combinations = greedy_plan(host, max_degree)
        assert [len(group) for group in combinations] == [1, 1, 1, 1, 1, max_degree - 1]   # 0, 5, .. 20 are in no gate
        got = [device.download(t) for t in dev.combine(combinations)]
        for have, expect in zip(got, host.combine(combinations)):
            assert np.array_equal(have, montgomery(expect) if form else expect)
        values = sorted(set(int(v) for v in host.combine(combinations)[-1][:, 0]))
        assert values == list(range(0, max_degree))


def test_device_entry_points_refuse_bad_segments_on_a_live_device(device):
    from halo2_gpu_specific_amd import synthesis

    dev = synthesis.DeviceSelectors(device, 2, 64)
    for segment in ((0, 60, 1, 5), (2, 0, 1, 1), (0, 0, 0, 2)):
        dev.queue = [(segment[0], 0) + segment[1:]]
        with pytest.raises(Exception, match="h2_dev_selectors_mark"):
            dev.flush()
    dev.queue = []
    assert not device_bitmaps(device, dev).any()


# -- the two assemblies ----------------------------------------------------------------------------------------------------------
def random_selector_circuit(seed, k):
    from halo2_gpu_specific_amd import synthesis

    class RandomSelectors(synthesis.Circuit):
        """12 selectors, simple or complex, in gates of random degree (or none), enabled over random strided ranges"""
        planner = synthesis.FlatFloorPlanner

        def without_witnesses(self):
            return self

        def configure(self, cs):
            rng = np.random.Generator(np.random.PCG64(seed))
            a = cs.advice_column()
            selectors = [cs.selector() if rng.random() < 0.75 else cs.complex_selector() for _ in range(12)]
            for sel in selectors:
                degree = int(rng.integers(0, 5))
                if degree:
                    poly = cs.query_selector(sel)
                    for _ in range(degree - 1):
                        poly = poly * cs.query_advice(a)
                    cs.create_gate("g%d" % sel.index, [poly])
            cs.set_minimum_degree(6)
            return a, selectors

        def synthesize(self, config, layouter):
            rng = np.random.Generator(np.random.PCG64(seed + 1))
            usable = (1 << k) - 6

            def body(region):
                region.assign_advice(config[0], 0, 0, count=usable)
                for sel in config[1]:
                    for _ in range(int(rng.integers(0, 4))):
                        stride = int(rng.integers(1, 40))
                        first = int(rng.integers(0, usable))
                        region.enable_selector(sel, first, stride, int(rng.integers(0, (usable - 1 - first) // stride + 2)))

            layouter.assign_region("rows", body)

    return RandomSelectors()


@pytest.mark.parametrize("which", ["simple-example", "two-chip", "selector-gates", "random-1", "random-2"])
def test_host_and_device_assemblies_agree(device, which):
    from halo2_gpu_specific_amd import circuits_frontend as fe, cs_format, synthesis

    circuit, k = {"simple-example": lambda: (fe.SimpleExample(), 4), "two-chip": lambda: (fe.TwoChip(), 4),
                  "selector-gates": lambda: (fe.SelectorGates(7), 7), "random-1": lambda: (random_selector_circuit(11, 8), 8),
                  "random-2": lambda: (random_selector_circuit(12, 6), 6)}[which]()
    cs, fixed, copies = synthesis.synthesize_keygen(None, circuit, k)
    assert cs.num_selectors and len(fixed) == cs.num_fixed
    for form in (False, True):
        dcs, dfixed, dcopies = synthesis.synthesize_keygen(device, circuit, k, resident=True, montgomery=form)
        assert cs_format.cs_store(dcs) == cs_format.cs_store(cs) and dcs.selector_map == cs.selector_map
        assert np.array_equal(dcopies, copies) and len(dfixed) == len(fixed)
        for index, (have, expect) in enumerate(zip(dfixed, fixed)):
            expect = np.array([limbs((v << 256) % R_MOD) for v in rp_ints(expect)], dtype=np.uint64) if form else expect
            assert np.array_equal(device.download(have), expect), "fixed column %d" % index


def rp_ints(column):
    return [sum(int(x) << (64 * j) for j, x in enumerate(row)) for row in column]


# -- end to end: the selector circuit and its twin laid out by hand --------------------------------------------------------------
SELECTOR_MAP = [3, 3, 4, 1, 2]                     # s_mul, s_add -> fixed 3 (values 1, 2); s_bool -> 4; s_idle -> 1; s_tab -> 2


def twin_by_hand(k):
    """circuits_frontend.SelectorGates after compress_selectors, written without a selector: fixed 0 the table, 1 s_idle, 2 s_tab,
    3 the combination of s_mul (1) and s_add (2), 4 s_bool; the substitutes q (2 - q) and q (1 - q) spelled out"""
    from halo2_gpu_specific_amd.circuit import Constant, ConstraintSystem

    cs = ConstraintSystem("SelectorGates")
    a, b, c = cs.advice_column(), cs.advice_column(), cs.advice_column()
    table, idle, tab, comb, boolean = (cs.fixed_column() for _ in range(5))
    cs.enable_equality(a)
    qa, qb, qc = cs.query_advice(a), cs.query_advice(b), cs.query_advice(c)
    qtable = cs.query_fixed(table)
    del idle
    cs.query_fixed(("fixed", 1))
    qtab, q, qbool = cs.query_fixed(tab), cs.query_fixed(comb), cs.query_fixed(boolean)
    cs.create_gate("mul", [(q * (Constant(2) - q)) * (qa * qb - qc)])
    cs.create_gate("add", [(q * (Constant(1) - q)) * (qa + qb - qc)])
    cs.create_gate("bool", [qbool * (qb * (Constant(1) - qb))])
    cs.lookup("a in table", [(qtab * qa, qtable)])
    cs.chunk_lookups()
    cs.num_selectors, cs.selector_map = 5, [("fixed", index) for index in SELECTOR_MAP]      # what write_cs records of them
    n, rows = 1 << k, ((1 << k) - 6) // 4 * 4
    r = np.arange(rows)
    values = [np.zeros(rows, dtype=np.uint64), r % 8 == 0, (r % 4 == 0) | (r % 4 == 3),
              np.where(r % 4 == 0, 1, np.where(r % 4 == 3, 0, 2)), r % 4 == 2]
    values[0][:16] = np.arange(16)
    fixed = [np.zeros((n, 4), dtype=np.uint64) for _ in values]
    for column, v in zip(fixed, values):
        column[:rows, 0] = v
    return cs, fixed, np.array([[0, 0, 0, 4]], dtype=np.int64)


class RefSelectorGates:
    """the twin in the form the big-integer prover takes"""
    num_advice, num_fixed = 3, 5
    advice_queries = [(0, 0), (1, 0), (2, 0)]
    fixed_queries = [(0, 0), (1, 0), (2, 0), (3, 0), (4, 0)]
    perm_columns = [("advice", 0)]
    degree = 5
    blinding_factors = 5
    name = "selector-gates"

    @classmethod
    def cs_bytes(cls):
        """write_cs of this class, with what write_cs keeps of compiled selectors put in: their number (the third word) and
        selector_map (a count and the columns, after the advice query counts)"""
        plain = rp.write_cs(cls)
        at = 20 + 4 * cls.num_advice
        le = lambda v: v.to_bytes(4, "little")   # noqa: E731
        return plain[:8] + le(5) + plain[12:at] + le(5) + b"".join(le(i) for i in SELECTOR_MAP) + plain[at + 4:]

    @staticmethod
    def gates(adv, fix):
        a, b, c, q = adv(0, 0), adv(1, 0), adv(2, 0), fix(3, 0)
        return [(q * (2 - q)) * (a * b - c) % rp.R, (q * (1 - q)) * (a + b - c) % rp.R, fix(4, 0) * (b * (1 - b)) % rp.R]

    lookups = [{"table": lambda adv, fix, inst: [fix(0, 0)],
                "input_sets": [[lambda adv, fix, inst: [fix(2, 0) * adv(0, 0) % rp.R]]]}]


@pytest.mark.parametrize("k", [6, 10])
def test_selector_circuit_proves_to_the_bytes_of_its_twin_by_hand(srs, device, k):
    from halo2_gpu_specific_amd import circuits_frontend as fe, cs_format, prover, verifier
    from halo2_gpu_specific_amd.rng import ProverRng

    circuit = fe.SelectorGates(k)
    params = srs(k)
    cs, fixed, copies = prover.synthesize_keygen(device, circuit, k, resident=True)
    pk = prover.keygen(device, params, cs, fixed, copies)
    tcs, tfixed, tcopies = twin_by_hand(k)
    assert cs_format.cs_store(cs) == cs_format.cs_store(tcs) == RefSelectorGates.cs_bytes()
    assert all(np.array_equal(device.download(a), b) for a, b in zip(fixed, tfixed)) and len(fixed) == len(tfixed)
    tpk = prover.keygen(device, params, tcs, tfixed, tcopies)
    assert pk.transcript_repr == tpk.transcript_repr and pk.fixed_commitments == tpk.fixed_commitments
    assert pk.perm_commitments == tpk.perm_commitments
    # the Montgomery out form gives the same key
    mcs, mfixed, mcopies = prover.synthesize_keygen(device, circuit, k, resident=True, montgomery=True)
    mpk = prover.keygen(device, params, mcs, mfixed, mcopies, fixed_montgomery=True)
    assert mpk.transcript_repr == pk.transcript_repr and mpk.fixed_commitments == pk.fixed_commitments

    advice, first_unassigned = prover.synthesize_witness(device, circuit, pk, k)
    rows = ((1 << k) - 6) // 4 * 4
    tadvice = [np.zeros((1 << k, 4), dtype=np.uint64) for _ in range(3)]
    for column, values in zip(tadvice, circuit.witness_columns(rows)):
        column[:rows, 0] = values
    assert all(np.array_equal(device.download(a), b) for a, b in zip(advice, tadvice))
    assert prover.check_witness(device, pk, advice) == ([], 0)
    vparams, vk = verifier.ParamsVerifier.from_params(params), verifier.VerifyingKey.from_proving_key(pk)
    if k == 6:
        rpk = rp.keygen(RefSelectorGates, k, S_TRAPDOOR, [rp_ints(f) for f in tfixed], [((0, 0), (0, 4))])
        assert pk.transcript_repr == rpk.transcript_repr and pk.fixed_commitments == rpk.fixed_commitments
    else:
        rpk = rp.Keys()
        rpk.cs, rpk.dom, rpk.s = RefSelectorGates, rp.Domain(k, cs.degree()), S_TRAPDOOR
        rpk.fixed_commitments, rpk.perm_commitments, rpk.transcript_repr = pk.fixed_commitments, pk.perm_commitments, pk.transcript_repr
    for seed, use_gwc in ((1, False), (2, True)):
        proof = prover.create_proof_ext(device, params, pk, [device.clone(a) for a in advice], ProverRng(seed), use_gwc,
                                        first_unassigned=first_unassigned)
        twin = prover.create_proof_ext(device, params, tpk, [a.copy() for a in tadvice], ProverRng(seed), use_gwc)
        assert proof == twin
        assert verifier.verify_proof_ext(device, vparams, vk, proof, (), use_gwc)
        if k == 6:
            want = rp.create_proof(rpk, [rp_ints(a) for a in tadvice], ProverRng(seed), use_gwc=use_gwc)
            first = next((i for i in range(min(len(proof), len(want))) if proof[i] != want[i]), None)
            assert len(proof) == len(want) and first is None, "differs from the big-integer prover at byte %s" % first
        if k == 6 or not use_gwc:
            assert rp.verify_proof(rpk, proof, use_gwc=use_gwc)


# -- check_witness over the compressed system ----------------------------------------------------------------------------------------
def test_check_witness_names_the_cell_under_an_enabled_selector(srs, device):
    from halo2_gpu_specific_amd import check, circuits_frontend as fe, prover

    k = 6
    circuit = fe.SelectorGates(k)
    cs, fixed, copies = prover.synthesize_keygen(device, circuit, k, resident=True)
    pk = prover.keygen(device, srs(k), cs, fixed, copies)
    advice = [device.download(a).copy() for a in prover.synthesize_witness(device, circuit, pk, k)[0]]
    assert prover.check_witness(device, pk, advice) == ([], 0)
    advice[2][8, 0] += np.uint64(1)                     # c of row 8, a multiplication row: gate 0 "mul", polynomial 0
    assert prover.check_witness(device, pk, advice) == ([check.ConstraintNotSatisfied(0, "mul", 0, 8, 0)], 1)
    advice[2][8, 0] -= np.uint64(1)
    advice[2][9, 0] += np.uint64(1)                     # ... of row 9, an addition row: gate 1 "add"
    assert prover.check_witness(device, pk, advice) == ([check.ConstraintNotSatisfied(1, "add", 0, 9, 0)], 1)
    advice[2][9, 0] -= np.uint64(1)
    advice[1][10, 0] = np.uint64(5)                     # b of row 10, where s_add and s_bool are both on (c - a was 0 or 1)
    got, total = prover.check_witness(device, pk, advice)
    assert total == 2 and got == [check.ConstraintNotSatisfied(1, "add", 0, 10, 0), check.ConstraintNotSatisfied(2, "bool", 0, 10, 0)]
    advice[1][10, 0] = np.uint64(int(advice[2][10, 0]) - int(advice[0][10, 0]))
    advice[2][11, 0] += np.uint64(1)                    # c of row 11: no selector that reads c is on
    advice[1][11, 0] += np.uint64(7)
    assert prover.check_witness(device, pk, advice) == ([], 0)
    advice[0][11, 0] = np.uint64(16)                    # a of row 11, under the complex s_tab: 16 is not in the table
    got, total = prover.check_witness(device, pk, advice)
    assert total == 1 and isinstance(got[0], check.Lookup) and got[0].row == 11


@pytest.mark.parametrize("which", ["simple-example", "two-chip"])
def test_examples_prove_and_their_wrong_public_input_is_a_permutation_failure(srs, device, which):
    from halo2_gpu_specific_amd import check, circuits_frontend as fe, prover, verifier
    from halo2_gpu_specific_amd.rng import ProverRng

    k = 4
    circuit = fe.SimpleExample() if which == "simple-example" else fe.TwoChip()
    params = srs(k)
    cs, fixed, copies = prover.synthesize_keygen(device, circuit, k, resident=True)
    pk = prover.keygen(device, params, cs, fixed, copies)
    instances = circuit.public_inputs()
    advice, first_unassigned = prover.synthesize_witness(device, circuit, pk, k, instances=instances)
    assert prover.check_witness(device, pk, advice, instances) == ([], 0)
    wrong = [[instances[0][0] + 1]]
    # the exposed cell is advice 0, row 1 (the last multiplication's region starts at row 0), tied to instance row 0
    assert prover.check_witness(device, pk, advice, wrong) == (
        sorted([check.Permutation(("instance", 0), 0, 0), check.Permutation(("advice", 0), 1, 0)],
               key=lambda f: cs.perm_columns.index(f.column)), 2)
    vparams, vk = verifier.ParamsVerifier.from_params(params), verifier.VerifyingKey.from_proving_key(pk)
    for use_gwc in (True, False):
        proof = prover.create_proof_ext(device, params, pk, [device.clone(a) for a in advice], ProverRng(3), use_gwc,
                                        instances=instances, first_unassigned=first_unassigned)
        assert verifier.verify_proof_ext(device, vparams, vk, proof, instances, use_gwc)
        assert not verifier.verify_proof_ext(device, vparams, vk, proof, wrong, use_gwc)
