"""check_assignments on the device (synthesis.DeviceCoverage over csrc/coverage.hip).

The device's failures against the host assembly's and against the brute-force model of tests/coverage_cases.py, as sorted
lists with equal totals: n = 16, 32, 64 and 2^10 with 1, 3 and 40 regions under both planners, strides 1, 2, 3, 31, 32, 33 and
37, planes that begin at rows 5, 31 and 33, one mark and one check launch per call.  The mark kernel's word path at its edges,
the downloaded bit array against numpy bit for bit.  5000 one-row regions in one launch, short record buffers, and the
circuit the feature is for at k = 5: s (a b - c) with a = 0 and c never assigned passes check_witness, is named by
check_assignments and check_circuit, and with c assigned proves and verifies."""
import numpy as np
import pytest

import coverage_cases as cc
from test_plonk_host import S_TRAPDOOR

pytestmark = pytest.mark.gpu

SIZES = [16, 32, 64, 1 << 10]
ALL = 1 << 16


@pytest.fixture(scope="module")
def device():
    from halo2_gpu_specific_amd import prover

    return prover.Device()


def planners():
    from halo2_gpu_specific_amd import synthesis as syn

    return {"flat": syn.FlatFloorPlanner, "v1": syn.V1}


def device_result(device, circuit, n, cap=ALL):
    """-> (failures, total) of one check on the device, which took one mark and one check launch at the most"""
    from halo2_gpu_specific_amd import check, synthesis as syn

    cov = syn.synthesize_coverage(device, circuit, n.bit_length() - 1)
    records, total = cov.check(cap)
    assert cov.mark_launches == (1 if len(cov.segments) else 0) and cov.check_launches == (1 if len(cov.build()[3]) else 0)
    assert len(records) == min(cap, total)
    return check.check_failures(None, records, cov), total, cov


def host_result(circuit, n):
    from halo2_gpu_specific_amd import check

    failures, total = check.check_assignments(None, circuit, n.bit_length() - 1, max_failures=ALL, resident=False)
    return sorted(failures), total


# -- device against host against model --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("planner", ["flat", "v1"])
@pytest.mark.parametrize("regions", [1, 3, 40])
@pytest.mark.parametrize("n", SIZES)
def test_device_host_and_model_agree(device, n, regions, planner):
    from halo2_gpu_specific_amd import synthesis as syn

    planner = planners()[planner]
    for seed in (n + regions, 7 * n + regions):
        spec = cc.random_spec(seed, planner, n, regions)
        circuit = cc.SpecCircuit(spec, planner)
        want = cc.model(spec, planner, n)
        failures, total, cov = device_result(device, circuit, n)
        assert (sorted(failures), total) == want == host_result(circuit, n)
        assert np.array_equal(cov.bitmap(), syn.synthesize_coverage(None, circuit, n.bit_length() - 1, resident=False).bitmap())
        complete, holed, expected = cc.paired_specs(seed, planner, n, regions)
        assert device_result(device, cc.SpecCircuit(complete, planner), n)[:2] == ([], 0)
        failures, total, cov = device_result(device, cc.SpecCircuit(holed, planner), n)
        assert (sorted(failures), total) == expected and expected[1] > 0 and cov.check_launches == 1 == cov.mark_launches


def test_planes_that_begin_at_rows_5_31_and_33(device):
    from halo2_gpu_specific_amd import synthesis as syn

    n, planner = 1 << 10, planners()["flat"]
    for seed in range(4):
        spec = cc.random_spec(100 + seed, planner, n, 3)
        origins = iter((5, 31, 33))                     # a cell at offset 0: advice 0's plane begins where its region does
        spec["regions"] = [(name, kind, base, ops) if kind == "table" else (name, kind, next(origins), ops + [("advice", 0, 0, 1, 1)])
                           for name, kind, base, ops in spec["regions"]]
        circuit = cc.SpecCircuit(spec, planner)
        failures, total, cov = device_result(device, circuit, n)
        assert (sorted(failures), total) == cc.model(spec, planner, n)
        host = syn.synthesize_coverage(None, circuit, 10, resident=False)
        assert np.array_equal(cov.bitmap(), host.bitmap())
        assert {int(lo) for lo in host.build()[0]["row_lo"]} >= {5, 31, 33}


# -- the word path's edges ------------------------------------------------------------------------------------------------------------
EDGES = {
    "one cell": [(0, 1, 1)],
    "a run inside one word": [(0, 1, 1), (3, 1, 7)],
    "exactly one word": [(0, 1, 32)],
    "a run ending at bit 31": [(0, 1, 1), (20, 1, 12)],
    "a run from bit 31 over three words": [(0, 1, 1), (31, 1, 35)],
    "two runs sharing a word": [(0, 1, 10), (10, 1, 31)],
    "a strided segment over a run": [(0, 1, 70), (1, 3, 30)],
    "two words and a bit": [(0, 1, 65)],
}


@pytest.mark.parametrize("origin", [0, 33])
@pytest.mark.parametrize("edge", sorted(EDGES))
def test_mark_edges_match_numpy_bit_for_bit(device, edge, origin):
    from halo2_gpu_specific_amd import synthesis as syn
    from halo2_gpu_specific_amd.circuit import ConstraintSystem

    cs = ConstraintSystem()
    columns = [cs.advice_column(), cs.advice_column()]
    dev = syn.DeviceCoverage(device, cs, 1 << 10)
    region = dev.enter_region("r", 0)
    want = []
    for column in columns:                             # two planes: the second one's words follow the first one's
        bits = np.zeros(32 * ((max(first + (count - 1) * stride for first, stride, count in EDGES[edge]) + 32) // 32), dtype=bool)
        for first, stride, count in EDGES[edge]:
            dev.assign(region, column, origin + first, stride, count)
            bits[first:first + (count - 1) * stride + 1:stride] = True
        want.append(np.packbits(bits, bitorder="little").view("<u4"))
    got = dev.bitmap()
    assert dev.mark_launches == 1 and got.dtype == np.dtype("<u4")
    assert np.array_equal(got, np.concatenate(want)), (got, want)


# -- many small regions, short record buffers -------------------------------------------------------------------------------------
def small_regions(count, usable):
    from halo2_gpu_specific_amd import synthesis as syn

    class SmallRegions(syn.Circuit):
        """`count` one-row regions on the rows i mod usable; every seventh forgets c of s (a b - c)"""
        planner = syn.FlatFloorPlanner

        def without_witnesses(self):
            return self

        def configure(self, cs):
            a, b, c = cs.advice_column(), cs.advice_column(), cs.advice_column()
            s = cs.selector()
            cs.create_gate("mul", [cs.query_selector(s) * (cs.query_advice(a) * cs.query_advice(b) - cs.query_advice(c))])
            return a, b, c, s

        def synthesize(self, config, layouter):
            a, b, c, s = config

            def body(i):
                def assign(region):
                    for column in (a, b) if i % 7 == 0 else (a, b, c):
                        region.assign_advice(column, i % usable, None)
                    region.enable_selector(s, i % usable)
                return assign

            for i in range(count):
                layouter.assign_region("r%d" % i, body(i))

    return SmallRegions()


def test_five_thousand_one_row_regions_in_one_launch(device):
    from halo2_gpu_specific_amd.check import CellNotAssigned

    n = 1 << 10
    usable = n - 6
    failures, total, cov = device_result(device, small_regions(5000, usable), n)
    assert len(cov.regions) == 5000 and cov.cells_marked == 15000 - 715 and cov.rows_enabled == 5000
    assert total == 715 and failures == [CellNotAssigned(0, "mul", i, "r%d" % i, ("advice", 2), 0, i % usable)
                                         for i in range(0, 5000, 7)]


@pytest.mark.parametrize("cap", [0, 3])
def test_a_short_record_buffer_keeps_the_total_exact(device, cap):
    n = 1 << 10
    circuit = small_regions(700, n - 6)
    truth, total, _ = device_result(device, circuit, n)
    assert total == 100 and len(truth) == 100
    failures, counted, _ = device_result(device, circuit, n, cap)
    assert counted == total and len(failures) == min(cap, total) == len(set(failures)) and set(failures) <= set(truth)
    from halo2_gpu_specific_amd import check

    assert check.check_assignments(device, circuit, 10, max_failures=cap)[1] == total


# -- end to end ---------------------------------------------------------------------------------------------------------------------
def forgetful(planner, assign_c):
    from halo2_gpu_specific_amd import synthesis as syn

    class Forgetful(syn.Circuit):
        """s (a b - c) on the third row of its region, a = 0, b = 5; c is assigned only with `assign_c`"""

        def without_witnesses(self):
            return self

        def configure(self, cs):
            a, b, c = cs.advice_column(), cs.advice_column(), cs.advice_column()
            s = cs.selector()
            cs.create_gate("mul", [cs.query_selector(s) * (cs.query_advice(a) * cs.query_advice(b) - cs.query_advice(c))])
            return a, b, c, s

        def synthesize(self, config, layouter):
            a, b, c, s = config

            def body(region):
                region.assign_advice(a, 2, 0)
                region.assign_advice(b, 2, 5)
                if assign_c:
                    region.assign_advice(c, 2, 0)
                region.enable_selector(s, 2)

            layouter.assign_region("product", body)

    Forgetful.planner = planner
    return Forgetful()


@pytest.mark.parametrize("planner", ["flat", "v1"])
def test_a_forgotten_cell_that_check_witness_cannot_see(device, planner):
    from halo2_gpu_specific_amd import check, prover, verifier
    from halo2_gpu_specific_amd.rng import ProverRng

    k, planner = 5, planners()[planner]
    params = prover.Params.unsafe_setup(device, k, S_TRAPDOOR)
    circuit = forgetful(planner, False)
    cs, fixed, copies = prover.synthesize_keygen(device, circuit, k, resident=True)
    pk = prover.keygen(device, params, cs, fixed, copies)
    advice, first_unassigned = prover.synthesize_witness(device, circuit, pk, k)
    assert prover.check_witness(device, pk, advice) == ([], 0)          # a = 0: the unassigned c, a zero, satisfies the gate
    missing = check.CellNotAssigned(0, "mul", 0, "product", ("advice", 2), 0, 2)
    assert prover.check_assignments(device, circuit, k) == ([missing], 1)
    assert prover.check_assignments(None, circuit, k, resident=False) == ([missing], 1)
    failures, total = prover.check_circuit(device, pk, circuit, k)
    assert failures[0] == missing and (failures, total) == ([missing], 1)
    with pytest.raises(ValueError, match="region 0 'product' enables gate 0 'mul' over advice column 2 at offset 0 \\(row 2\\)"):
        prover.assert_circuit_satisfied(device, pk, circuit, k)

    whole = forgetful(planner, True)
    timings = {}
    assert prover.check_assignments(device, whole, k, timings=timings) == ([], 0)
    assert sorted(timings) == ["check", "download", "mark", "synthesize"]
    assert prover.check_circuit(device, pk, whole, k) == ([], 0)
    prover.assert_circuit_satisfied(device, pk, whole, k)
    advice, first_unassigned = prover.synthesize_witness(device, whole, pk, k)
    assert prover.check_witness(device, pk, advice) == ([], 0)
    proof = prover.create_proof_ext(device, params, pk, advice, ProverRng(1), True, first_unassigned=first_unassigned)
    vparams, vk = verifier.ParamsVerifier.from_params(params), verifier.VerifyingKey.from_proving_key(pk)
    assert verifier.verify_proof(device, vparams, vk, proof)


def test_device_entry_points_refuse_bad_tables_on_a_live_device(device):
    from halo2_gpu_specific_amd import synthesis as syn
    from halo2_gpu_specific_amd.circuit import ConstraintSystem

    cs = ConstraintSystem()
    a = cs.advice_column()
    s = cs.selector()
    cs.create_gate("g", [cs.query_selector(s) * cs.query_advice(a)])
    dev = syn.DeviceCoverage(device, cs, 64)
    region = dev.enter_region("r", 0)
    dev.assign(region, a, 3, 1, 4)
    dev.enable(region, 0, 3, 1, 4)
    planes, segments, queries, uses, earlier, words = dev.build()
    segments["count"][0] = 5                             # one cell beyond the plane
    with pytest.raises(Exception, match="h2_dev_coverage_mark: a segment reaches outside its plane"):
        dev.mark()
    segments["count"][0] = 4
    dev.bits = None
    uses["first_row"][0] = 61                            # the last row would be 64
    with pytest.raises(Exception, match="h2_dev_coverage_check: a use reaches beyond row n - 1"):
        dev.check(4)
    uses["first_row"][0] = 3
    records, total = dev.check(4)
    assert total == 0 and len(records) == 0 and dev.bitmap().tolist() == [0b1111]
