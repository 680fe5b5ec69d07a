"""verify_proof on the GPU: device proofs of the product circuits are accepted through the real BN254 pairing -- instance
commitments and both sums of the PairMSM as device MSMs, the pairing on the host -- with no use of the setup's trapdoor, and
tampered proofs, wrong instances and parameters of another setup are rejected."""
import numpy as np
import pytest

import ref_plonk as rp
from h2util import ints_to_arr
from product_circuits import lookup_shuffle_cs

pytestmark = pytest.mark.gpu

S_TRAPDOOR = 0x1D0C5F0A3B7E91C2A4D6F8091B2C3D4E5F60718293A4B5C6D7E8F9010203


@pytest.fixture(scope="module")
def device():
    from halo2_gpu_specific_amd import prover

    return prover.Device()


@pytest.fixture(scope="module")
def setups(device):
    """Params::unsafe_setup per k (on the device) with the ParamsVerifier made from it"""
    from halo2_gpu_specific_amd import prover, verifier

    made = {}

    def get(k):
        if k not in made:
            params = prover.Params.unsafe_setup(device, k, S_TRAPDOOR)
            made[k] = (params, verifier.ParamsVerifier.from_params(params))
        return made[k]

    return get


def flip(proof, pos, bit=0):
    bad = bytearray(proof)
    bad[pos] ^= 1 << bit
    return bytes(bad)


def prove_and_verify(device, setups, cs, k, adv, fixed, copies, instances=(), circuits=None, wrong_instances=None):
    """both multiopen schemes: accepted; one flipped bit in a commitment, in an evaluation and in the last opening point, and
    a wrong instance value: rejected.  Returns the key and the SHPLONK proof."""
    from halo2_gpu_specific_amd import prover, verifier
    from halo2_gpu_specific_amd.rng import ProverRng

    params, pv = setups(k)
    pk = prover.keygen(device, params, cs, fixed, copies)
    vk = verifier.VerifyingKey.from_proving_key(pk)
    proofs = {}
    for seed, use_gwc in ((1, False), (2, True)):
        proof = prover.create_proof_ext(device, params, pk, adv, ProverRng(seed), use_gwc, instances=instances)
        report = {}
        assert verifier.verify_proof_ext(device, pv, vk, proof, instances, use_gwc, circuits, report=report), report
        evals_at = 32 * (len(proof) // 64)
        for pos in (3, evals_at + 1, len(proof) - 30):
            assert not verifier.verify_proof_ext(device, pv, vk, flip(proof, pos), instances, use_gwc, circuits), pos
        assert not verifier.verify_proof_ext(device, pv, vk, proof, instances, not use_gwc, circuits)
        if wrong_instances is not None:
            assert not verifier.verify_proof_ext(device, pv, vk, proof, wrong_instances, use_gwc, circuits)
        proofs[use_gwc] = proof
    # the named entry points are the two schemes
    assert verifier.verify_proof(device, pv, pk, proofs[True], instances, circuits)
    assert verifier.verify_proof_with_shplonk(device, pv, pk, proofs[False], instances, circuits)
    return pk, proofs[False]


@pytest.mark.timeout(900)
@pytest.mark.parametrize("k", [8, 16, 22])
def test_mini_plonk_proofs_verify_with_the_real_pairing(device, setups, k):
    from halo2_gpu_specific_amd import circuits

    adv, fixed, copies = circuits.mini_plonk_synthesize(k)
    prove_and_verify(device, setups, circuits.mini_plonk(), k, adv, fixed, copies)


@pytest.mark.timeout(900)
@pytest.mark.parametrize("which", ["wide", "lookup_api", "shuffle_api_group", "shuffle_gates", "range_check"])
def test_product_circuits_verify_with_the_real_pairing(device, setups, which):
    from halo2_gpu_specific_amd import circuits

    if which == "wide":
        k, cs = 12, circuits.wide()
        adv, fixed, copies = circuits.wide_synthesize(k)
    elif which == "range_check":
        k, cs = 18, circuits.range_check()
        adv, fixed, copies = circuits.range_check_synthesize(k)
    else:
        k, cs = 7, getattr(circuits, which)()
        adv, fixed, copies = getattr(circuits, which + "_synthesize")(k)
    prove_and_verify(device, setups, cs, k, adv, fixed, copies)


def test_two_circuit_instances_with_public_inputs(device, setups):
    k = 6
    adv_a, fixed, copies, inst_a = rp.LookupShuffle.synthesize(k)
    adv_b = [c[:] for c in adv_a]
    adv_b[11][0] = 43
    inst_b = [[43, 7]]
    advs = [[ints_to_arr(c) for c in a] for a in (adv_a, adv_b)]
    prove_and_verify(device, setups, lookup_shuffle_cs(), k, advs, [ints_to_arr(c) for c in fixed],
                     [(l[0], l[1], r[0], r[1]) for l, r in copies], instances=[inst_a, inst_b], circuits=2,
                     wrong_instances=[inst_b, inst_a])
    # one circuit, its instance column; a wrong value, too many columns and too many values are rejected
    from halo2_gpu_specific_amd import prover, verifier
    from halo2_gpu_specific_amd.rng import ProverRng

    params, pv = setups(k)
    pk = prover.keygen(device, params, lookup_shuffle_cs(), [ints_to_arr(c) for c in fixed],
                       [(l[0], l[1], r[0], r[1]) for l, r in copies])
    proof = prover.create_proof_with_shplonk(device, params, pk, advs[0], ProverRng(3), instances=inst_a)
    assert verifier.verify_proof_with_shplonk(device, pv, pk, proof, inst_a)
    report = {}
    assert not verifier.verify_proof_with_shplonk(device, pv, pk, proof, [[43, 7]], report=report)
    assert not verifier.verify_proof_with_shplonk(device, pv, pk, proof, [[42, 7], [1]], report=report)
    assert isinstance(report["error"], verifier.InvalidInstances)
    assert not verifier.verify_proof_with_shplonk(device, pv, pk, proof, [[1] * 64], report=report)
    assert isinstance(report["error"], verifier.InstanceTooLarge)
    # a ParamsVerifier with fewer Lagrange points than public inputs refuses, one with exactly enough verifies
    assert verifier.verify_proof_with_shplonk(device, verifier.ParamsVerifier.from_params(params, public_inputs_size=2), pk, proof, inst_a)
    assert not verifier.verify_proof_with_shplonk(device, verifier.ParamsVerifier.from_params(params, public_inputs_size=1), pk, proof,
                                                  inst_a, report=report)
    assert isinstance(report["error"], verifier.InstanceTooLarge)


def test_params_from_an_srs_file_and_from_another_setup(device, setups, tmp_path):
    """s_g2 through the SRS file's additional_data (params_write -> params_read -> ParamsVerifier.from_params), a key from the
    circuit-data file alone, a verifier-params file; and the [s]G2 of a different s rejects the same proof"""
    from halo2_gpu_specific_amd import circuits, formats, pairing, prover, verifier
    from halo2_gpu_specific_amd.rng import ProverRng

    k = 9
    params, pv = setups(k)
    adv, fixed, copies = circuits.mini_plonk_synthesize(k)
    pk = prover.keygen(device, params, circuits.mini_plonk(), fixed, copies)
    proof = prover.create_proof(device, params, pk, adv, ProverRng(7))
    path = str(tmp_path / "srs.params")
    formats.params_write(device, params, path, formats.params_additional_data(params))
    params2, additional = formats.params_read(device, path)
    assert not hasattr(params2, "s_g2") and len(additional) == 64
    pv2 = verifier.ParamsVerifier.from_params(params2, additional)
    assert np.array_equal(pv2.s_g2, pv.s_g2)
    assert verifier.verify_proof(device, pv2, pk, proof)
    # a proof made under the parameters read back, verified with a key that never saw the proving key's polynomials
    pk2 = prover.keygen(device, params2, circuits.mini_plonk(), fixed, copies)
    proof2 = prover.create_proof_with_shplonk(device, params2, pk2, adv, ProverRng(8))
    data = str(tmp_path / "circuit.data")
    formats.circuit_data_write(data, device, params2, pk2)
    vk = verifier.VerifyingKey.from_info(formats.circuit_data_read(data, "mini-plonk"))
    assert vk.transcript_repr == pk2.transcript_repr
    assert verifier.verify_proof_with_shplonk(device, pv2, vk, proof2)
    # the verifier-params file, written from the device's points and read back on the host
    vpath = str(tmp_path / "verifier.params")
    formats.params_verifier_write(verifier.ParamsVerifier.from_params(params2, additional, public_inputs_size=4), vpath, device)
    pv3 = formats.params_verifier_read(vpath)
    assert pv3.public_inputs_size == 4 and verifier.verify_proof_with_shplonk(device, pv3, vk, proof2)
    # another setup
    other = prover.Params.unsafe_setup(device, k, S_TRAPDOOR + 1)
    assert not np.array_equal(other.s_g2, params.s_g2)
    assert not verifier.verify_proof(device, verifier.ParamsVerifier.from_params(other), pk, proof)
    assert not verifier.verify_proof(device, verifier.ParamsVerifier(k, pairing.g2_mul_generator(S_TRAPDOOR + 1), params.g_lagrange), pk, proof)


@pytest.mark.timeout(900)
def test_full_height_instance_column(device, setups):
    """n - (blinding_factors + 1) public inputs at k = 20: the verifier's O(n) step, one device MSM over g_lagrange"""
    from halo2_gpu_specific_amd import circuit as hc, prover, verifier
    from halo2_gpu_specific_amd.rng import ProverRng

    k = 20
    n = 1 << k
    cs = hc.ConstraintSystem("public-column")
    a, q, inst = cs.advice_column(), cs.fixed_column(), cs.instance_column()
    # (degree 3, so that both pieces of the quotient are non-zero polynomials: the identity cannot enter a transcript)
    cs.create_gate("public", [cs.query_fixed(q) * cs.query_advice(a) * (cs.query_advice(a) - cs.query_instance(inst))])
    usable = n - (cs.blinding_factors() + 1)
    values = (np.arange(usable, dtype=np.uint64) * np.uint64(2654435761) + np.uint64(17)) % np.uint64(1 << 40)
    adv = np.zeros((n, 4), dtype=np.uint64)
    adv[:usable, 0] = values
    fixed = np.zeros((n, 4), dtype=np.uint64)
    fixed[:usable, 0] = 1
    instances = [[int(v) for v in values]]
    params, pv = setups(k)
    pk = prover.keygen(device, params, cs, [fixed], np.zeros((0, 4), dtype=np.int64))
    proof = prover.create_proof_with_shplonk(device, params, pk, [adv], ProverRng(20), instances=instances)
    timings, report = {}, {}
    assert verifier.verify_proof_with_shplonk(device, pv, pk, proof, instances, timings=timings, report=report), report
    print("verify k=20, %d public inputs (ms):" % usable, {nm: round(t * 1e3, 2) for nm, t in timings.items()})
    as_array = np.zeros((usable, 4), dtype=np.uint64)          # the same values as a canonical (m, 4) array
    as_array[:, 0] = values
    assert verifier.verify_proof_with_shplonk(device, pv, pk, proof, [as_array])
    as_array[usable - 1, 0] += 1
    assert not verifier.verify_proof_with_shplonk(device, pv, pk, proof, [as_array])
    assert not verifier.verify_proof_with_shplonk(device, pv, pk, proof, [instances[0] + [0]], report=report)
    assert isinstance(report["error"], verifier.InstanceTooLarge)


@pytest.mark.timeout(900)
def test_batch_verifier(device, setups, monkeypatch):
    """36 proofs of k = 8 .. 12 (mini-PLONK by both schemes, and the lookup / shuffle circuit with public inputs): one
    accumulation, exactly two evaluation MSMs and one pairing check; one bad proof among them rejects"""
    from halo2_gpu_specific_amd import circuits, prover, verifier
    from halo2_gpu_specific_amd.rng import ProverRng

    entries = []                       # (vk, proof, instances, use_gwc, ParamsVerifier)
    for k in (8, 9, 10, 11, 12):
        params, pv = setups(k)
        adv, fixed, copies = circuits.mini_plonk_synthesize(k)
        pk = prover.keygen(device, params, circuits.mini_plonk(), fixed, copies)
        vk = verifier.VerifyingKey.from_proving_key(pk)
        for j in range(6):
            adv_j = circuits.mini_plonk_synthesize(k, a=5 + j)[0]
            use_gwc = j % 2 == 1
            entries.append((vk, prover.create_proof_ext(device, params, pk, adv_j, ProverRng(100 * k + j), use_gwc), (), use_gwc, pv))
    for k in (8, 9):
        params, pv = setups(k)
        adv, fixed, copies, inst = rp.LookupShuffle.synthesize(k)
        pk = prover.keygen(device, params, lookup_shuffle_cs(), [ints_to_arr(c) for c in fixed],
                           [(l[0], l[1], r[0], r[1]) for l, r in copies])
        vk = verifier.VerifyingKey.from_proving_key(pk)
        for j in range(3):
            proof = prover.create_proof_ext(device, params, pk, [ints_to_arr(c) for c in adv], ProverRng(7 * k + j), j == 1,
                                            instances=inst)
            entries.append((vk, proof, inst, j == 1, pv))
    assert len(entries) == 36

    counts = {"msm": 0, "msm_batch": 0, "pairing": 0}
    real_msm, real_batch, real_check = prover.Device.msm, prover.Device.msm_batch, verifier.pairing_check

    def counted(name, fn):
        def wrapper(*a, **kw):
            counts[name] += 1
            return fn(*a, **kw)
        return wrapper

    monkeypatch.setattr(prover.Device, "msm", counted("msm", real_msm))
    monkeypatch.setattr(prover.Device, "msm_batch", counted("msm_batch", real_batch))
    monkeypatch.setattr(verifier, "pairing_check", counted("pairing", real_check))

    def run(items, seed):
        batch = verifier.BatchVerifier(device, setups(12)[1], ProverRng(seed))
        for vk, proof, inst, use_gwc, pv in items:
            batch.process(vk, proof, inst, use_gwc, params=pv)
        for key in counts:
            counts[key] = 0
        return batch.finalize(), batch

    ok, batch = run(entries, 1)
    assert ok, batch.failed
    # two evaluation MSMs (each one Device.msm -> one msm_batch) + one msm_batch per (key, column length) of public inputs
    assert counts == {"msm": 2, "msm_batch": 2 + 2, "pairing": 1}
    print("batch of %d (ms):" % len(entries), {nm: round(t * 1e3, 2) for nm, t in batch.timings.items()},
          "terms:", len(batch.acc.left), len(batch.acc.right))
    for bad_at in (0, 17, 35):
        items = list(entries)
        vk, proof, inst, use_gwc, pv = items[bad_at]
        items[bad_at] = (vk, flip(proof, len(proof) // 2 + 1, 2), inst, use_gwc, pv)
        ok, batch = run(items, 2 + bad_at)
        assert not ok
    items = list(entries)
    vk, proof, inst, use_gwc, pv = items[31]
    items[31] = (vk, proof, [[43, 7]], use_gwc, pv)                       # a wrong public input
    assert not run(items, 9)[0]
    assert counts["msm"] == 2 and counts["pairing"] == 1
