"""The host half of the product verifier (halo2-gpu-specific_amd/verifier.py: pair_msm, PairMSM, BatchVerifier), the read
side of the transcript and the verifier-params file, against the big-integer twin tests/ref_plonk.py.  Proofs come from the
twin's prover at k <= 7; the decision runs through the library's host pairing.  No device is needed or touched."""
import random

import numpy as np
import pytest

import bn254_pairing as bp
import ref_plonk as rp
from product_circuits import lookup_shuffle_cs, rot_gate_cs

from halo2_gpu_specific_amd import circuits, formats, pairing, prover, transcript, verifier
from halo2_gpu_specific_amd.rng import ProverRng

S_TRAPDOOR = 0x1D0C5F0A3B7E91C2A4D6F8091B2C3D4E5F60718293A4B5C6D7E8F9010203
NO_POINTS = np.zeros((0, 8), dtype=np.uint64)


class Case:
    """a twin circuit with its key, the product-side verifying key of the same circuit and a witness"""

    def __init__(self, name, W, cs, k, adv, fixed, copies, inst=(), circuits_=None):
        self.name, self.W, self.k, self.adv, self.inst, self.circuits = name, W, k, adv, inst, circuits_
        self.pk = rp.keygen(W, k, S_TRAPDOOR, fixed, copies)
        self.vk = verifier.VerifyingKey(cs, prover.Domain(k, cs.degree()), self.pk.fixed_commitments,
                                        self.pk.perm_commitments, self.pk.transcript_repr)
        self.proofs = {}

    def proof(self, use_gwc):
        if use_gwc not in self.proofs:
            self.proofs[use_gwc] = rp.create_proof(self.pk, self.adv, ProverRng(4), use_gwc=use_gwc, instances=self.inst)
        return self.proofs[use_gwc]

    def commitments(self, instances=None):
        """the instance commitments, by the twin's trapdoor commit (the device makes them in the product)"""
        sets = [self.inst if instances is None else instances] if self.circuits is None else (instances or self.inst)
        dom = self.pk.dom
        return [[rp.commit(self.pk, dom.lagrange_to_coeff(list(v) + [0] * (dom.n - len(v)))) for v in inst] for inst in sets]

    def twin(self, proof, use_gwc, instances=None, pairing_=False):
        return rp.verify_proof(self.pk, proof, use_gwc=use_gwc, pairing=pairing_,
                               instances=self.inst if instances is None else instances, circuits=self.circuits)

    def pair(self, proof, use_gwc, instances=None):
        inst = self.inst if instances is None else instances
        return verifier.pair_msm(self.vk, proof, inst, self.commitments(instances), use_gwc, circuits=self.circuits)


def _cases():
    out = []
    adv, fixed, copies = rp.MiniPlonk.synthesize(4)
    out.append(Case("mini", rp.MiniPlonk, circuits.mini_plonk(), 4, adv, fixed, copies))
    adv, fixed, copies = rp.RotGate.synthesize(5)
    out.append(Case("rot", rp.RotGate, rot_gate_cs(), 5, adv, fixed, copies))
    adv, fixed, copies, inst = rp.LookupShuffle.synthesize(5)
    out.append(Case("lookup-shuffle", rp.LookupShuffle, lookup_shuffle_cs(), 5, adv, fixed, copies, inst))
    k, vmax, step = 7, 30, 2
    W = rp.range_check_class(0, vmax, step)
    radv, rfixed, _ = circuits.range_check_synthesize(k, vmin=0, vmax=vmax, count=60)
    want = W.complete(k, [int(v) for v in radv[0][:, 0]])
    out.append(Case("range-check", W, circuits.range_check(0, vmax, step), k, want, [[int(v) for v in f[:, 0]] for f in rfixed], []))
    adv2 = [c[:] for c in adv]
    adv2[11][0] = 43                                   # the second circuit's public input
    out.append(Case("two-instances", rp.LookupShuffle, lookup_shuffle_cs(), 5, [adv, adv2], fixed, copies,
                    [inst, [[43, 7]]], circuits_=2))
    return out


@pytest.fixture(scope="module")
def cases():
    return {c.name: c for c in _cases()}


@pytest.fixture(scope="module")
def params():
    return verifier.ParamsVerifier(7, pairing.g2_mul_generator(S_TRAPDOOR), NO_POINTS)


@pytest.fixture()
def recorded(monkeypatch):
    """the (left, right) points ref_plonk.verify_proof hands to its opening_check"""
    seen, original = [], rp.opening_check

    def recording(pk, left, right, pairing_):
        seen.append((left, right))
        return original(pk, left, right, pairing_)

    monkeypatch.setattr(rp, "opening_check", recording)
    return seen


def eval_with_twin(msm):
    acc = None
    for scalar, base in msm.items():
        acc = rp.g1_add(acc, rp.g1_mul(base, scalar))
    return acc


NAMES = ["mini", "rot", "lookup-shuffle", "range-check", "two-instances"]


@pytest.mark.parametrize("use_gwc", [False, True])
@pytest.mark.parametrize("name", NAMES)
def test_pair_msm_and_decision_match_the_twin(cases, params, recorded, name, use_gwc):
    c = cases[name]
    proof = c.proof(use_gwc)
    want = c.twin(proof, use_gwc, pairing_=True)
    assert want is True and len(recorded) == 1
    pair = c.pair(proof, use_gwc)
    assert (eval_with_twin(pair.left), eval_with_twin(pair.right)) == recorded[0]
    assert (verifier.msm_eval_host(pair.left), verifier.msm_eval_host(pair.right)) == recorded[0]
    assert verifier.decide_host(params, pair) is want
    # under the [s]G2 of another setup the same proof is rejected
    other = verifier.ParamsVerifier(c.k, pairing.g2_mul_generator(S_TRAPDOOR + 1), NO_POINTS)
    assert verifier.decide_host(other, pair) is False


def product_decision(c, params, proof, use_gwc, instances=None):
    """(decision, error): the product's host path, every rejection a return value or a typed error"""
    try:
        return verifier.decide_host(params, c.pair(proof, use_gwc, instances)), None
    except (verifier.VerifyError, transcript.TranscriptError, pairing.PointError) as e:
        return False, e


def twin_decision(c, proof, use_gwc, instances=None):
    """the twin's decision, None where it asserts instead of returning"""
    try:
        return c.twin(proof, use_gwc, instances)
    except (AssertionError, IndexError, ValueError):
        return None


def sections(c, use_gwc):
    """(name, first byte) of every distinct section of the proof stream, in the transcript's order (verifier.rs:165-260)"""
    cs, n = c.vk.cs, c.circuits or 1
    chunk = cs.degree() - 2
    nsets = (len(cs.perm_columns) + chunk - 1) // chunk
    layout = [("advice commitments", n * cs.num_advice), ("lookup m commitments", n * len(cs.lookups)),
              ("permutation z commitments", n * nsets), ("lookup z commitments", n * sum(len(s) for _, _, s in cs.lookups)),
              ("shuffle z commitments", n * len(cs.shuffles)), ("random commitment", 1),
              ("h commitments", c.vk.domain.quotient_poly_degree), ("instance evals", n * len(cs.instance_queries)),
              ("advice evals", n * len(cs.advice_queries)), ("fixed evals", len(cs.fixed_queries)), ("random eval", 1),
              ("sigma evals", len(cs.perm_columns)), ("permutation z evals", n * max(0, 3 * nsets - 1)),
              ("lookup evals", n * sum(1 + 3 * len(s) - 1 for _, _, s in cs.lookups)),
              ("shuffle evals", n * 2 * len(cs.shuffles))]
    out, pos = [], 0
    for name, count in layout:
        if count:
            out.append((name, pos))
        pos += 32 * count
    total = len(c.proof(use_gwc))
    assert pos < total and (total - pos) % 32 == 0
    out.append(("opening points", pos))
    out.append(("last opening point", total - 32))
    return out


@pytest.mark.parametrize("use_gwc", [False, True])
@pytest.mark.parametrize("name", NAMES)
def test_tampered_proofs_are_rejected_without_assertions(cases, params, name, use_gwc):
    c = cases[name]
    proof = c.proof(use_gwc)
    assert product_decision(c, params, proof, use_gwc) == (True, None)
    corpus = []
    for what, pos in sections(c, use_gwc):
        for bit in (0, 3):
            bad = bytearray(proof)
            bad[pos + 1] ^= 1 << bit
            corpus.append(("%s bit %d" % (what, bit), bytes(bad), None))
    corpus.append(("truncated", proof[:-32], None))
    corpus.append(("cut inside a field", proof[:-5], None))
    corpus.append(("empty", b"", None))
    corpus.append(("one byte appended", proof + b"\x00", None))
    first_scalar = dict(sections(c, use_gwc)).get("advice evals")
    corpus.append(("a scalar equal to r", proof[:first_scalar] + rp.R.to_bytes(32, "little") + proof[first_scalar + 32:], None))
    x = next(x for x in range(2, 100) if pow((x ** 3 + 3) % rp.Q, (rp.Q - 1) // 2, rp.Q) != 1)
    corpus.append(("an x with no square root", x.to_bytes(32, "little") + proof[32:], None))
    corpus.append(("an x of q or above", (rp.Q + 1).to_bytes(32, "little") + proof[32:], None))
    if c.vk.cs.num_instance:
        single = c.inst if c.circuits is None else c.inst[0]
        wrong = [[(single[0][0] + 1) % rp.R] + list(single[0][1:])] + [list(v) for v in single[1:]]
        corpus.append(("a wrong instance value", proof, wrong if c.circuits is None else [wrong] + list(c.inst[1:])))
    for what, bad, instances in corpus:
        got, error = product_decision(c, params, bad, use_gwc, instances)        # (anything else raised fails the test)
        assert got is False, what
        want = twin_decision(c, bad, use_gwc, instances)
        assert want in (None, False), what
        if what.startswith(("truncated", "cut", "empty", "one byte", "a scalar", "an x")):
            assert isinstance(error, transcript.TranscriptError), what


def test_instance_checks_are_typed_errors(cases, params):
    c = cases["lookup-shuffle"]
    proof = c.proof(False)
    usable = c.pk.dom.n - (c.vk.cs.blinding_factors() + 1)
    with pytest.raises(verifier.InstanceTooLarge):
        verifier.pair_msm(c.vk, proof, [[1] * (usable + 1)], [[rp.G1]], False)
    with pytest.raises(verifier.InvalidInstances):
        verifier.pair_msm(c.vk, proof, [[42, 7], [1]], [[rp.G1, rp.G1]], False)
    with pytest.raises(verifier.InvalidInstances):
        verifier.pair_msm(c.vk, proof, [], [[]], False)
    with pytest.raises(verifier.InvalidInstances):
        verifier.pair_msm(c.vk, proof, [c.inst], [[rp.G1]], False, circuits=2)
    assert issubclass(verifier.InstanceTooLarge, verifier.VerifyError) and not issubclass(verifier.VerifyError, AssertionError)
    # too many values for the ParamsVerifier's Lagrange points: refused before anything is committed
    few = verifier.ParamsVerifier(5, params.s_g2, np.zeros((1, 8), dtype=np.uint64))
    with pytest.raises(verifier.InstanceTooLarge):
        verifier.commit_instances(None, few, c.vk, [[[42, 7]]])


class FixedRng:
    def __init__(self, values):
        self.values = list(values)

    def fr(self):
        return self.values.pop(0)


def test_batch_verifier_accumulates_the_random_combination(cases, params):
    batch_cases = [(cases["mini"], False), (cases["rot"], True), (cases["lookup-shuffle"], False), (cases["range-check"], True)]
    pairs = [c.pair(c.proof(g), g) for c, g in batch_cases]
    rnd = ProverRng(99)
    rs = [rnd.fr() for _ in pairs]
    batch = verifier.BatchVerifier(None, params, ProverRng(99))
    for p in pairs:
        batch.accumulate(p)
    # by hand: acc = r_i * acc + pair_i  ==  sum_i (prod_{j > i} r_j) pair_i
    want_left = want_right = None
    for i, p in enumerate(pairs):
        w = 1
        for r in rs[i + 1:]:
            w = w * r % rp.R
        want_left = rp.g1_add(want_left, rp.g1_mul(eval_with_twin(p.left), w))
        want_right = rp.g1_add(want_right, rp.g1_mul(eval_with_twin(p.right), w))
    assert (eval_with_twin(batch.acc.left), eval_with_twin(batch.acc.right)) == (want_left, want_right)
    assert verifier.decide_host(params, batch.acc) is True
    assert rp.g1_mul(want_left, S_TRAPDOOR) == want_right                       # the trapdoor statement of the same sum
    # any one proof replaced by a tampered one: the batch rejects
    for bad_at in range(len(batch_cases)):
        batch = verifier.BatchVerifier(None, params, ProverRng(5 + bad_at))
        for i, (c, g) in enumerate(batch_cases):
            proof = c.proof(g)
            if i == bad_at:
                pos = dict(sections(c, g))["advice evals"]
                proof = proof[:pos] + ((int.from_bytes(proof[pos:pos + 32], "little") + 1) % rp.R).to_bytes(32, "little") + proof[pos + 32:]
            batch.accumulate(c.pair(proof, g))
        assert verifier.decide_host(params, batch.acc) is False, bad_at
    # parameters of another setup cannot join a batch
    other = verifier.ParamsVerifier(4, pairing.g2_mul_generator(5), NO_POINTS)
    with pytest.raises(ValueError):
        verifier.BatchVerifier(None, params, ProverRng(1)).process(cases["mini"].vk, b"", params=other)


def test_blake2b_read_reproduces_every_challenge():
    rnd = random.Random(11)
    w = transcript.Blake2bWrite()
    script, challenges = [], []
    w.common_scalar(12345)
    for step in range(40):
        kind = rnd.choice("psc")
        if kind == "p":
            P = rp.g1_mul(rp.G1, rnd.randrange(1, rp.R))
            w.write_point(P)
            script.append(("p", P))
        elif kind == "s":
            v = rnd.choice([0, 1, rp.R - 1, rnd.randrange(rp.R)])
            w.write_scalar(v)
            script.append(("s", v))
        else:
            challenges.append(w.squeeze_challenge_scalar())
            script.append(("c", None))
    proof = w.finalize()
    r = transcript.Blake2bRead(proof)
    r.common_scalar(12345)
    got = []
    for kind, value in script:
        if kind == "p":
            assert r.read_point() == value
        elif kind == "s":
            assert r.read_scalar() == value
        else:
            got.append(r.squeeze_challenge_scalar())
    assert got == challenges and len(set(got)) == len(got)
    assert r.remaining() == 0
    r.expect_end()
    with pytest.raises(transcript.TranscriptError):
        r.read_scalar()
    with pytest.raises(transcript.TranscriptError):
        transcript.Blake2bRead(proof + b"\x01").expect_end()
    with pytest.raises(transcript.TranscriptError):
        transcript.Blake2bRead(rp.R.to_bytes(32, "little")).read_scalar()
    with pytest.raises(transcript.TranscriptError):
        transcript.Blake2bRead((rp.Q).to_bytes(32, "little")).read_point()
    with pytest.raises(transcript.TranscriptError):
        transcript.Blake2bRead(bytes(32)).read_point()          # the identity cannot enter the transcript
    with pytest.raises(transcript.TranscriptError):
        transcript.Blake2bRead(bytes(31)).read_point()
    assert issubclass(transcript.TranscriptError, ValueError) and not issubclass(transcript.TranscriptError, AssertionError)


def test_params_verifier_file_round_trips(tmp_path):
    points = [rp.g1_mul(rp.G1, 3 + i) for i in range(5)] + [None]
    g_lagrange = np.array([pairing.g1_limbs(P) for P in points], dtype=np.uint64)
    pv = verifier.ParamsVerifier(9, pairing.g2_mul_generator(S_TRAPDOOR), g_lagrange)
    path = str(tmp_path / "verifier.params")
    formats.params_verifier_write(pv, path)
    raw = open(path, "rb").read()
    assert len(raw) == 4 + 4 + 32 + 64 + 64 + 32 * 6 and raw[:8] == (9).to_bytes(4, "little") + (6).to_bytes(4, "little")
    assert raw[8:40] == transcript.point_to_bytes((1, 2)) and raw[168:200] == transcript.point_to_bytes(points[0])
    back = formats.params_verifier_read(path)
    assert (back.k, back.n, back.public_inputs_size, back.g1) == (9, 512, 6, (1, 2))
    assert np.array_equal(back.g2, pv.g2) and np.array_equal(back.s_g2, pv.s_g2)
    assert np.array_equal(back.g_lagrange, g_lagrange)
    assert pairing.g2_compress(back.s_g2) == raw[104:168]
    open(path, "wb").write(raw[:-1])
    with pytest.raises(IOError):
        formats.params_verifier_read(path)
    open(path, "wb").write(raw[:104] + bytes(63) + b"\x80" + raw[168:])
    with pytest.raises(ValueError):
        formats.params_verifier_read(path)
    # Params::verifier from (Params, additional_data): the [s]G2 of the SRS file, or the one unsafe_setup recorded
    class P:
        k, n, g_lagrange = 3, 8, np.zeros((8, 8), dtype=np.uint64)
    via_file = verifier.ParamsVerifier.from_params(P, pairing.g2_compress(pv.s_g2), public_inputs_size=2)
    assert np.array_equal(via_file.s_g2, pv.s_g2) and via_file.public_inputs_size == 2 and via_file.g_lagrange.shape == (2, 8)
    with pytest.raises(ValueError):
        verifier.ParamsVerifier.from_params(P)
    P.s_g2 = pv.s_g2
    assert np.array_equal(verifier.ParamsVerifier.from_params(P).s_g2, pv.s_g2)
    with pytest.raises(ValueError):
        verifier.ParamsVerifier.from_params(P, public_inputs_size=9)
    assert bp.g2_mul(bp.G2, S_TRAPDOOR) is not None
