"""The reference's examples/two-chip.rs: d = (a + b) * c by an add chip and a mul chip, each under a simple selector of its own, d
a public input (halo2-gpu-specific_amd/circuits_frontend.py: TwoChip).  As the example does: configure, synthesize and
check the witness -- MockProver::verify is prover.check_witness -- with the right public input and with a wrong one, which the
permutation check rejects.  Going beyond it: keygen, create_proof and verify_proof.  The selectors never become 32-byte
columns on the host: their activations are marked into device bitmaps and the fixed columns compress_selectors asks for are
written there (csrc/selectors.hip).

usage: python examples/two_chip.py [gwc|shplonk]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")  # before HIP initialises (halo2-gpu-specific_amd/__init__.py says why)
import torch  # noqa: E402  (first: the library binds to torch's HIP runtime)

torch.cuda.init()

from halo2_gpu_specific_amd import check, circuits_frontend, prover, verifier  # noqa: E402
from halo2_gpu_specific_amd.rng import ProverRng  # noqa: E402

use_gwc = (sys.argv[1] if len(sys.argv) > 1 else "shplonk") == "gwc"
S = 0x1D0C5F0A3B7E91C2A4D6F8091B2C3D4E5F60718293A4B5C6D7E8F9010203   # Params::unsafe_setup's toxic scalar, fixed here
k = 4                                                                 # the example's own size

D = prover.Device()
circuit = circuits_frontend.TwoChip(a=11, b=13, c=17)                     # the example draws a, b, c at random
public_inputs = circuit.public_inputs()                               # [[(11 + 13) * 17]]
params = prover.Params.unsafe_setup(D, k, S)
cs, fixed, copies = prover.synthesize_keygen(D, circuit, k, resident=True)
print("selectors -> fixed columns: %s; regions start at rows %s" % (cs.selector_map, prover.region_starts(circuit)))
pk = prover.keygen(D, params, cs, fixed, copies)

advice, first_unassigned = prover.synthesize_witness(D, circuit, pk, k, instances=public_inputs)
assert prover.check_witness(D, pk, advice, public_inputs) == ([], 0)             # assert_eq!(prover.verify(), Ok(()))
wrong = [[public_inputs[0][0] + 1]]
failures, total = prover.check_witness(D, pk, advice, wrong)                     # assert!(prover.verify().is_err())
assert total == 2 and all(isinstance(f, check.Permutation) for f in failures)
print("wrong public input:", failures)

proof = prover.create_proof_ext(D, params, pk, advice, ProverRng(), use_gwc, instances=public_inputs,
                                first_unassigned=first_unassigned)
vparams = verifier.ParamsVerifier.from_params(params)
vk = verifier.VerifyingKey.from_proving_key(pk)
ok = verifier.verify_proof_ext(D, vparams, vk, proof, public_inputs, use_gwc)
bad = verifier.verify_proof_ext(D, vparams, vk, proof, wrong, use_gwc)
print("proof of %d bytes (%s): verify_proof %s; under the wrong public input %s" % (len(proof), "GWC" if use_gwc else "SHPLONK", ok, bad))
assert ok and not bad
