"""configure -> synthesize -> check -> prove -> verify on the circuit of the reference's examples/shuffle.rs with its witness
COMPUTED ON THE DEVICE: circuits_frontend.ShuffleGatesValues draws the random originals on the host (the same seeded stream as
circuits.shuffle_gates_witness), and everything after that -- the shuffled columns, the theta-compressions, the quotients
(compress(original) + beta) / (compress(shuffled) + beta) and their running product z -- is Value arithmetic (values.py): two
launches of the fused evaluator, one batch inversion, one scan, at the full height of the 2^K rows.

usage: python examples/shuffle_values.py [K]"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")  # before HIP initialises (halo2-gpu-specific_amd/__init__.py says why)
import torch  # noqa: E402  (first: the library binds to torch's HIP runtime)

torch.cuda.init()

from halo2_gpu_specific_amd import circuits_frontend as fe, prover, verifier  # noqa: E402
from halo2_gpu_specific_amd.rng import ProverRng  # noqa: E402

k = int(sys.argv[1]) if len(sys.argv) > 1 else 12
S = 0x1D0C5F0A3B7E91C2A4D6F8091B2C3D4E5F60718293A4B5C6D7E8F9010203   # Params::unsafe_setup's toxic scalar, fixed here

D = prover.Device()
height = (1 << k) - 7                      # usable - 1: z takes one row more
circuit = fe.ShuffleGatesValues(k, height=height, device=D)
t0 = time.perf_counter()
params = prover.Params.unsafe_setup(D, k, S)
cs, fixed, copies = prover.synthesize_keygen(D, circuit, k)
pk = prover.keygen(D, params, cs, fixed, copies)
D.sync()
print("setup + keygen: %.3f s (%d advice / %d fixed columns, height %d)" % (time.perf_counter() - t0, cs.num_advice, cs.num_fixed, height))
t0 = time.perf_counter()
advice, _ = prover.synthesize_witness(D, circuit, cs, k)
D.sync()
print("synthesize_witness: %.1f ms (%d evaluator launches, %d batch inversions)" % (
    (time.perf_counter() - t0) * 1e3, D.values_launches, D.values_inversions))
z = circuit.columns()[-1]
assert z[height].to_ints() == [1], "the running product does not return to 1"
failures, total = prover.check_witness(D, pk, advice)
assert total == 0, failures
t0 = time.perf_counter()
proof = prover.create_proof_with_shplonk(D, params, pk, advice, ProverRng(1))
D.sync()
print("create_proof: %.1f ms, %d bytes" % ((time.perf_counter() - t0) * 1e3, len(proof)))
ok = verifier.verify_proof_with_shplonk(D, verifier.ParamsVerifier.from_params(params), verifier.VerifyingKey.from_proving_key(pk), proof)
print("verify_proof: %s" % ok)
assert ok
