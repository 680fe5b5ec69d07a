"""configure -> synthesize -> check -> prove -> verify on a circuit whose witness needs a cell read as an INTEGER:
circuits_frontend.LimbDecomposition multiplies two seeded u64 columns, keeps the low 32 bits of the product and splits them into
four 8-bit limbs, each looked up in a 256-row range table and tied to the product by a gate.  The product, its low bits and the
limbs are Value arithmetic (values.py: `(a * b).low(32)` and `.limbs(8, 4, strict=True)`), computed on the device at the full
height of the 2^K rows; nothing of the witness is computed on the host.

usage: python examples/limb_decomposition.py [K]"""
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
circuit = fe.LimbDecomposition(k, device=D)
t0 = time.perf_counter()
params = prover.Params.unsafe_setup(D, k, S)
cs, fixed, copies = prover.synthesize_keygen(D, circuit, k)
pk = prover.keygen(D, params, cs, fixed, copies)
D.sync()
print("setup + keygen: %.3f s (%d advice / %d fixed columns, height %d)" % (time.perf_counter() - t0, cs.num_advice, cs.num_fixed, circuit.height))
t0 = time.perf_counter()
advice, _ = prover.synthesize_witness(D, circuit, cs, k)
D.sync()
print("synthesize_witness: %.1f ms (%d evaluator launches)" % ((time.perf_counter() - t0) * 1e3, D.values_launches))
a, b, p = (column[:3].to_ints() for column in circuit.columns()[:3])
limbs = [column[:3].to_ints() for column in circuit.columns()[3:]]
for row in range(3):
    assert p[row] == a[row] * b[row] % (1 << 32) == sum(limb[row] << (8 * j) for j, limb in enumerate(limbs))
failures, total = prover.check_witness(D, pk, advice)
assert total == 0, failures
t0 = time.perf_counter()
proof = prover.create_proof_with_shplonk(D, params, pk, advice, ProverRng(1))
D.sync()
print("create_proof: %.1f ms, %d bytes" % ((time.perf_counter() - t0) * 1e3, len(proof)))
ok = verifier.verify_proof_with_shplonk(D, verifier.ParamsVerifier.from_params(params), verifier.VerifyingKey.from_proving_key(pk), proof)
print("verify_proof: %s" % ok)
assert ok
