"""configure -> synthesize -> check -> prove -> verify on a circuit whose witness needs its rows ORDERED: the memory-consistency
table of circuits_frontend.SortedAccessLog.  A seeded log of 2^(K-1) accesses (address, time, value, write flag) in program
order stands next to the same rows ordered by (address, time); a shuffle ties the two sides together, gates make a read return
what its address held, and a lookup of the gap between neighbours makes the order strict.  The sorted side is
`Value.sort_by([a, t], [a, t, v, w])` (values.py; csrc/sort.hip) and the gap columns are Value arithmetic over it: the log is
uploaded once and nothing of the witness is computed on the host.

usage: python examples/sorted_access_log.py [K]"""
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
circuit = fe.SortedAccessLog(k, addr_bits=max(1, k - 4), device=D)
t0 = time.perf_counter()
params = prover.Params.unsafe_setup(D, k, S)
cs, fixed, copies = prover.synthesize_keygen(D, circuit, k)
pk = prover.keygen(D, params, cs, fixed, copies)
D.sync()
print("setup + keygen: %.3f s (%d advice / %d fixed columns, degree %d, height %d)" % (
    time.perf_counter() - t0, cs.num_advice, cs.num_fixed, cs.degree(), circuit.height))
t0 = time.perf_counter()
advice, _ = prover.synthesize_witness(D, circuit, cs, k)
D.sync()
print("synthesize_witness: %.1f ms (%d sort, %d evaluator launches, %d inversion)" % (
    (time.perf_counter() - t0) * 1e3, D.values_sorts, D.values_launches, D.values_inversions))
A, T = (column[:6].to_ints() for column in circuit.columns()[4:6])
assert all((A[i], T[i]) < (A[i + 1], T[i + 1]) for i in range(5))
print("the sorted side begins (address, time): %s" % list(zip(A, T)))
failures, total = prover.check_witness(D, pk, advice)
assert total == 0, failures
t0 = time.perf_counter()
proof = prover.create_proof_with_shplonk(D, params, pk, advice, ProverRng(1))
D.sync()
print("create_proof: %.1f ms, %d bytes" % ((time.perf_counter() - t0) * 1e3, len(proof)))
ok = verifier.verify_proof_with_shplonk(D, verifier.ParamsVerifier.from_params(params), verifier.VerifyingKey.from_proving_key(pk), proof)
print("verify_proof: %s" % ok)
assert ok
