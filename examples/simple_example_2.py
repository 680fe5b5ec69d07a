"""keygen -> create_proof -> verify on the mini-PLONK circuit of the reference's examples/simple-example-2.rs:177-288
(3 advice columns a, b, c with equality, 4 fixed columns sm, sa, sb, sc, one gate a*sa + b*sb + a*b*sm - c*sc,
2^(k-4) multiply / add pairs with two copy constraints each, witness a = 5), on one MI355X.

Prover and verifier are the product path (halo2-gpu-specific_amd/prover.py and verifier.py over libhalo2_hip.so: there is no
CPU fallback): the verifier's MSMs run on the device, its BN254 pairing check on the host, and nothing of it knows the
setup's toxic scalar -- only the [s]G2 that `unsafe_setup` hands to the ParamsVerifier.

usage: python examples/simple_example_2.py [k] [gwc|shplonk]"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")  # before HIP initialises (halo2-gpu-specific_amd/__init__.py says why)
import torch  # noqa: E402  (first: the library binds to torch's HIP runtime)

torch.cuda.init()

from halo2_gpu_specific_amd import circuits, prover, verifier  # noqa: E402
from halo2_gpu_specific_amd.rng import ProverRng  # noqa: E402

k = int(sys.argv[1]) if len(sys.argv) > 1 else 8
use_gwc = (sys.argv[2] if len(sys.argv) > 2 else "shplonk") == "gwc"
S = 0x1D0C5F0A3B7E91C2A4D6F8091B2C3D4E5F60718293A4B5C6D7E8F9010203   # Params::unsafe_setup's toxic scalar, fixed here

D = prover.Device()
t0 = time.perf_counter()
params = prover.Params.unsafe_setup(D, k, S)                       # poly/commitment.rs:56-124, on the device
advice, fixed, copies = circuits.mini_plonk_synthesize(k, alloc=D.pinned_columns)
pk = prover.keygen(D, params, circuits.mini_plonk(), fixed, copies)  # keygen_vk + keygen_pk
print("setup + keygen: %.3f s" % (time.perf_counter() - t0))

t0 = time.perf_counter()
proof = prover.create_proof_ext(D, params, pk, advice, ProverRng(), use_gwc)
D.sync()
print("create_proof (%s): %.1f ms, %d bytes" % ("GWC" if use_gwc else "SHPLONK", (time.perf_counter() - t0) * 1e3, len(proof)))

vparams = verifier.ParamsVerifier.from_params(params)               # Params::verifier: k, g1, g2, [s]G2, g_lagrange
vk = verifier.VerifyingKey.from_proving_key(pk)
timings = {}
t0 = time.perf_counter()
ok = verifier.verify_proof_ext(D, vparams, vk, proof, (), use_gwc, timings=timings)
print("verify_proof: %s in %.1f ms %s" % (ok, (time.perf_counter() - t0) * 1e3, {a: round(b * 1e3, 2) for a, b in timings.items()}))
tampered = bytearray(proof)
tampered[40] ^= 1
why = {}
bad = verifier.verify_proof_ext(D, vparams, vk, bytes(tampered), (), use_gwc, report=why)
print("tampered proof: %s (%s)" % (bad, why.get("error")))
assert ok and not bad
