"""configure -> synthesize -> keygen -> create_proof -> verify for the reference's examples/lookup_api.rs, written the way the
reference writes it: a `Circuit` with `configure` and `synthesize`, laid out by the V1 floor planner
(halo2-gpu-specific_amd/circuits_frontend.py: LookupApi; synthesis.py: Layouter, Region, Table, V1).  Nothing here fills a
column by hand: the fixed columns, the table's default fill, the copy constraints and the witness come out of the front end,
the witness assembled in device memory by one launch of h2_dev_cells_place.

usage: python examples/lookup_api.py [k] [gwc|shplonk]"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")  # before HIP initialises (halo2-gpu-specific_amd/__init__.py says why)
import torch  # noqa: E402  (first: the library binds to torch's HIP runtime)

torch.cuda.init()

from halo2_gpu_specific_amd import circuits_frontend, prover, verifier  # noqa: E402
from halo2_gpu_specific_amd.rng import ProverRng  # noqa: E402

k = int(sys.argv[1]) if len(sys.argv) > 1 else 10
use_gwc = (sys.argv[2] if len(sys.argv) > 2 else "shplonk") == "gwc"
S = 0x1D0C5F0A3B7E91C2A4D6F8091B2C3D4E5F60718293A4B5C6D7E8F9010203   # Params::unsafe_setup's toxic scalar, fixed here

D = prover.Device()
circuit = circuits_frontend.LookupApi()
params = prover.Params.unsafe_setup(D, k, S)
t0 = time.perf_counter()
cs, fixed, copies = prover.synthesize_keygen(D, circuit, k, resident=True)      # configure + the keygen pass under V1
pk = prover.keygen(D, params, cs, fixed, copies)
print("regions start at rows %s; synthesize + keygen: %.3f s" % (prover.region_starts(circuit), time.perf_counter() - t0))

t0 = time.perf_counter()
advice, first_unassigned = prover.synthesize_witness(D, circuit, pk, k)          # the witness pass, columns resident
assert prover.check_witness(D, pk, advice) == ([], 0)                            # MockProver::verify
proof = prover.create_proof_ext(D, params, pk, advice, ProverRng(), use_gwc, first_unassigned=first_unassigned)
D.sync()
print("synthesize + check + create_proof (%s): %.1f ms, %d bytes" % ("GWC" if use_gwc else "SHPLONK",
                                                                     (time.perf_counter() - t0) * 1e3, len(proof)))

vparams = verifier.ParamsVerifier.from_params(params)
vk = verifier.VerifyingKey.from_proving_key(pk)
ok = verifier.verify_proof_ext(D, vparams, vk, proof, (), use_gwc)
tampered = bytearray(proof)
tampered[40] ^= 1
bad = verifier.verify_proof_ext(D, vparams, vk, bytes(tampered), (), use_gwc)
print("verify_proof: %s; tampered proof: %s" % (ok, bad))
assert ok and not bad
