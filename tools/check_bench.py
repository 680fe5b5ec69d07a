"""prover.check_witness per phase next to one create_proof_ext of the same witness in the same process: the wide circuit
(circuits.wide, compact witness in pinned host memory, as wide_bench.py's `compact`) and mini-PLONK, real SRS from the
device setup.   usage: python tools/check_bench.py [k] [quads]"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")  # before HIP initialises (halo2-gpu-specific_amd/__init__.py says why)
import torch  # noqa: E402

torch.cuda.init()

from halo2_gpu_specific_amd import circuits, prover  # noqa: E402
from halo2_gpu_specific_amd.rng import ProverRng  # noqa: E402

k = int(sys.argv[1]) if len(sys.argv) > 1 else 20
quads = int(sys.argv[2]) if len(sys.argv) > 2 else 16
D = prover.Device()
params = prover.Params.unsafe_setup(D, k, 0x1D0C5F0A3B7E91C2A4D6F8091B2C3D4E5F60718293A4B5C6D7E8F9010203)
legs = [("wide-%d" % quads, circuits.wide(quads), lambda: circuits.wide_synthesize(k, quads, alloc=D.pinned_columns, compact=True)),
        ("mini-plonk", circuits.mini_plonk(), lambda: circuits.mini_plonk_synthesize(k, alloc=D.pinned_columns))]
for name, cs, synthesize in legs:
    adv, fixed, copies = synthesize()
    t0 = time.perf_counter()
    pk = prover.keygen(D, params, cs, fixed, copies)
    D.sync()
    print("%s k=%d: keygen %.3f s" % (name, k, time.perf_counter() - t0))
    prover.create_proof_ext(D, params, pk, adv, ProverRng(0), False)      # warm-up (and the generated kernels' first build)
    prover.check_witness(D, pk, adv)
    D.sync()
    ta = time.perf_counter()
    prover.create_proof_ext(D, params, pk, adv, ProverRng(1), False)
    D.sync()
    proof_ms = (time.perf_counter() - ta) * 1e3
    for rep in range(3):
        phases = {}
        ta = time.perf_counter()
        failures, total = prover.check_witness(D, pk, adv)
        whole = (time.perf_counter() - ta) * 1e3
        assert (failures, total) == ([], 0), "the benchmark witness does not satisfy its circuit"
        timed = {}
        prover.check_witness(D, pk, adv, timings=timed)       # the same check synchronised between phases
        print("%s k=%d rep %d: check %.1f ms (proof %.1f ms, ratio %.3f); phases %s" % (
            name, k, rep, whole, proof_ms, whole / proof_ms, {a: round(b * 1e3, 2) for a, b in timed.items()}))
    del pk, adv, fixed
