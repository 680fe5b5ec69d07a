"""verify_proof and BatchVerifier timed per phase on the device: mini-PLONK at 2^K rows, one proof (both multiopen schemes)
and a batch of M proofs.  Phases (verifier.PHASES): the instance commitments (device MSMs over g_lagrange; mini-PLONK has
no instance column, so the phase is empty here), the host pair_msm, the evaluation of the PairMSM (two device MSMs) and the
pairing check (host).  The create_proof time of the same proof is printed next to it.  One JSON line per measurement.
usage: python tools/verify_bench.py K [M] [--reps N]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")  # before HIP initialises (halo2-gpu-specific_amd/__init__.py says why)
import torch  # noqa: E402  (first: the library binds to torch's HIP runtime)

torch.cuda.init()

from halo2_gpu_specific_amd import circuits, prover, verifier  # noqa: E402
from halo2_gpu_specific_amd.rng import ProverRng  # noqa: E402

S = 0x1D0C5F0A3B7E91C2A4D6F8091B2C3D4E5F60718293A4B5C6D7E8F9010203


def ms(seconds):
    return round(seconds * 1e3, 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("k", type=int)
    ap.add_argument("batch", type=int, nargs="?", default=0)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    D = prover.Device()
    params = prover.Params.unsafe_setup(D, args.k, S)
    pv = verifier.ParamsVerifier.from_params(params)
    advice, fixed, copies = circuits.mini_plonk_synthesize(args.k)
    pk = prover.keygen(D, params, circuits.mini_plonk(), fixed, copies)
    vk = verifier.VerifyingKey.from_proving_key(pk)
    for use_gwc in (False, True):
        prove = []
        for rep in range(2):
            t0 = time.perf_counter()
            proof = prover.create_proof_ext(D, params, pk, advice, ProverRng(rep), use_gwc)
            D.sync()
            prove.append(time.perf_counter() - t0)
        runs, totals = [], []
        for rep in range(args.reps + 1):
            timings = {}
            t0 = time.perf_counter()
            ok = verifier.verify_proof_ext(D, pv, vk, proof, (), use_gwc, timings=timings)
            totals.append(time.perf_counter() - t0)
            assert ok, "the proof was rejected"
            runs.append(timings)
        runs, totals = runs[1:], totals[1:]                     # the first run builds the pairing's constants and warms the MSM
        print(json.dumps({"what": "verify_proof", "circuit": "mini-plonk", "k": args.k, "scheme": "gwc" if use_gwc else "shplonk",
                          "proof_bytes": len(proof), "reps": args.reps, "create_proof_ms": ms(min(prove)),
                          "verify_ms": ms(statistics.median(totals)),
                          "phases_ms": {name: ms(statistics.median(r[name] for r in runs)) for name in verifier.PHASES}}))
    if args.batch:
        proofs = []
        for j in range(args.batch):
            adv_j = circuits.mini_plonk_synthesize(args.k, a=5 + j % 7)[0]
            proofs.append((prover.create_proof_ext(D, params, pk, adv_j, ProverRng(1000 + j), j % 2 == 1), j % 2 == 1))
        runs, totals = [], []
        for rep in range(args.reps + 1):
            batch = verifier.BatchVerifier(D, pv, ProverRng())
            for proof, use_gwc in proofs:
                batch.process(vk, proof, (), use_gwc)
            t0 = time.perf_counter()
            ok = batch.finalize()
            totals.append(time.perf_counter() - t0)
            assert ok, batch.failed
            runs.append(batch.timings)
        runs, totals = runs[1:], totals[1:]
        single = []
        for proof, use_gwc in proofs:
            t0 = time.perf_counter()
            assert verifier.verify_proof_ext(D, pv, vk, proof, (), use_gwc)
            single.append(time.perf_counter() - t0)
        print(json.dumps({"what": "BatchVerifier", "circuit": "mini-plonk", "k": args.k, "proofs": args.batch, "reps": args.reps,
                          "terms": [len(batch.acc.left), len(batch.acc.right)], "finalize_ms": ms(statistics.median(totals)),
                          "phases_ms": {name: ms(statistics.median(r[name] for r in runs)) for name in verifier.PHASES},
                          "one_by_one_ms": ms(sum(single))}))


if __name__ == "__main__":
    main()
