"""What completing the witness of range-checked columns costs, on the host and on the device, and what it does to a proof.

usage: python tools/range_check_bench.py K [PAIRS]

The circuit is examples/range-check.rs's with PAIRS `advice_column_range` columns (0 ..= 65535, step 2; default 1) at 2^K rows,
each filled with random 16-bit values up to the rows the range is planted in.  Reported, best of three:
  host     prover.complete_range_check_witness on fresh host copies (numpy: plant + bincount + repeat)
  device   prover.range_check_complete_device on resident columns: wall time with the status download, the time between two
           stream events around the call (the three kernels and the counters' memset), and the bytes per second that is for
           one read and one write of n cells per pair (2 x n x 32 B: the columns are canonical (n, 4) cells; the Montgomery
           and compact forms are not benchmarked)
  proofs   create_proof_ext wall time from host columns (host completion), from host columns with range_checks_on_device, and
           from resident columns (the upload not counted), the three taking turns: best and median of five
One JSON line at the end carries the same figures."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")  # before HIP initialises (halo2-gpu-specific_amd/__init__.py says why)
import numpy as np  # noqa: E402
import torch  # noqa: E402  (first: the library binds to torch's HIP runtime)

torch.cuda.init()

from halo2_gpu_specific_amd import prover  # noqa: E402
from halo2_gpu_specific_amd.circuit import ConstraintSystem  # noqa: E402
from halo2_gpu_specific_amd.rng import ProverRng  # noqa: E402

HBM_PEAK = 8.0e12                                # bytes per second, the MI355X's specified HBM3E rate
S = 0x1D0C5F0A3B7E91C2A4D6F8091B2C3D4E5F60718293A4B5C6D7E8F9010203
VMIN, VMAX, STEP = 0, 0xFFFF, 2


def circuit(pairs):
    cs = ConstraintSystem("range-check-x%d" % pairs)
    l_0, l_active, l_last_active = cs.fixed_column(), cs.fixed_column(), cs.fixed_column()
    for _ in range(pairs):
        cs.advice_column_range(l_0, l_active, l_last_active, VMIN, VMAX, STEP)
    cs.chunk_shuffles()
    return cs


def synthesize(cs, k, alloc):
    n = 1 << k
    usable = n - (cs.blinding_factors() + 1)
    lo = usable - len(prover.range_check_assigner(VMIN, VMAX, STEP))
    assert lo > 1, "the range does not fit 2^%d rows" % k
    adv = alloc(cs.num_advice, n)
    rng = np.random.Generator(np.random.PCG64(0x52414E4745))
    for origin, _, vmin, vmax, _ in cs.range_checks:
        adv[origin][:lo - 1, 0] = rng.integers(vmin, vmax + 1, size=lo - 1, dtype=np.uint64)
    fixed = [np.zeros((n, 4), dtype=np.uint64) for _ in range(3)]
    fixed[0][0, 0] = 1
    fixed[1][:usable, 0] = 1
    fixed[2][usable - 1, 0] = 1
    return adv, fixed, np.zeros((0, 4), dtype=np.int64), usable


def best(f, reps=3):
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        out.append(time.perf_counter() - t0)
    return min(out)


def main():
    k = int(sys.argv[1]) if len(sys.argv) > 1 else 18
    pairs = int(sys.argv[2]) if len(sys.argv) > 2 else 1
    n = 1 << k
    D = prover.Device()
    cs = circuit(pairs)
    adv, fixed, copies, usable = synthesize(cs, k, D.pinned_columns)
    result = {"k": k, "pairs": pairs, "form": "canonical"}

    # ---- the completion alone ------------------------------------------------------------------------------------------
    copies_host = [[c.copy() for c in adv] for _ in range(3)]
    it = iter(copies_host)
    result["host_ms"] = best(lambda: prover.complete_range_check_witness(cs, n, next(it))) * 1e3
    del copies_host, it

    def device_pairs():
        cols = [D.upload(c) for c in adv]
        return [(cols[o], cols[s], prover.RC_FORM_CANONICAL, prover.RC_FORM_CANONICAL, vmin, vmax, step, None)
                for o, s, vmin, vmax, step in cs.range_checks]

    prover.range_check_complete_device(D, device_pairs(), usable, n)          # (first call: code objects, scratch)
    walls, events = [], []
    for _ in range(3):
        ps = device_pairs()
        D.sync()
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        start.record(D.tstream)
        status = prover.range_check_complete_device(D, ps, usable, n)
        stop.record(D.tstream)
        D.sync()
        walls.append(time.perf_counter() - t0)
        events.append(start.elapsed_time(stop) * 1e-3)
        assert not status[:, 0].any(), status
    moved = 2 * n * 32 * pairs
    result.update(device_wall_ms=min(walls) * 1e3, device_stream_ms=min(events) * 1e3, bytes=moved,
                  bytes_per_s=moved / min(events), hbm_peak_fraction=moved / min(events) / HBM_PEAK)
    print("completion of %d canonical pair(s) at k = %d (Montgomery and compact columns are not benchmarked): host %.2f ms; device %.3f ms wall, %.3f ms on the stream = %.2f TB/s of "
          "2 x n x 32 B per pair (%.2f of the HBM peak)" % (pairs, k, result["host_ms"], result["device_wall_ms"],
                                                           result["device_stream_ms"], result["bytes_per_s"] / 1e12,
                                                           result["hbm_peak_fraction"]))

    # ---- proofs --------------------------------------------------------------------------------------------------------
    params = prover.Params.unsafe_setup(D, k, S)
    pk = prover.keygen(D, params, cs, fixed, copies)
    D.sync()
    pristine = [c.copy() for c in adv]

    def restore():
        for a, b in zip(adv, pristine):
            a[:] = b

    intakes = [("host", {}), ("opt_in", {"range_checks_on_device": True}), ("resident", {})]
    times, out = {label: [] for label, _ in intakes}, {}
    for rep in range(6):                           # the intakes take turns, so that a busy host weighs on all alike
        for label, kw in intakes:
            restore()                              # (the host path completes the caller's columns in place)
            cols = [D.upload(c) for c in adv] if label == "resident" else adv
            D.sync()
            t0 = time.perf_counter()
            out[label] = prover.create_proof_ext(D, params, pk, cols, ProverRng(1), False, **kw)
            D.sync()
            times[label].append(time.perf_counter() - t0)
    for label, _ in intakes:                       # (the first turn warms up: code objects, pools)
        result["proof_%s_ms" % label] = min(times[label][1:]) * 1e3
        result["proof_%s_median_ms" % label] = float(np.median(times[label][1:])) * 1e3
    assert out["host"] == out["opt_in"] == out["resident"], "the three intakes disagree"
    print("create_proof_ext, best (median) of five: host path %.1f (%.1f) ms, range_checks_on_device %.1f (%.1f) ms, resident "
          "%.1f (%.1f) ms (%d bytes, equal)" % (
              result["proof_host_ms"], result["proof_host_median_ms"], result["proof_opt_in_ms"],
              result["proof_opt_in_median_ms"], result["proof_resident_ms"], result["proof_resident_median_ms"],
              len(out["host"])))
    print(json.dumps(result))


if __name__ == "__main__":
    main()
