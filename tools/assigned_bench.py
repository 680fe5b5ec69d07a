"""What resolving rational (`Assigned`) columns costs on the device, against the composition of the older entry points.

usage: python tools/assigned_bench.py K COLS [dense|compact|sparse:FRACTION] --reps R
       python tools/assigned_bench.py --sweep [--reps R]        k = 20, 22 x 1, 8, 64 columns x dense, compact, sparse:0.01, sparse:0.5
       python tools/assigned_bench.py --proof K [INVERSE_COLUMNS]

COLS columns of 2^K rows, seeded random field elements:
  dense     num and den canonical 32-byte cells           compact   num and den 8-byte cells
  sparse:F  num canonical 32-byte cells, a denominator (32-byte) for a random fraction F of the rows
  fused     ONE h2_dev_assigned_resolve for all columns, Montgomery cells out
  composed  (dense only) per column what the same job took before: h2_dev_batch_mont of num and of den, h2_dev_batch_invert of
            den with its n-element scratch, h2_dev_eval_op product -- on copies of the same data, in the same process, the two
            taking turns
Times are between two stream events around the call(s), after a warm-up: median, minimum and maximum of R repetitions
(default 9), and the bytes the kernels move per column (reads + writes of whole cells, the model in `moved`).
--proof: the is-zero circuit with INVERSE_COLUMNS (default 8) gadgets at 2^K rows: create_proof wall time from Rational
columns against pre-resolved columns (taking turns, median of 5), and what the host inversions cost that the second kind needs
first (pow(d, -1, r) timed on 2^14 cells and scaled)."""
import argparse
import ctypes
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
from halo2_gpu_specific_amd._lib import check  # noqa: E402
from halo2_gpu_specific_amd.rng import ProverRng  # noqa: E402

_vp = ctypes.c_void_p
C, M, K = prover.ASSIGNED_FORM_CANONICAL, prover.ASSIGNED_FORM_MONTGOMERY, prover.ASSIGNED_FORM_COMPACT
S = 0x1D0C5F0A3B7E91C2A4D6F8091B2C3D4E5F60718293A4B5C6D7E8F9010203


def random_cells(D, n, seed, compact=False):
    if compact:
        with torch.cuda.stream(D.tstream):
            g = torch.Generator(device=D.dev)
            g.manual_seed(seed)
            return torch.randint(1, 1 << 62, (n,), dtype=torch.int64, device=D.dev, generator=g)
    t = D.empty(n)
    check(D.L.h2_dev_random_fr(seed.to_bytes(32, "little"), n, t.data_ptr(), D.stream), "h2_dev_random_fr")
    return t


def moved(kind, n, fraction):
    """bytes per column: fused, composed"""
    if kind == "dense":        # forward: den in, prefix out; backward: den, prefix, num in, result out
        return 6 * 32 * n, (4 + 5 + 3) * 32 * n
    if kind == "compact":
        return (3 * 8 + 3 * 32) * n, None
    m = int(n * fraction)      # copy + conversion of the whole column, then the chain over m rows (row indices twice)
    return 4 * 32 * n + m * (6 * 32 + 8), None


def stats(ms):
    return {"median_ms": float(np.median(ms)), "min_ms": min(ms), "max_ms": max(ms)}


def timed(D, fn):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record(D.tstream)
    fn()
    stop.record(D.tstream)
    D.sync()
    return start.elapsed_time(stop)


def bench(D, k, cols, kind, reps):
    n, L = 1 << k, D.L
    fraction = float(kind.split(":")[1]) if kind.startswith("sparse") else 1.0
    name = kind.split(":")[0]
    compact = name == "compact"
    num = [random_cells(D, n, 2 * i + 1, compact) for i in range(cols)]
    m = n if name != "sparse" else int(n * fraction)
    den = [random_cells(D, m, 2 * i + 2, compact) for i in range(cols)]
    rows = None
    if name == "sparse":
        with torch.cuda.stream(D.tstream):
            g = torch.Generator(device=D.dev)
            g.manual_seed(k)
            rows = [torch.randperm(n, device=D.dev, generator=g)[:m].sort().values.to(torch.int32) for _ in range(cols)]
    out = [D.empty(n) for _ in range(cols)]
    with torch.cuda.stream(D.tstream):
        status = torch.empty(cols * prover.ASSIGNED_STATUS_WORDS, dtype=torch.int32, device=D.dev)
    ptrs = lambda ts: (_vp * cols)(*[t.data_ptr() for t in ts])                       # noqa: E731
    form = (ctypes.c_uint32 * cols)(*([K if compact else C] * cols))
    args = (ptrs(num), form, ptrs(den), form, ptrs(rows) if rows else None, (ctypes.c_uint64 * cols)(*([m] * cols)) if rows else None,
            ptrs(out), cols, n, M, status.data_ptr(), D.stream)

    def fused():
        check(L.h2_dev_assigned_resolve(*args), "h2_dev_assigned_resolve")

    composed = None
    if name == "dense":
        cnum, cden, cout, tmp = [D.clone(t) for t in num], [D.clone(t) for t in den], [D.empty(n) for _ in range(cols)], D.empty(n)

        def composed():
            for a, b, o in zip(cnum, cden, cout):
                check(L.h2_dev_batch_mont(a.data_ptr(), n, D.stream), "h2_dev_batch_mont")
                check(L.h2_dev_batch_mont(b.data_ptr(), n, D.stream), "h2_dev_batch_mont")
                check(L.h2_dev_batch_invert(b.data_ptr(), tmp.data_ptr(), n, D.stream), "h2_dev_batch_invert")
                D.eval_op(3, o, a, b)                                                 # H2_OP_MUL

    fused()
    if composed:
        composed()
        with torch.cuda.stream(D.tstream):                                            # the first turn computes the same cells
            assert all(torch.equal(a, b) for a, b in zip(out, cout)), "the fused call and the composition disagree"
    D.sync()
    t_fused, t_comp = [], []
    for _ in range(reps):
        t_fused.append(timed(D, fused))
        if composed:
            t_comp.append(timed(D, composed))
    with torch.cuda.stream(D.tstream):
        assert not status.cpu().numpy().view(np.uint32).reshape(cols, -1)[:, 0].any()
    b_fused, b_comp = moved(name, n, fraction)
    res = {"k": k, "cols": cols, "kind": kind, "reps": reps, "fused": stats(t_fused), "fused_bytes_per_col": b_fused}
    line = "k = %d, %2d x %-11s fused %8.3f ms (%.3f .. %.3f) = %.3f ms/col, %5.2f TB/s of %d B/cell" % (
        k, cols, kind, res["fused"]["median_ms"], res["fused"]["min_ms"], res["fused"]["max_ms"], res["fused"]["median_ms"] / cols,
        b_fused * cols / res["fused"]["median_ms"] / 1e9, b_fused // n)
    if composed:
        res.update(composed=stats(t_comp), composed_bytes_per_col=b_comp)
        line += "; composed %8.3f ms (%.3f .. %.3f) = %.3f ms/col, %5.2f TB/s of %d B/cell; fused / composed = %.2f" % (
            res["composed"]["median_ms"], res["composed"]["min_ms"], res["composed"]["max_ms"], res["composed"]["median_ms"] / cols,
            b_comp * cols / res["composed"]["median_ms"] / 1e9, b_comp // n, res["fused"]["median_ms"] / res["composed"]["median_ms"])
    print(line, flush=True)
    return res


# ---- the proof-level line --------------------------------------------------------------------------------------------------

def is_zero_circuit(gadgets):
    from halo2_gpu_specific_amd.circuit import Constant, ConstraintSystem

    cs = ConstraintSystem("is-zero-%d" % gadgets)
    q = cs.fixed_column()
    for _ in range(gadgets):
        v, inv, z = cs.advice_column(), cs.advice_column(), cs.advice_column()
        fq, av, ai, az = cs.query_fixed(q), cs.query_advice(v), cs.query_advice(inv), cs.query_advice(z)
        cs.create_gate("is zero", [fq * av * az, fq * (az - (Constant(1) - av * ai))])
    return cs


def proof_line(D, k, gadgets):
    n = 1 << k
    cs = is_zero_circuit(gadgets)
    usable = n - (cs.blinding_factors() + 1)
    rng = np.random.Generator(np.random.PCG64(k))
    # v from a table of 4096 values (0 among them) so that the resolved twin needs 4096 host inversions, not 2^k per column
    table = np.array([0] + [int(x) for x in rng.integers(1, 1 << 62, size=4095, dtype=np.uint64)], dtype=np.uint64)
    inverse = np.zeros((4096, 4), dtype=np.uint64)
    for i, x in enumerate(table):
        y = pow(int(x), -1, prover.R_MOD) if x else 0
        inverse[i] = [(y >> (64 * j)) & ((1 << 64) - 1) for j in range(4)]
    sample = [int(x) for x in rng.integers(1, 1 << 62, size=1 << 14, dtype=np.uint64)]
    t0 = time.perf_counter()
    for x in sample:
        pow(x, -1, prover.R_MOD)
    host_inversions_s = (time.perf_counter() - t0) / len(sample) * usable * gadgets
    rational, resolved = [], []
    ones = np.ones(n, dtype=np.uint64)
    for _ in range(gadgets):
        pick = rng.integers(0, 4096, size=n)
        pick[usable:] = 0
        v = table[pick]
        z = (v == 0).astype(np.uint64)
        z[usable:] = 0
        inv = inverse[pick]
        resolved += [v, inv, z]
        rational += [v, prover.Rational(ones, v), z]
    fixed = np.zeros(n, dtype=np.uint64)
    fixed[:usable] = 1
    params = prover.Params.unsafe_setup(D, k, S)
    pk = prover.keygen(D, params, cs, [fixed], np.zeros((0, 4), dtype=np.int64))
    times, proofs = {"rational": [], "resolved": []}, {}
    for _ in range(6):                                  # the first turn warms up
        for label, adv in (("rational", rational), ("resolved", resolved)):
            D.sync()
            t0 = time.perf_counter()
            proofs[label] = prover.create_proof(D, params, pk, adv, ProverRng(1))
            D.sync()
            times[label].append(time.perf_counter() - t0)
    assert proofs["rational"] == proofs["resolved"], "the two witnesses prove to different bytes"
    res = {"k": k, "inverse_columns": gadgets, "host_inversions_s_extrapolated": host_inversions_s}
    for label in times:
        res["proof_%s_ms" % label] = stats([t * 1e3 for t in times[label][1:]])
    print("is-zero circuit, %d inverse columns (%d advice columns) at k = %d: create_proof from Rational columns %.1f ms (%.1f .. %.1f), "
          "from pre-resolved columns %.1f ms (%.1f .. %.1f), median of 5, equal bytes; the host inversions the second kind needs first: "
          "%.1f s (pow(d, -1, r), one thread, scaled from 2^14 cells)" % (
              gadgets, 3 * gadgets, k, res["proof_rational_ms"]["median_ms"], res["proof_rational_ms"]["min_ms"],
              res["proof_rational_ms"]["max_ms"], res["proof_resolved_ms"]["median_ms"], res["proof_resolved_ms"]["min_ms"],
              res["proof_resolved_ms"]["max_ms"], host_inversions_s), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("k", nargs="?", type=int)
    ap.add_argument("cols", nargs="?", type=int)
    ap.add_argument("kind", nargs="?", default="dense")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--proof", action="store_true")
    a = ap.parse_args()
    D = prover.Device()
    if a.proof:
        results = [proof_line(D, a.k or 20, a.cols or 8)]
    elif a.sweep:
        results = [bench(D, k, cols, kind, max(a.reps, 9)) for k in (20, 22) for cols in (1, 8, 64)
                   for kind in ("dense", "compact", "sparse:0.01", "sparse:0.5")]
    else:
        if a.k is None or a.cols is None:
            ap.error("K and COLS are needed")
        kind = a.kind
        if kind not in ("dense", "compact") and not kind.startswith("sparse:"):
            ap.error("kind is dense, compact or sparse:FRACTION")
        results = [bench(D, a.k, a.cols, kind, max(a.reps, 1))]
    for r in results:
        print(json.dumps(r))


if __name__ == "__main__":
    main()
