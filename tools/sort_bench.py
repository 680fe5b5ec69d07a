"""What ordering a witness costs on the device (Value.argsort: csrc/sort.hip, h2_dev_sort_permutation) next to the round trip
it replaces.

usage: python tools/sort_bench.py K [--reps R]

Four key sets over 2^K rows of seeded random data, columns resident on the device, one process:
  16-bit            one canonical column of values below 2^16, no promise: 2 of 32 candidate positions move data
  64-bit compact    one compact column (8-byte cells) of random 64-bit values: 8 positions
  254-bit           one canonical column of random field elements: 32 positions
  16-bit, 32-bit    two canonical columns under the promises bits = [16, 32]: 2 + 4 positions
Per key set: the time of one sort between two stream events (median, minimum and maximum of R repetitions, default 5: the
survey of the keys, the decision, every pass, the permutation written as 8-byte indices), the passes that moved data
(d_status[3]), and the bytes moved per second by this model of a call over n rows:
  survey            the cells of every key once (32 n, 8 n compact)
  per moving pass   histogram: 4 n indices read (0 in the first pass: the identity), n gathered bytes, n digits written;
                    scatter: n digits and 4 n indices read, 4 n indices written -- 15 n (11 n in the first pass).  The gather
                    reads ONE byte of a 32-byte cell: the memory system moves a 32-byte sector for it, which the model does
                    not count (the line `sector bytes` states the rate with them)
  the permutation   4 n read, 8 n written
Next to it the baseline the sort replaces: the same columns downloaded, np.lexsort over their 64-bit limbs (np.argsort,
stable, for a single compact column) on the host, the permutation uploaded -- wall clock, once.  One JSON line at the end."""
import argparse
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

from halo2_gpu_specific_amd import prover, values as V  # noqa: E402
from halo2_gpu_specific_amd._lib import check  # noqa: E402


def random_fr(D, n, seed):
    t = D.empty(n)
    check(D.L.h2_dev_random_fr(seed.to_bytes(32, "little"), n, t.data_ptr(), D.stream), "h2_dev_random_fr")
    check(D.L.h2_dev_batch_unmont(t.data_ptr(), n, D.stream), "h2_dev_batch_unmont")      # canonical cells
    return t


def random_small(D, n, seed, bits, compact=False):
    with torch.cuda.stream(D.tstream):
        g = torch.Generator(device=D.dev)
        g.manual_seed(seed)
        if bits == 64:
            low = torch.randint(-(1 << 63), (1 << 63) - 1, (n,), dtype=torch.int64, device=D.dev, generator=g)
        else:
            low = torch.randint(0, 1 << bits, (n,), dtype=torch.int64, device=D.dev, generator=g)
        if compact:
            return low
        t = torch.zeros((n, 4), dtype=torch.int64, device=D.dev)
        t[:, 0] = low
        return t


def model_bytes(n, forms, passes):
    survey = sum(8 * n if f == V.FORM_COMPACT else 32 * n for f in forms)
    moved = 15 * n * passes - (4 * n if passes else 0)
    sectors = 31 * n * passes                                   # what a 32-byte sector per gathered byte adds
    return survey + moved + 12 * n, survey + moved + 12 * n + sectors


def host_round_trip(D, columns, forms):
    t0 = time.perf_counter()
    host = [D.download(c) for c in columns]
    t1 = time.perf_counter()
    if len(host) == 1 and forms[0] == V.FORM_COMPACT:
        perm = np.argsort(host[0], kind="stable")
    else:
        limbs = []                                              # np.lexsort: the LAST key is the primary one
        for column in reversed(host):
            limbs += [column] if column.ndim == 1 else [column[:, j] for j in range(4)]
        perm = np.lexsort(limbs)
    t2 = time.perf_counter()
    up = D.upload(perm.astype(np.uint64), widen=False)
    D.sync()
    t3 = time.perf_counter()
    return perm, up, {"download_s": t1 - t0, "lexsort_s": t2 - t1, "upload_s": t3 - t2, "total_s": t3 - t0}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("k", type=int)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    n = 1 << args.k
    D = prover.Device()
    be = V._backend(D)
    C, K = V.FORM_CANONICAL, V.FORM_COMPACT
    cases = [
        ("16-bit", [random_small(D, n, 1, 16)], [C], [0]),
        ("64-bit compact", [random_small(D, n, 2, 64, compact=True)], [K], [0]),
        ("254-bit", [random_fr(D, n, 3)], [C], [0]),
        ("16-bit, 32-bit", [random_small(D, n, 4, 16), random_small(D, n, 5, 32)], [C, C], [16, 32]),
    ]
    D.sync()
    out = {"k": args.k, "reps": args.reps, "cases": {}}
    print("%-16s %28s %7s %14s %14s %12s %s" % ("keys, 2^%d rows" % args.k, "sort ms: median (min .. max)", "passes", "model GB/s",
                                                "sector GB/s", "baseline s", "(download + lexsort + upload)"))
    for name, columns, forms, bits in cases:
        be.sort(columns, forms, bits, n)                        # the scratch grown, the kernels loaded
        D.sync()
        ms, status, perm = [], None, None
        for _ in range(args.reps):
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record(D.tstream)
            perm, status = be.sort(columns, forms, bits, n)
            stop.record(D.tstream)
            D.sync()
            ms.append(start.elapsed_time(stop))
        assert status[0] == V.SORT_OK, status
        want, _, base = host_round_trip(D, columns, forms)
        assert np.array_equal(D.download(perm), want.astype(np.uint64)), name
        med = float(np.median(ms))
        model, sectors = model_bytes(n, forms, status[3])
        out["cases"][name] = {"median_ms": med, "min_ms": float(min(ms)), "max_ms": float(max(ms)), "passes": status[3],
                              "model_bytes": model, "model_gbs": model / med / 1e6, "sector_gbs": sectors / med / 1e6,
                              "baseline": base, "speedup": base["total_s"] * 1e3 / med}
        print("%-16s %9.3f (%7.3f .. %7.3f) %7d %14.1f %14.1f %12.3f (%.3f + %.3f + %.3f)  x%.0f" % (
            name, med, min(ms), max(ms), status[3], model / med / 1e6, sectors / med / 1e6, base["total_s"], base["download_s"],
            base["lexsort_s"], base["upload_s"], base["total_s"] * 1e3 / med))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
