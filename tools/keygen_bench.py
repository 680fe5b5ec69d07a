"""The copy constraints' cycle mapping of keygen, host route against device route, on the same copies in the same process:
prover.permutation_mapping (numpy + scipy on one host thread) in seconds; prover.permutation_mapping_device per phase in
milliseconds (HIP events: the copies' upload, components, compaction + sort, successors; then the download into the
(ncols, n) host arrays keygen keeps as pk.mapping); and the whole keygen of a circuit with NCOLS equality-enabled advice
columns both ways (H2_PERM_MAPPING=host for the host route).  The two mappings are compared entry by entry.
  usage: python tools/keygen_bench.py K NCOLS COPIES [random|chain|star|pairs] [--reps R]
  random  COPIES pairs of uniformly random cells
  chain   cell i of a column copied to cell i + 1, whole columns one after the other until COPIES are made
  star    cell (0, 0) copied to COPIES random cells
  pairs   COPIES disjoint pairs of random cells (COPIES <= NCOLS * 2^K / 2)"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")  # before HIP initialises (halo2-gpu-specific_amd/__init__.py says why)
import numpy as np  # noqa: E402
import torch  # noqa: E402

torch.cuda.init()

from halo2_gpu_specific_amd import prover  # noqa: E402
from halo2_gpu_specific_amd.circuit import ConstraintSystem  # noqa: E402


def make_copies(pattern, ncols, n, count, seed=1):
    rng = np.random.Generator(np.random.PCG64(seed))
    cells = ncols * n
    if pattern == "random":
        left, right = rng.integers(0, cells, size=count), rng.integers(0, cells, size=count)
    elif pattern == "chain":
        count = min(count, ncols * (n - 1))
        i = np.arange(count, dtype=np.int64)
        left = i // (n - 1) * n + i % (n - 1)
        right = left + 1
    elif pattern == "star":
        left, right = np.zeros(count, dtype=np.int64), rng.integers(0, cells, size=count)
    elif pattern == "pairs":
        count = min(count, cells // 2)
        p = rng.permutation(cells)
        left, right = p[:count], p[count:2 * count]
    else:
        raise SystemExit("unknown pattern %r" % pattern)
    return np.stack([left // n, left % n, right // n, right % n], axis=1).astype(np.int64)


def equality_circuit(ncols):
    """NCOLS advice columns under the permutation argument, one gate the all-zero fixed column switches off"""
    cs = ConstraintSystem("equality-%d" % ncols)
    adv = [cs.advice_column() for _ in range(ncols)]
    q = cs.query_fixed(cs.fixed_column())
    for col in adv:
        cs.enable_equality(col)
    a, z = cs.query_advice(adv[0]), cs.query_advice(adv[-1])
    cs.create_gate("square", [q * (a * a + z * (-1))])
    return cs


def spread(values, unit):
    return "min %.3f  median %.3f  max %.3f %s" % (min(values), statistics.median(values), max(values), unit)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("k", type=int)
    ap.add_argument("ncols", type=int)
    ap.add_argument("copies", type=int)
    ap.add_argument("pattern", nargs="?", default="random")
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    k, ncols, n = args.k, args.ncols, 1 << args.k
    copies = make_copies(args.pattern, ncols, n, args.copies)
    print("keygen_bench k=%d ncols=%d copies=%d pattern=%s reps=%d (mapping: 2 x %.0f MiB)" % (
        k, ncols, len(copies), args.pattern, args.reps, ncols * n * 4 / 2**20))
    D = prover.Device()
    # host route: the parent's code
    host_s = []
    for rep in range(args.reps):
        t0 = time.perf_counter()
        want = prover.permutation_mapping(ncols, n, copies)
        host_s.append(time.perf_counter() - t0)
        print("  host   rep %d: permutation_mapping %.3f s" % (rep, host_s[-1]))
    # device route, as keygen runs it: upload, build, one download
    prover.permutation_mapping_device(D, ncols, n, copies[:1])      # (the library's first call in the process)
    D.sync()
    device_ms = []
    for rep in range(args.reps):
        phases = []
        D.sync()
        t0 = time.perf_counter()
        d_col, d_row = prover.permutation_mapping_device(D, ncols, n, copies, phase_ms=phases)
        t1 = time.perf_counter()
        with torch.cuda.stream(D.tstream):
            got = tuple(t.cpu().numpy().view(np.uint32).reshape(ncols, n) for t in (d_col, d_row))
        t2 = time.perf_counter()
        device_ms.append((t2 - t0) * 1e3)
        print("  device rep %d: total %.2f ms = call %.2f (upload %.2f, components %.2f, compaction + sort %.2f, successors %.2f; "
              "the rest: conversion to u32, allocation, status) + download %.2f" % (
                  rep, device_ms[-1], (t1 - t0) * 1e3, phases[0], phases[1], phases[2], phases[3], (t2 - t1) * 1e3))
        if rep == 0:
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), "the two routes disagree"
        del d_col, d_row, got
    print("  mapping: host %s | device %s | host median / device median = %.1f" % (
        spread(host_s, "s"), spread(device_ms, "ms"), statistics.median(host_s) * 1e3 / statistics.median(device_ms)))
    print("  device slower than host in any pairing of repetitions: %s" % (max(device_ms) >= min(host_s) * 1e3))
    del want
    # the whole keygen both ways (timing-only SRS: the same work, no trapdoor)
    params = prover.Params.synthetic(D, k)
    cs = equality_circuit(ncols)
    fixed = [np.zeros((n, 4), dtype=np.uint64)]
    facts = {}
    for route in ("warm-up", "device", "host"):
        if route == "host":
            os.environ["H2_PERM_MAPPING"] = "host"
        D.sync()
        t0 = time.perf_counter()
        pk = prover.keygen(D, params, cs, fixed, copies if route != "warm-up" else copies[:1])
        D.sync()
        if route != "warm-up":
            facts[route] = (pk.transcript_repr, time.perf_counter() - t0)
            print("  keygen through the %s route: %.3f s" % (route, facts[route][1]))
        del pk
    os.environ.pop("H2_PERM_MAPPING", None)
    assert facts["device"][0] == facts["host"][0], "the two keys differ"
    print("  the two keys have the same digest")


if __name__ == "__main__":
    main()
