"""Params.verify from the command line: the report of an SRS file, or the check timed next to Params.from_powers.
usage: python tools/params_check.py FILE [--k K] [--seed N] [--no-locate]
       python tools/params_check.py --bench K [K ...] [--reps N]

FILE: the SRS file is read (formats.params_read, with --k the parameters of 2^K rows derived from it), checked against the
[s]G2 of its additional_data, and the report is printed with the milliseconds of each phase: screen, scalars, inverse NTT,
MSMs, pairing, location.  The exit status is 0 for parameters that are ok, 1 otherwise.

--bench: on Params.unsafe_setup parameters of each K, one JSON line with `verify` (per phase, the best of --reps by total,
after a warm-up) next to `from_powers` of the same K from the same run -- the only way to check a basis without this check --
and the screening kernel alone (device events around both tables' calls) as GB/s of the points it reads."""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")  # before HIP initialises (halo2-gpu-specific_amd/__init__.py says why)

PHASES = ("screen", "scalars", "intt", "msm", "pairing", "locate", "total")
BENCH_TRAPDOOR = 0x1D0C5F0A3B7E91C2A4D6F8091B2C3D4E5F60718293A4B5C6D7E8F9010203


def print_report(report):
    from halo2_gpu_specific_amd.params_check import KIND_NAMES, describe

    print(describe(report))
    for table, index, kind in report.points:
        print("  bad point: %s[%d] %s" % (table, index, KIND_NAMES.get(kind, kind)))
    if report.points_total > len(report.points):
        print("  ... %d bad points in all" % report.points_total)
    print("  ms: " + "  ".join("%s %.3f" % (name, report.timings[name]) for name in PHASES if name in report.timings))


def check_file(args):
    from halo2_gpu_specific_amd import formats, prover

    D = prover.Device()
    params, additional = formats.params_read(D, args.file, k=args.k)
    print("%s: k = %d, additional_data %d bytes" % (args.file, params.k, len(additional)))
    report = params.verify(D, s_g2=additional if len(additional) == 64 else None, seed=args.seed, locate=not args.no_locate)
    print_report(report)
    return 0 if report.ok else 1


def timed(D, fn):
    """device milliseconds of fn() on the compute stream (h2_timer_*)"""
    from halo2_gpu_specific_amd._lib import check

    ms = ctypes.c_float()
    check(D.L.h2_timer_start(D.stream), "h2_timer_start")
    out = fn()
    check(D.L.h2_timer_stop(D.stream, ctypes.byref(ms)), "h2_timer_stop")
    return ms.value, out


def bench(args):
    import gc

    import torch

    from halo2_gpu_specific_amd import params_check as pc
    from halo2_gpu_specific_amd import prover

    D = prover.Device()
    for k in args.bench:
        n = 1 << k
        P = prover.Params.unsafe_setup(D, k, BENCH_TRAPDOOR)
        runs = [P.verify(D, seed=1 + i) for i in range(args.reps + 1)][1:]          # the first is the warm-up
        assert all(r.ok for r in runs), "unsafe_setup parameters must verify"
        best = min(runs, key=lambda r: r.timings["total"])
        # the screen alone: both tables, no download inside the window
        screens = []
        for _ in range(args.reps + 1):
            with torch.cuda.stream(D.tstream):
                blob = torch.zeros(8, dtype=torch.int32, device=D.dev)

            def both():
                for index, t in enumerate((P.g, P.g_lagrange)):
                    pc.check(D.L.h2_dev_g1_check_points(t.data_ptr(), n, index, pc.FORBID_IDENTITY, blob.data_ptr(), None, 0,
                                                        D.stream), "h2_dev_g1_check_points")

            screens.append(timed(D, both)[0])
        screen_ms = min(screens[1:])
        # the tampered case: what location adds (two swapped Lagrange entries; a copy without tables)
        with torch.cuda.stream(D.tstream):
            gl = P.g_lagrange.clone()
            gl[[3, n - 5]] = gl[[n - 5, 3]]
        T = prover.Params(D, k, P.g, gl, tables=False)
        T.s_g2 = P.s_g2
        located = T.verify(D, seed=9)
        assert located.lagrange is False and located.first_bad_lagrange == 3 and located.powers is True
        del T, gl
        prover.Params.from_powers(D, k, P.g, tables=False)                           # warm-up: plan, code objects
        from_powers_ms = min(timed(D, lambda: prover.Params.from_powers(D, k, P.g, tables=False))[0] for _ in range(args.reps))
        print(json.dumps({
            "k": k, "reps": args.reps, "tables": P.table_bytes > 0,
            "verify_ms": {name: round(best.timings[name], 3) for name in PHASES if name in best.timings},
            "verify_total_ms_all": [round(r.timings["total"], 3) for r in runs],
            "locate_ms_swapped_lagrange": round(located.timings["locate"], 3),
            "from_powers_ms": round(from_powers_ms, 3),
            "from_powers_over_verify": round(from_powers_ms / best.timings["total"], 1),
            "screen_kernels_ms": round(screen_ms, 4),
            "screen_GBps": round(2 * n * 64 / (screen_ms * 1e-3) / 1e9, 1),
        }), flush=True)
        del P, runs, best, located
        gc.collect()
        torch.cuda.empty_cache()
    return 0


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("file", nargs="?")
    ap.add_argument("--k", type=int, default=None)
    ap.add_argument("--seed", type=int, default=None)
    ap.add_argument("--no-locate", action="store_true")
    ap.add_argument("--bench", type=int, nargs="+", metavar="K")
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    if (args.file is None) == (args.bench is None):
        ap.error("give an SRS file or --bench K ...")
    import torch

    torch.cuda.init()
    return bench(args) if args.bench else check_file(args)


if __name__ == "__main__":
    sys.exit(main())
