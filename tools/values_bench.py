"""What computing a witness with Values (values.py, csrc/values.hip) costs on the device.

usage: python tools/values_bench.py K [--reps R] [--python-height H] [--integers] [--stream-gbs RATE]

Three cases over 2^K rows of seeded random data, one process, after the clock-settling load bench.py uses:
  (a) a*b*c + d from four COMPACT leaves (8-byte cells), one fused launch, canonical cells out -- and the same composed from
      the older entry points: 4 x h2_dev_widen_u64, 4 x h2_dev_batch_mont, h2_dev_eval_op MUL, MUL, SUM, h2_dev_batch_unmont
  (b) the same from four CANONICAL leaves (32-byte cells) -- composed: 4 x batch_mont, MUL, MUL, SUM, batch_unmont
  (c) the shuffle argument's running product of width 4: z = ((compress(orig) + beta) / (compress(shuf) + beta)).cumprod()
      -- two fused launches, one batch inversion, one scan; against circuits.shuffle_gates_witness (Python integers) at
      --python-height rows (default 2^17, about a second), the ratio stated per row
With --integers, two more (and case (c) is left out):
  (d) a COMPACT u64 column to four 16-bit limb columns in canonical form, `from_u64(...).limbs(16, 4)`: one launch, no field
      product -- against what there was before: torch shifts and masks on the u64 tensor, then 4 x h2_dev_widen_u64
  (e) a MONTGOMERY column to 32 8-bit limb columns, `limbs(8, 32)`: ceil(32 / outputs cap) = 8 launches, each converting the
      column again (one product per row and launch) -- against download + Python integers + upload, which is timed at
      --python-height rows (2^16 in the recorded runs) and scaled per row.  Bytes moved are also stated as a share of
      --stream-gbs, the streaming rate tools/membench reads and writes with on the same device (GB/s; given by the caller).
Times are between two stream events around the call(s): median, minimum and maximum of R repetitions (default 9), the
variants of a case taking turns.  `fused` is the launch of the compiled program (its argument tables built, the kernel run);
`fused_with_compile` the whole `Value` expression from scratch, whose host time (building and scheduling the expression, about
0.1 ms) lies between the two events while the device idles.  Per case: bytes moved per second (the kernels' reads and writes of whole cells), field
products per second, and those as a share of the multiplier's rate measured in the same run (a launch of 120 dependent
squarings per row over Montgomery cells: nothing but products) -- which says whether a case sits under the multiplier or
under HBM.  One JSON line."""
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

from halo2_gpu_specific_amd import circuits, circuits_frontend as fe, prover, values as V  # noqa: E402
from halo2_gpu_specific_amd._lib import check  # noqa: E402
from halo2_gpu_specific_amd.values import Value  # noqa: E402


def stats(ms):
    return {"median_ms": float(np.median(ms)), "min_ms": float(min(ms)), "max_ms": float(max(ms))}


def timed(D, fn):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record(D.tstream)
    fn()
    stop.record(D.tstream)
    D.sync()
    return start.elapsed_time(stop)


def spin(D, fn, seconds=0.15):
    end = time.perf_counter() + seconds
    while time.perf_counter() < end:
        fn()
        D.sync()


def random_cells(D, n, seed, compact):
    if compact:
        with torch.cuda.stream(D.tstream):
            g = torch.Generator(device=D.dev)
            g.manual_seed(seed)
            return torch.randint(1, 1 << 62, (n,), dtype=torch.int64, device=D.dev, generator=g)
    t = D.empty(n)
    check(D.L.h2_dev_random_fr(seed.to_bytes(32, "little"), n, t.data_ptr(), D.stream), "h2_dev_random_fr")
    check(D.L.h2_dev_batch_unmont(t.data_ptr(), n, D.stream), "h2_dev_batch_unmont")      # canonical cells
    return t


def fused_abcd(D, cells, compact):
    make = Value.from_u64 if compact else Value.from_limbs
    a, b, c, d = (make(D, t) for t in cells)
    return (a * b * c + d).tensor()


def composed_abcd(D, cells, compact, work):
    L, n = D.L, cells[0].shape[0]
    for t, w in zip(cells, work):
        if compact:
            check(L.h2_dev_widen_u64(t.data_ptr(), n, w.data_ptr(), D.stream), "h2_dev_widen_u64")
        else:
            with torch.cuda.stream(D.tstream):
                w.copy_(t)                                                      # the composition converts in place
        check(L.h2_dev_batch_mont(w.data_ptr(), n, D.stream), "h2_dev_batch_mont")
    out = work[4]
    D.eval_op(prover.OP_MUL, out, work[0], work[1])
    D.eval_op(prover.OP_MUL, out, out, work[2])
    D.eval_op(prover.OP_SUM, out, out, work[3])
    check(L.h2_dev_batch_unmont(out.data_ptr(), n, D.stream), "h2_dev_batch_unmont")
    return out


def compiled(D, value, montgomery=False):
    """-> (the result, relaunch): `relaunch()` launches the one program `value` compiled to again, into the same tensor --
    the kernel and its argument tables without the compiler's host time"""
    del V.LAST_PROGRAMS[:]
    out = value.tensor(montgomery)
    (prog,) = V.LAST_PROGRAMS
    form = V.FORM_MONTGOMERY if montgomery else V.FORM_CANONICAL
    return out, lambda: V._launch(prog, [(out, 0)], form, len(value), V._backend(D))


def compiled_many(D, values):
    """-> (the results, relaunch, launches): like `compiled` for several Values materialised together, in canonical form"""
    del V.LAST_PROGRAMS[:]
    outs = Value.materialize(values)
    progs = list(V.LAST_PROGRAMS)
    cap, m, be = V.limits()["outputs"], len(values[0]), V._backend(D)
    groups = [outs[i:i + cap] for i in range(0, len(outs), cap)]
    assert len(groups) == len(progs)

    def relaunch():
        for prog, group in zip(progs, groups):
            V._launch(prog, [(t, 0) for t in group], V.FORM_CANONICAL, m, be)

    return outs, relaunch, len(progs)


def integer_cases(D, n, args, out):
    L = D.L
    stream_rate = args.stream_gbs * 1e9 if args.stream_gbs else None
    # (d) compact u64 -> four 16-bit limbs
    cells = random_cells(D, n, 31, True)
    limbs, launch_fn, launches = compiled_many(D, Value.from_u64(D, cells).limbs(16, 4))
    work = [D.empty(n) for _ in range(4)]

    def composed_fn():
        with torch.cuda.stream(D.tstream):
            parts = [(cells >> (16 * j)) & 0xFFFF for j in range(4)]
        for part, w in zip(parts, work):
            check(L.h2_dev_widen_u64(part.data_ptr(), n, w.data_ptr(), D.stream), "h2_dev_widen_u64")
        return work

    same = all(np.array_equal(D.download(x), D.download(y)) for x, y in zip(limbs, composed_fn()))
    spin(D, launch_fn)
    fused_ms, composed_ms = [], []
    for _ in range(args.reps):
        fused_ms.append(timed(D, launch_fn))
        composed_ms.append(timed(D, composed_fn))
    f, c = stats(fused_ms), stats(composed_ms)
    fused_bytes = (8 + 4 * 32) * n
    composed_bytes = 4 * (8 + 8 + 8 + 8) * n + 4 * (8 + 32) * n            # shift: 8 in 8 out; mask: 8 in 8 out; widen: 8 in 32 out
    out["d_compact_limbs"] = {"equal_results": bool(same), "fused": f, "composed": c, "launches_per_call": launches, "products_per_row": 0,
                              "fused_bytes_per_s": fused_bytes / (f["median_ms"] * 1e-3), "composed_bytes_per_s": composed_bytes / (c["median_ms"] * 1e-3),
                              "composed_over_fused": c["median_ms"] / f["median_ms"]}
    # (e) a Montgomery column -> 32 8-bit limbs
    cells = D.empty(n)
    check(L.h2_dev_random_fr((41).to_bytes(32, "little"), n, cells.data_ptr(), D.stream), "h2_dev_random_fr")
    limbs, launch_fn, launches = compiled_many(D, Value.from_limbs(D, cells, montgomery=True).limbs(8, 32))
    h = min(args.python_height, n)
    t0 = time.perf_counter()
    ints = [v * V._R_INV % V.R_MOD for v in V.limbs_to_ints(D.download(cells[:h]))]
    python = [D.upload(np.array([[(v >> (8 * j)) & 0xFF, 0, 0, 0] for v in ints], dtype=np.uint64), widen=False) for j in range(32)]
    D.sync()
    python_s = time.perf_counter() - t0
    same = all(np.array_equal(D.download(x[:h]), D.download(y)) for x, y in zip(limbs, python))
    spin(D, launch_fn)
    e = stats([timed(D, launch_fn) for _ in range(args.reps)])
    moved = launches * (32 + V.limits()["outputs"] * 32) * n
    out["e_montgomery_limbs"] = {"equal_results": bool(same), "fused": e, "launches_per_call": launches, "products_per_row": launches,
                                 "fused_bytes_per_s": moved / (e["median_ms"] * 1e-3),
                                 "fused_products_per_s": launches * n / (e["median_ms"] * 1e-3),
                                 "python_height": h, "python_seconds": python_s,
                                 "per_row_speedup": (python_s / h) / (e["median_ms"] * 1e-3 / n)}
    if stream_rate:
        out["stream_bytes_per_s"] = stream_rate
        for name in ("d_compact_limbs", "e_montgomery_limbs"):
            out[name]["fused_share_of_stream"] = out[name]["fused_bytes_per_s"] / stream_rate


def multiplier_rate(D, n, reps):
    """field products per second of the evaluator's multiplier site: 120 dependent squarings per row, 64 bytes per row"""
    y = Value.from_limbs(D, random_cells(D, n, 99, False), montgomery=True)
    for _ in range(120):
        y = y.square()
    _, run = compiled(D, y, montgomery=True)
    spin(D, run)
    ms = [timed(D, run) for _ in range(reps)]
    return 120 * n / (float(np.median(ms)) * 1e-3), stats(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("k", type=int)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--python-height", type=int, default=1 << 17)
    ap.add_argument("--integers", action="store_true", help="cases (d) and (e) instead of (c)")
    ap.add_argument("--stream-gbs", type=float, default=0.0, help="tools/membench's streaming rate on this device, GB/s")
    args = ap.parse_args()
    D = prover.Device()
    n = 1 << args.k
    out = {"k": args.k, "reps": args.reps, "limits": V.limits()}
    rate, rate_ms = multiplier_rate(D, n, args.reps)
    out["multiplier"] = {"products_per_s": rate, **rate_ms}
    for name, compact in (("a_compact", True), ("b_canonical", False)):
        cells = [random_cells(D, n, 11 + i, compact) for i in range(4)]
        work = [D.empty(n) for _ in range(5)]
        fused_fn = lambda: fused_abcd(D, cells, compact)                     # noqa: E731
        composed_fn = lambda: composed_abcd(D, cells, compact, work)         # noqa: E731
        same = np.array_equal(D.download(fused_fn()), D.download(composed_fn()))
        make = Value.from_u64 if compact else Value.from_limbs
        a, b, c, d = (make(D, t) for t in cells)
        _, launch_fn = compiled(D, a * b * c + d)
        spin(D, launch_fn)
        fused_ms, composed_ms, whole_ms = [], [], []
        before = D.values_launches
        for _ in range(args.reps):
            fused_ms.append(timed(D, launch_fn))
            composed_ms.append(timed(D, composed_fn))
            whole_ms.append(timed(D, fused_fn))                  # with the compiler: its host time lies between the two events
        cell = 8 if compact else 32
        # products: one conversion per 8-byte or canonical leaf, two of the expression, one for the canonical output
        products = 4 + 2 + 1
        f, c = stats(fused_ms), stats(composed_ms)
        fused_bytes = (4 * cell + 32) * n
        composed_bytes = ((4 * (cell + 32) if compact else 4 * 64) + 4 * 64 + 3 * 96 + 64) * n
        out[name] = {"equal_results": bool(same), "fused": f, "composed": c, "fused_with_compile": stats(whole_ms),
                     "launches_per_call": (D.values_launches - before) // (2 * args.reps),
                     "fused_bytes_per_s": fused_bytes / (f["median_ms"] * 1e-3), "composed_bytes_per_s": composed_bytes / (c["median_ms"] * 1e-3),
                     "fused_products_per_s": products * n / (f["median_ms"] * 1e-3),
                     "fused_share_of_multiplier": products * n / (f["median_ms"] * 1e-3) / rate,
                     "composed_over_fused": c["median_ms"] / f["median_ms"]}
    if args.integers:
        integer_cases(D, n, args, out)
        out["e_montgomery_limbs"]["fused_share_of_multiplier"] = out["e_montgomery_limbs"]["fused_products_per_s"] / rate
        print(json.dumps(out))
        return
    # (c) the shuffle's running product at full height
    height = n - 7

    seeded = fe.ShuffleGatesValues(args.k, height=height, device=D, seed=7)
    with torch.cuda.stream(D.tstream):
        originals = [Value.from_limbs(D, random_cells(D, height, 21 + i, False)) for i in range(4)]
    order = torch.randperm(height, device=D.dev)
    torch.cuda.synchronize()                      # torch made `order` on its own stream

    def shuffle_once():
        shuffled = [col.take(order) for col in originals]
        compress = lambda cols: ((cols[0] * seeded.theta + cols[1]) * seeded.theta + cols[2]) * seeded.theta + cols[3]   # noqa: E731
        z = ((compress(originals) + seeded.beta) / (compress(shuffled) + seeded.beta)).cumprod()
        return z.tensor()

    z = shuffle_once()
    ends_at_one = D.download(z[height:height + 1]).tolist() == [[1, 0, 0, 0]]
    spin(D, shuffle_once)
    before = (D.values_launches, D.values_inversions)
    ms = [timed(D, shuffle_once) for _ in range(args.reps)]
    launches, inversions = (D.values_launches - before[0]) // args.reps, (D.values_inversions - before[1]) // args.reps
    t0 = time.perf_counter()
    circuits.shuffle_gates_witness(max(args.python_height + 7, 8).bit_length(), 4, args.python_height)
    python_s = time.perf_counter() - t0
    s = stats(ms)
    out["c_shuffle"] = {"height": height, "z_ends_at_one": bool(ends_at_one), **s, "launches_per_call": launches, "inversions_per_call": inversions,
                        "python_height": args.python_height, "python_seconds": python_s,
                        "per_row_speedup": (python_s / args.python_height) / (s["median_ms"] * 1e-3 / height)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
