"""The wide circuit's witness (circuits.wide: 4 * quads advice columns), timed from nothing to "columns resident" three ways:

  1  circuits.wide_synthesize into pinned (n, 4) columns + the upload create_proof_ext does       (today's path)
  2  the front end (circuits_frontend.Wide) on the host assembly, pinned columns + the same upload
  3  the front end on the device assembly: compact values staged in the page-locked arena, one upload, one launch of
     h2_dev_cells_place

and the placement kernel's achieved bytes per second (8 bytes read and 32 written per cell of route 3; the launch timed by
events, the copy of its segment table included).  Every route runs twice; the second run, which finds its pinned memory
already allocated, is reported -- page-locking is a cost of the first proof, not of every one.

With `selectors` as third argument the tool times a selector-bearing keygen instead (circuits_frontend.SelectorGates: five
selectors over all usable rows, four combination columns), medians of five runs each:

  A  the host assembly (numpy activations, conflicts and combination columns) + the upload of every fixed column
  B  the device assembly: segments marked into bitmaps, conflicts and combination columns by csrc/selectors.hip

and the bytes per second of h2_dev_selectors_combine alone (32 bytes written per row and column, 4 bytes read per member and
32 rows; timed by events).
usage: python tools/synthesis_bench.py [K] [QUADS] [selectors]"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")  # before HIP initialises (halo2-gpu-specific_amd/__init__.py says why)
import numpy as np  # noqa: E402
import torch  # noqa: E402

torch.cuda.init()

from halo2_gpu_specific_amd import circuits, circuits_frontend, prover  # noqa: E402

k = int(sys.argv[1]) if len(sys.argv) > 1 else 20
quads = int(sys.argv[2]) if len(sys.argv) > 2 else 16
n, ncols = 1 << k, 4 * quads
D = prover.Device()


def selector_leg():
    from halo2_gpu_specific_amd import synthesis

    circuit = circuits_frontend.SelectorGates(k)

    def host_route():
        _, fixed, _ = prover.synthesize_keygen(None, circuit, k)
        resident = [D.upload(column) for column in fixed]
        D.sync()
        return resident

    def device_route():
        _, fixed, _ = prover.synthesize_keygen(D, circuit, k, resident=True)
        D.sync()
        return fixed

    results = {}
    for name, route in (("A host assembly + upload", host_route), ("B device assembly", device_route)):
        times = []
        for _ in range(5):
            D.sync()
            begin = time.perf_counter()
            results[name] = route()
            times.append(time.perf_counter() - begin)
        print("selector keygen, k = %d, route %-26s median %.2f ms (runs: %s)"
              % (k, name, 1e3 * float(np.median(times)), ", ".join("%.2f" % (1e3 * t) for t in times)))
    for a, b in zip(*results.values()):
        assert torch.equal(a[:4096], b[:4096]) and torch.equal(a[n - 4096:], b[n - 4096:]), "the routes differ"
    # the combine kernel alone: the circuit's own activations and plan
    cs, _, _ = prover.synthesize_keygen(None, circuits_frontend.SelectorGates(6), 6)
    rows = (n - 6) // 4 * 4
    dev = synthesis.DeviceSelectors(D, 5, n)
    for selector, first, stride in ((0, 0, 4), (1, 1, 4), (1, 2, 4), (2, 2, 4), (4, 0, 4), (4, 3, 4), (3, 0, 8)):
        dev.enable(selector, first, stride, (rows - first + stride - 1) // stride)
    dev.flush()
    combinations = [[3], [4], [0, 1], [2]]
    assert [cs.selector_map[s][1] - 1 for group in combinations for s in group] == [0, 1, 2, 2, 3]
    times = []
    for _ in range(5):
        begin, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        begin.record(D.tstream)
        dev.combine(combinations)
        end.record(D.tstream)
        end.synchronize()
        times.append(begin.elapsed_time(end))
    moved = len(combinations) * n * 32 + sum(len(g) for g in combinations) * n // 8
    print("h2_dev_selectors_combine, k = %d: %d columns, %.1f MiB, median %.3f ms: %.2f TB/s (runs: %s ms)"
          % (k, len(combinations), moved / 2**20, float(np.median(times)), moved / (float(np.median(times)) * 1e-3) / 1e12,
             ", ".join("%.3f" % t for t in times)))


if sys.argv[3:4] == ["selectors"]:
    selector_leg()
    sys.exit(0)
circuit = circuits_frontend.Wide(k, quads)
cs = circuits.wide(quads)

pinned = {}


def alloc(count, rows, compact=False):
    """pinned columns kept between the runs of a route, handed out zeroed (as Device.pinned_columns makes them)"""
    key = (count, rows, compact)
    if key not in pinned:
        pinned[key] = D.pinned_columns(count, rows, compact)
    else:
        for column in pinned[key]:
            column[...] = 0
    marks.append(("pinned columns zeroed", time.perf_counter()))
    return pinned[key]


def upload(columns):
    """what create_proof_ext does with host columns: asynchronous copies of the pinned ones, then the wait for them"""
    resident = []
    for column in columns:
        tensor, event = D.upload_async(column)
        if event is not None:
            D.tstream.wait_event(event)
        resident.append(tensor)
    D.sync()
    D.copy_stream.synchronize()
    return resident


def route_hand():
    advice, _, _ = circuits.wide_synthesize(k, quads, alloc=alloc)
    marks.append(("synthesize", time.perf_counter()))
    return upload(advice)


def route_front_end_host():
    advice, _ = prover.synthesize_witness(D, circuit, cs, k, resident=False, alloc=alloc)
    marks.append(("synthesize", time.perf_counter()))
    return upload(advice)


def route_front_end_device():
    advice, _ = prover.synthesize_witness(D, circuit, cs, k, resident=True, stats=stats)
    D.sync()
    return advice


reference = None
print("wide circuit, k = %d, %d advice columns: %.2f GiB canonical, %.2f GiB compact" % (k, ncols, ncols * n * 32 / 2**30, ncols * n * 8 / 2**30))
for name, route in (("1 hand layout + upload", route_hand), ("2 front end, host assembly + upload", route_front_end_host),
                    ("3 front end, device assembly", route_front_end_device)):
    for run in range(2):
        marks, stats = [], {}
        D.sync()
        begin = time.perf_counter()
        columns = route()
        total = time.perf_counter() - begin
    parts = ", ".join("%s at %.3f s" % (what, at - begin) for what, at in marks)
    print("route %-38s %.3f s%s" % (name, total, " (%s, then the upload)" % parts if parts else ""))
    if stats:
        moved = stats["cells_placed"] * 40
        print("    computing the values (numpy) and the rest of the host %.3f s; staging them in the arena %.3f s; flush (upload + "
              "launch, waited for) %.3f s; %d launch(es), %d cells, %.3f ms: %.2f TB/s"
              % (total - stats["pack_seconds"] - stats["flush_seconds"], stats["pack_seconds"], stats["flush_seconds"],
                 stats["flushes"], stats["cells_placed"], stats["kernel_ms"], moved / (stats["kernel_ms"] * 1e-3) / 1e12))
    # every route must leave the same columns behind
    sample = [D.download(columns[c][:4096]).copy() for c in (0, 1, ncols - 1)] + [D.download(columns[3][n - 4096:]).copy()]
    if reference is None:
        reference = sample
    assert all(np.array_equal(a, b) for a, b in zip(sample, reference)), "route %s differs" % name
    del columns
