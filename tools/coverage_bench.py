"""prover.check_assignments on the wide circuit (circuits_frontend.Wide: COLUMNS advice columns assigned over every usable row in
one region), with the gate's fixed column q replaced by a selector enabled on every usable row -- as circuits written against
the front end have it, and without it there is no enabled row to check:

  1  the host assembly (numpy) and the device assembly (csrc/coverage.hip), seconds per phase: synthesize, mark, check, download
  2  h2_dev_coverage_mark alone, by events: cells marked per second -- stride-1 segments, one atomic OR per 32 cells -- next to
     h2_dev_selectors_mark over the same number of rows of the same length (COLUMNS selectors enabled on every usable row),
     the kernel that issues one atomic OR per cell
  3  h2_dev_coverage_check alone, by events: enabled rows (each read through the gate's COLUMNS queries) per second
  4  prover.check_witness of the same circuit's witness by the code path of tools/check_bench.py, whole and per phase: what
     check_circuit adds to it is the device line of 1

usage: python tools/coverage_bench.py [K] [COLUMNS] [--no-witness]"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")  # before HIP initialises (halo2-gpu-specific_amd/__init__.py says why)
import numpy as np  # noqa: E402
import torch  # noqa: E402

torch.cuda.init()

from halo2_gpu_specific_amd import circuits, circuits_frontend, prover, synthesis  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
k = int(args[0]) if args else 20
columns = int(args[1]) if len(args) > 1 else 64
quads, n = columns // 4, 1 << k
usable = n - 6
D = prover.Device()


class WideSelected(circuits_frontend.Wide):
    """Wide with `mul3` switched by a selector; no values: check_assignments looks at none"""

    def __init__(self):
        circuits_frontend.Wide.__init__(self, k, quads, witness=False)

    def without_witnesses(self):
        return self

    def configure(self, cs):
        config = circuits_frontend.Wide.configure(self, cs)
        name, polys = cs.gates.pop()
        config.s = cs.selector()
        cells = [cs.query_advice(col) for col in config.advice]
        cs.create_gate(name, [cs.query_selector(config.s) * (cells[4 * i] * cells[4 * i + 1] * cells[4 * i + 2] + cells[4 * i + 3] * (-1))
                              for i in range(quads)])
        return config

    def synthesize(self, config, layouter):
        def body(region):
            region.assign_fixed(config.t, 0, np.arange(min(usable, 1 << 16), dtype=np.uint64))
            for column in config.advice:
                region.assign_advice(column, 0, None, count=usable)
            region.enable_selector(config.s, 0, count=usable)

        layouter.assign_region("rows", body)


def by_events(call, runs=5):
    times = []
    for _ in range(runs):
        begin, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        begin.record(D.tstream)
        call()
        end.record(D.tstream)
        end.synchronize()
        times.append(begin.elapsed_time(end))
    return float(np.median(times)), ", ".join("%.3f" % t for t in times)


circuit = WideSelected()
print("wide circuit with a selector, k = %d, %d advice columns: %d cells to mark, %d enabled rows x %d queried cells"
      % (k, columns, columns * usable + min(usable, 1 << 16), usable, columns))
for name, resident in (("host assembly", False), ("device assembly", True)):
    for run in range(2):                            # the second run finds the scratch allocated
        phases = {}
        D.sync()
        begin = time.perf_counter()
        result = prover.check_assignments(D, circuit, k, resident=resident, timings=phases)
        whole = time.perf_counter() - begin
    assert result == ([], 0), result
    if not resident:                                # the host assembly marks and checks in one call: no phases inside
        phases = {"synthesize": phases["synthesize"], "mark + check": whole - phases["synthesize"]}
    print("check_assignments, %-16s %.4f s: %s" % (name, whole, ", ".join("%s %.4f s" % (p, s) for p, s in phases.items())))

coverage = prover.synthesize_coverage(D, circuit, k)


def mark():
    coverage.bits = None
    coverage.mark()


ms, runs = by_events(mark)
print("h2_dev_coverage_mark (with the zeroing of its %d-word bit array): %d segments, %d cells, median %.3f ms: %.2f G cells/s (runs: %s ms)"
      % (coverage.build()[5], len(coverage.segments), coverage.cells_marked, ms, coverage.cells_marked / (ms * 1e-3) / 1e9, runs))
selectors = synthesis.DeviceSelectors(D, columns, n)


def mark_selectors():
    for s in range(columns):
        selectors.enable(s, 0, 1, usable)
    selectors.flush()


ms, runs = by_events(mark_selectors)
print("h2_dev_selectors_mark: %d segments, %d rows, median %.3f ms: %.2f G rows/s (runs: %s ms)"
      % (columns, columns * usable, ms, columns * usable / (ms * 1e-3) / 1e9, runs))
ms, runs = by_events(lambda: coverage.check(16))
print("h2_dev_coverage_check (with its mark-free set-up and the download of 16 records): %d rows x %d queries, median %.3f ms: "
      "%.2f G rows/s, %.1f G cells/s (runs: %s ms)" % (coverage.rows_enabled, columns, ms, coverage.rows_enabled / (ms * 1e-3) / 1e9,
                                                      coverage.rows_enabled * columns / (ms * 1e-3) / 1e9, runs))
del coverage, selectors

if "--no-witness" not in sys.argv:
    params = prover.Params.unsafe_setup(D, k, 0x1D0C5F0A3B7E91C2A4D6F8091B2C3D4E5F60718293A4B5C6D7E8F9010203)
    adv, fixed, copies = circuits.wide_synthesize(k, quads, alloc=D.pinned_columns, compact=True)
    pk = prover.keygen(D, params, circuits.wide(quads), fixed, copies)
    prover.check_witness(D, pk, adv)                # warm-up (and the generated kernels' first build)
    D.sync()
    begin = time.perf_counter()
    assert prover.check_witness(D, pk, adv) == ([], 0)
    whole = time.perf_counter() - begin
    timed = {}
    prover.check_witness(D, pk, adv, timings=timed)
    print("check_witness, wide-%d k=%d: %.4f s; phases %s" % (quads, k, whole, {a: round(b, 4) for a, b in timed.items()}))
