"""check_witness, check_assignments and check_circuit: MockProver::run(..).verify() (dev.rs:932-1340) on the device, reported as
MockProver's failures."""
import ctypes
import hashlib
import time
from collections import namedtuple

import numpy as np

from ._lib import check
from .circuit import compile_compress
from .domain import _vp
from .synthesis import CHECK_CELL, synthesize_coverage, synthesize_witness
from .transcript import R_MOD
from .witness import _compress, _compress_desc, _instance_columns, _witness_sets

CHECK_GATE, CHECK_LOOKUP, CHECK_SHUFFLE, CHECK_COPY = 0, 1, 2, 3      # h2_check_record.kind & 0xff (include/halo2_hip.h)
# MockProver's VerifyFailure variants (dev.rs), with the index of the circuit instance in `circuit`
ConstraintNotSatisfied = namedtuple("ConstraintNotSatisfied", "gate_index gate_name poly_index row circuit")
Lookup = namedtuple("Lookup", "name lookup_index input_set_index input_fail_index row circuit")
Shuffle = namedtuple("Shuffle", "name group_index shuffle_index row circuit")
Permutation = namedtuple("Permutation", "column row circuit")
# dev.rs:959-1000: `column` = (kind, index) of the cell gate `gate_index` reads at `row`, `offset` = row - the region's start
CellNotAssigned = namedtuple("CellNotAssigned", "gate_index gate_name region_index region_name column offset row")


def _record_order(r):
    """cell failures first (verify_at_rows chains them first), by (region, gate, query, row); then the rest"""
    circuit, k = r[0] >> 8, r[0] & 0xFF
    return (circuit, -1, r[2], r[1], r[3]) if k == CHECK_CELL else (circuit, k, r[1], r[2], r[3])


def check_failures(cs, records, coverage=None):
    """h2_check_records -- (kind, index, sub, row) rows, kind = H2_CHECK_* | circuit << 8 -- as MockProver's failures, in the
    order MockProver chains them: circuit by circuit; unassigned cells (by region, gate, queried cell and row), gates, lookups,
    shuffles, then the permutation; within a kind by index, sub-index and row.  Records of kind H2_CHECK_CELL are named with
    the region and gate tables of `coverage` (synthesize_coverage), the others with `cs`."""
    gate_of = [(gi, name, pi) for gi, (name, polys) in enumerate(cs.gates) for pi in range(len(polys))] if cs is not None else []
    keyed = []
    for kind, index, sub, row in sorted({tuple(int(v) for v in r) for r in records}, key=_record_order):
        circuit, k = kind >> 8, kind & 0xFF
        if k == CHECK_CELL:
            if coverage is None:
                raise ValueError("check: a cell record needs the coverage it came from")
            name, _, cells = coverage.gates[index >> 16]
            keyed.append(CellNotAssigned(index >> 16, name, sub, coverage.regions[sub][0], cells[index & 0xFFFF][0],
                                         row - coverage.start(sub), row))
        elif k == CHECK_GATE:
            gi, name, pi = gate_of[index]
            keyed.append(ConstraintNotSatisfied(gi, name, pi, row, circuit))
        elif k == CHECK_LOOKUP:
            keyed.append(Lookup(cs.lookups[index][0], index, sub >> 16, sub & 0xFFFF, row, circuit))
        elif k == CHECK_SHUFFLE:
            keyed.append(Shuffle(cs.shuffles[index][sub][0], index, sub, row, circuit))
        elif k == CHECK_COPY:
            keyed.append(Permutation(cs.perm_columns[index], row, circuit))
        else:
            raise ValueError("check: unknown record kind %d" % kind)
    return keyed


def _check_scalar(seed, what):
    """a non-zero field element drawn from the caller's seed (the screen's y, the compressions' theta)"""
    h = hashlib.blake2b(b"halo2 check_witness " + what + int(seed).to_bytes(16, "little", signed=True), digest_size=64)
    return int.from_bytes(h.digest(), "little") % (R_MOD - 1) + 1


def check_witness(device, pk, advice, instances=(), seed=0, max_failures=1024, montgomery=False, first_unassigned=None,
                  timings=None, range_checks_on_device=False, strict_rationals=False):
    """Checks a witness against the circuit of `pk` on the device, as MockProver::run(..).verify() does (dev.rs:932-1340), and
    returns (failures, total): `failures` the first max_failures of them (check_failures: named tuples with MockProver's field
    names, sorted as MockProver chains its errors), `total` the exact number of failures.

    The witness is taken as create_proof_ext takes it -- canonical (n, 4) columns, Montgomery ones with montgomery=True,
    compact 1-D columns, device tensors, `Rational` columns (resolved first; `strict_rationals` as there), several circuit
    instances as a list of column lists with one instance list each --
    and is not modified: range-checked columns are completed on copies (complete_range_check_witness, or its device form
    for resident / Montgomery columns and with `range_checks_on_device`; the ValueError propagates) and no blinding value
    is written.  Under a multi-rank Device the check runs on this rank's GPU alone.

      gates     every polynomial of every gate at the usable rows: all of them Horner-folded in a random y (from `seed`) in one
                base-domain evaluation, then the rows where that is non-zero interpreted polynomial by polynomial
      lookups   every input tuple (theta-compressed, theta from `seed`) of every usable row in the usable rows of its table; a
                row reports its first missing (set, input)
      shuffles  the input rows whose compressed value occurs a different number of times on the two sides (MockProver reports
                rows of its sorted tuples instead, an order compression destroys)
      copies    every cell of every permutation column, all n rows, against the cell its cycle maps it to
    A reported failure is always real; a real one is missed with probability <= (parts or tuple length) x n / r < 2^-200.

    Out of scope: MockProver's ConstraintPoisoned (cells in rows >= usable are read as the caller supplied them), gate rows in
    the blinding region, any change to create_proof*, and the Rust shims under integration/.  An unassigned cell of a dense
    witness is a zero here; a gate enabled over one is found by check_assignments, which takes the circuit and not the witness.
    `timings` (a dict): filled with the seconds of each phase (synchronising between them)."""
    D, L, torch = device, device.L, device.torch
    cs, dom = pk.cs, pk.domain
    n = dom.n
    usable = n - (cs.blinding_factors() + 1)
    advice_sets, instance_sets = _witness_sets(cs, n, advice, instances, montgomery, first_unassigned, copy_range_columns=True,
                                               device=D, range_checks_on_device=range_checks_on_device,
                                               strict_rationals=strict_rationals)
    cap = max(int(max_failures), 0)
    y, theta = _check_scalar(seed, b"y"), _check_scalar(seed, b"theta")
    t_last = [time.perf_counter()]

    def phase(name):
        if timings is not None:
            D.sync()
            now = time.perf_counter()
            timings[name] = timings.get(name, 0.0) + now - t_last[0]
            t_last[0] = now

    # one device block for the count and every record: [u64 count, pad][cap x 16 B]; one download at the end
    with torch.cuda.stream(D.tstream):
        blob = torch.zeros(4 * (cap + 1), dtype=torch.int32, device=D.dev)
        rows_list = torch.empty(max(usable, 1), dtype=torch.int32, device=D.dev)
        row_count = torch.zeros(1, dtype=torch.int64, device=D.dev)
    out = (blob.data_ptr(), blob.data_ptr() + 16, cap)
    scratch = None
    gate_prog = pk.__dict__.get("_check_gate_program")
    if gate_prog is None:
        gate_prog = pk._check_gate_program = compile_compress([p for _, polys in cs.gates for p in polys])
    ncols = len(cs.perm_columns)
    if ncols:
        map_col, map_row = pk.mapping
        with torch.cuda.stream(D.tstream):
            maps = torch.from_numpy(np.concatenate([np.ascontiguousarray(c, dtype=np.uint32) for c in list(map_col) + list(map_row)])
                                    .view(np.int32)).to(D.dev)
    for ci, (adv_in, inst_in) in enumerate(zip(advice_sets, instance_sets)):
        if len(adv_in) != cs.num_advice:
            raise ValueError("check_witness: %d advice columns for a circuit of %d" % (len(adv_in), cs.num_advice))
        inst = _instance_columns(D, cs, n, usable, inst_in)
        adv = []
        for col in adv_in:
            t, arrived = D.upload_async(col)          # a copy on the device: the caller's column is only read
            if arrived is not None:
                D.tstream.wait_event(arrived)
            if montgomery:
                check(L.h2_dev_batch_unmont(t.data_ptr(), n, D.stream), "h2_dev_batch_unmont")
            check(L.h2_dev_batch_mont(t.data_ptr(), n, D.stream), "h2_dev_batch_mont")
            adv.append(t)
        phase("upload")
        fixed = pk.fixed_values
        if gate_prog[1]:
            screen = _compress(D, dom, gate_prog, y, fixed, adv, inst)
            with torch.cuda.stream(D.tstream):
                row_count.zero_()
            check(L.h2_dev_check_nonzero_rows(screen.data_ptr(), usable, rows_list.data_ptr(), row_count.data_ptr(), D.stream),
                  "h2_dev_check_nonzero_rows")
            phase("screen")
            b = _compress_desc(D, dom, gate_prog, y, fixed, adv, inst)
            check(L.h2_dev_check_gates(ctypes.byref(b.desc), rows_list.data_ptr(), row_count.data_ptr(), ci, *out, D.stream),
                  "h2_dev_check_gates")
            del screen
            phase("localise")

        def compress(program):
            return _compress(D, dom, program, theta, fixed, adv, inst)

        if cs.lookups or cs.shuffles:
            nbytes = L.h2_check_scratch_bytes(n)
            scratch = D.scratch(nbytes)
        for li, (table_prog, set_progs) in enumerate(pk.lookup_programs):
            table = compress(table_prog)
            inputs, tags = [], []
            for si, progs in enumerate(set_progs):
                for ii, pr in enumerate(progs):
                    inputs.append(compress(pr))
                    tags.append(si << 16 | ii)
            ptrs = (_vp * len(inputs))(*[c.data_ptr() for c in inputs])
            check(L.h2_dev_check_lookup(table.data_ptr(), ptrs, (ctypes.c_uint32 * len(tags))(*tags), len(inputs), usable, n, li,
                                        ci, scratch.data_ptr(), nbytes, *out, D.stream), "h2_dev_check_lookup")
        phase("lookups")
        for gi, group in enumerate(pk.shuffle_programs):
            for ui, (ip, sp) in enumerate(group):
                inp, shf = compress(ip), compress(sp)         # (both held: a freed vector's memory is reused at once)
                check(L.h2_dev_check_shuffle(inp.data_ptr(), shf.data_ptr(), usable, n, gi, ui, ci, scratch.data_ptr(), nbytes,
                                             *out, D.stream), "h2_dev_check_shuffle")
        phase("shuffles")
        if ncols:
            colvals = {"advice": adv, "fixed": fixed, "instance": inst}
            with torch.cuda.stream(D.tstream):
                col_ptrs = torch.tensor([colvals[kd][i].data_ptr() for kd, i in cs.perm_columns], dtype=torch.int64).to(D.dev)
            check(L.h2_dev_check_copies(col_ptrs.data_ptr(), ncols, maps.data_ptr(), maps.data_ptr() + ncols * n * 4, n, ci,
                                        *out, D.stream), "h2_dev_check_copies")
        phase("copies")
        del adv, inst
    with torch.cuda.stream(D.tstream):
        host = blob.cpu().numpy().view(np.uint32)
    phase("download")
    return check_result(cs, host, cap)


def check_result(cs, words, cap, coverage=None):
    """(failures, total) of check_witness's downloaded block: u32 words = [u64 count, 2 pad][cap records of 4]; when the
    count exceeds cap only the first cap slots hold records"""
    total = int(np.ascontiguousarray(words[:2]).view(np.uint64)[0])
    return check_failures(cs, words[4:4 + 4 * cap].reshape(-1, 4)[:min(total, cap)], coverage), total


def check_assignments(device, circuit, k, planner=None, max_failures=1024, resident=True, timings=None):
    """MockProver's VerifyFailure::CellNotAssigned (dev.rs:959-1000): every cell that a gate reads from a row on which a
    region enabled one of the gate's selectors must have been assigned BY THAT REGION.  -> (failures, total): the first
    max_failures of them as CellNotAssigned tuples sorted by (region, gate, queried cell, row), and their exact number.

    One assignment pass of `circuit` (synthesize_coverage: no value is placed, missing ones are keygen's business) queues the
    regions' assignments and enabled rows; with `resident` one launch marks the cells in a device bit array and one launch
    tests every enabled row of every gate against it (csrc/coverage.hip); otherwise numpy does both (`device` may be None).
    The definition, with what differs from the reference, is DESIGN.md 3b, "Checking assignments".  `timings` (a dict): the
    seconds of synthesize, mark, check and download."""
    cap = max(int(max_failures), 0)
    begin = time.perf_counter()
    coverage = synthesize_coverage(device, circuit, k, planner, resident)
    if timings is not None:
        timings["synthesize"] = timings.get("synthesize", 0.0) + time.perf_counter() - begin
    records, total = coverage.check(cap, timings) if resident else coverage.check(cap)
    return check_failures(None, records, coverage), total


def check_circuit(device, pk, circuit, k, instances=(), planner=None, seed=0, max_failures=1024, resident=True, timings=None):
    """MockProver::run(k, &circuit, instances).verify(): check_assignments, then the witness pass of `circuit`
    (synthesize_witness) and check_witness on what it assigned.  -> (failures, total): the unassigned cells first, the rest in
    check_witness's order, at most max_failures of either; `total` counts both exactly."""
    cells, cell_total = check_assignments(device, circuit, k, planner, max_failures, resident, timings)
    advice, first_unassigned = synthesize_witness(device, circuit, pk, k, planner, resident, instances=list(instances) or None)
    failures, total = check_witness(device, pk, advice, list(instances), seed, max_failures, first_unassigned=first_unassigned,
                                    timings=timings)
    return cells + failures, cell_total + total


def _describe_failure(f):
    if isinstance(f, CellNotAssigned):
        return "region %d '%s' enables gate %d '%s' over %s column %d at offset %d (row %d), a cell it never assigned" % (
            f.region_index, f.region_name, f.gate_index, f.gate_name, f.column[0], f.column[1], f.offset, f.row)
    where = "circuit %d: " % f.circuit if f.circuit else ""
    if isinstance(f, ConstraintNotSatisfied):
        return "%sgate %d '%s' polynomial %d is not satisfied at row %d" % (where, f.gate_index, f.gate_name, f.poly_index, f.row)
    if isinstance(f, Lookup):
        return "%slookup %d '%s' (input set %d, input %d): row %d is not in the table" % (
            where, f.lookup_index, f.name, f.input_set_index, f.input_fail_index, f.row)
    if isinstance(f, Shuffle):
        return "%sshuffle '%s' (group %d, unit %d): the value of row %d is not shuffled" % (
            where, f.name, f.group_index, f.shuffle_index, f.row)
    return "%scopy constraint of %s column %d broken at row %d" % (where, f.column[0], f.column[1], f.row)


def _raise_failures(what, name, failures, total, shown):
    lines = [_describe_failure(f) for f in failures[:shown]]
    more = total - len(lines)
    raise ValueError("%s does not satisfy circuit '%s': %d failure(s)\n  %s%s" % (
        what, name, total, "\n  ".join(lines), "\n  ... and %d more" % more if more > 0 else ""))


def assert_circuit_satisfied(device, pk, circuit, k, instances=(), planner=None, seed=0, max_failures=1024, resident=True, shown=10):
    """MockProver::assert_satisfied (dev.rs:1354-1370) over check_circuit: raises ValueError with the first `shown` failures
    described and the total when there is any"""
    failures, total = check_circuit(device, pk, circuit, k, instances, planner, seed, max_failures, resident)
    if total:
        _raise_failures("the circuit's synthesis", pk.cs.name, failures, total, shown)


def assert_satisfied(device, pk, advice, instances=(), seed=0, max_failures=1024, montgomery=False, first_unassigned=None,
                     shown=10):
    """MockProver::assert_satisfied (dev.rs:1354-1370): check_witness, raising ValueError with the first `shown` failures
    (gate, lookup or column name and row) and the total when there is any"""
    failures, total = check_witness(device, pk, advice, instances, seed, max_failures, montgomery, first_unassigned)
    if total:
        _raise_failures("the witness", pk.cs.name, failures, total, shown)
