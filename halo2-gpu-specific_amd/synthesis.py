"""A circuit front end: `Circuit`, `Layouter`, `Region`, `Table`, the floor planners `FlatFloorPlanner` and `V1`, and the two
assemblies the assignments end up in.

  Circuit / Layouter / Region / Table   circuit.rs (Layouter :393-474, Region :172-360, Table :362-391)
  SimpleTableLayouter                   circuit/floor_planner/single_pass.rs:56-110, flat.rs:177-233
  FlatFloorPlanner                      circuit/floor_planner/flat.rs:33-95
  V1                                    circuit/floor_planner/v1.rs:65-161, v1/strategy.rs:107-225
  errors                                plonk/error.rs

The front end is a BULK one: an assignment covers a range of cells (`count` cells `stride` rows apart), never one Python call
per cell of a 2^22-row column.  Values are a Python integer (one cell, or the same value for `count` cells), a 1-D u64 array
(compact cells: 8 bytes each), an (m, 4) u64 array (canonical cells), a device tensor of either shape (values torch code
computed on the device: they never visit the host), a `Value` (values.py: field arithmetic computed on the device; an unknown
Value is None with its count), or None (keygen, `without_witnesses`).

Selectors (`cs.selector()`, `Region.enable_selector`) are kept as one bit per row -- `HostSelectors` in numpy, `DeviceSelectors`
as device bitmaps (csrc/selectors.hip) -- and become fixed columns after the planner has run: the conflict matrix of the
activations, `ConstraintSystem.compress_selectors`, then one combination column per group, appended to the fixed columns.

Two assemblies sit behind one interface: `HostColumns` writes numpy columns; `DeviceColumns` gathers the ranges into a segment
list that ONE launch of h2_dev_cells_place (csrc/place.hip) places into resident columns.  The reference lets a later
assignment of a cell win; the device assembly keeps that by flushing its queue before it queues a segment that may overlap a
queued one of the same column.

A third pass keeps no value at all: `synthesize_coverage` records WHICH cells each region assigns and which selector rows it
enables -- `HostCoverage` in numpy, `DeviceCoverage` as region-tagged bits on the device (csrc/coverage.hip) -- for
check.check_assignments, MockProver's CellNotAssigned ("Checking assignments").
"""
import math
import time

import numpy as np

from ._lib import check
from .circuit import R_MOD, ConstraintSystem, gate_cells
from .values import Value

PLACE_FORM_CANONICAL, PLACE_FORM_COMPACT, PLACE_FORM_BROADCAST = 0, 1, 2               # H2_PLACE_FORM_*
PLACE_OUT_CANONICAL, PLACE_OUT_MONTGOMERY = 0, 1                                       # H2_PLACE_OUT_*
# h2_place_segment: dst, src, first_row, stride, count (u64 each), form, reserved (u32 each)
PLACE_SEGMENT = np.dtype([("dst", "<u8"), ("src", "<u8"), ("first_row", "<u8"), ("stride", "<u8"), ("count", "<u8"),
                          ("form", "<u4"), ("reserved", "<u4")])
# h2_selector_segment, h2_selector_column, h2_selector_member
SELECTOR_SEGMENT = np.dtype([("selector", "<u4"), ("reserved", "<u4"), ("first_row", "<u8"), ("stride", "<u8"), ("count", "<u8")])
SELECTOR_COLUMN = np.dtype([("dst", "<u8"), ("first_member", "<u4"), ("num_members", "<u4")])
SELECTOR_MEMBER = np.dtype([("value", "<u8", (4,)), ("selector", "<u4"), ("reserved", "<u4")])
# h2_coverage_plane, h2_coverage_segment, h2_coverage_query, h2_coverage_use
COVERAGE_PLANE = np.dtype([("first_word", "<u8"), ("row_lo", "<u4"), ("rows", "<u4")])
COVERAGE_SEGMENT = np.dtype([("plane", "<u4"), ("reserved", "<u4"), ("first_row", "<u8"), ("stride", "<u8"), ("count", "<u8")])
COVERAGE_QUERY = np.dtype([("plane", "<u4"), ("column", "<u4"), ("rotation", "<i4"), ("reserved", "<u4")])
COVERAGE_USE = np.dtype([("region", "<u4"), ("gate", "<u4"), ("first_query", "<u4"), ("num_queries", "<u4"),
                         ("first_earlier", "<u4"), ("num_earlier", "<u4"), ("first_row", "<u8"), ("stride", "<u8"), ("count", "<u8")])
COVERAGE_NO_PLANE = 0xFFFFFFFF                                                         # H2_COVERAGE_NO_PLANE
COVERAGE_MAX_WORDS = 1 << 30                                                           # the bit array: 4 GiB at the most
CHECK_CELL = 4                                                                         # H2_CHECK_CELL
_MASK64 = (1 << 64) - 1
# Column's Ord (plonk/circuit.rs:47-105); a region's selectors order after all real columns (RegionColumn, layouter.rs:143-166)
_COLUMN_ORDER = {"instance": 0, "advice": 1, "fixed": 2, "selector": 3}


# -- errors (plonk/error.rs) ---------------------------------------------------------------------------------------------
class SynthesisError(Exception):
    """Error::Synthesis: a table used wrongly, a value missing where one is needed"""


class NotEnoughRowsAvailable(SynthesisError):
    """a cell at or beyond the usable rows of a 2^k-row circuit"""

    def __init__(self, k):
        SynthesisError.__init__(self, "k = %d is too small for the given circuit" % k)
        self.current_k = k


class NotEnoughColumnsForConstants(SynthesisError):
    """more constants than free cells in the columns of `enable_constant`"""


class ColumnNotInPermutation(SynthesisError):
    """a copy constraint on a column without `enable_equality`"""

    def __init__(self, column):
        SynthesisError.__init__(self, "column %s[%d] is not in the permutation (enable_equality)" % column)
        self.column = column


class BoundsFailure(SynthesisError):
    """a column the constraint system does not have"""


# -- values --------------------------------------------------------------------------------------------------------------
def _limbs(v):
    v %= R_MOD
    return [(v >> (64 * j)) & _MASK64 for j in range(4)]


class _Values:
    """one assignment's values: kind = "none" | "int" | "host" | "device"; compact = one u64 per cell.  A known Value is
    canonical cells of its backend, materialised when `data` is first read (a pass that keeps no values never does)"""

    def __init__(self, values, count):
        self._lazy, self.data, self.compact = None, values, False
        if isinstance(values, Value):
            if count is not None and count != values.count:
                raise ValueError("%d values for %d cells" % (values.count, count))
            self.count = values.count
            if values.known:
                self.kind, self._lazy = "host" if values.device is None else "device", values
            else:
                self.kind, self.data = "none", None
        elif values is None:
            self.kind, self.count = "none", 1 if count is None else count
        elif isinstance(values, (int, np.integer)):
            self.kind, self.data, self.count = "int", int(values) % R_MOD, 1 if count is None else count
        elif isinstance(values, np.ndarray):
            if values.dtype != np.uint64 or not (values.ndim == 1 or (values.ndim == 2 and values.shape[1] == 4)):
                raise TypeError("cell values are u64 arrays of shape (m,) or (m, 4)")
            self.kind, self.compact, self.count = "host", values.ndim == 1, len(values)
        elif hasattr(values, "data_ptr"):
            if not values.is_cuda or values.element_size() != 8 or not (values.dim() == 1 or (values.dim() == 2 and values.shape[1] == 4)):
                raise TypeError("resident cell values are 64-bit device tensors of shape (m,) or (m, 4)")
            if not values.is_contiguous():
                values = self.data = values.contiguous()
            self.kind, self.compact, self.count = "device", values.dim() == 1, values.shape[0]
        else:
            raise TypeError("cell values: an integer, a u64 array, a device tensor or None")
        if count is not None and self.kind in ("host", "device") and count != self.count:
            raise ValueError("%d values for %d cells" % (self.count, count))

    @property
    def data(self):
        if self._lazy is not None:
            self._data, self._lazy = self._lazy.tensor(), None
        return self._data

    @data.setter
    def data(self, values):
        self._data = values

    def first(self):
        """the first value as an integer (a table column's default)"""
        if self.kind == "int":
            return self.data
        if self.kind == "none" or self.count == 0:
            return None
        head = self.data[:1]
        if self.kind == "device":
            head = head.cpu().numpy().view(np.uint64)
        return int(head[0]) if self.compact else sum(int(x) << (64 * j) for j, x in enumerate(head[0]))


class AssignedCells:
    """`count` assigned cells of one column, `stride` rows apart from `row` on: what an assignment returns and what the
    constraints of a region take.  Slicing gives the sub-range.  `value()`: the Value the cells were assigned from
    (`AssignedCell::value()`, circuit.rs), unknown when they were assigned from anything else."""

    def __init__(self, column, row, count=1, stride=1, value=None):
        self.column, self.row, self.count, self.stride, self._value = column, row, count, stride, value

    def value(self):
        return self._value if self._value is not None else Value.unknown(self.count)

    def __len__(self):
        return self.count

    def __getitem__(self, key):
        if isinstance(key, slice):
            start, stop, step = key.indices(self.count)
            if step < 1:
                raise ValueError("cells are sliced forwards")
            return AssignedCells(self.column, self.row + start * self.stride, len(range(start, stop, step)), self.stride * step,
                                 None if self._value is None else self._value[key])
        if not -self.count <= key < self.count:
            raise IndexError(key)
        return AssignedCells(self.column, self.row + (key % self.count) * self.stride, 1, 1,
                             None if self._value is None else self._value[key])

    def rows(self):
        return self.row + self.stride * np.arange(self.count, dtype=np.int64)

    def __repr__(self):
        return "AssignedCells(%s[%d], row %d, %d x %d)" % (self.column + (self.row, self.count, self.stride))


# -- the two assemblies --------------------------------------------------------------------------------------------------
class HostColumns:
    """`count` canonical (n, 4) u64 numpy columns, zero until assigned; `alloc(count, n)` supplies them (Device.pinned_columns)"""

    def __init__(self, count, n, alloc=None):
        self.n = n
        self.columns = list(alloc(count, n)) if alloc and count else [np.zeros((n, 4), dtype=np.uint64) for _ in range(count)]

    def place(self, index, row, stride, vals):
        if vals.count == 0:
            return
        target = self.columns[index][row:row + (vals.count - 1) * stride + 1:stride]
        if vals.kind == "int":
            target[:] = np.array(_limbs(vals.data), dtype=np.uint64)
            return
        data = vals.data if vals.kind == "host" else vals.data.cpu().numpy().view(np.uint64)
        if vals.compact:
            target[:, 0], target[:, 1:] = data, 0
        else:
            target[:] = data

    def finish(self):
        return self.columns


class _Arena:
    """page-locked staging of one form's host values: appended to as the regions assign, uploaded once per flush"""

    def __init__(self, torch, width):
        self.torch, self.width, self.used, self.buf, self.busy = torch, width, 0, None, None
        self.pack_seconds = 0.0

    def append(self, data):
        begin = time.perf_counter()
        at = self._append(data)
        self.pack_seconds += time.perf_counter() - begin
        return at

    def _append(self, data):
        if self.busy is not None:                 # the previous flush's upload still reads the buffer
            self.busy.synchronize()
            self.busy = None
        need = self.used + len(data)
        if self.buf is None or need > len(self.buf):
            grown = self.torch.empty((max(need, 2 * (len(self.buf) if self.buf is not None else 0), 1 << 12), self.width),
                                     dtype=self.torch.int64).pin_memory()
            if self.used:
                grown[:self.used] = self.buf[:self.used]
            self.buf = grown
        self.buf.numpy().view(np.uint64)[self.used:need] = data.reshape(len(data), self.width)
        self.used = need
        return need - len(data)


class DeviceColumns:
    """`count` resident (n, 4) columns, zero until assigned, written by h2_dev_cells_place: canonical, or Montgomery residues
    (`montgomery`: keygen's fixed columns).  Host values are staged in one page-locked arena per form and cross PCIe once per
    flush, compact cells at 8 bytes; device tensors are read where they are.  A segment that may overlap a queued one of its
    column flushes the queue first, so that the later assignment wins as it does in the reference."""

    def __init__(self, device, count, n, montgomery=False, timed=False):
        self.D, self.n, self.out_form = device, n, PLACE_OUT_MONTGOMERY if montgomery else PLACE_OUT_CANONICAL
        self.columns = [device.zeros(n) for _ in range(count)]
        # the staging arenas stay with the Device between syntheses (page-locking memory costs more than filling it); an
        # assembly takes a pair for its lifetime and hands it back in finish()
        pool = device.__dict__.setdefault("_place_arenas", [])
        self.arenas = pool.pop() if pool else {False: _Arena(device.torch, 4), True: _Arena(device.torch, 1)}
        for arena in self.arenas.values():
            arena.pack_seconds = 0.0
        self.queue, self.boxes, self.keep = [], {}, []
        self.cells_placed = self.flushes = 0
        self.timed, self.kernel_ms, self.flush_seconds = timed, 0.0, 0.0

    @staticmethod
    def _may_overlap(a, b):
        (r0, s0, c0), (r1, s1, c1) = a, b
        if r0 + (c0 - 1) * s0 < r1 or r1 + (c1 - 1) * s1 < r0:
            return False
        return (r1 - r0) % math.gcd(s0, s1) == 0

    def _overlaps_queued(self, index, row, stride, count):
        """may this range write a cell that a queued segment of the column writes?  Exact for single cells, conservative for
        two strided ranges (same residue modulo the gcd of the strides, inside each other's bounds)"""
        box = self.boxes.get(index)
        last = row + (count - 1) * stride
        if box is None or last < box[0] or row > box[1]:
            return False
        spans, singles = box[2], box[3]
        if count == 1:
            if row in singles:
                return True
        elif singles and any(row <= r <= last and (r - row) % stride == 0 for r in singles):
            return True
        return any(self._may_overlap((row, stride, count), other) for other in spans)

    def place(self, index, row, stride, vals):
        if vals.count == 0:
            return
        if self._overlaps_queued(index, row, stride, vals.count):
            self.flush()
        last = row + (vals.count - 1) * stride
        box = self.boxes.setdefault(index, [row, last, [], set()])
        box[0], box[1] = min(box[0], row), max(box[1], last)
        if vals.count == 1:
            box[3].add(row)
        else:
            box[2].append((row, stride, vals.count))
        if vals.kind == "int":
            form, source = PLACE_FORM_BROADCAST, (False, self.arenas[False].append(np.array([_limbs(vals.data)], dtype=np.uint64)))
        elif vals.kind == "host":
            form = PLACE_FORM_COMPACT if vals.compact else PLACE_FORM_CANONICAL
            source = (vals.compact, self.arenas[vals.compact].append(vals.data))
        else:
            form, source = PLACE_FORM_COMPACT if vals.compact else PLACE_FORM_CANONICAL, vals.data
            self.keep.append(vals.data)
        self.queue.append((index, row, stride, vals.count, form, source))

    def flush(self):
        if not self.queue:
            return
        started = time.perf_counter()
        self._flush()
        self.flush_seconds += time.perf_counter() - started

    def _flush(self):
        D, torch = self.D, self.D.torch
        caller = torch.cuda.current_stream(D.dev)
        with torch.cuda.stream(D.tstream):
            if self.keep:                          # tensors of the caller's stream: ordered before the launch, alive until after
                ready = torch.cuda.Event()
                ready.record(caller)
                D.tstream.wait_event(ready)
                for t in self.keep:
                    t.record_stream(D.tstream)
            base = {}
            for compact, arena in self.arenas.items():
                if arena.used:
                    staged = arena.buf[:arena.used].to(D.dev, non_blocking=True)
                    arena.busy = torch.cuda.Event()
                    arena.busy.record(D.tstream)
                    base[compact] = (staged, staged.data_ptr(), 8 if compact else 32)
                    arena.used = 0
        segs = np.zeros(len(self.queue), dtype=PLACE_SEGMENT)
        for i, (index, row, stride, count, form, source) in enumerate(self.queue):
            if isinstance(source, tuple):
                _, ptr, width = base[source[0]]
                src = ptr + source[1] * width
            else:
                src = source.data_ptr()
            segs[i] = (self.columns[index].data_ptr(), src, row, stride, count, form, 0)
        nbytes = D.L.h2_cells_place_scratch_bytes(len(segs))
        scratch = D.scratch(nbytes)
        if self.timed:                             # tools/synthesis_bench.py: the launch (with its segment table's copy) by events
            begin, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            begin.record(D.tstream)
        check(D.L.h2_dev_cells_place(segs.ctypes.data, len(segs), self.n, self.out_form, scratch.data_ptr(), nbytes,
                                     D.stream), "h2_dev_cells_place")
        if self.timed:
            end.record(D.tstream)
            end.synchronize()
            self.kernel_ms += begin.elapsed_time(end)
        self.cells_placed += int(segs["count"].sum())
        self.flushes += 1
        for staged, _, _ in base.values():
            staged.record_stream(D.tstream)
        self.queue, self.boxes, self.keep = [], {}, []

    def finish(self):
        self.flush()
        if self.arenas is not None:
            self.pack_seconds = sum(arena.pack_seconds for arena in self.arenas.values())
            self.D.__dict__.setdefault("_place_arenas", []).append(self.arenas)
            self.arenas = None
        return self.columns


# -- selector activations: one bit per row, two assemblies ------------------------------------------------------------------
def selector_plan_tables(combinations, destinations, montgomery):
    """the h2_selector_column / h2_selector_member tables of `combinations` (ConstraintSystem.compress_selectors: the member
    selectors of each new column, in root order) written to the columns at the addresses `destinations`: member i takes the
    value i + 1, canonical or as a Montgomery residue"""
    plan = np.zeros(len(combinations), dtype=SELECTOR_COLUMN)
    members = np.zeros(sum(len(c) for c in combinations), dtype=SELECTOR_MEMBER)
    at = 0
    for c, (group, dst) in enumerate(zip(combinations, destinations)):
        plan[c] = (dst, at, len(group))
        for root, selector in enumerate(group, start=1):
            members[at] = (_limbs((root << 256) % R_MOD if montgomery else root), selector, 0)
            at += 1
    return plan, members


class HostSelectors:
    """numpy boolean activations, (num_selectors, n)"""

    def __init__(self, count, n):
        self.count, self.n = count, n
        self.bits = np.zeros((count, n), dtype=bool)

    def enable(self, index, row, stride, count):
        if count:
            self.bits[index, row:row + (count - 1) * stride + 1:stride] = True

    def conflicts(self):
        """the exclusion matrix of compress_selectors.rs:102-127, whole: 1 where two different selectors share a row"""
        packed = np.packbits(self.bits, axis=1)
        matrix = np.zeros((self.count, self.count), dtype=np.uint8)
        for i in range(self.count):
            for j in range(i):
                matrix[i, j] = matrix[j, i] = np.bitwise_and(packed[i], packed[j]).any()
        return matrix

    def bitmaps(self):
        """the activations as h2_dev_selectors_mark leaves them: (num_selectors, ceil(n / 32)) u32 words"""
        words = (self.n + 31) // 32
        padded = np.zeros((self.count, words * 32), dtype=bool)
        padded[:, :self.n] = self.bits
        return np.ascontiguousarray(np.packbits(padded, axis=1, bitorder="little")).view("<u4").reshape(self.count, words)

    def combine(self, combinations):
        """-> one canonical (n, 4) u64 column per combination: i + 1 on the rows of member i"""
        columns = []
        for group in combinations:
            column = np.zeros((self.n, 4), dtype=np.uint64)
            for root, selector in enumerate(group, start=1):
                column[self.bits[selector], 0] = root
            columns.append(column)
        return columns


class DeviceSelectors:
    """(num_selectors, ceil(n / 32)) u32 bitmaps on the device.  `enable` queues a segment; the queue is flushed by ONE launch of
    h2_dev_selectors_mark.  The conflict matrix (num_selectors^2 bytes: all the host sees of the activations) and the
    combination columns -- canonical, or Montgomery with `montgomery`, as DeviceColumns writes the other fixed columns -- are
    computed where the bits are (csrc/selectors.hip)."""

    def __init__(self, device, count, n, montgomery=False):
        self.D, self.count, self.n = device, count, n
        self.montgomery, self.out_form = montgomery, PLACE_OUT_MONTGOMERY if montgomery else PLACE_OUT_CANONICAL
        self.words = (n + 31) // 32
        torch = device.torch
        with torch.cuda.stream(device.tstream):
            self.bitmaps = torch.zeros(count * self.words, dtype=torch.int32, device=device.dev)
        self.queue, self.rows_marked, self.flushes = [], 0, 0

    def enable(self, index, row, stride, count):
        if count:
            self.queue.append((index, 0, row, stride if count > 1 else 1, count))     # one row: any stride is stride 1

    def flush(self):
        if not self.queue:
            return
        D = self.D
        segs = np.array(self.queue, dtype=SELECTOR_SEGMENT)
        nbytes = D.L.h2_selectors_mark_scratch_bytes(len(segs))
        scratch = D.scratch(nbytes)
        check(D.L.h2_dev_selectors_mark(segs.ctypes.data, len(segs), self.n, self.count, self.bitmaps.data_ptr(),
                                        scratch.data_ptr(), nbytes, D.stream), "h2_dev_selectors_mark")
        self.rows_marked += int(segs["count"].sum())
        self.flushes += 1
        self.queue = []

    def conflicts(self):
        self.flush()
        D, torch = self.D, self.D.torch
        with torch.cuda.stream(D.tstream):
            matrix = torch.empty(self.count * self.count, dtype=torch.uint8, device=D.dev)
        check(D.L.h2_dev_selectors_conflicts(self.bitmaps.data_ptr(), self.count, self.n, matrix.data_ptr(), D.stream),
              "h2_dev_selectors_conflicts")
        with torch.cuda.stream(D.tstream):
            return matrix.cpu().numpy().reshape(self.count, self.count)

    def combine(self, combinations):
        self.flush()
        D = self.D
        columns = [D.empty(self.n) for _ in combinations]           # every row is written
        plan, members = selector_plan_tables(combinations, [c.data_ptr() for c in columns], self.montgomery)
        check(D.L.h2_dev_selectors_combine(plan.ctypes.data, len(plan), members.ctypes.data, len(members), self.n, self.count,
                                           self.bitmaps.data_ptr(), self.out_form, D.stream), "h2_dev_selectors_combine")
        return columns


# -- which cells each region assigned: MockProver's CellNotAssigned, two assemblies ---------------------------------------------
class _Coverage:
    """The regions of one assignment pass: their names and planner starts, the cells they assigned and the selector rows
    they enabled, both as queued (first_row, stride, count) segments, and -- once the pass has ended and every extent is known
    -- the tables of include/halo2_hip.h over them ("Checking assignments").  `check(cap)` of the two
    subclasses gives (records, total): the (H2_CHECK_CELL, gate << 16 | query, region, cell_row) rows of the failures, at most
    `cap` of them, and their exact number."""

    def __init__(self, cs, n):
        self.n = n
        self.gates = gate_cells(cs)                   # (name, S(g), Q(g)) per gate
        if len(self.gates) >= 1 << 16 or any(len(cells) >= 1 << 16 for _, _, cells in self.gates):
            raise ValueError("check_assignments takes fewer than 2^16 gates of fewer than 2^16 queried cells each")
        if any(abs(rotation) >= n for _, _, cells in self.gates for _, rotation in cells):
            raise ValueError("a gate queries a rotation of n rows or more")
        self.gates_of = {}
        for g, (_, selectors, _) in enumerate(self.gates):
            for s in selectors:
                self.gates_of.setdefault(s, []).append(g)
        self.regions, self.segments, self.enables = [], [], []      # (name, planner start); (region, column, row, stride, count) x 2
        self.starts = self.tables = None

    def enter_region(self, name, start):
        self.regions.append((name, start))
        return len(self.regions) - 1

    def assign(self, region, column, row, stride, count):
        if count:
            self.segments.append((region, column, row, stride if count > 1 else 1, count))

    def enable(self, region, selector, row, stride, count):
        if count:
            self.enables.append((region, selector, row, stride if count > 1 else 1, count))

    def build(self):
        """-> (planes, segments, queries, uses, earlier, words): the tables of the pass, built once; fills `starts`"""
        if self.tables is not None:
            return self.tables
        extents = {}                                  # (region, column) -> [first row, last row]: a plane, in order of appearance
        for region, column, row, stride, count in self.segments:
            last = row + (count - 1) * stride
            box = extents.setdefault((region, column), [row, last])
            box[0], box[1] = min(box[0], row), max(box[1], last)
        plane_of, planes, words = {}, np.zeros(len(extents), dtype=COVERAGE_PLANE), 0
        self.starts = [start for _, start in self.regions]
        lowest = {}
        for i, ((region, column), (lo, hi)) in enumerate(extents.items()):
            plane_of[(region, column)] = i
            planes[i] = (words, lo, hi - lo + 1)
            words += (hi - lo + 1 + 31) // 32
            lowest[region] = min(lowest.get(region, lo), lo)
        for region, lo in lowest.items():            # dev.rs:286-330: a region starts at its smallest assigned row
            self.starts[region] = lo
        if words > COVERAGE_MAX_WORDS:
            raise ValueError("the regions' extents add up to %d cells: more than the 2^35 bits (4 GiB) of one coverage bit array"
                             % (32 * words))
        segments = np.zeros(len(self.segments), dtype=COVERAGE_SEGMENT)
        if self.segments:
            segments["plane"] = [plane_of[(region, column)] for region, column, _, _, _ in self.segments]
            segments["first_row"], segments["stride"], segments["count"] = np.array(
                [seg[2:] for seg in self.segments], dtype=np.uint64).T
        queries, query_at, uses, earlier, seen = [], {}, [], [], {}
        for region, selector, row, stride, count in self.enables:
            for g in self.gates_of.get(selector, ()):
                key, cells = (region, g), self.gates[g][2]
                if key not in query_at:
                    query_at[key] = len(queries)
                    queries.extend((plane_of.get((region, column), COVERAGE_NO_PLANE), _COLUMN_ORDER[column[0]] << 28 | column[1],
                                    rotation, 0) for column, rotation in cells)
                # the uses of this region and gate so far that may hold one of these rows: the kernel skips what they hold
                singles, spans = seen.setdefault(key, ({}, []))
                first_earlier, last = len(earlier), row + (count - 1) * stride
                if count == 1:
                    if row in singles:
                        earlier.append(singles[row])
                else:
                    earlier.extend(u for r, u in singles.items() if row <= r <= last and (r - row) % stride == 0)
                earlier.extend(u for other, u in spans if DeviceColumns._may_overlap((row, stride, count), other))
                if count == 1:
                    singles.setdefault(row, len(uses))
                else:
                    spans.append(((row, stride, count), len(uses)))
                uses.append((region, g, query_at[key], len(cells), first_earlier, len(earlier) - first_earlier, row, stride, count))
        self.tables = (planes, segments, np.array(queries, dtype=COVERAGE_QUERY).reshape(-1),
                       np.array(uses, dtype=COVERAGE_USE).reshape(-1), np.array(earlier, dtype=np.uint32), max(words, 1))
        self.cells_marked = int(segments["count"].sum())
        self.rows_enabled = int(self.tables[3]["count"].sum())
        return self.tables

    def start(self, region):
        """the row `offset`s of region `region` count from: its smallest assigned row; the planner's start if it assigned none"""
        self.build()
        return self.starts[region]


def _sorted_cell_records(records):
    """(m, 4) u32 records of kind H2_CHECK_CELL by (region, gate, query, row)"""
    return records[np.lexsort((records[:, 3], records[:, 1], records[:, 2]))] if len(records) else records


class HostCoverage(_Coverage):
    """numpy over the same tables: one boolean per bit of the planes, the uses' rows as index arrays.  The host path of
    check_assignments (`device` may be None) and the twin the device's result is tested against; failures come out sorted."""

    def mark(self):
        planes, segments, _, _, _, words = self.build()
        bits = np.zeros(32 * words, dtype=bool)
        for plane, _, row, stride, count in segments.tolist():
            at = 32 * int(planes[plane]["first_word"]) + row - int(planes[plane]["row_lo"])
            bits[at:at + (count - 1) * stride + 1:stride] = True
        return bits

    def bitmap(self):
        """the marked bits as h2_dev_coverage_mark leaves them: u32 words"""
        return np.ascontiguousarray(np.packbits(self.mark(), bitorder="little")).view("<u4")

    def check(self, cap=None):
        planes, _, queries, uses, _, _ = self.build()
        bits, found = self.mark(), []
        for region, gate, first_query, num_queries, _, _, row, stride, count in uses.tolist():
            rows = row + stride * np.arange(count, dtype=np.int64)
            for q in range(num_queries):
                plane, _, rotation, _ = queries[first_query + q].tolist()
                cell = (rows + self.n + rotation) % self.n
                ok = np.zeros(count, dtype=bool)
                if plane != COVERAGE_NO_PLANE:
                    first_word, lo, height = planes[plane].tolist()
                    inside = (cell >= lo) & (cell < lo + height)
                    ok[inside] = bits[32 * first_word + cell[inside] - lo]
                bad = cell[~ok]
                if len(bad):
                    found.append(np.stack([np.full(len(bad), CHECK_CELL), np.full(len(bad), gate << 16 | q),
                                           np.full(len(bad), region), bad], axis=1))
        records = np.unique(np.concatenate(found), axis=0).astype(np.uint32) if found else np.zeros((0, 4), dtype=np.uint32)
        records = _sorted_cell_records(records)
        return (records if cap is None else records[:cap]), len(records)


class DeviceCoverage(_Coverage):
    """The bit array on the device: ONE launch of h2_dev_coverage_mark for every queued assignment, ONE launch of
    h2_dev_coverage_check for every enabled row of every gate (csrc/coverage.hip); the failure block comes back in one
    download.  `timings` (a dict) receives the seconds of mark, check and download, synchronising between them."""

    def __init__(self, device, cs, n):
        _Coverage.__init__(self, cs, n)
        self.D, self.bits, self.mark_launches, self.check_launches = device, None, 0, 0

    def mark(self):
        if self.bits is not None:
            return self.bits
        D, torch = self.D, self.D.torch
        planes, segments, _, _, _, words = self.build()
        with torch.cuda.stream(D.tstream):
            self.bits = torch.zeros(words, dtype=torch.int32, device=D.dev)
        if len(segments):
            nbytes = D.L.h2_coverage_scratch_bytes(len(segments), 0, 0, 0, 0)
            scratch = D.scratch(nbytes)
            check(D.L.h2_dev_coverage_mark(planes.ctypes.data, len(planes), segments.ctypes.data, len(segments), self.bits.data_ptr(),
                                           words, scratch.data_ptr(), nbytes, D.stream), "h2_dev_coverage_mark")
            self.mark_launches += 1
        return self.bits

    def bitmap(self):
        with self.D.torch.cuda.stream(self.D.tstream):
            return self.mark().cpu().numpy().view("<u4")

    def check(self, cap=1024, timings=None):
        D, torch = self.D, self.D.torch
        planes, _, queries, uses, earlier, words = self.build()
        begin = time.perf_counter()

        def phase(name):
            nonlocal begin
            if timings is not None:
                D.sync()
                timings[name] = timings.get(name, 0.0) + time.perf_counter() - begin
                begin = time.perf_counter()

        bits = self.mark()
        phase("mark")
        with torch.cuda.stream(D.tstream):            # [u64 count, pad][cap x 16 B], as check_witness's block
            blob = torch.zeros(4 * (cap + 1), dtype=torch.int32, device=D.dev)
        if len(uses):
            nbytes = D.L.h2_coverage_scratch_bytes(0, len(planes), len(queries), len(uses), len(earlier))
            scratch = D.scratch(nbytes)
            check(D.L.h2_dev_coverage_check(planes.ctypes.data, len(planes), queries.ctypes.data, len(queries), uses.ctypes.data,
                                            len(uses), earlier.ctypes.data, len(earlier), self.n, bits.data_ptr(), words,
                                            scratch.data_ptr(), nbytes, blob.data_ptr(), blob.data_ptr() + 16, cap, D.stream),
                  "h2_dev_coverage_check")
            self.check_launches += 1
        phase("check")
        with torch.cuda.stream(D.tstream):
            host = blob.cpu().numpy().view(np.uint32)
        phase("download")
        total = int(np.ascontiguousarray(host[:2]).view(np.uint64)[0])
        return _sorted_cell_records(host[4:4 + 4 * cap].reshape(-1, 4)[:min(total, cap)]), total


# -- the constraint-system side of an assignment pass -------------------------------------------------------------------------
class _Assembly:
    """What the layouters assign into (the reference's `Assignment`): keygen keeps fixed cells, copies and constants and drops
    advice values (keygen.rs:100-215); the witness pass keeps advice and drops the rest (prover.rs:85-162)."""

    def __init__(self, cs, k, keygen, columns, instances=None, selectors=None):
        self.cs, self.k, self.n, self.keygen, self.columns, self.instances = cs, k, 1 << k, keygen, columns, instances
        self.selectors = selectors                   # keygen: HostSelectors / DeviceSelectors of a circuit that has selectors
        self.usable = self.n - (cs.blinding_factors() + 1)
        self.copies, self.first_unassigned = [], {}
        self.positions = {column: i for i, column in enumerate(cs.perm_columns)}

    def _check(self, column, row, last):
        kind, index = column
        if index >= {"advice": self.cs.num_advice, "fixed": self.cs.num_fixed, "instance": self.cs.num_instance}[kind]:
            raise BoundsFailure("no column %s[%d]" % column)
        if row < 0 or last >= self.usable:
            raise NotEnoughRowsAvailable(self.k)

    def assign(self, column, row, stride, vals):
        if vals.count == 0:
            return
        last = row + (vals.count - 1) * stride
        self._check(column, row, last)
        if column[0] == "advice":
            self.first_unassigned[column[1]] = max(self.first_unassigned.get(column[1], 0), last + 1)
        if self.keygen != (column[0] == "fixed"):
            return
        if vals.kind == "none":
            raise SynthesisError("no value for %s[%d]" % column)
        self.columns.place(column[1], row, stride, vals)

    def enable_selector(self, selector, row, stride, count):
        """keygen.rs:122-137; the witness pass ignores selectors (prover.rs: WitnessCollection::enable_selector)"""
        if not self.keygen or count == 0:
            return
        if selector.index >= self.cs.num_selectors or self.selectors is None:
            raise BoundsFailure("no selector %d" % selector.index)
        if row < 0 or row + (count - 1) * stride >= self.usable:
            raise NotEnoughRowsAvailable(self.k)
        self.selectors.enable(selector.index, row, stride, count)

    def fill_from_row(self, column, row, value):
        if row >= self.usable:                       # keygen.rs:206
            raise NotEnoughRowsAvailable(self.k)
        if self.keygen:
            self.columns.place(column[1], row, 1, _Values(value, self.usable - row))

    def copy(self, left, lrows, right, rrows):
        if not self.keygen:
            return
        for column, rows in ((left, lrows), (right, rrows)):
            if len(rows):
                self._check(column, int(rows.min()), int(rows.max()))
        if not len(lrows):
            return
        pos = []
        for column in (left, right):
            if column not in self.positions:
                raise ColumnNotInPermutation(column)
            pos.append(np.full(len(lrows), self.positions[column], dtype=np.int64))
        self.copies.append(np.stack([pos[0], lrows, pos[1], rrows], axis=1))

    def query_instance(self, column, row):
        if row >= self.usable:
            raise NotEnoughRowsAvailable(self.k)
        if self.keygen or self.instances is None:
            return None
        vals = self.instances[column[1]]
        return int(vals[row]) % R_MOD if row < len(vals) else 0

    def copies_array(self):
        return np.concatenate(self.copies) if self.copies else np.zeros((0, 4), dtype=np.int64)


class _CoverageAssembly(_Assembly):
    """The assembly of check_assignments: it places no values and records, per region, which cells are assigned and which
    selector rows enabled (dev.rs:600-760).  Towards missing values it is keygen -- advice cells need none, fixed cells do --
    and it keeps keygen's NotEnoughRowsAvailable and BoundsFailure checks.  What happens outside every region (a table's
    fill_from_row, the planners' constants) belongs to none (dev.rs:691, :729: current_region is None)."""

    def __init__(self, cs, k, coverage):
        _Assembly.__init__(self, cs, k, True, None)
        self.coverage, self.region = coverage, None

    def enter_region(self, name, start):
        self.region = self.coverage.enter_region(name, start)

    def exit_region(self):
        self.region = None

    def assign(self, column, row, stride, vals):
        if vals.count == 0:
            return
        self._check(column, row, row + (vals.count - 1) * stride)
        if column[0] == "fixed" and vals.kind == "none":
            raise SynthesisError("no value for %s[%d]" % column)
        if self.region is not None:
            self.coverage.assign(self.region, column, row, stride, vals.count)

    def enable_selector(self, selector, row, stride, count):
        if count == 0:
            return
        if selector.index >= self.cs.num_selectors:
            raise BoundsFailure("no selector %d" % selector.index)
        if row < 0 or row + (count - 1) * stride >= self.usable:
            raise NotEnoughRowsAvailable(self.k)
        self.coverage.enable(self.region, selector.index, row, stride, count)

    def fill_from_row(self, column, row, value):
        if row >= self.usable:
            raise NotEnoughRowsAvailable(self.k)

    def copy(self, left, lrows, right, rrows):
        for column, rows in ((left, lrows), (right, rrows)):
            if len(rows):
                self._check(column, int(rows.min()), int(rows.max()))
            if len(lrows) and column not in self.positions:
                raise ColumnNotInPermutation(column)


# -- what a circuit's `synthesize` sees ---------------------------------------------------------------------------------------
class Circuit:
    """plonk/circuit.rs:476-500.  `planner` is the reference's associated type FloorPlanner."""
    planner = None

    def configure(self, cs):
        raise NotImplementedError

    def synthesize(self, config, layouter):
        raise NotImplementedError

    def without_witnesses(self):
        raise NotImplementedError


class Region:
    """One region of an assignment pass.  Offsets are relative to the region's start (absolute rows under FlatFloorPlanner)."""

    def __init__(self, assembly, start, constants, shape=None):
        self._asm, self._start, self._constants, self._shape = assembly, start, constants, shape

    def _assign(self, kind, column, offset, values, stride, count):
        if column[0] != kind:
            raise TypeError("%s is not a %s column" % (column, kind))
        if stride < 1 or offset < 0:
            raise ValueError("offset >= 0 and stride >= 1")
        vals = _Values(values, count)
        if self._shape is not None:                  # V1's measurement pass (v1.rs:240-300): columns and height only
            self._shape.columns.add(column)
            if vals.count:
                self._shape.row_count = max(self._shape.row_count, offset + (vals.count - 1) * stride + 1)
        else:
            self._asm.assign(column, self._start + offset, stride, vals)
        return AssignedCells(column, self._start + offset, vals.count, stride, values if isinstance(values, Value) else None)

    def assign_advice(self, column, offset, values, stride=1, count=None):
        """`values` to the cells offset, offset + stride, ... of an advice column; an integer with `count`: that value in
        `count` cells; None (keygen): `count` cells without a value"""
        return self._assign("advice", column, offset, values, stride, count)

    def assign_fixed(self, column, offset, values, stride=1, count=None):
        return self._assign("fixed", column, offset, values, stride, count)

    def enable_selector(self, selector, offset, stride=1, count=1):
        """enables `selector` on the rows offset, offset + stride, ... (`count` of them) of the region"""
        if stride < 1 or offset < 0 or count < 0:
            raise ValueError("offset >= 0, stride >= 1 and count >= 0")
        if self._shape is not None:                  # v1.rs:453: a selector is a column of the region's shape
            self._shape.columns.add(("selector", selector.index))
            if count:
                self._shape.row_count = max(self._shape.row_count, offset + (count - 1) * stride + 1)
        else:
            self._asm.enable_selector(selector, self._start + offset, stride, count)

    def assign_advice_from_constant(self, column, offset, constant):
        cells = self.assign_advice(column, offset, int(constant))
        cells._value = Value.full(None, 1, int(constant))
        self.constrain_constant(cells, constant)
        return cells

    def assign_advice_from_instance(self, instance_column, row, advice_column, offset):
        """-> (cell, value): the advice cell takes the instance's value and is tied to it (flat.rs:398-416)"""
        if self._shape is not None:
            return self.assign_advice(advice_column, offset, None), None
        value = self._asm.query_instance(instance_column, row)
        if value is None and not self._asm.keygen:
            raise SynthesisError("no instance values were given")
        cell = self.assign_advice(advice_column, offset, value)
        self._asm.copy(cell.column, cell.rows(), instance_column, np.array([row], dtype=np.int64))
        return cell, value

    def constrain_constant(self, cells, constant):
        if self._shape is None and self._asm.keygen:
            self._constants.extend((int(constant) % R_MOD, cells.column, int(r)) for r in cells.rows())

    def constrain_equal(self, left, right):
        """`count` copy constraints between two ranges of equal length"""
        if len(left) != len(right):
            raise ValueError("constrain_equal: %d cells against %d" % (len(left), len(right)))
        if self._shape is None:
            self._asm.copy(left.column, left.rows(), right.column, right.rows())


class Table:
    """SimpleTableLayouter (single_pass.rs:56-110): the cells of a lookup table's columns, assigned from row 0"""

    def __init__(self, assembly, used):
        self._asm, self._used, self.columns = assembly, used, {}            # column -> [default, [(offset, count)]]

    def assign_cell(self, column, offset, values, count=None):
        if column[0] != "fixed":
            raise TypeError("%s is not a table column" % (column,))
        if column in self._used:
            raise SynthesisError("fixed[%d] already belongs to another table" % column[1])
        vals = _Values(values, count)
        if vals.count == 0:
            return
        entry = self.columns.setdefault(column, [None, []])
        if offset == 0:
            if entry[0] is not None:
                raise SynthesisError("row 0 of table column fixed[%d] assigned twice" % column[1])
            entry[0] = vals.first() if self._asm.keygen else 0
        entry[1].append((offset, vals.count))
        self._asm.assign(column, offset, 1, vals)

    def finish(self):
        """flat.rs:198-231: every column assigned from row 0 without holes and to one length; the rest takes the default"""
        lengths = set()
        for column, (default, spans) in self.columns.items():
            end = 0
            for offset, count in sorted(spans):
                if offset > end:
                    raise SynthesisError("table column fixed[%d] has unassigned rows below %d" % (column[1], offset))
                end = max(end, offset + count)
            if default is None:
                raise SynthesisError("table column fixed[%d] has no row 0" % column[1])
            lengths.add(end)
        if len(lengths) != 1:
            raise SynthesisError("the columns of a table differ in length" if lengths else "an empty table")
        first_unused = lengths.pop()
        self._used.update(self.columns)
        for column, (default, _) in self.columns.items():
            self._asm.fill_from_row(column, first_unused, default)


class _Shape:
    def __init__(self, index):
        self.index, self.columns, self.row_count = index, set(), 0


class Layouter:
    """One pass over a circuit's `synthesize`.  `starts`: the rows V1 gave the regions (None: every region starts at row 0,
    FlatFloorPlanner); `shapes`: a list that makes this V1's measurement pass."""

    def __init__(self, assembly, starts=None, shapes=None):
        self._asm, self._starts, self._shapes = assembly, starts, shapes
        self._regions, self._tables, self.constants = 0, set(), []

    def _announced(self, name, start, body):
        """`body()` between enter_region(name, start) and exit_region() of an assembly that tracks regions (the coverage
        assembly); tables are regions too (flat.rs:188, v1.rs:367)"""
        if not hasattr(self._asm, "enter_region"):
            return body()
        self._asm.enter_region(name, start)
        try:
            return body()
        finally:
            self._asm.exit_region()

    def assign_region(self, name, fn):
        index = self._regions
        self._regions += 1
        if self._shapes is not None:
            self._shapes.append(_Shape(index))
            return fn(Region(self._asm, 0, self.constants, self._shapes[-1]))
        start = 0 if self._starts is None else self._starts[index]
        return self._announced(name, start, lambda: fn(Region(self._asm, start, self.constants)))

    def assign_table(self, name, fn):
        if self._shapes is not None:                  # v1.rs:209: tables take no part in the measurement
            return

        def body():
            table = Table(self._asm, self._tables)
            fn(table)
            table.finish()

        self._announced(name, 0, body)

    def constrain_instance(self, cells, instance_column, row):
        if self._shapes is None:
            self._asm.copy(cells.column, cells.rows(), instance_column, row + np.arange(len(cells), dtype=np.int64))

    def namespace(self, name):
        return self


# -- floor planners ------------------------------------------------------------------------------------------------------------
def _column_key(column):
    return (_COLUMN_ORDER[column[0]], column[1])


def _sorted_constants(constants):
    """by the (column, row) of the advice cell (flat.rs:52-58, v1.rs:134-140); stable, as the reference's sort_by"""
    return sorted(constants, key=lambda c: (_column_key(c[1]), c[2]))


def _assign_constants(assembly, constants, positions):
    for (column, row), (value, cell_column, cell_row) in zip(positions, constants):
        assembly.assign(column, row, 1, _Values(value, None))
        assembly.copy(column, np.array([row], dtype=np.int64), cell_column, np.array([cell_row], dtype=np.int64))


class FlatFloorPlanner:
    """flat.rs: offsets are absolute rows.  Keygen: the constants go to rows 0, 1, ... of the FIRST constants column, in the
    order of their advice cells, one copy each.  Proving: fixed cells and copies are dropped by the assembly."""

    @staticmethod
    def synthesize(assembly, circuit, config):
        layouter = Layouter(assembly)
        circuit.synthesize(config, layouter)
        if assembly.keygen:
            constants = _sorted_constants(layouter.constants)
            columns = assembly.cs.constants
            if constants and not columns:
                raise NotEnoughColumnsForConstants("the circuit constrains constants and has no constants column")
            _assign_constants(assembly, constants, [(columns[0], row) for row in range(len(constants))] if constants else [])
        return layouter


def free_intervals(allocations, start, end):
    """Allocations::free_intervals (v1/strategy.rs:64-98): the unallocated intervals [a, b) that meet [start, end); b = None
    is the unbounded one.  `allocations`: {start row: length}."""
    row = start
    for s in sorted(allocations):
        if end is not None and s >= end:
            continue
        if row < s:
            yield row, s
        row = max(row, s + allocations[s])
    if end is None or row < end:
        yield row, end


def first_fit_region(column_allocations, columns, length, start, slack):
    """v1/strategy.rs:107-161"""
    if not columns:
        return start
    c, rest = columns[0], columns[1:]
    end = None if slack is None else start + length + slack
    for lo, hi in list(free_intervals(column_allocations.setdefault(c, {}), start, end)):
        s_slack = None if hi is None else (hi - lo) - length
        if s_slack is None or s_slack >= 0:
            row = first_fit_region(column_allocations, rest, length, lo, s_slack)
            if row is not None:
                column_allocations[c].setdefault(row, length)        # a BTreeSet ordered by start: an equal start is kept
                return row
    return None


def slot_in_biggest_advice_first(shapes):
    """v1/strategy.rs:198-225 -> (start row per region, {column: allocations}).  The reference sorts with
    sort_unstable_by_key and reverses, which leaves the order of equal areas open; here: a STABLE ascending sort, then the
    reverse -- among equal areas the region declared LAST is placed first."""
    area = lambda sh: sum(1 for c in sh.columns if c[0] == "advice") * sh.row_count   # noqa: E731
    order = sorted(shapes, key=area)[::-1]
    allocations, starts = {}, {}
    for sh in order:
        starts[sh.index] = first_fit_region(allocations, sorted(sh.columns, key=_column_key), sh.row_count, 0, None)
    return [starts[i] for i in range(len(shapes))], allocations


class V1:
    """v1.rs:65-161: a measurement pass over `without_witnesses()`, slot_in_biggest_advice_first, the assignment pass, then
    the constants into the free cells of the constants columns below the first unassigned row."""

    @staticmethod
    def plan(circuit, config):
        shapes = []
        circuit.without_witnesses().synthesize(config, Layouter(None, shapes=shapes))
        return slot_in_biggest_advice_first(shapes)

    @staticmethod
    def synthesize(assembly, circuit, config):
        starts, allocations = V1.plan(circuit, config)
        first_unassigned_row = max([max(s + l for s, l in a.items()) for a in allocations.values() if a] + [0])
        layouter = Layouter(assembly, starts=starts)
        circuit.synthesize(config, layouter)
        if assembly.keygen:
            positions = [(c, row) for c in assembly.cs.constants
                         for lo, hi in free_intervals(allocations.get(c, {}), 0, first_unassigned_row) for row in range(lo, hi)]
            if len(positions) < len(layouter.constants):
                raise NotEnoughColumnsForConstants("%d constants, %d free cells in the constants columns"
                                                   % (len(layouter.constants), len(positions)))
            _assign_constants(assembly, _sorted_constants(layouter.constants), positions)
        return layouter


# -- entry points ----------------------------------------------------------------------------------------------------------------
def _planner(circuit, planner):
    return planner or circuit.planner or V1


def synthesize_keygen(device, circuit, k, planner=None, resident=False, montgomery=False):
    """configure + the keygen pass of `circuit` (keygen.rs:236-300) -> (cs, fixed, copies), as `keygen` takes them.
    `planner`: the circuit's own (`Circuit.planner`), V1 when it names none.  `resident`: the fixed columns are built on
    `device` (DeviceColumns) and returned as device tensors -- canonical, or with `montgomery` as the residues
    `keygen(..., fixed_montgomery=True)` takes as they are; otherwise numpy columns (`device` may be None).  A circuit with
    selectors comes back with them compiled away: `cs` is the compressed constraint system and `fixed` ends with its
    combination columns, built from device bitmaps when `resident`."""
    cs = ConstraintSystem(type(circuit).__name__)
    config = circuit.configure(cs)
    cs.chunk_lookups()
    cs.chunk_shuffles()
    n = 1 << k
    if n < cs.minimum_rows():
        raise NotEnoughRowsAvailable(k)
    columns = DeviceColumns(device, cs.num_fixed, n, montgomery) if resident else HostColumns(cs.num_fixed, n)
    selectors = None
    if cs.num_selectors:
        selectors = DeviceSelectors(device, cs.num_selectors, n, montgomery) if resident else HostSelectors(cs.num_selectors, n)
    assembly = _Assembly(cs, k, True, columns, selectors=selectors)
    _planner(circuit, planner).synthesize(assembly, circuit.without_witnesses(), config)
    fixed = columns.finish()
    if selectors is not None:                        # keygen.rs:276-282: the selectors become fixed columns
        combinations = cs.compress_selectors(selectors.conflicts())
        fixed = list(fixed) + selectors.combine(combinations)
    return cs, fixed, assembly.copies_array()


def synthesize_witness(device, circuit, cs_or_pk, k, planner=None, resident=True, instances=None, alloc=None, stats=None):
    """the witness pass of `circuit` (prover.rs:85-204) -> (advice, first_unassigned), as create_proof_ext / check_witness
    take them: `advice` resident canonical columns (`resident`, DeviceColumns) or numpy ones (`alloc(count, n)` supplies
    them, e.g. Device.pinned_columns); first_unassigned = {advice column: 1 + its last assigned row}, the record the
    range-check completion asks for.  `cs_or_pk`: the constraint system of synthesize_keygen, or the proving key made of it.
    `instances`: the instance columns' values, for assign_advice_from_instance.  `stats`: a dict that receives the device
    assembly's counters and times (cells placed, launches, seconds spent staging values and flushing, the launches' milliseconds by
    events -- which makes every flush wait for its launch)."""
    cs = getattr(cs_or_pk, "cs", cs_or_pk)
    probe = ConstraintSystem(cs.name)
    config = circuit.configure(probe)               # configure is deterministic: the same columns as at keygen
    # a compressed `cs` has one more fixed column per combination of selectors than `configure` declares
    declared_fixed = cs.num_fixed - len(set(cs.selector_map))
    if (probe.num_advice, probe.num_fixed, probe.num_instance, probe.num_selectors) != (cs.num_advice, declared_fixed,
                                                                                      cs.num_instance, cs.num_selectors):
        raise ValueError("the circuit does not configure the constraint system it is proved under")
    n = 1 << k
    columns = DeviceColumns(device, cs.num_advice, n, timed=stats is not None) if resident else HostColumns(cs.num_advice, n, alloc)
    assembly = _Assembly(cs, k, False, columns, instances)
    _planner(circuit, planner).synthesize(assembly, circuit, config)
    advice = columns.finish()
    if stats is not None and resident:
        stats.update(cells_placed=columns.cells_placed, flushes=columns.flushes, pack_seconds=columns.pack_seconds,
                     flush_seconds=columns.flush_seconds, kernel_ms=columns.kernel_ms)
    return advice, dict(assembly.first_unassigned)


def synthesize_coverage(device, circuit, k, planner=None, resident=True):
    """configure + one assignment pass of `circuit` that keeps WHICH cells each region assigns and which selector rows it
    enables, and no value -> the coverage object: DeviceCoverage (`resident`: the bits live on `device`) or HostCoverage
    (`device` may be None), with the region table (`regions`: (name, planner start) in the order of the assign_region /
    assign_table calls; `start(r)`) and the gate table (`gates`) of the constraint system as `configure` leaves it, selectors
    uncompressed.  `check(cap)` runs the check; check.check_assignments wraps it."""
    cs = ConstraintSystem(type(circuit).__name__)
    config = circuit.configure(cs)
    n = 1 << k
    if n < cs.minimum_rows():
        raise NotEnoughRowsAvailable(k)
    coverage = DeviceCoverage(device, cs, n) if resident else HostCoverage(cs, n)
    _planner(circuit, planner).synthesize(_CoverageAssembly(cs, k, coverage), circuit, config)
    coverage.build()
    return coverage


def region_starts(circuit, planner=None):
    """the first row of every region of `circuit`, in the order `synthesize` declares them"""
    cs = ConstraintSystem("plan")
    config = circuit.configure(cs)
    if _planner(circuit, planner) is FlatFloorPlanner:
        shapes = []
        circuit.without_witnesses().synthesize(config, Layouter(None, shapes=shapes))
        return [0] * len(shapes)
    return V1.plan(circuit, config)[0]
