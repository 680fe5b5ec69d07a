"""`Value`: bulk arithmetic over the BN254 scalar field for the bodies of `synthesize` -- the reference's `Value<F>`,
`AssignedCell::value()` and `Assigned<F>` (circuit.rs, plonk/assigned.rs), for ranges of cells instead of one cell.

A Value is a lazily evaluated array of `count` field elements bound to a `Device` (or to no device: the host backend of the
CPU suite).  Operators build an expression; nothing runs until `tensor()`, `to_ints()`, `Value.materialize([...])` or an
assignment asks for the elements.  Then the compiler below turns the expression into as few launches of the fused evaluator
(csrc/values.hip, h2_dev_values_eval; DESIGN.md 3b, "Computing a witness") as its caps allow:

  common subexpressions   equal subexpressions of the Values materialised together are evaluated once (hash-consing, with
                          the operands of + and * in one order)
  evaluation order        Sethi-Ullman: the operand that needs more slots first
  slots                   assigned by last use, the lowest free slot first (slot 0 is a register in the kernel); a result
                          that only the next op reads takes no slot (the kernel's `last`)
  over the caps           the largest subexpression that fits a launch is materialised on its own and read back as a leaf
  slices                  a[i:j:s] is a view; it reaches the leaves as an offset and a stride and costs nothing
  inversions              staged by depth: every denominator of one depth is written into one buffer, inverted by ONE
                          h2_dev_batch_invert (Montgomery residues in and out, zeros stay zero) and read back as leaves --
                          k nested levels of division cost k + 1 evaluator launches and k inversions (per distinct length,
                          and per `outputs` denominators of one length)
  scans, concat, take     their operands are materialised first; their results are leaves
  argsort, sort, sort_by  the keys are materialised first (a whole leaf goes as it stands, in any form); ONE stable radix sort
                          (csrc/sort.hip, h2_dev_sort_permutation; DESIGN.md 3b, "Sorting a witness") orders up to four key
                          columns as integers in [0, r) where they live; the permutation is a compact leaf that `take`
                          gathers by without a bounds check
  integers                bits / >> / low / bit / limbs, & | ^ and lt / le / gt / ge read a cell as the integer in [0, r).
                          Inside a program a value is a field element or an integer (`_Node.vkind`); the compiler inserts
                          to_int / to_field where an operand's kind is not what the op takes, hash-consing shares them (one
                          to_int serves every limb of a value), and a to_int of a compact leaf costs no product.  Users never
                          see kinds: every Value reads back as field elements

Device work is allocated and launched under the device's compute stream, as check.py does, so that an assignment's flush
(DeviceColumns._flush) sees finished values.  `device.values_launches` / `device.values_inversions` / `device.values_sorts` count the calls.
"""
import numpy as np

from ._lib import check, lib
from .circuit import R_MOD
from .domain import _fr

FORM_CANONICAL, FORM_MONTGOMERY, FORM_COMPACT = 0, 1, 2                                  # H2_ASSIGNED_FORM_*
OP_CODES = {"add": 0, "sub": 1, "mul": 2, "sqr": 3, "neg": 4, "select": 5, "iszero": 6,  # H2_VALUES_*
            "to_int": 16, "to_field": 17, "extract": 18, "lt": 19, "and": 20, "or": 21, "xor": 22}
FIELD, INT = "field", "int"                                                              # what a value inside a program is
INT_RESULT = ("to_int", "extract", "lt", "and", "or", "xor")                             # ops that give an integer
INT_OPERANDS = ("to_field", "extract", "lt", "and", "or", "xor")                         # ops that take integers
KIND_LEAF, KIND_CONST, KIND_SLOT, KIND_LAST = 0, 1, 2, 3                                 # H2_VALUES_LEAF / CONST / SLOT / LAST
NO_SLOT = 0xFFFFFFFF                                                                     # H2_VALUES_NO_SLOT
# h2_values_leaf, h2_values_op, h2_values_output, h2_values_caps
VALUES_LEAF = np.dtype([("ptr", "<u8"), ("first", "<u8"), ("stride", "<u8"), ("len", "<u8"), ("form", "<u4"), ("reserved", "<u4")])
VALUES_OP = np.dtype([("op", "<u4"), ("dst", "<u4"), ("a", "<u4"), ("b", "<u4"), ("c", "<u4")])
VALUES_OUTPUT = np.dtype([("ptr", "<u8"), ("first", "<u8"), ("slot", "<u4"), ("form", "<u4")])
VALUES_CAPS = np.dtype([("leaves", "<u4"), ("ops", "<u4"), ("constants", "<u4"), ("outputs", "<u4"), ("slots", "<u4"),
                        ("blocks", "<u4"), ("threads", "<u4"), ("reserved", "<u4")])
SORT_CAPS = np.dtype([("tile", "<u4"), ("max_keys", "<u4"), ("status_words", "<u4"), ("reserved", "<u4")])   # h2_sort_caps
SORT_OK, SORT_OUT_OF_RANGE, SORT_STATUS_WORDS = 0, 1, 4                                  # H2_SORT_*
_MASK64 = (1 << 64) - 1
_R = (1 << 256) % R_MOD
_R_INV = pow(_R, -1, R_MOD)
_LIMITS = None


def limits():
    """h2_values_limits as a dict: the caps of one launch (leaves, ops, constants, outputs, slots) and its grid (blocks, threads)"""
    global _LIMITS
    if _LIMITS is None:
        caps = np.zeros(1, dtype=VALUES_CAPS)
        check(lib().h2_values_limits(caps.ctypes.data), "h2_values_limits")
        _LIMITS = {name: int(caps[0][name]) for name in VALUES_CAPS.names if name != "reserved"}
    return _LIMITS


def sort_limits():
    """h2_sort_limits as a dict: the rows a workgroup of a sorting pass ranks, the most key columns, the status words"""
    caps = np.zeros(1, dtype=SORT_CAPS)
    check(lib().h2_sort_limits(caps.ctypes.data), "h2_sort_limits")
    return {name: int(caps[0][name]) for name in SORT_CAPS.names if name != "reserved"}


def ints_to_limbs(values):
    return np.array([[(v >> (64 * j)) & _MASK64 for j in range(4)] for v in values], dtype=np.uint64).reshape(len(values), 4)


def limbs_to_ints(a):
    a = np.ascontiguousarray(a, dtype=np.uint64)
    return [int.from_bytes(row.tobytes(), "little") for row in a]


# -- backends ----------------------------------------------------------------------------------------------------------------
class _HostBackend:
    """numpy buffers, h2_values_eval, Python integers for inversions and scans: the test oracle's second opinion"""
    device = None

    def __init__(self):
        self.values_launches = self.values_inversions = self.values_sorts = 0

    def count(self, launches=0, inversions=0):
        self.values_launches += launches
        self.values_inversions += inversions

    def empty(self, n):
        return np.zeros((n, 4), dtype=np.uint64)

    def data(self, buf):
        if not isinstance(buf.data, np.ndarray):
            raise TypeError("a Value without a device holds numpy arrays")
        return buf.data

    def ptr(self, a):
        return a.ctypes.data

    def eval(self, *tables):
        check(lib().h2_values_eval(*tables), "h2_values_eval")

    def invert(self, a):
        """Montgomery residues, in place; zeros stay zero"""
        ints = [v * _R_INV % R_MOD for v in limbs_to_ints(a)]
        a[:] = ints_to_limbs([pow(v, -1, R_MOD) * _R % R_MOD if v else 0 for v in ints])

    def zero_rows(self, a):
        return np.flatnonzero(~a.any(axis=1))

    def scan(self, f, m, init, product):
        ints, z = [v * _R_INV % R_MOD for v in limbs_to_ints(f[:m])], [init % R_MOD]
        for v in ints:
            z.append(z[-1] * v % R_MOD if product else (z[-1] + v) % R_MOD)
        return ints_to_limbs([v * _R % R_MOD for v in z])

    def gather(self, a, indices):
        return np.ascontiguousarray(a[np.asarray(indices, dtype=np.int64)])

    def rows_at_or_above(self, a, bound):
        """the rows of canonical cells whose integer is `bound` (< 2^63) or more"""
        return np.flatnonzero(a[:, 1:].any(axis=1) | (a[:, 0] >= np.uint64(bound)))

    def low_words(self, a):
        return a[:, 0].astype(np.int64)

    def upload(self, a):
        return np.ascontiguousarray(a)

    def download(self, a):
        return a

    def sort(self, datas, forms, bits, n):
        """h2_sort_permutation -> (the permutation as compact cells, the status words)"""
        self.values_sorts += 1
        perm, status = np.zeros(n, dtype=np.uint64), np.zeros(SORT_STATUS_WORDS, dtype=np.uint32)
        datas = [np.ascontiguousarray(d) for d in datas]
        keys = np.array([d.ctypes.data for d in datas], dtype=np.uint64)
        forms, bits = np.array(forms, dtype=np.uint32), np.array(bits, dtype=np.uint32)
        check(lib().h2_sort_permutation(keys.ctypes.data, forms.ctypes.data, bits.ctypes.data, len(datas), n, perm.ctypes.data, 8,
                                        status.ctypes.data), "h2_sort_permutation")
        return perm, [int(w) for w in status]

    def publish(self):
        pass


HOST = _HostBackend()


class _DeviceBackend:
    def __init__(self, device):
        self.device = self.D = device
        device.__dict__.setdefault("values_launches", 0)
        device.__dict__.setdefault("values_inversions", 0)
        device.__dict__.setdefault("values_sorts", 0)

    def count(self, launches=0, inversions=0):
        self.D.values_launches += launches
        self.D.values_inversions += inversions

    def empty(self, n):
        return self.D.empty(n)

    def data(self, buf):
        D, torch = self.D, self.D.torch
        if isinstance(buf.data, np.ndarray):                 # a host array crosses PCIe once, compact cells at 8 bytes
            buf.data, buf.ordered = D.upload(np.ascontiguousarray(buf.data), widen=False), True
        elif not buf.ordered:                                # a tensor of the caller's stream: ordered before our launches
            ready = torch.cuda.Event()
            ready.record(torch.cuda.current_stream(D.dev))
            D.tstream.wait_event(ready)
            buf.data.record_stream(D.tstream)
            buf.ordered = True
        return buf.data

    def ptr(self, t):
        return t.data_ptr()

    def eval(self, *tables):
        check(self.D.L.h2_dev_values_eval(*(tables + (self.D.stream,))), "h2_dev_values_eval")

    def invert(self, t):
        n = t.shape[0]
        check(self.D.L.h2_dev_batch_invert(t.data_ptr(), self.D.empty(n).data_ptr(), n, self.D.stream), "h2_dev_batch_invert")

    def zero_rows(self, t):
        with self.D.torch.cuda.stream(self.D.tstream):
            return (t == 0).all(dim=1).nonzero().flatten().cpu().numpy()

    def scan(self, f, m, init, product):
        z = self.D.empty(m + 1)
        kernel = self.D.L.h2_dev_prefix_product if product else self.D.L.h2_dev_prefix_sum
        check(kernel(f.data_ptr() if m else None, m + 1, _fr(init), z.data_ptr(), self.D.stream), "h2_dev_prefix_scan")
        return z

    def gather(self, t, indices):
        torch = self.D.torch
        with torch.cuda.stream(self.D.tstream):
            if not torch.is_tensor(indices):
                indices = torch.from_numpy(np.ascontiguousarray(indices, dtype=np.int64)).to(self.D.dev)
            return t[indices.to(torch.int64)].contiguous()

    def rows_at_or_above(self, t, bound):
        with self.D.torch.cuda.stream(self.D.tstream):               # 64-bit words are signed here: negative is 2^63 or more
            return ((t[:, 1:] != 0).any(dim=1) | (t[:, 0] < 0) | (t[:, 0] >= bound)).nonzero().flatten().cpu().numpy()

    def low_words(self, t):
        return t[:, 0]

    def upload(self, a):
        return self.D.upload(np.ascontiguousarray(a), widen=False)

    def download(self, t):
        return self.D.download(t)

    def sort(self, datas, forms, bits, n):
        """h2_dev_sort_permutation on the compute stream, its scratch from Device.scratch (one sort at a time: the stream
        orders them) -> (the permutation as compact cells, the status words).  The 16 bytes of status are the only thing that
        comes back, but reading them waits for the compute stream: every sort inside a `synthesize` body is a host
        synchronisation, as the bounds check of a `take` by a Value is"""
        D, torch = self.D, self.D.torch
        D.values_sorts += 1
        need = D.L.h2_sort_scratch_bytes(n, len(datas))
        scratch = D.scratch(need)
        with torch.cuda.stream(D.tstream):
            perm = torch.empty(n, dtype=torch.int64, device=D.dev)
            status = torch.empty(SORT_STATUS_WORDS, dtype=torch.int32, device=D.dev)
        keys = np.array([d.data_ptr() for d in datas], dtype=np.uint64)
        forms, bits = np.array(forms, dtype=np.uint32), np.array(bits, dtype=np.uint32)
        check(D.L.h2_dev_sort_permutation(keys.ctypes.data, forms.ctypes.data, bits.ctypes.data, len(datas), n, perm.data_ptr(), 8,
                                          status.data_ptr(), scratch.data_ptr(), need, D.stream), "h2_dev_sort_permutation")
        with torch.cuda.stream(D.tstream):
            words = status.cpu().numpy().view(np.uint32)
        return perm, [int(w) for w in words]

    def publish(self):
        """what was launched on the compute stream is ordered before whatever the caller's stream does next"""
        torch = self.D.torch
        caller = torch.cuda.current_stream(self.D.dev)
        if caller != self.D.tstream:
            done = torch.cuda.Event()
            done.record(self.D.tstream)
            caller.wait_event(done)


def _backend(device):
    if device is None:
        return HOST
    be = device.__dict__.get("_values_backend")
    if be is None:
        be = device.__dict__["_values_backend"] = _DeviceBackend(device)
    return be


# -- expressions -------------------------------------------------------------------------------------------------------------
class _Buffer:
    """`length` field elements a leaf reads: a host array, a device tensor, or (data None) the result of `pending`"""
    __slots__ = ("data", "form", "length", "pending", "ordered", "rows")

    def __init__(self, data, form, length, pending=None, ordered=False):
        self.data, self.form, self.length, self.pending, self.ordered = data, form, length, pending, ordered
        self.rows = None    # an argsort's result: a permutation of this many rows -- a take of that many needs no bounds check


class _Pending:
    """what an unresolved buffer waits for: kind = inv | cumprod | cumsum | concat | take | limbs | argsort"""
    __slots__ = ("kind", "args", "extra")

    def __init__(self, kind, args, extra=None):
        self.kind, self.args, self.extra = kind, args, extra


class _Node:
    """kind = leaf (buffer) | const (value) | an op of OP_CODES (args: Values; extract: value = (lo, n)); `count` elements
    before any view; vkind: the result is a field element or an integer inside a program"""
    __slots__ = ("kind", "args", "count", "buffer", "value", "cache", "vkind")

    def __init__(self, kind, count, args=(), buffer=None, value=None):
        self.kind, self.count, self.args, self.buffer, self.value, self.cache = kind, count, args, buffer, value, None
        if kind == "select":
            self.vkind = INT if args[1]._node.vkind == args[2]._node.vkind == INT else FIELD
        else:
            self.vkind = INT if kind in INT_RESULT else FIELD


class Value:
    """`count` field elements, lazily evaluated; see the module's docstring"""
    __slots__ = ("device", "count", "_node", "_first", "_step", "_cache")

    def __init__(self, device, count, node, first=0, step=1):
        self.device, self.count, self._node, self._first, self._step, self._cache = device, count, node, first, step, {}

    # -- constructors ------------------------------------------------------------------------------------------------------
    @staticmethod
    def _leaf(device, data, form, length):
        return Value(device, length, _Node("leaf", length, buffer=_Buffer(data, form, length)))

    @staticmethod
    def from_u64(device, values):
        """compact cells: a 1-D u64 array (or anything numpy makes one of), or a 1-D 64-bit device tensor"""
        if hasattr(values, "data_ptr"):
            if values.dim() != 1 or values.element_size() != 8:
                raise TypeError("compact cells are a 1-D 64-bit tensor")
            return Value._leaf(device, values.contiguous(), FORM_COMPACT, values.shape[0])
        values = np.ascontiguousarray(values, dtype=np.uint64)
        if values.ndim != 1:
            raise TypeError("compact cells are a 1-D u64 array")
        return Value._leaf(device, values, FORM_COMPACT, len(values))

    @staticmethod
    def from_limbs(device, values, montgomery=False):
        """(m, 4) u64 cells: canonical (any 256-bit integer; reduced on load) or reduced Montgomery residues"""
        form = FORM_MONTGOMERY if montgomery else FORM_CANONICAL
        if hasattr(values, "data_ptr"):
            if values.dim() != 2 or values.shape[1] != 4 or values.element_size() != 8:
                raise TypeError("cells are an (m, 4) 64-bit tensor")
            return Value._leaf(device, values.contiguous(), form, values.shape[0])
        values = np.ascontiguousarray(values, dtype=np.uint64)
        if values.ndim != 2 or values.shape[1] != 4:
            raise TypeError("cells are an (m, 4) u64 array")
        return Value._leaf(device, values, form, len(values))

    @staticmethod
    def from_ints(device, values):
        return Value.from_limbs(device, ints_to_limbs([int(v) % R_MOD for v in values]))

    @staticmethod
    def full(device, count, value):
        return Value(device, count, _Node("const", count, value=int(value) % R_MOD))

    @staticmethod
    def unknown(count):
        return Value(None, count, None)

    @property
    def known(self):
        return self._node is not None

    def __len__(self):
        return self.count

    def __repr__(self):
        return "Value(%s, %d)" % (self._node.kind if self.known else "unknown", self.count)

    # -- views ---------------------------------------------------------------------------------------------------------------
    def __getitem__(self, key):
        if isinstance(key, slice):
            start, stop, step = key.indices(self.count)
            if step < 1:
                raise ValueError("values are sliced forwards")
            count = len(range(start, stop, step))
        else:
            if not -self.count <= key < self.count:
                raise IndexError(key)
            start, step, count = key % self.count, 1, 1
        if not self.known:
            return Value.unknown(count)
        return Value(self.device, count, self._node, self._first + start * self._step, self._step * step)

    # -- elementwise ---------------------------------------------------------------------------------------------------------
    def _lift(self, other):
        if isinstance(other, Value):
            return other
        if isinstance(other, (int, np.integer)):
            return Value.full(self.device, self.count, int(other))
        return None

    @staticmethod
    def _op(kind, *args, value=None):
        count = args[0].count
        for other in args[1:]:
            if other.count != count:
                raise ValueError("values of %d and %d elements do not combine" % (count, other.count))
        if not all(a.known for a in args):
            return Value.unknown(count)
        device = None
        for a in args:
            if a.device is not None:
                if device is not None and a.device is not device:
                    raise ValueError("values of two devices do not combine")
                device = a.device
        if device is not None and any(a.device is None and a._node.kind != "const" for a in args):
            raise ValueError("a host value and a device value do not combine")
        return Value(device, count, _Node(kind, count, args, value=value))

    def _binary(self, kind, other, swap=False):
        other = self._lift(other)
        if other is None:
            return NotImplemented
        return Value._op(kind, other, self) if swap else Value._op(kind, self, other)

    def __add__(self, other):
        return self._binary("add", other)

    __radd__ = __add__

    def __sub__(self, other):
        return self._binary("sub", other)

    def __rsub__(self, other):
        return self._binary("sub", other, swap=True)

    def __mul__(self, other):
        return self._binary("mul", other)

    __rmul__ = __mul__

    def __neg__(self):
        return Value._op("neg", self)

    def square(self):
        return Value._op("sqr", self)

    def __pow__(self, e):
        if not isinstance(e, (int, np.integer)) or e < 0:
            raise TypeError("** takes a small non-negative integer")
        if e == 0:
            return Value.full(self.device, self.count, 1) if self.known else Value.unknown(self.count)
        acc = self
        for bit in bin(int(e))[3:]:
            acc = acc.square()
            if bit == "1":
                acc = acc * self
        return acc

    def is_zero(self):
        return Value._op("iszero", self)

    @staticmethod
    def select(cond, a, b):
        """a where cond != 0, else b"""
        base = next((v for v in (cond, a, b) if isinstance(v, Value)), None)
        if base is None:
            raise TypeError("select takes at least one Value")
        return Value._op("select", *(base._lift(v) for v in (cond, a, b)))

    # -- a cell as the integer in [0, r): bit fields, limbs, bitwise operations, comparisons ----------------------------------
    def bits(self, lo, n):
        """(v >> lo) mod 2^n of the integer v in [0, r)"""
        lo, n = int(lo), int(n)
        if not (0 <= lo <= 255 and 1 <= n):
            raise ValueError("bits(lo, n): 0 <= lo <= 255 and n >= 1")
        return Value._op("extract", self, value=(lo, min(n, 256)))

    def __rshift__(self, k):
        if not isinstance(k, (int, np.integer)) or k < 0:
            raise TypeError(">> takes a non-negative integer")
        if k >= 256:
            return Value.full(self.device, self.count, 0) if self.known else Value.unknown(self.count)
        return self.bits(k, 256 - k)

    def low(self, n):
        """v mod 2^n"""
        return self.bits(0, n)

    def bit(self, i):
        return self.bits(i, 1)

    def __and__(self, other):
        return self._binary("and", other)

    __rand__ = __and__

    def __or__(self, other):
        return self._binary("or", other)

    __ror__ = __or__

    def __xor__(self, other):
        return self._binary("xor", other)

    __rxor__ = __xor__

    def lt(self, other):
        """1 where self < other as integers in [0, r), else 0"""
        return self._binary("lt", other)

    def gt(self, other):
        return self._binary("lt", other, swap=True)

    def le(self, other):
        return 1 - self.gt(other)

    def ge(self, other):
        return 1 - self.lt(other)

    def limbs(self, bits, count, strict=False):
        """`count` Values: limb j = (v >> bits * j) mod 2^bits.  Materialised together they cost ceil(count / outputs cap)
        launches and one to_int.  `strict`: a row whose value is 2^(bits * count) or more raises ValueError on
        materialisation, naming the first (the rest of v >> bits * count is one more output)"""
        bits, count = int(bits), int(count)
        if bits < 1 or count < 1 or bits * count > 256:
            raise ValueError("limbs(bits, count): 1 <= bits, 1 <= count and bits * count <= 256")
        parts = [self.bits(bits * j, bits) for j in range(count)]
        if not strict or not self.known:
            return parts
        if bits * count < 256:
            parts.append(self >> bits * count)
        group = []
        pending = _Pending("limbs", tuple(parts), (bits, count, group))
        for _ in range(count):
            group.append(_Buffer(None, FORM_CANONICAL, self.count, pending))
        return [Value(self.device, self.count, _Node("leaf", self.count, buffer=buf)) for buf in group]

    # -- inversion, scans, concat, take: results are leaves over a buffer that is filled on materialisation ------------------
    def _deferred(self, kind, count, args, extra=None, device=None):
        pending = _Pending(kind, args, extra)
        return Value(self.device if device is None else device, count,
                     _Node("leaf", count, buffer=_Buffer(None, FORM_MONTGOMERY, count, pending)))

    def invert(self, strict=False):
        """1 / x, and 0 where x = 0 (`Assigned::evaluate`, ff::BatchInvert); `strict`: a zero raises on materialisation"""
        if not self.known:
            return Value.unknown(self.count)
        return self._deferred("inv", self.count, (self,), strict)

    def __truediv__(self, other):
        other = self._lift(other)
        if other is None:
            return NotImplemented
        return Value._op("mul", self, other.invert()) if self.known and other.known else Value._op("mul", self, other)

    def __rtruediv__(self, other):
        other = self._lift(other)
        return NotImplemented if other is None else other / self

    def _scan(self, kind, init):
        if not self.known:
            return Value.unknown(self.count + 1)
        return self._deferred(kind, self.count + 1, (self,), int(init) % R_MOD)

    def cumprod(self, init=1):
        """count + 1 elements: z[0] = init, z[i] = z[i - 1] * self[i - 1]"""
        return self._scan("cumprod", init)

    def cumsum(self, init=0):
        return self._scan("cumsum", init)

    @staticmethod
    def concat(parts):
        parts = list(parts)
        count = sum(p.count for p in parts)
        if not all(p.known for p in parts):
            return Value.unknown(count)
        device = next((p.device for p in parts if p.device is not None), None)
        return parts[0]._deferred("concat", count, tuple(parts), device=device) if parts else Value.from_ints(None, [])

    def take(self, indices):
        """self[indices]: materialises, then gathers.  `indices`: a host array, a tensor, or a Value of integers -- that one
        is materialised and checked against len(self) where it lives (IndexError names the first row out of range; the
        gather is not issued), and only the offending row ever reaches the host"""
        if isinstance(indices, Value):
            if not (self.known and indices.known):
                return Value.unknown(len(indices))
            device = self.device if self.device is not None else indices.device
            if indices.device is not None and indices.device is not device:
                raise ValueError("values of two devices do not combine")
            return self._deferred("take", len(indices), (self, indices), None, device=device)
        if not self.known:
            return Value.unknown(len(indices))
        return self._deferred("take", len(indices), (self,), indices)

    # -- ordering ------------------------------------------------------------------------------------------------------------
    # On purpose neither a staticmethod nor a method with `self`: one plain function serves both call forms.  Looked up on the
    # class, Value.argsort([a, b]) passes the list as `keys`; looked up on an instance, v.argsort(bits) binds v to `keys`.
    def argsort(keys, bits=None):  # noqa: N805
        """Value.argsort(keys, bits=None) or v.argsort(bits=None): the permutation that orders the rows by `keys` -- a Value,
        or a list of up to `sort_limits()["max_keys"]` Values, the most significant first -- each cell read as the integer in
        [0, r); equal rows keep their order.  The result is a Value of integers (compact cells): perm[i] = the row of the
        i-th smallest.  `bits` (one number, or one per key; None = no promise) promises key < 2^bits and spares the passes
        above it; a cell that breaks the promise raises ValueError on materialisation, naming key, row and value, and only
        that cell reaches the host.  Deferred like `take`: the keys are materialised first (a whole leaf is passed as it
        stands, in whatever form, with no launch -- a canonical leaf of unreduced cells is ordered by the cells as they
        stand), then ONE h2_dev_sort_permutation (csrc/sort.hip; `device.values_sorts` counts them) orders them where they
        live."""
        keys = [keys] if isinstance(keys, Value) else list(keys)
        if not keys:
            raise ValueError("argsort takes at least one key")
        count = keys[0].count
        if any(k.count != count for k in keys):
            raise ValueError("keys of different lengths do not sort together")
        if isinstance(bits, (int, np.integer)) or bits is None:
            bits = [bits] * len(keys)
        bits = [0 if b is None else int(b) for b in bits]
        if len(bits) != len(keys) or any(not 0 <= b <= 254 for b in bits):
            raise ValueError("bits: one promise of 1 .. 254 bits (None or 0: no promise) per key")
        if not all(k.known for k in keys):
            return Value.unknown(count)
        device = _common_device(keys)
        if device is not None and any(k.device is None and k._node.kind != "const" for k in keys):
            raise ValueError("a host value and a device value do not combine")
        pending = _Pending("argsort", tuple(keys), bits)
        return Value(device, count, _Node("leaf", count, buffer=_Buffer(None, FORM_COMPACT, count, pending)))

    def sort(self, bits=None):
        """the elements in ascending order of the integers in [0, r) they stand for: one argsort, one take"""
        return self.take(self.argsort(bits))

    @staticmethod
    def sort_by(keys, payloads, bits=None):
        """every payload permuted by the order of `keys` (see argsort): one argsort, one take per payload"""
        perm = Value.argsort(keys, bits)
        return [p.take(perm) for p in payloads]

    # -- materialisation -----------------------------------------------------------------------------------------------------
    @staticmethod
    def materialize(values, montgomery=False):
        """the elements of several Values at once (their common subexpressions evaluated once) -> [(count, 4) arrays]"""
        values = list(values)
        form = FORM_MONTGOMERY if montgomery else FORM_CANONICAL
        todo = [v for v in values if v._cached(form) is None]
        if todo:
            if not all(v.known for v in todo):
                raise ValueError("an unknown Value has no elements")
            be = _backend(_common_device(todo))
            _resolve_pending(todo, be)
            for v, data in zip(todo, _evaluate(todo, be, form)):
                v._store(form, data)
            be.publish()
        return [v._cached(form) for v in values]

    def _whole(self):
        return self.known and self._first == 0 and self._step == 1 and self.count == self._node.count

    def _cached(self, form):
        if form in self._cache:
            return self._cache[form]
        if self._whole() and self._node.cache and form in self._node.cache:
            return self._node.cache[form]
        return None

    def _store(self, form, data):
        self._cache[form] = data
        if self._whole():
            if self._node.cache is None:
                self._node.cache = {}
            self._node.cache[form] = data

    def tensor(self, montgomery=False):
        """the (count, 4) device tensor (a numpy array without a device), canonical or Montgomery; computed once"""
        return Value.materialize([self], montgomery)[0]

    def to_ints(self):
        data = self.tensor()
        return limbs_to_ints(_backend(self.device).download(data)) if self.count else []


def _common_device(values):
    device = None
    for v in values:
        if v.device is not None:
            if device is not None and device is not v.device:
                raise ValueError("values of two devices do not materialise together")
            device = v.device
    return device


# -- deferred buffers: inversions by depth, scans, concat, take ---------------------------------------------------------------
def _direct(values):
    """the unresolved buffers `values` read, without looking into what those wait for"""
    out, seen, stack = {}, set(), [v._node for v in values]
    while stack:
        node = stack.pop()
        if id(node) in seen:
            continue
        seen.add(id(node))
        if node.kind == "leaf":
            if node.buffer.data is None:
                out[id(node.buffer)] = node.buffer
        elif node.kind != "const" and not node.cache:
            stack.extend(a._node for a in node.args)
    return list(out.values())


def _ready(values):
    """the unresolved buffers below `values` that wait for nothing unresolved: the innermost depth"""
    ready, seen, frontier = [], set(), _direct(values)
    while frontier:
        buf = frontier.pop()
        if id(buf) in seen:
            continue
        seen.add(id(buf))
        below = _direct(buf.pending.args)
        if below:
            frontier.extend(below)
        else:
            ready.append(buf)
    return ready


def _resolve_pending(values, be):
    while True:
        ready = _ready(values)
        if not ready:
            return
        inversions = [buf for buf in ready if buf.pending.kind == "inv"]
        for buf in ready:
            if buf.pending is not None and buf.pending.kind != "inv":   # the limbs of one group resolve together
                _resolve_other(buf, be)
        if inversions:
            _resolve_inversions(inversions, be)


def _resolve_inversions(bufs, be):
    """every denominator of this depth into consecutive segments of one buffer, one batch inversion over it"""
    total = sum(buf.length for buf in bufs)
    whole, at, outs = be.empty(total), 0, []
    for buf in bufs:
        outs.append((whole, at))
        at += buf.length
    _evaluate([buf.pending.args[0] for buf in bufs], be, FORM_MONTGOMERY, outs)
    at = 0
    for buf in bufs:
        if buf.pending.extra and buf.length:                        # strict
            zeros = be.zero_rows(whole[at:at + buf.length])
            if len(zeros):
                raise ZeroDivisionError("invert(strict=True): element %d of the %d is zero" % (int(zeros[0]), buf.length))
        at += buf.length
    if total:
        be.invert(whole)
        be.count(inversions=1)
    at = 0
    for buf in bufs:
        buf.data, buf.ordered, buf.pending = whole[at:at + buf.length], True, None
        at += buf.length


def _resolve_other(buf, be):
    kind, args, extra = buf.pending.kind, buf.pending.args, buf.pending.extra
    if kind in ("cumprod", "cumsum"):
        m = args[0].count
        f = _evaluate([args[0]], be, FORM_MONTGOMERY)[0] if m else None
        data = be.scan(f, m, extra, kind == "cumprod")
    elif kind == "concat":
        data, at, outs = be.empty(buf.length), 0, []
        for part in args:
            outs.append((data, at))
            at += part.count
        _evaluate(list(args), be, FORM_MONTGOMERY, outs)
    elif kind == "limbs":
        _resolve_limbs(buf.pending, be)
        return
    elif kind == "argsort":
        data = _resolve_argsort(args, extra, be)
        buf.rows = buf.length
    else:                                                           # take
        index = args[1]._node if len(args) == 2 else None
        if index is not None and index.kind == "leaf" and args[1]._whole() and index.buffer.rows == args[0].count:
            extra = be.data(index.buffer)                           # an argsort over as many rows: in range as it stands
        elif index is not None:                                     # a Value of integers: checked where it lives
            index = _evaluate([args[1]], be, FORM_CANONICAL)[0]
            bad = be.rows_at_or_above(index, args[0].count) if args[1].count else []
            if len(bad):
                row = int(bad[0])
                value = limbs_to_ints(be.download(index[row:row + 1]))[0]
                raise IndexError("take: index %d at row %d is out of range for %d elements" % (value, row, args[0].count))
            extra = be.low_words(index)
        node = args[0]._node
        if node.kind == "leaf" and args[0]._whole():                # elements as they stand, in whatever form: no launch
            data, buf.form = be.gather(be.data(node.buffer), extra), node.buffer.form
        else:
            data = be.gather(_evaluate([args[0]], be, FORM_MONTGOMERY)[0], extra)
    buf.data, buf.ordered, buf.pending = data, True, None


def _resolve_argsort(keys, bits, be):
    """the keys as they stand where they are whole leaves, evaluated (together, canonical) where they are not; one sort"""
    n = keys[0].count
    datas, forms, rest = [None] * len(keys), [FORM_CANONICAL] * len(keys), []
    for i, v in enumerate(keys):
        node = v._node
        if node.kind == "leaf" and v._whole():
            datas[i], forms[i] = be.data(node.buffer), node.buffer.form
        else:
            rest.append(i)
    for i, data in zip(rest, _evaluate([keys[i] for i in rest], be, FORM_CANONICAL)):
        datas[i] = data
    for i, form in enumerate(forms):
        if form == FORM_COMPACT and bits[i] > 64:
            bits = bits[:i] + [64] + bits[i + 1:]
    if n == 0:
        return be.upload(np.zeros(0, dtype=np.uint64))
    perm, status = be.sort(datas, forms, bits, n)
    if status[0] != SORT_OK:
        row, key = status[1], status[2]
        cell = np.ascontiguousarray(be.download(datas[key][row:row + 1])).view(np.uint64)
        value = int(cell[0]) if forms[key] == FORM_COMPACT else limbs_to_ints(cell.reshape(1, 4))[0]
        if forms[key] == FORM_MONTGOMERY:
            value = value * _R_INV % R_MOD
        raise ValueError("argsort: key %d at row %d is %d, which is not below 2^%d" % (key, row, value, bits[key] or 254))
    return perm


def _resolve_limbs(pending, be):
    """limbs(strict=True): every limb into its own canonical buffer, and what is left above them checked to be zero"""
    bits, count, group = pending.extra
    m = group[0].length
    outs = [(be.empty(m), 0) for _ in pending.args]
    _evaluate(list(pending.args), be, FORM_CANONICAL, outs)
    if len(pending.args) > count and m:
        high = be.zero_rows(outs[count][0])
        if len(high) < m:
            zero = np.zeros(m, dtype=bool)
            zero[high] = True
            raise ValueError("limbs(strict=True): element %d of the %d does not fit %d limbs of %d bits" % (
                int(np.flatnonzero(~zero)[0]), m, count, bits))
    for buf, (data, _) in zip(group, outs):
        buf.data, buf.ordered, buf.pending = data, True, None


# -- the compiler --------------------------------------------------------------------------------------------------------------
class _Overflow(Exception):
    pass


class _Dag:
    """hash-consed expressions: the ids of ops ascend from operands to results.  An entry is ("leaf", buffer, first, stride,
    form), ("const", value) or (op, operand ids) -- ("extract", (id,), (lo, n)); kinds[id]: FIELD or INT.  Leaves and
    constants are field values; an operand of another kind than its op takes goes through a to_int / to_field, interned
    like everything else, so every reader of one value shares one conversion"""

    def __init__(self):
        self.entries, self.kinds, self.index, self.memo = [], [], {}, {}

    def _intern(self, key, entry):
        at = self.index.get(key)
        if at is None:
            at = self.index[key] = len(self.entries)
            self.entries.append(entry)
            if entry[0] == "select":
                self.kinds.append(self.kinds[entry[1][1]])
            else:
                self.kinds.append(INT if entry[0] in INT_RESULT else FIELD)
        return at

    def op(self, kind, ids, params=None):
        """the id of op `kind` over `ids`, conversions inserted"""
        if kind == "select":
            arms = INT if self.kinds[ids[1]] == self.kinds[ids[2]] == INT else FIELD
            ids = (ids[0], self.convert(ids[1], arms), self.convert(ids[2], arms))
        elif kind != "iszero":
            want = INT if kind in INT_OPERANDS else FIELD
            ids = tuple(self.convert(at, want) for at in ids)
        if kind in ("add", "mul", "and", "or", "xor"):
            ids = tuple(sorted(ids))
        key = (kind, ids) if params is None else (kind, ids, params)
        return self._intern(key, key)

    def convert(self, at, want):
        if self.kinds[at] == want:
            return at
        entry = self.entries[at]
        if entry[0] in ("to_int", "to_field") and self.kinds[entry[1][0]] == want:     # there and back again: the value itself
            return entry[1][0]
        kind = "to_int" if want == INT else "to_field"
        return self._intern((kind, (at,)), (kind, (at,)))

    def replace_by_leaf(self, at, buffer, first, form):
        """entry `at` was materialised into `buffer`: from now on it is read, not computed.  A leaf is a field value, so an
        integer keeps its id as the to_int of a new leaf (leaves take no part in the order of ids)"""
        leaf = ("leaf", buffer, first, 1, form)
        if self.kinds[at] == INT:
            self.entries.append(leaf)
            self.kinds.append(FIELD)
            self.entries[at] = ("to_int", (len(self.entries) - 1,))
        else:
            self.entries[at] = leaf

    def leaf(self, buffer, first, stride, form):
        return self._intern(("leaf", id(buffer), first, stride, form), ("leaf", buffer, first, stride, form))

    def interior(self, at):
        return self.entries[at][0] not in ("leaf", "const")

    def add(self, value):
        """the id of `value`, its view pushed down to the leaves"""
        key_of = lambda item: (id(item[0]),) + item[1:]             # noqa: E731
        root = (value._node, value._first, value._step, value.count)
        stack = [root]
        while stack:
            item = stack[-1]
            key = key_of(item)
            if key in self.memo:
                stack.pop()
                continue
            node, first, step, count = item
            if node.kind == "leaf" or node.cache:
                if node.kind == "leaf":
                    buffer = node.buffer
                else:                                               # materialised before: read, not computed again
                    form = FORM_MONTGOMERY if FORM_MONTGOMERY in node.cache else FORM_CANONICAL
                    buffer = node.cache.get("buffer%d" % form)
                    if buffer is None:
                        buffer = node.cache["buffer%d" % form] = _Buffer(node.cache[form], form, node.count, ordered=True)
                self.memo[key] = self.leaf(buffer, first, 1 if count <= 1 else step, buffer.form)
            elif node.kind == "const":
                self.memo[key] = self._intern(("const", node.value), ("const", node.value))
            else:
                kids = [(a._node, a._first + first * a._step, step * a._step, count) for a in node.args]
                missing = [k for k in kids if key_of(k) not in self.memo]
                if missing:
                    stack.extend(missing)
                    continue
                self.memo[key] = self.op(node.kind, tuple(self.memo[key_of(k)] for k in kids), node.value)
            stack.pop()
        return self.memo[key_of(root)]

    def cone(self, roots):
        """the interior ids reachable from `roots`, ascending"""
        seen, stack = set(), [r for r in roots if self.interior(r)]
        while stack:
            at = stack.pop()
            if at in seen:
                continue
            seen.add(at)
            stack.extend(c for c in self.entries[at][1] if self.interior(c))
        return sorted(seen)


class _Program:
    """one launch: leaves [(buffer, first, stride, form)], constants [int], ops [(code, dst, a, b, c)], the roots' slots"""

    def __init__(self):
        self.leaves, self.constants, self.ops, self.slots_used, self.root_slots = [], [], [], 0, []


def _schedule(dag, roots, caps):
    """the program that computes `roots` (ids of `dag`), or _Overflow naming the cap it does not fit"""
    if len(roots) > caps["outputs"]:
        raise _Overflow("outputs")
    prog = _Program()
    cone = dag.cone(roots)
    if len(cone) > caps["ops"]:
        raise _Overflow("ops")
    # Sethi-Ullman labels, operands before results
    label = {}
    for at in cone:
        kids = sorted((label[c] for c in dag.entries[at][1] if dag.interior(c)), reverse=True)
        label[at] = max([l + i for i, l in enumerate(kids)] + [1])
    order, done = [], set()
    stack = [(r, False) for r in reversed(roots) if dag.interior(r)]
    while stack:
        at, expanded = stack.pop()
        if at in done:
            continue
        if expanded:
            done.add(at)
            order.append(at)
            continue
        stack.append((at, True))
        kids = [c for c in dict.fromkeys(dag.entries[at][1]) if dag.interior(c) and c not in done]
        for c in sorted(kids, key=lambda c: label[c]):              # popped last first: the largest label is evaluated first
            stack.append((c, False))
    uses = {}
    for at in order:
        for c in dag.entries[at][1]:
            if dag.interior(c):
                uses[c] = uses.get(c, 0) + 1
    for r in roots:
        uses[r] = uses.get(r, 0) + 1                                # an output reads the slot at the end: never freed
    leaf_index, const_index, slot_of, free = {}, {}, {}, list(range(caps["slots"]))

    def terminal(at):
        entry = dag.entries[at]
        if entry[0] == "leaf":
            if at not in leaf_index:
                if len(prog.leaves) == caps["leaves"]:
                    raise _Overflow("leaves")
                leaf_index[at] = len(prog.leaves)
                prog.leaves.append(entry[1:])
            return KIND_LEAF << 24 | leaf_index[at]
        if at not in const_index:
            if len(prog.constants) == caps["constants"]:
                raise _Overflow("constants")
            const_index[at] = len(prog.constants)
            prog.constants.append(entry[1])
        return KIND_CONST << 24 | const_index[at]

    def emit(kind, kids, transient, params=()):
        words = [(KIND_LAST << 24 if slot_of[c] is None else KIND_SLOT << 24 | slot_of[c]) if dag.interior(c) else terminal(c)
                 for c in kids] + list(params)                      # extract: lo and n ride in b and c as plain numbers
        for c in kids:
            if dag.interior(c):
                uses[c] -= 1
                if uses[c] == 0 and slot_of[c] is not None:
                    free.append(slot_of[c])
        if len(prog.ops) == caps["ops"]:
            raise _Overflow("ops")
        if transient:
            prog.ops.append((OP_CODES[kind], NO_SLOT) + tuple(words + [0] * (3 - len(words))))
            return None
        if not free:
            raise _Overflow("slots")
        dst = min(free)
        free.remove(dst)
        prog.slots_used = max(prog.slots_used, caps["slots"] - len(free))
        if len(prog.ops) == caps["ops"]:
            raise _Overflow("ops")
        prog.ops.append((OP_CODES[kind], dst) + tuple(words + [0] * (3 - len(words))))
        return dst

    for p, at in enumerate(order):
        kind, kids = dag.entries[at][:2]
        # read once, by the very next op, and no output: it lives in the kernel's `last` and takes no slot
        transient = uses[at] == 1 and at not in roots and p + 1 < len(order) and at in dag.entries[order[p + 1]][1]
        slot_of[at] = emit(kind, kids, transient, dag.entries[at][2] if kind == "extract" else ())
    zero = None
    for r in roots:
        if dag.interior(r):
            prog.root_slots.append(slot_of[r])
        else:                                                       # a bare leaf or constant: + 0 brings it into a slot
            if zero is None:
                zero = dag._intern(("const", 0), ("const", 0))
            words = [terminal(r), terminal(zero)]
            if not free:
                raise _Overflow("slots")
            dst = min(free)
            free.remove(dst)
            prog.slots_used = max(prog.slots_used, caps["slots"] - len(free))
            if len(prog.ops) == caps["ops"]:
                raise _Overflow("ops")
            prog.ops.append((OP_CODES["add"], dst, words[0], words[1], 0))
            prog.root_slots.append(dst)
    return prog


def _launch(prog, outs, form, m, be):
    """outs: [(array, first element)] per root"""
    leaves = np.zeros(len(prog.leaves), dtype=VALUES_LEAF)
    keep = []
    for i, (buffer, first, stride, lform) in enumerate(prog.leaves):
        data = be.data(buffer)
        keep.append(data)
        leaves[i] = (be.ptr(data), first, stride, buffer.length, lform, 0)
    constants = ints_to_limbs(prog.constants) if prog.constants else np.zeros((0, 4), dtype=np.uint64)
    ops = np.array(prog.ops, dtype=np.uint32).reshape(len(prog.ops), 5).view(VALUES_OP).reshape(-1) if prog.ops else np.zeros(0, dtype=VALUES_OP)
    outputs = np.zeros(len(outs), dtype=VALUES_OUTPUT)
    for i, ((data, first), slot) in enumerate(zip(outs, prog.root_slots)):
        outputs[i] = (be.ptr(data), first, slot, form)
    be.eval(leaves.ctypes.data, len(leaves), constants.ctypes.data, len(constants), ops.ctypes.data, len(ops),
            outputs.ctypes.data, len(outputs), m)
    be.count(launches=1)
    LAST_PROGRAMS.append(prog)
    if len(LAST_PROGRAMS) > 256:
        del LAST_PROGRAMS[:128]


LAST_PROGRAMS = []          # the programs launched most recently (tests and tools read the op and slot counts); kept short


def _split_candidate(dag, roots, caps):
    """the largest proper subexpression that fits a launch of its own -> (id, its program).  An integer is read back through
    a to_int (_Dag.replace_by_leaf), so giving one up shortens the program only if it is more than one op"""
    total = dag.cone(roots)
    sizes = sorted(((len(dag.cone([at])), at) for at in total), reverse=True)
    for size, at in sizes:
        if size > caps["ops"] or (size == len(total) and len(roots) == 1) or (size == 1 and dag.kinds[at] == INT):
            continue
        try:
            return at, _schedule(dag, [at], caps)
        except _Overflow:
            continue
    raise RuntimeError("no subexpression of this Value fits a launch")


def _evaluate(values, be, form, outs=None):
    """pure elementwise Values (every buffer resolved) -> their elements; `outs`: [(array, first element)] to write into
    instead of fresh arrays"""
    caps = limits()
    results = [None] * len(values)
    by_count = {}
    for i, v in enumerate(values):
        by_count.setdefault(v.count, []).append(i)
    for m, group in by_count.items():
        for lo in range(0, len(group), caps["outputs"]):
            chunk = group[lo:lo + caps["outputs"]]
            dests = []
            for i in chunk:
                v = values[i]
                if outs is not None:
                    dests.append(outs[i])
                    continue
                node = v._node
                if node.kind == "leaf" and v._whole() and node.buffer.form == form:        # the elements as they stand
                    results[i] = be.data(node.buffer)
                    dests.append(None)
                else:
                    results[i] = be.empty(m)
                    dests.append((results[i], 0))
            chunk = [i for i, d in zip(chunk, dests) if d is not None]
            dests = [d for d in dests if d is not None]
            if m == 0 or not chunk:
                continue
            dag = _Dag()
            roots = [dag.add(values[i]) for i in chunk]
            _run(dag, roots, dests, form, m, be, caps)
    return results


def _run(dag, roots, dests, form, m, be, caps):
    """launch `roots` into `dests`, splitting while the whole does not fit"""
    roots, dests = list(roots), list(dests)
    while roots:
        # two roots that are one expression share a slot; the outputs stay two
        try:
            prog = _schedule(dag, roots, caps)
        except _Overflow:
            at, sub = _split_candidate(dag, roots, caps)
            if at in roots:                                         # a root on its own: straight to where it belongs
                k = roots.index(at)
                data, first = dests[k]
                _launch(sub, [dests[k]], form, m, be)
                buffer, lfirst, lform = _Buffer(data, form, first + m, ordered=True), first, form
                del roots[k], dests[k]
            else:                                                   # in the form that costs no product either way
                data, lform = be.empty(m), FORM_CANONICAL if dag.kinds[at] == INT else FORM_MONTGOMERY
                _launch(sub, [(data, 0)], lform, m, be)
                buffer, lfirst = _Buffer(data, lform, m, ordered=True), 0
            dag.replace_by_leaf(at, buffer, lfirst, lform)
            continue
        _launch(prog, dests, form, m, be)
        return


def plan(values):
    """the programs a materialisation of `values` would launch if their buffers were resolved, without running anything:
    [(ops, slots used, leaves)] -- for tests and tools; a program over the caps is split as _run splits it"""
    caps = limits()
    dag = _Dag()
    roots = [dag.add(v) for v in values]
    out = []
    while True:
        try:
            prog = _schedule(dag, roots, caps)
        except _Overflow:
            at, sub = _split_candidate(dag, roots, caps)
            out.append(sub)
            dag.replace_by_leaf(at, _Buffer(None, FORM_MONTGOMERY, values[0].count), 0, FORM_MONTGOMERY)
            if at in roots:
                roots.remove(at)
                if not roots:
                    return out
            continue
        out.append(prog)
        return out
