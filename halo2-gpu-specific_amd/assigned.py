"""Rational (Assigned) columns, resolved on a duck-typed Device (`_assigned_operand` / `_assigned_call`) before anything reads them."""
import ctypes

import numpy as np

from .domain import _vp

ASSIGNED_FORM_CANONICAL, ASSIGNED_FORM_MONTGOMERY, ASSIGNED_FORM_COMPACT = 0, 1, 2       # H2_ASSIGNED_FORM_*
ASSIGNED_OK, ASSIGNED_BAD_ROWS = 0, 1                                                    # H2_ASSIGNED_*
ASSIGNED_STATUS_WORDS = 4


class Rational:
    """A column of rational cells num / den (the reference's `Assigned<F>`, plonk/assigned.rs) that may stand wherever a
    column may: in `advice` of create_proof* and check_witness, in `fixed` of keygen.  It is resolved on the device
    (Device.resolve_rational: one batch inversion for all rational columns of a circuit instance); a zero denominator
    gives 0, as `Assigned::evaluate` does.

    num: the n numerators -- an (n, 4) u64 column, a compact 1-D u64 column, or a device tensor of either shape.
    den: the denominators, likewise: n of them, or len(rows) with `rows`, the strictly increasing indices of the rows that
    HAVE a denominator (the reference's `Option<F>`: only they cross PCIe); every other row is num.
    32-byte cells are in the form of the call they are handed to (canonical integers, or Montgomery residues under
    `montgomery` / `fixed_montgomery`).  Host arrays are checked here, without a device."""

    def __init__(self, num, den, rows=None):
        self.num, self.den = self._column(num, "num"), self._column(den, "den")
        self.n = int(self.num.shape[0])
        if self.n == 0:
            raise ValueError("Rational: a column has at least one row")
        self.rows = None
        if rows is not None:
            if hasattr(rows, "data_ptr"):
                raise ValueError("Rational: rows is a host array of row indices")
            r = np.asarray(rows)
            if r.ndim != 1 or (r.size and r.dtype.kind not in "ui"):
                raise ValueError("Rational: rows is a 1-D array of row indices")
            r = r.astype(np.int64)
            if r.size and (r[0] < 0 or r[-1] >= self.n or np.any(r[1:] <= r[:-1]) or np.any(r >= self.n)):
                raise ValueError("Rational: rows must be strictly increasing and below n = %d" % self.n)
            self.rows = np.ascontiguousarray(r.astype(np.uint32))
        want = self.n if self.rows is None else len(self.rows)
        if int(self.den.shape[0]) != want:
            raise ValueError("Rational: den has %d entries for %d %s" % (int(self.den.shape[0]), want,
                                                                         "rows" if self.rows is None else "listed rows"))

    @staticmethod
    def _column(a, what):
        if hasattr(a, "data_ptr"):                                   # a device (or host) tensor of i64 words
            if a.dim() not in (1, 2) or (a.dim() == 2 and a.shape[1] != 4) or a.element_size() != 8 or not a.is_contiguous():
                raise ValueError("Rational: %s is an (n, 4) or 1-D tensor of contiguous 64-bit words" % what)
            return a
        a = np.asarray(a)
        if a.dtype != np.uint64 or a.ndim not in (1, 2) or (a.ndim == 2 and a.shape[1] != 4):
            raise ValueError("Rational: %s is an (n, 4) u64 column or a compact 1-D u64 column" % what)
        return np.ascontiguousarray(a)


def resolve_rational(device, columns, n, montgomery, strict=False, input_montgomery=None, names=None):
    """Device.resolve_rational: the Rational `columns` of n rows -> one (n, 4) vector each, Montgomery residues under
    `montgomery`, else canonical integers.  ONE h2_dev_assigned_resolve (h2_assigned_resolve on the host-slice device) and
    one download of its status.  `input_montgomery`: the form of the 32-byte input cells (default: as `montgomery`).
    ValueError for a bad `rows` (device tensors are first checked there) and, with `strict`, for a zero denominator -- the
    reference's `unwrap` at prover.rs:1609 -- naming the column (`names`) and its first such row; without, the cell is 0."""
    D = device
    count = len(columns)
    if not count:
        return []
    wide = ASSIGNED_FORM_MONTGOMERY if (montgomery if input_montgomery is None else input_montgomery) else ASSIGNED_FORM_CANONICAL
    names = list(names) if names is not None else ["rational column %d" % i for i in range(count)]
    keep, ptrs = [], {"num": [], "den": [], "rows": [], "out": []}
    forms = {"num": [], "den": []}
    counts = []
    for c in columns:
        if not isinstance(c, Rational) or c.n != n:
            raise ValueError("resolve_rational: every column is a Rational of %d rows" % n)
        for what in ("num", "den"):
            t = D._assigned_operand(getattr(c, what))
            keep.append(t)
            ptrs[what].append(t.data_ptr() if t.shape[0] else None)
            forms[what].append(ASSIGNED_FORM_COMPACT if t.dim() == 1 else wide)
        if c.rows is None:
            ptrs["rows"].append(None)
            counts.append(n)
        else:
            # (an empty list still says "sparse": one index that is never read keeps the pointer non-null)
            t = D._assigned_operand(c.rows if len(c.rows) else np.zeros(1, dtype=np.uint32))
            keep.append(t)
            ptrs["rows"].append(t.data_ptr())
            counts.append(len(c.rows))
    outs = [D.empty(n) for _ in columns]
    arr = lambda key: (_vp * count)(*ptrs[key])                         # noqa: E731
    u32s = lambda vals: (ctypes.c_uint32 * count)(*vals)                # noqa: E731
    out_form = ASSIGNED_FORM_MONTGOMERY if montgomery else ASSIGNED_FORM_CANONICAL
    status = D._assigned_call(arr("num"), u32s(forms["num"]), arr("den"), u32s(forms["den"]), arr("rows"),
                              (ctypes.c_uint64 * count)(*counts), (_vp * count)(*[t.data_ptr() for t in outs]), count, n, out_form)
    del keep
    for name, rec in zip(names, status.reshape(count, ASSIGNED_STATUS_WORDS)):
        if rec[0] != ASSIGNED_OK:
            raise ValueError("%s: rows[%d] is not a row below n above its predecessor" % (name, int(rec[3])))
        if strict and rec[1]:
            raise ValueError("%s: zero denominator at row %d (%d in all)" % (name, int(rec[2]), int(rec[1])))
    return outs


def _resolve_rational_columns(device, cols, n, montgomery, strict, what, input_montgomery=None):
    """the Rational entries of the column list `cols` replaced by their resolved vectors (in the list; one call)"""
    at = [i for i, c in enumerate(cols) if isinstance(c, Rational)]
    if at:
        if device is None:
            raise ValueError("Rational columns are resolved on a device: none was given")
        done = device.resolve_rational([cols[i] for i in at], n, montgomery, strict=strict, input_montgomery=input_montgomery,
                                       names=["%s column %d" % (what, i) for i in at])
        for i, t in zip(at, done):
            cols[i] = t
    return cols
