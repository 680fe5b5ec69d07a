"""A proof's witness as the phases take it: theta-compression, instance columns, range-check completion, `_witness_sets`."""
import ctypes
import os

import numpy as np

from . import evaluation as ev
from ._lib import check
from .assigned import _resolve_rational_columns
from .domain import DELTA, ZETA, _vp
from .transcript import fr_to_mont_limbs


def _compress_desc(D, dom, program, theta, fixed, advice, instance, rows=None):
    """the base-domain evaluate_h descriptor of a compression program (`_compress`), bound to these columns and theta"""
    g, parts = program
    cache = D.__dict__.setdefault("_compress_descs", {})
    pointers = dict(fixed=[t.data_ptr() for t in fixed], advice=[t.data_ptr() for t in advice],
                    instance=[t.data_ptr() for t in instance])
    hit = cache.get((id(program), dom.k))
    if hit is not None and hit[0] is program:
        b = hit[1].rebind(y=fr_to_mont_limbs(theta), theta=fr_to_mont_limbs(theta), **pointers)
        b.desc.row_begin, b.desc.row_count = rows if rows is not None else (0, 0)
    else:
        zero = fr_to_mont_limbs(0)
        b = ev.Builder().build(
            k=dom.k, extended_k=dom.k, blinding_factors=0, chunk_len=1,
            constants=np.array([fr_to_mont_limbs(c) for c in g.constants], dtype=np.uint64), rotations=g.rotations,
            calculations=g.calculations, value_parts=parts,
            y=fr_to_mont_limbs(theta), beta=zero, gamma=zero, theta=fr_to_mont_limbs(theta),
            delta=fr_to_mont_limbs(DELTA), zeta=fr_to_mont_limbs(ZETA), extended_omega=fr_to_mont_limbs(dom.omega),
            row_begin=rows[0] if rows is not None else 0, row_count=rows[1] if rows is not None else 0, **pointers)
        cache[(id(program), dom.k)] = (program, b)
    return b


def _compress(D, dom, program, theta, fixed, advice, instance, rows=None):
    """evaluate_with_theta (plonk/evaluation.rs:2330-2398): the theta-compression of an expression list over the
    n-point Lagrange domain = the evaluator program with y := theta and extended_k := k.  The descriptor of a program
    is built once per device and re-bound to the columns / theta of each call (building it costs ~0.1 ms of host time,
    a k = 18 proof compresses eight expression lists).  `rows` = (first, count): only these rows are computed (one rank's
    share of a proof dealt by rows); the result is a full-size vector valid there."""
    g, parts = program
    # the pure-column fast path of the reference (plonk/evaluation.rs:2266-2276): ONE expression that is a plain query at the
    # current rotation compresses to the column itself -- no kernel, no copy (the callers only read the result; an advice column
    # keeps its Lagrange values until the quotient phase turns it into coefficients, after every lookup pass has consumed them)
    if len(parts) == 1 and not g.calculations and parts[0].kind in (ev.VS_FIXED, ev.VS_ADVICE, ev.VS_INSTANCE) and \
            g.rotations[parts[0].rot] == 0 and os.environ.get("H2_COMPRESS_PURE", "1") != "0":
        return {ev.VS_FIXED: fixed, ev.VS_ADVICE: advice, ev.VS_INSTANCE: instance}[parts[0].kind][parts[0].index]
    b = _compress_desc(D, dom, program, theta, fixed, advice, instance, rows)
    out = D.empty(dom.n)
    check(D.L.h2_dev_evaluate_h(ctypes.byref(b.desc), out.data_ptr(), D.stream), "h2_dev_evaluate_h (compress)")
    return out


def range_check_assigner(vmin, vmax, step):
    """RangeCheckRelAssigner (plonk/range_check.rs:40-63): vmin, vmin + step, ... capped at vmax, then vmax itself"""
    out, cur = [], vmin
    while True:
        value = cur
        if value < vmax:
            cur = min(value + step, vmax)
            out.append(value)
        elif cur == vmax:
            cur += step
            out.append(value)
        else:
            return out


def complete_range_check_witness(cs, n, advice, first_unassigned=None):
    """What `create_proof` does to the witness of every `advice_column_range` after synthesis (plonk/prover.rs:1699-1783):
    every value of the range is planted in the unused cells of the range-checked column from the last usable row upwards
    (so that its sorted copy starts at min, ends at max and has no gap wider than step), and the companion column
    becomes the counting sort of the usable rows (`sort`, prover.rs:164-200).  In place on canonical (n, 4) u64 host
    columns, like the reference; `first_unassigned[column]` (optional) is checked as the reference asserts it."""
    usable = n - (cs.blinding_factors() + 1)
    last_active = usable - 1
    for origin, sort, vmin, vmax, step in cs.range_checks:
        col, companion = advice[origin], advice[sort]
        if not isinstance(col, np.ndarray) or not isinstance(companion, np.ndarray):
            raise TypeError("range check: the range-checked column and its companion must be host columns")
        low = lambda c: c if c.ndim == 1 else c[:, 0]            # noqa: E731  (compact columns hold limb 0 only)
        values = np.array(range_check_assigner(vmin, vmax, step), dtype=np.uint64)
        lo = last_active + 1 - len(values)
        # the reference asserts first_unassigned_offset <= (the offset below the last planted cell) = lo - 1 (prover.rs:1731)
        if lo < 1 or (first_unassigned is not None and first_unassigned.get(origin, 0) >= lo):
            raise ValueError("range check: the range does not fit the unused cells of its column")
        if first_unassigned is None:
            # synthesis did not say which cells it assigned: the cells about to be planted (and the spare one below them)
            # must be untouched -- zero -- or already hold exactly the planted values (the same host columns proved again);
            # a witness that uses them would otherwise be silently overwritten and a different statement proved
            target = low(col)[lo:last_active + 1]
            wide_clear = col.ndim == 1 or not col[lo - 1:last_active + 1, 1:].any()
            planted = np.array_equal(target, values[::-1])
            if not wide_clear or low(col)[lo - 1] != 0 or not (planted or not target.any()):
                raise ValueError("range check: the witness already uses the cells the range is planted in")
        low(col)[lo:last_active + 1] = values[::-1]
        if col.ndim == 2:
            col[lo:last_active + 1, 1:] = 0
        body = low(col)[:usable]
        if (col.ndim == 2 and col[:usable, 1:].any()) or int(body.max()) > vmax or int(body.min()) < vmin:
            raise ValueError("range check: a value of the column lies outside its range")   # the reference's HashMap lookup panics
        if vmax - vmin < (1 << 24):         # the reference's counting sort (`sort`, prover.rs:164-200): O(n + range)
            counts = np.bincount((body - np.uint64(vmin)).astype(np.int64), minlength=vmax - vmin + 1)
            low(companion)[:usable] = np.repeat(np.arange(vmin, vmax + 1, dtype=np.uint64), counts)
        else:
            low(companion)[:usable] = np.sort(body, kind="stable")
        if companion.ndim == 2:
            companion[:usable, 1:] = 0
    return advice


RC_FORM_CANONICAL, RC_FORM_MONTGOMERY, RC_FORM_COMPACT = 0, 1, 2                      # H2_RANGE_CHECK_FORM_*
RC_OK, RC_NO_FIT, RC_IN_USE, RC_OUT_OF_RANGE, RC_UNSUPPORTED = 0, 1, 2, 3, 4           # H2_RANGE_CHECK_*
RC_STATUS_WORDS = 8
_RC_ERRORS = {
    RC_NO_FIT: "range check: the range does not fit the unused cells of its column",
    RC_IN_USE: "range check: the witness already uses the cells the range is planted in",
    RC_OUT_OF_RANGE: "range check: a value of the column lies outside its range",
    RC_UNSUPPORTED: "range check: a range of 2^24 values or more cannot be completed on the device",
}


def range_check_complete_device(device, pairs, usable, n):
    """h2_dev_range_check_complete for the column pairs of one circuit instance, in one call and one download:
    pairs = [(origin, companion, origin form, companion form, vmin, vmax, step, first_unassigned or None)], the columns
    device tensors in the form named (RC_FORM_*: (n, 4) canonical, (n, 4) Montgomery, 1-D compact), completed in place.
    Returns the status records, a (len(pairs), RC_STATUS_WORDS) u32 array: [code (RC_*), first offending row, pair, ...];
    a pair whose code is not RC_OK was left untouched."""
    D, L = device, device.L
    count = len(pairs)
    if not count:
        return np.zeros((0, RC_STATUS_WORDS), dtype=np.uint32)
    u64s = lambda vals: (ctypes.c_uint64 * count)(*vals)                # noqa: E731
    origins = (_vp * count)(*[p[0].data_ptr() for p in pairs])
    companions = (_vp * count)(*[p[1].data_ptr() for p in pairs])
    oforms = (ctypes.c_uint32 * count)(*[p[2] for p in pairs])
    cforms = (ctypes.c_uint32 * count)(*[p[3] for p in pairs])
    vmin, vmax, step = u64s([p[4] for p in pairs]), u64s([p[5] for p in pairs]), u64s([p[6] for p in pairs])
    unknown = (1 << 64) - 1
    first = u64s([unknown if p[7] is None else min(int(p[7]), unknown - 1) for p in pairs])
    nbytes = L.h2_range_check_scratch_bytes(vmin, vmax, count)
    with D.torch.cuda.stream(D.tstream):
        status = D.torch.empty(count * RC_STATUS_WORDS, dtype=D.torch.int32, device=D.dev)
    check(L.h2_dev_range_check_complete(origins, companions, oforms, cforms, vmin, vmax, step, first, count, usable, n,
                                        status.data_ptr(), D.scratch(nbytes).data_ptr(), nbytes, D.stream),
          "h2_dev_range_check_complete")
    with D.torch.cuda.stream(D.tstream):
        return status.cpu().numpy().view(np.uint32).reshape(count, RC_STATUS_WORDS)


def complete_range_check_witness_device(device, cs, n, advice, first_unassigned=None, montgomery=False):
    """complete_range_check_witness on the device (csrc/rangecheck.hip): the same planting, the same counting sort and the
    same ValueErrors, for range-checked columns and companions in any form the prover takes -- canonical (n, 4) u64,
    Montgomery residues (`montgomery`), compact 1-D u64 -- and wherever they live.

    A column that is a device tensor is completed in place.  A host column is uploaded, and the completed device tensor
    takes its place in the list `advice`: the caller's host array is NOT written (unlike complete_range_check_witness).  A
    compact column is completed as such and then widened: its entry of `advice` becomes a canonical (n, 4) tensor.
    Nothing of a pair is written unless all its checks pass; after a ValueError the columns of the failing pair are as
    they were and the library stays usable.  A range of 2^24 values or more is a ValueError here (the host path sorts it)."""
    D, torch = device, device.torch
    usable = n - (cs.blinding_factors() + 1)
    pairs = []
    for origin, sort, vmin, vmax, step in cs.range_checks:
        forms = []
        for c in (origin, sort):
            col = advice[c]
            if not torch.is_tensor(col):
                col = advice[c] = D.upload(col, widen=False)
            if col.dim() == 1 and montgomery:
                raise ValueError("range check: a compact column cannot hold Montgomery residues")
            if col.shape[0] != n or not col.is_contiguous():
                raise ValueError("range check: a column of %d contiguous rows is needed" % n)
            forms.append(RC_FORM_COMPACT if col.dim() == 1 else RC_FORM_MONTGOMERY if montgomery else RC_FORM_CANONICAL)
        pairs.append((advice[origin], advice[sort], forms[0], forms[1], vmin, vmax, step,
                      None if first_unassigned is None else first_unassigned.get(origin, 0)))
    status = range_check_complete_device(D, pairs, usable, n)
    for rec in status:
        if rec[0] != RC_OK:
            raise ValueError(_RC_ERRORS[int(rec[0])])
    for origin, sort, _, _, _ in cs.range_checks:
        for c in (origin, sort):
            if advice[c].dim() == 1:
                advice[c] = D.widen(advice[c])
    return advice


def _witness_sets(cs, n, advice, instances, montgomery, first_unassigned, copy_range_columns=False, device=None,
                  range_checks_on_device=False, strict_rationals=False):
    """The witness intake of create_proof_ext: (advice_sets, instance_sets), one list per circuit instance, with the
    range-checked columns completed (complete_range_check_witness, in place on the caller's columns unless
    `copy_range_columns`, which completes copies of them instead).  An instance whose range-checked columns or companions
    are device tensors, or Montgomery residues, or every instance with `range_checks_on_device`, is completed on the device
    (complete_range_check_witness_device: host columns are uploaded, not written).  An instance of host columns with a range
    of 2^24 values or more stays on the host under `range_checks_on_device` too, completed on copies.
    A `Rational` column is resolved first (Device.resolve_rational, one call per circuit instance that has any; a zero
    denominator is a ValueError under `strict_rationals`) and is a device vector from there on; without one the caller's
    columns go through as they are."""
    multi = len(advice) > 0 and isinstance(advice[0], (list, tuple))
    advice_sets = [list(a) for a in advice] if multi else [list(advice)]
    instance_sets = [list(i) for i in instances] if multi else [list(instances)]
    if len(instance_sets) != len(advice_sets):
        raise ValueError("InvalidInstances")
    nadv = len(advice_sets[0])
    if any(len(a) != nadv for a in advice_sets):
        raise ValueError("every circuit instance needs the same advice columns")
    for ci, a in enumerate(advice_sets):                      # rational cells first: a resolved column is a resident one
        _resolve_rational_columns(device, a, n, montgomery, strict_rationals,
                                  "advice" if len(advice_sets) == 1 else "circuit instance %d: advice" % ci)
    if cs.range_checks:
        fu = first_unassigned if isinstance(first_unassigned, (list, tuple)) else [first_unassigned] * len(advice_sets)
        for a, f in zip(advice_sets, fu):                     # prover.rs:1699-1783: plant the range, sort the companion
            resident = any(not isinstance(a[c], np.ndarray) for origin, sort, _, _, _ in cs.range_checks for c in (origin, sort))
            on_device = device is not None and (montgomery or resident or range_checks_on_device)
            copies = copy_range_columns
            if on_device and not (montgomery or resident) and any(vmax - vmin >= 1 << 24 for _, _, vmin, vmax, _ in cs.range_checks):
                # opted in, but a range is past the device's counting-sort cap: host columns keep the host path, which sorts
                # it -- on copies, since the opt-in promises not to write the caller's arrays
                on_device, copies = False, True
            if montgomery and not on_device:
                raise ValueError("range-check witness completion needs canonical advice columns")
            if copies:
                for origin, sort, _, _, _ in cs.range_checks:
                    for c in (origin, sort):
                        if isinstance(a[c], np.ndarray):
                            if not on_device:                 # (the device path uploads host columns: a copy already)
                                a[c] = a[c].copy()
                        elif on_device:
                            a[c] = device.clone(a[c])
            if on_device:
                complete_range_check_witness_device(device, cs, n, a, f, montgomery)
            else:
                complete_range_check_witness(cs, n, a, f)
    return advice_sets, instance_sets


def _instance_columns(D, cs, n, usable, inst):
    """the instance columns of one circuit instance on the device, zero-padded (prover.rs:85-162)"""
    if len(inst) != cs.num_instance:
        raise ValueError("InvalidInstances")
    cols = []
    for vals in inst:
        if len(vals) > usable:
            raise ValueError("InstanceTooLarge")
        t = D.zeros(n)
        D.set_rows(t, 0, list(vals))
        cols.append(t)
    return cols
