"""A big-integer MockProver (dev.rs:932-1340) for the tests of prover.check_witness: Expression trees evaluated row by row on
canonical integers, rotations modulo n, with the semantics check_witness documents -- gates and lookup / shuffle inputs at
the usable rows, copies at all n rows, a lookup row reporting its first missing (set, input), a shuffle reporting the input
rows whose tuple occurs a different number of times on its two sides.  Tuples are compared whole (no compression).

Returns h2_check_record-shaped tuples (kind | circuit << 8, index, sub, row); prover.check_failures turns them into failures."""
from collections import Counter

from halo2_gpu_specific_amd import circuit as hc
from halo2_gpu_specific_amd.transcript import R_MOD

GATE, LOOKUP, SHUFFLE, COPY = 0, 1, 2, 3


def evaluate(e, row, n, cols):
    """an Expression at one row over canonical integer columns {"advice" | "fixed" | "instance": [column][row]}"""
    if isinstance(e, hc.Constant):
        return e.v
    if isinstance(e, hc.Query):
        return cols[e.name][e.column][(row + e.rotation) % n]
    if isinstance(e, hc.Negated):
        return -evaluate(e.e, row, n, cols) % R_MOD
    if isinstance(e, hc.Sum):
        return (evaluate(e.a, row, n, cols) + evaluate(e.b, row, n, cols)) % R_MOD
    if isinstance(e, hc.Product):
        return evaluate(e.a, row, n, cols) * evaluate(e.b, row, n, cols) % R_MOD
    return evaluate(e.e, row, n, cols) * e.c % R_MOD          # Scaled


def columns_to_ints(col, n):
    """a canonical (n, 4) u64 column, a compact 1-D one, or a list of integers -> n integers"""
    if isinstance(col, list):
        return [int(v) % R_MOD for v in col] + [0] * (n - len(col))
    if col.ndim == 1:
        return [int(v) for v in col]
    return [int(a) | int(b) << 64 | int(c) << 128 | int(d) << 192 for a, b, c, d in col.tolist()]


def reference_check(cs, n, advice, fixed, instances, mapping, circuit=0, gate_rows=None, lookups=True):
    """advice / fixed / instances: columns as columns_to_ints takes them (instance columns: lists of public inputs, padded
    with zeros); mapping = (map_col, map_row) as prover.permutation_mapping returns it.  `gate_rows`: only these rows of the
    gates (large k); `lookups` False skips lookups and shuffles.  -> sorted records."""
    usable = n - (cs.blinding_factors() + 1)
    cols = {"advice": [columns_to_ints(c, n) for c in advice], "fixed": [columns_to_ints(c, n) for c in fixed],
            "instance": [columns_to_ints(list(c), n) for c in instances]}
    out = []
    kind = lambda k: k | circuit << 8  # noqa: E731
    part = 0
    rows = range(usable) if gate_rows is None else sorted(r for r in set(gate_rows) if 0 <= r < usable)
    for _, polys in cs.gates:
        for p in polys:
            out += [(kind(GATE), part, 0, r) for r in rows if evaluate(p, r, n, cols) != 0]
            part += 1
    tup = lambda exprs, r: tuple(evaluate(e, r, n, cols) for e in exprs)  # noqa: E731
    if lookups:
        for li, (_, table, sets) in enumerate(cs.lookups):
            have = {tup(table, r) for r in range(usable)}
            for r in range(usable):
                miss = next(((si, ii) for si, st in enumerate(sets) for ii, inputs in enumerate(st) if tup(inputs, r) not in have),
                            None)
                if miss is not None:
                    out.append((kind(LOOKUP), li, miss[0] << 16 | miss[1], r))
        for gi, group in enumerate(cs.shuffles):
            for ui, (_, inp, shf) in enumerate(group):
                a = [tup(inp, r) for r in range(usable)]
                ca, cb = Counter(a), Counter(tup(shf, r) for r in range(usable))
                out += [(kind(SHUFFLE), gi, ui, r) for r in range(usable) if ca[a[r]] != cb[a[r]]]
    map_col, map_row = mapping
    for c, (kd, i) in enumerate(cs.perm_columns):
        for r in range(n):
            kd2, i2 = cs.perm_columns[int(map_col[c][r])]
            if cols[kd][i][r] != cols[kd2][i2][int(map_row[c][r])]:
                out.append((kind(COPY), c, 0, r))
    return sorted(out, key=lambda t: (t[0] >> 8, t[0] & 0xFF, t[1], t[2], t[3]))
