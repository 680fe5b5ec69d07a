"""The constraint system's binary form (write_cs / read_cs, helpers.rs:406-561) and the verifying key's digest over it: host
code only -- formats.py puts it into CircuitData files, keygen and the host verifier hash it."""
import hashlib
import struct

from . import circuit
from .transcript import Q_MOD, R_MOD, point_to_bytes

# Every integer is a little-endian u32; rotations are stored as `i32 as u32`; field constants as their canonical
# 32-byte little-endian representation.  Selectors are compiled away before a key is written (compress_selectors,
# circuit.rs:1603-1734): what remains of them is their count and `selector_map`, the fixed column each went to
# (write_fixed_columns, helpers.rs:386-395: a count and the columns' indices); a selector LEAF has no code and is refused.
_ANY = {"advice": 0, "fixed": 1, "instance": 2}          # plonk/circuit.rs:79-86
_ANY_NAME = {v: k for k, v in _ANY.items()}
_E_CONSTANT, _E_FIXED, _E_ADVICE, _E_INSTANCE, _E_NEGATED, _E_SUM, _E_PRODUCT, _E_SCALED = range(8)   # helpers.rs:590-599


def _u32(v):
    return struct.pack("<I", v & 0xFFFFFFFF)


class _Reader:
    def __init__(self, buf):
        self.buf, self.pos = buf, 0

    def take(self, n):
        if self.pos + n > len(self.buf):
            raise IOError("truncated circuit data")
        out = self.buf[self.pos:self.pos + n]
        self.pos += n
        return out

    def u32(self):
        return struct.unpack("<I", self.take(4))[0]

    def i32(self):
        return struct.unpack("<i", self.take(4))[0]

    def fr(self):
        v = int.from_bytes(self.take(32), "little")
        if v >= circuit.R_MOD:
            raise IOError("non-canonical field element in circuit data")
        return v


def _expression_store(cs, e, out):
    """Expression::store (helpers.rs:687-757)"""
    if isinstance(e, circuit.Constant):
        out += [_u32(_E_CONSTANT), (e.v % circuit.R_MOD).to_bytes(32, "little")]
    elif isinstance(e, circuit.Query):
        code, kind = {circuit.Fixed: (_E_FIXED, "fixed"), circuit.Advice: (_E_ADVICE, "advice"),
                      circuit.Instance: (_E_INSTANCE, "instance")}[type(e)]
        out += [_u32(code), _u32(cs.get_any_query_index((kind, e.column), e.rotation)), _u32(e.column), _u32(e.rotation)]
    elif isinstance(e, circuit.Negated):
        out.append(_u32(_E_NEGATED))
        _expression_store(cs, e.e, out)
    elif isinstance(e, (circuit.Sum, circuit.Product)):
        out.append(_u32(_E_SUM if isinstance(e, circuit.Sum) else _E_PRODUCT))
        _expression_store(cs, e.a, out)
        _expression_store(cs, e.b, out)
    elif isinstance(e, circuit.Scaled):
        out.append(_u32(_E_SCALED))
        _expression_store(cs, e.e, out)
        out.append((e.c % circuit.R_MOD).to_bytes(32, "little"))
    elif isinstance(e, circuit.SelectorQuery):
        raise circuit.SelectorNotCompiled("selector %d was not compiled away: the binary form has no selector leaf"
                                          % e.selector.index)
    else:
        raise TypeError("cannot serialise %r" % (e,))


def _expression_fetch(r):
    """Expression::fetch (helpers.rs:628-685)"""
    code = r.u32()
    if code == _E_CONSTANT:
        return circuit.Constant(r.fr())
    if code in (_E_FIXED, _E_ADVICE, _E_INSTANCE):
        r.u32()  # query_index: implied by the query lists
        column, rotation = r.u32(), r.i32()
        return {_E_FIXED: circuit.Fixed, _E_ADVICE: circuit.Advice, _E_INSTANCE: circuit.Instance}[code](column, rotation)
    if code == _E_NEGATED:
        return circuit.Negated(_expression_fetch(r))
    if code in (_E_SUM, _E_PRODUCT):
        a = _expression_fetch(r)
        b = _expression_fetch(r)
        return (circuit.Sum if code == _E_SUM else circuit.Product)(a, b)
    if code == _E_SCALED:
        e = _expression_fetch(r)
        return circuit.Scaled(e, r.fr())
    raise IOError("unknown expression code %d" % code)


def _expressions_store(cs, exprs, out):
    out.append(_u32(len(exprs)))
    for e in exprs:
        _expression_store(cs, e, out)


def _expressions_fetch(r):
    return [_expression_fetch(r) for _ in range(r.u32())]


def _queried_cells(e, cells):
    """the (column, rotation) pairs a gate polynomial touches, in first-use order (Gate::queried_cells)"""
    if isinstance(e, circuit.Query):
        cell = (e.name, e.column, e.rotation)
        if cell not in cells:
            cells.append(cell)
    for child in ("e", "a", "b"):
        if hasattr(e, child):
            _queried_cells(getattr(e, child), cells)


def cs_store(cs):
    """write_cs (helpers.rs:406-456) -> bytes"""
    if cs.num_selectors != len(cs.selector_map):
        raise circuit.SelectorNotCompiled("%d selectors were not compiled away: ConstraintSystem.compress_selectors"
                                          % cs.num_selectors)
    out = [_u32(cs.num_advice), _u32(cs.num_instance), _u32(cs.num_selectors), _u32(cs.num_fixed),
           _u32(len(cs.num_advice_queries))]
    out += [_u32(v) for v in cs.num_advice_queries]
    out.append(_u32(len(cs.selector_map)))                      # selector_map: write_fixed_columns
    out += [_u32(index) for _, index in cs.selector_map]
    out.append(_u32(len(cs.constants)))                         # constants: write_fixed_columns (helpers.rs:386-395)
    out += [_u32(index) for _, index in cs.constants]
    for queries in (cs.advice_queries, cs.instance_queries, cs.fixed_queries):
        out.append(_u32(len(queries)))
        for column, rotation in queries:
            out += [_u32(column), _u32(rotation)]
    out.append(_u32(len(cs.perm_columns)))
    for kind, index in cs.perm_columns:
        out += [_u32(index), _u32(_ANY[kind])]
    out.append(_u32(len(cs.lookups)))
    for _, table, sets in cs.lookups:
        out.append(_u32(len(sets)))
        for st in sets:
            out.append(_u32(len(st)))
            for inputs in st:
                _expressions_store(cs, inputs, out)
        _expressions_store(cs, table, out)
    out.append(_u32(len(cs.shuffles)))
    for group in cs.shuffles:
        out.append(_u32(len(group)))
        for _, inputs, shuffle in group:
            _expressions_store(cs, inputs, out)
            _expressions_store(cs, shuffle, out)
    out.append(_u32(len(cs.range_checks)))                      # range_check arguments (helpers.rs:444-451)
    for origin, sort, vmin, vmax, step in cs.range_checks:
        out += [_u32(origin), _u32(sort), _u32(vmin), _u32(vmax), _u32(step)]
    out.append(_u32(0))                                         # named_advices
    out.append(_u32(len(cs.gates)))
    for _, polys in cs.gates:
        _expressions_store(cs, polys, out)
        cells = []
        for p in polys:
            _queried_cells(p, cells)
        out.append(_u32(len(cells)))
        for kind, column, rotation in cells:
            out += [_u32(column), _u32(_ANY[kind]), _u32(rotation)]
    return b"".join(out)


def cs_fetch(r, name="circuit"):
    """read_cs (helpers.rs:458-561) -> ConstraintSystem; refuses selectors that were not compiled away (a selector
    count without a selector_map of that length)"""
    cs = circuit.ConstraintSystem(name)
    cs.num_advice, cs.num_instance = r.u32(), r.u32()
    cs.num_selectors = r.u32()
    cs.num_fixed = r.u32()
    cs.num_advice_queries = [r.u32() for _ in range(r.u32())]
    cs.selector_map = [("fixed", r.u32()) for _ in range(r.u32())]
    if len(cs.selector_map) != cs.num_selectors:
        raise IOError("circuit data with live selectors")
    if any(index >= cs.num_fixed for _, index in cs.selector_map):
        raise IOError("a selector mapped to a fixed column the circuit data does not have")
    cs.selectors = [None] * cs.num_selectors                    # simple or complex: keygen-time information only
    if cs.num_selectors:
        cs.uncompressed_fixed = cs.num_fixed - len(set(cs.selector_map))
    cs.constants = [("fixed", r.u32()) for _ in range(r.u32())]
    lists = []
    for _ in range(3):
        lists.append([(r.u32(), r.i32()) for _ in range(r.u32())])
    cs.advice_queries, cs.instance_queries, cs.fixed_queries = lists
    for _ in range(r.u32()):
        index, kind = r.u32(), r.u32()
        cs.perm_columns.append((_ANY_NAME[kind], index))
    for _ in range(r.u32()):
        sets = [[_expressions_fetch(r) for _ in range(r.u32())] for _ in range(r.u32())]
        table = _expressions_fetch(r)
        cs.lookups.append(("", table, sets))
    for _ in range(r.u32()):
        group = []
        for _ in range(r.u32()):
            inputs = _expressions_fetch(r)
            group.append(("", inputs, _expressions_fetch(r)))
        cs.shuffles.append(group)
    for _ in range(r.u32()):                                    # range_check arguments (helpers.rs:520-536)
        cs.range_checks.append((r.u32(), r.u32(), r.u32(), r.u32(), r.u32()))
    for _ in range(r.u32()):                                    # named_advices: (String, u32)
        r.take(r.u32())
        r.u32()
    for _ in range(r.u32()):
        polys = _expressions_fetch(r)
        for _ in range(r.u32()):
            r.take(12)                                          # queried cells: recomputable from the polynomials
        cs.gates.append(("", polys))
    return cs


def vk_digest(cs, dom, fixed_commitments, perm_commitments):
    """VerifyingKey::hash_into (plonk.rs:91-109): Blake2b-512 ("Halo2-Verify-Key") over a u64 length and the pinned
    verifying key, reduced by from_bytes_wide.  The reference pins `format!("{:?}", vk.pinned())` -- the Debug text of
    the domain, the whole constraint system and the commitments -- which cannot be reproduced without the Rust binary
    (parity unpinned); this build hashes the same CONTENT in a canonical binary form: domain (k, extended_k, omega),
    both field moduli, the write_cs serialisation of the constraint system (gates, queries, permutation columns, lookups,
    shuffles, instance columns: cs_store) and the fixed / permutation commitments.  Two circuits that differ in
    any gate, lookup or query therefore get different transcripts.  `keygen(..., transcript_repr=...)` overrides the
    value with one dumped from the Rust side (tools/ref_dump) once that can be pinned."""
    h = hashlib.blake2b(digest_size=64, person=b"Halo2-Verify-Key")
    h.update(vk_digest_preimage(cs, dom, fixed_commitments, perm_commitments))
    return int.from_bytes(h.digest(), "little") % R_MOD


def vk_digest_preimage(cs, dom, fixed_commitments, perm_commitments):
    """what vk_digest hashes: a u64 length, then the pinned verifying key in this build's binary form.  The constants
    columns of the constraint system (PinnedConstraintSystem's `constants`, circuit.rs:1137-1152) are part of it through
    cs_store, as a count and the columns' indices; a circuit without any contributes the zero count it always has."""
    cs_bytes = cs_store(cs)
    body = [b"halo2-hip-vk-v2", dom.k.to_bytes(4, "little"), dom.extended_k.to_bytes(4, "little"),
            dom.omega.to_bytes(32, "little"), R_MOD.to_bytes(32, "little"), Q_MOD.to_bytes(32, "little"),
            len(cs_bytes).to_bytes(4, "little"), cs_bytes]
    for group in (fixed_commitments, perm_commitments):
        body.append(len(group).to_bytes(4, "little"))
        body += [point_to_bytes(p) for p in group]
    body = b"".join(body)
    return len(body).to_bytes(8, "little") + body
