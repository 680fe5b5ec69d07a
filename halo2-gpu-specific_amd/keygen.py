"""keygen_vk + keygen_pk (plonk/keygen.rs:330-440) and the copy-constraint permutation they need
(plonk/permutation/keygen.rs:112-261): on the device, or by the host function that alone names scipy."""
import ctypes
import os
import warnings

import numpy as np

from . import evaluation as ev
from ._lib import H2Error, check
from .arithmetic import OP_CONSTANT, OP_SUB, OP_SUM
from .assigned import Rational, _resolve_rational_columns
from .circuit import compile_compress, compile_evaluator
from .cs_format import vk_digest
from .device import CosetTables
from .domain import DELTA, Domain, _fr
from .transcript import fr_to_mont_limbs, point_to_bytes


def permutation_mapping(ncols, n, copies):
    """`copies`: (m, 4) integers (left column position, left row, right column position, right row).
    Returns (map_col, map_row) u32 arrays of shape (ncols, n): every cycle sorted by (column, row), each cell
    pointing at its successor (plonk/permutation/keygen.rs:112-143)."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components

    ids = np.arange(ncols * n, dtype=np.int64)
    nxt = ids.copy()
    copies = np.asarray(copies, dtype=np.int64).reshape(-1, 4)
    if len(copies):
        l = copies[:, 0] * n + copies[:, 1]
        r = copies[:, 2] * n + copies[:, 3]
        nodes, inv = np.unique(np.concatenate([l, r]), return_inverse=True)
        m = len(nodes)
        graph = coo_matrix((np.ones(len(l), dtype=np.int8), (inv[:len(l)], inv[len(l):])), shape=(m, m))
        _, labels = connected_components(graph, directed=False)
        order = np.lexsort((nodes, labels))          # by cycle, then by (column, row)
        sl, sn = labels[order], nodes[order]
        succ = np.roll(sn, -1)
        ends = np.flatnonzero(sl != np.roll(sl, -1)) if m > 1 else np.array([0])
        starts = np.concatenate([[0], ends[:-1] + 1])
        succ[ends] = sn[starts]
        nxt[sn] = succ
    return (nxt // n).astype(np.uint32).reshape(ncols, n), (nxt % n).astype(np.uint32).reshape(ncols, n)


PM_OK, PM_OUT_OF_BOUNDS, PM_INTERNAL = 0, 1, 2                                         # H2_PERM_MAPPING_*
PM_STATUS_WORDS = 2
PERM_MAPPING_SORT_TILE = 4096                                                          # H2_PERM_MAPPING_SORT_TILE
_U32_MAX = 0xFFFFFFFF
_ANY = {"advice": ev.ANY_ADVICE, "fixed": ev.ANY_FIXED, "instance": ev.ANY_INSTANCE}


def permutation_mapping_device(device, ncols, n, copies, phase_ms=None):
    """permutation_mapping on the device (csrc/permmap.hip): the same (map_col, map_row), as two device tensors of
    ncols * n u32 words (int32 storage), column-major -- entry c * n + r is where cell (c, r) maps to.  `copies` crosses
    to the device once, as u32; a copy whose column position or row is out of bounds raises ValueError (the reference's
    Error::BoundsFailure) naming the lowest such copy.  ncols * n must be below 2^32.  The scratch of the call is
    released before this returns.  `phase_ms`: a list that receives [upload, components, compaction + sort, successors]
    in milliseconds, the device's phases timed by HIP events (tools/keygen_bench.py)."""
    D, L, torch = device, device.L, device.torch
    copies = np.asarray(copies).reshape(-1, 4)
    m = len(copies)
    if copies.dtype != np.uint32:
        # a value no u32 holds is out of bounds whatever n is: 0xffffffff keeps it so (ncols, n <= ncols * n < 2^32)
        wide = np.asarray(copies, dtype=np.int64)
        if m and (wide.min() < 0 or wide.max() > _U32_MAX):
            wide = np.where((wide < 0) | (wide > _U32_MAX), _U32_MAX, wide)
        copies = wide.astype(np.uint32)
    copies = np.ascontiguousarray(copies)
    cells = ncols * n
    if cells > _U32_MAX:
        raise ValueError("permutation mapping: %d columns of %d rows are 2^32 cells or more" % (ncols, n))
    if cells == 0:
        if m:
            raise ValueError("permutation mapping: copy 0 is out of bounds (BoundsFailure)")
        with torch.cuda.stream(D.tstream):
            return tuple(torch.empty(0, dtype=torch.int32, device=D.dev) for _ in range(2))
    nbytes = L.h2_permutation_mapping_scratch_bytes(ncols, n, m)
    with torch.cuda.stream(D.tstream):
        begin = end = None
        if phase_ms is not None:
            begin, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            begin.record(D.tstream)
        d_copies = torch.from_numpy(copies.view(np.int32)).to(D.dev) if m else None
        if phase_ms is not None:
            end.record(D.tstream)
        map_col = torch.empty(cells, dtype=torch.int32, device=D.dev)
        map_row = torch.empty(cells, dtype=torch.int32, device=D.dev)
        status = torch.empty(PM_STATUS_WORDS, dtype=torch.int32, device=D.dev)
        scratch = torch.empty(nbytes, dtype=torch.uint8, device=D.dev)
    args = (d_copies.data_ptr() if m else None, m, ncols, n, map_col.data_ptr(), map_row.data_ptr(), status.data_ptr(),
            scratch.data_ptr(), nbytes)
    if phase_ms is None:
        check(L.h2_dev_permutation_mapping(*args, D.stream), "h2_dev_permutation_mapping")
    else:
        ms = (ctypes.c_float * 3)()
        check(L.h2_dev_permutation_mapping_phases(*args, ms, D.stream), "h2_dev_permutation_mapping")
        phase_ms[:] = [begin.elapsed_time(end)] + list(ms)
    with torch.cuda.stream(D.tstream):
        code, index = status.cpu().numpy().view(np.uint32).tolist()
    del scratch, d_copies
    if code == PM_OUT_OF_BOUNDS:
        raise ValueError("permutation mapping: copy %d is out of bounds (BoundsFailure)" % index)
    if code != PM_OK:
        raise H2Error("h2_dev_permutation_mapping: status %d (a bounded loop of the union-find ran out)" % code)
    return map_col, map_row


class ProvingKey:
    pass


def program_descriptor(cs, k, extended_k, graph=None, value_parts=None, lookup_calcs=None, shuffle_calcs=None):
    """the evaluate_h descriptor of a circuit's PROGRAM alone -- constants, rotations, calculations, value parts, lookup /
    shuffle calculations, the permutation argument's shape; every column pointer null -- as h2_evalh_prepare /
    h2_evalh_compile / h2_evalh_source take it"""
    if graph is None:
        graph, value_parts, lookup_calcs, shuffle_calcs = compile_evaluator(cs)
    ncols, chunk = len(cs.perm_columns), cs.degree() - 2
    nsets = (ncols + chunk - 1) // chunk if ncols else 0
    zero = fr_to_mont_limbs(0)
    nz = [len(sets) for _, _, sets in cs.lookups]
    return ev.Builder().build(
        k=k, extended_k=extended_k, blinding_factors=cs.blinding_factors(), chunk_len=chunk,
        constants=np.array([fr_to_mont_limbs(c) for c in graph.constants], dtype=np.uint64), rotations=graph.rotations,
        calculations=graph.calculations, value_parts=value_parts, lookups=lookup_calcs, shuffles=shuffle_calcs,
        fixed=[0] * cs.num_fixed, advice=[0] * cs.num_advice, instance=[0] * cs.num_instance,
        perm_z=[0] * nsets, perm_columns=[(_ANY[kd], i) for kd, i in cs.perm_columns], perm_sigma=[0] * ncols,
        lookup_z=[0] * sum(nz), lookup_m=[0] * len(nz), shuffle_z=[0] * len(shuffle_calcs),
        y=zero, beta=zero, gamma=zero, theta=zero, delta=zero, zeta=zero, extended_omega=zero)


def keygen(device, params, cs, fixed, copies, mapping=None, fixed_montgomery=False, transcript_repr=None, strict_rationals=False):
    """keygen_vk + keygen_pk.  fixed: list of canonical (n, 4) u64 columns, host arrays or device tensors; copies: see
    permutation_mapping.
    `mapping` = (map_col, map_row) replaces `copies` and `fixed_montgomery` marks columns already in the in-memory
    representation: the two things a CircuitData file holds (keygen_pk_from_info, plonk/keygen.rs:458-553).
    A fixed column may be a `Rational` (batch_invert_assigned, keygen.rs:276): resolved on the device straight to the
    in-memory representation, all of them by one call; `strict_rationals` makes a zero denominator a ValueError."""
    D, L = device, device.L
    dom = Domain(params.k, cs.degree())
    n, bf = dom.n, cs.blinding_factors()
    assert n >= cs.minimum_rows()
    pk = ProvingKey()
    pk.cs, pk.domain = cs, dom
    plan = D.coset_plan(dom)
    # one device under a memory budget: when the extended cosets do not fit, the proving key keeps coefficient forms only
    # and the extended-domain phase runs coset by coset (all quotient_poly_degree of them, tables built on demand).
    # Decided before anything of this key is allocated: the estimate is compared with the memory that is free NOW.
    pk.residency, keep = ("cosets", None) if plan is not None else D.residency(cs, dom)
    if plan is None and pk.residency == "cosets":
        plan = (dom.quotient_poly_degree, 1, list(range(dom.quotient_poly_degree)))
    # fixed columns: values, coefficient form, extended cosets
    pk.fixed_values = []
    rational = [isinstance(col, Rational) for col in fixed]
    if any(rational):
        fixed = _resolve_rational_columns(D, list(fixed), n, True, strict_rationals, "fixed", input_montgomery=fixed_montgomery)
    for col, resolved in zip(fixed, rational):
        if resolved:                                                 # Montgomery already
            pk.fixed_values.append(col)
            continue
        # a resident column (synthesis.synthesize_keygen on the device): Montgomery residues stay with the key as they
        # are, canonical values are converted in a copy -- the caller's tensor is not written
        t = D.upload(col) if not D.torch.is_tensor(col) else col if fixed_montgomery else D.clone(col)
        if not fixed_montgomery:
            check(L.h2_dev_batch_mont(t.data_ptr(), n, D.stream), "h2_dev_batch_mont")
        pk.fixed_values.append(t)
    pk.fixed_commitments = D.msm_batch(pk.fixed_values, params.g_lagrange, n, 254)
    pk.fixed_polys = [D.intt(D.clone(t), dom) for t in pk.fixed_values]
    pk.fixed_cosets = [D.coeff_to_extended(t, dom) for t in pk.fixed_polys] if plan is None else None
    # permutation: sigma columns (Lagrange), polys, cosets
    ncols = len(cs.perm_columns)
    if mapping is None and D.dev.type == "cuda" and ncols * n <= _U32_MAX and os.environ.get("H2_PERM_MAPPING") != "host":
        # built on the device and downloaded once: formats.circuit_data_write and check_witness read pk.mapping
        d_col, d_row = permutation_mapping_device(D, ncols, n, copies)
        with D.torch.cuda.stream(D.tstream):
            pk.mapping = tuple(t.cpu().numpy().view(np.uint32).reshape(ncols, n) for t in (d_col, d_row))
    else:
        # a given mapping (keygen_from_info), 2^32 cells or more, H2_PERM_MAPPING=host, or a Device whose vectors live in
        # host memory (the host-slice data flow: the reference's cycles are host data): one block each
        map_col, map_row = mapping if mapping is not None else permutation_mapping(ncols, n, copies)
        assert len(map_col) == ncols and all(len(c) == n for c in map_col)
        pk.mapping = (map_col, map_row)
        with D.torch.cuda.stream(D.tstream):
            d_col, d_row = (D.torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.uint32).reshape(-1)).view(np.int32))
                            .to(D.dev) for a in (map_col, map_row))
    pk.sigma_values = []
    for i in range(ncols):
        out = D.empty(n)
        check(L.h2_dev_permutation_sigma(out.data_ptr(), d_col[i * n:(i + 1) * n].data_ptr(), d_row[i * n:(i + 1) * n].data_ptr(),
                                         n, _fr(DELTA), _fr(dom.omega), D.stream), "h2_dev_permutation_sigma")
        pk.sigma_values.append(out)
    del d_col, d_row
    pk.perm_commitments = D.msm_batch(pk.sigma_values, params.g_lagrange, n, 254)
    pk.sigma_polys = [D.intt(D.clone(t), dom) for t in pk.sigma_values]
    pk.sigma_cosets = [D.coeff_to_extended(t, dom) for t in pk.sigma_polys] if plan is None else None
    # l0, l_last, l_active_row = 1 - (l_last + l_blind) on the extended coset (keygen.rs:395-425)
    def lagrange_poly(rows):
        t = D.zeros(n)
        D.set_rows(t, rows[0], [1] * len(rows))
        return D.intt(t, dom)

    l0_poly, l_last_poly = lagrange_poly([0]), lagrange_poly([n - bf - 1])
    l_blind_poly = lagrange_poly(list(range(n - bf, n)))

    def active_row(l_last, l_blind, size):
        tmp = D.eval_op(OP_SUM, D.empty(size), l_last, l_blind)
        one = D.eval_op(OP_CONSTANT, D.empty(size), c=1)
        return D.eval_op(OP_SUB, one, one, tmp)

    def coset_tables(j):
        nf, ns = len(pk.fixed_polys), len(pk.sigma_polys)
        vals = D.coeffs_to_coset(list(pk.fixed_polys) + list(pk.sigma_polys) + [l0_poly, l_last_poly, l_blind_poly], dom, j)
        return {
            "fixed": vals[:nf], "sigma": vals[nf:nf + ns], "l0": vals[nf + ns], "l_last": vals[nf + ns + 1],
            "l_active_row": active_row(vals[nf + ns + 1], vals[nf + ns + 2], n),
        }

    # kept with the key (three n-vectors behind the closure): a proof of SEVERAL circuit instances may not fit the
    # residency decided here for one and then runs coset by coset from tables built on demand (create_proof_ext)
    pk.coset_builder = coset_tables
    pk.l0_poly, pk.l_last_poly = l0_poly, l_last_poly     # (the cuda-shaped evaluator takes l0 / l_last as coefficient forms)
    if plan is None:
        pk.l0, pk.l_last = D.coeff_to_extended(l0_poly, dom), D.coeff_to_extended(l_last_poly, dom)
        pk.l_active_row = active_row(pk.l_last, D.coeff_to_extended(l_blind_poly, dom), dom.extended_n)
        pk.coset = None
    else:
        # one proof over several ranks: only the cosets this rank evaluates, each an n-point table
        # (under a memory budget on one device: every coset, built on demand and retained up to `keep` of them)
        pk.l0 = pk.l_last = pk.l_active_row = None
        pk.coset = CosetTables(coset_tables, plan[2], keep)
        if keep is None:                       # one proof over several ranks: this rank's cosets stay resident
            for j in plan[2]:
                pk.coset[j]
    # read by every proof, never written (sigma_values: the permutation argument's denominators, permutation/prover.rs:89-128;
    # l_active_row: the extended values the evaluator takes as they are)
    D.retain(list(pk.fixed_polys) + list(pk.sigma_polys) + [l0_poly, l_last_poly] + list(pk.sigma_values) +
             ([pk.l_active_row] if pk.l_active_row is not None else []), owner=pk)
    pk.t_evaluations = D.upload(np.array([fr_to_mont_limbs(v) for v in dom.t_evaluations], dtype=np.uint64))
    # Evaluator::new: the gate program with the lookup / shuffle result calculations, and the compression programs
    # (evaluate_with_theta) of every lookup / shuffle expression list
    pk.graph, pk.value_parts, pk.lookup_calcs, pk.shuffle_calcs = compile_evaluator(cs)
    pk.lookup_programs = [(compile_compress(table), [[compile_compress(inputs) for inputs in st] for st in sets])
                          for _, table, sets in cs.lookups]
    pk.shuffle_programs = [[(compile_compress(inp), compile_compress(shf)) for _, inp, shf in group]
                           for group in cs.shuffles]
    # The library generates and compiles the program's kernels itself the first time a descriptor carries it
    # (csrc/evalh_gen.cpp, hipRTC); doing that here moves the cost from the first proof to keygen and reports what was built.
    # None = the interpreter kernels run (H2_EVALH_JIT=0, or no hipRTC on this machine).
    pk.evalh_stats = None
    if os.environ.get("H2_EVALH_JIT", "1") != "0":
        try:
            pk.evalh_stats = ev.prepare(program_descriptor(cs, dom.k, dom.extended_k, pk.graph, pk.value_parts, pk.lookup_calcs,
                                                           pk.shuffle_calcs))
        except H2Error as e:
            warnings.warn("evaluate_h keeps the interpreter kernels: %s" % e)
    pk.transcript_repr = (transcript_repr if transcript_repr is not None else
                          vk_digest(cs, dom, pk.fixed_commitments, pk.perm_commitments))
    D.sync()
    return pk


def keygen_from_info(device, params, info):
    """CircuitData::into_proving_key (plonk.rs:196-198): `info` = formats.circuit_data_read(path).  The commitments
    are recomputed from the columns and must equal the ones the file carries."""
    if info["k"] != params.k:
        raise ValueError("circuit data for k = %d under params of k = %d" % (info["k"], params.k))
    pk = keygen(device, params, info["cs"], info["fixed"], None, mapping=info["mapping"], fixed_montgomery=True)
    have = [point_to_bytes(P) for P in list(pk.fixed_commitments) + list(pk.perm_commitments)]
    if have != list(info["fixed_commitments"]) + list(info["perm_commitments"]):
        raise ValueError("circuit data: the verifying key's commitments do not match its columns under these params")
    return pk
