"""create_proof on the device-resident C ABI: the caller of the hot path -- and the package's public
surface: the names of device.py, params.py, keygen.py, witness.py, check.py, assigned.py and synthesis.py are re-exported
below.

Every polynomial lives in HBM from upload to the last opening; the host sees only what the protocol hashes
(commitments, evaluations) plus the handful of low coefficients SHPLONK adjusts.  Orchestration follows

  plonk/prover.rs:206-850              create_proof_ext (advice, challenges, permutation products, vanishing
                                       argument, evaluations, multiopen)
  plonk/permutation/prover.rs:47-330   commit / evaluate / open
  plonk/vanishing/prover.rs:40-160     random poly, h pieces, h(x)

All arithmetic on vectors runs in libhalo2_hip.so (`h2_dev_*`); torch only owns the device buffers and the
stream.  There is no CPU path in this file: without the library or a GPU it raises.
"""
import ctypes
import hashlib
import os
import sys
import time

import numpy as np

from . import evaluation as ev, parallel as _par
from ._lib import H2Error, check  # noqa: F401
from .arithmetic import (OP_ADDGAMMA, OP_CONSTANT, OP_LCBETA, OP_LCTHETA, OP_MUL, OP_MUL_C, OP_SUB, OP_SUM,  # noqa: F401
                         OP_SUM_C)                          # Device.eval_op's operations: H2_OP_* of include/halo2_hip.h
from .assigned import (ASSIGNED_BAD_ROWS, ASSIGNED_FORM_CANONICAL, ASSIGNED_FORM_COMPACT, ASSIGNED_FORM_MONTGOMERY,  # noqa: F401
                       ASSIGNED_OK, ASSIGNED_STATUS_WORDS, Rational, resolve_rational)
from .check import (CHECK_CELL, CHECK_COPY, CHECK_GATE, CHECK_LOOKUP, CHECK_SHUFFLE, CellNotAssigned, ConstraintNotSatisfied,  # noqa: F401
                    Lookup, Permutation, Shuffle, assert_circuit_satisfied, assert_satisfied, check_assignments, check_circuit,
                    check_failures, check_result, check_witness)
from .circuit import compile_evaluator  # noqa: F401
from .cs_format import vk_digest, vk_digest_preimage  # noqa: F401
from .device import CosetTables, Device, footprint, g1_ntt, max_scalar_bits, parse_bytes, sharding_description  # noqa: F401
from .domain import DELTA, ROOT_OF_UNITY, ZETA, Domain, _fr, _vp  # noqa: F401
from .keygen import (PERM_MAPPING_SORT_TILE, PM_INTERNAL, PM_OK, PM_OUT_OF_BOUNDS, PM_STATUS_WORDS, ProvingKey, _ANY,  # noqa: F401
                     keygen, keygen_from_info, permutation_mapping, permutation_mapping_device, program_descriptor)
from .multiopen import _gwc, _shplonk
from .parallel import allgather_rows, allreduce_counts, allreduce_max, coset_unmix_matrix, exchange_cosets, msm_split_range, scatter_cosets
from .params import Params  # noqa: F401
from .synthesis import (AssignedCells, BoundsFailure, Circuit, ColumnNotInPermutation, DeviceColumns, DeviceCoverage,  # noqa: F401
                        FlatFloorPlanner, HostColumns, HostCoverage, Layouter, NotEnoughColumnsForConstants, NotEnoughRowsAvailable, Region, SynthesisError, Table, V1,
                        region_starts, synthesize_coverage, synthesize_keygen, synthesize_witness)
from .transcript import Blake2bWrite, R_MOD, fr_to_mont_limbs, g1_add_affine
from .values import Value  # noqa: F401
from .witness import (RC_FORM_CANONICAL, RC_FORM_COMPACT, RC_FORM_MONTGOMERY, RC_IN_USE, RC_NO_FIT, RC_OK, RC_OUT_OF_RANGE,  # noqa: F401
                      RC_STATUS_WORDS, RC_UNSUPPORTED, _compress, _instance_columns, _witness_sets, complete_range_check_witness,
                      complete_range_check_witness_device, range_check_assigner, range_check_complete_device)

TRACE_TRANSCRIPT = os.environ.get("H2_TRACE_TRANSCRIPT") == "1"     # create_proof prints a hash of the proof stream per phase


def create_proof(device, params, pk, advice, rng, timings=None, instances=(), strict_rationals=False):
    """plonk/prover.rs:877-893: the GWC multiopen, as the reference's `create_proof`"""
    return create_proof_ext(device, params, pk, advice, rng, True, timings, instances, strict_rationals=strict_rationals)


def create_proof_with_shplonk(device, params, pk, advice, rng, timings=None, instances=(), strict_rationals=False):
    """plonk/prover.rs:856-871"""
    return create_proof_ext(device, params, pk, advice, rng, False, timings, instances, strict_rationals=strict_rationals)


def create_proof_from_witness(device, params, pk, witness, rng, use_gwc=True, timings=None, instances=(), strict_rationals=False):
    """plonk/prover.rs:916-1500: the advice columns come from a witness file (formats.witness_fetch), i.e. in the
    in-memory Montgomery representation"""
    return create_proof_ext(device, params, pk, witness, rng, use_gwc, timings, instances, montgomery=True,
                            strict_rationals=strict_rationals)


class _Lookup:
    """one lookup of one circuit instance (logup/prover.rs): what its phases hand on"""

    def __init__(self, table, inputs):
        self.table = table                  # theta-compressed table column; None once the grand sums are committed
        self.inputs = inputs                # per input set: its theta-compressed columns; None once the grand sums are committed
        self.m = None                       # the multiplicities: Lagrange values, coefficients from the end of the grand-sum phase
        self.m_bits = None                  # what log2(rows x inputs) allows m
        self.m_usable_bits = None           # the measured width of the largest count (None: not measured)
        self.inv_inputs = None              # per input set [1 / (beta + f_i)]: only between the batch inversion and the grand sums
        self.inv_table = None               # 1 / (beta + t): only between the batch inversion and the grand sums
        self.z = []                         # grand-sum columns: Lagrange values, coefficients from the end of the grand-sum phase


class _Circuit:
    """one circuit instance of a proof: its columns as the phases leave them"""

    def __init__(self, instance, instance_polys):
        self.instance, self.instance_polys = instance, instance_polys
        self.advice = None                  # blinded Lagrange columns: from the advice phase; None once the quotient has the coefficients
        self.advice_polys = None            # from the quotient phase on
        self.advice_extended = None         # extended-domain values made on the side stream (small proofs), else None
        self.lookups = []                   # [_Lookup]
        self.shuffles = []                  # per group [(compressed input, compressed shuffle)]; None once the products are committed
        self.nums = self.inv = None         # numerators / the batch-inverted buffer: only inside the grand-product phase
        self.shuffle_inv = None             # per shuffle group its slot of `inv`: only inside the grand-product phase
        self.z = []                         # permutation products: Lagrange values, coefficients from the end of that phase
        self.shuffle_z = []                 # shuffle products: likewise


class _Proof:
    """what the phases of create_proof_ext share"""

    def __init__(self, device, params, pk, rng, timings):
        D = device
        self.D, self.L, self.params, self.pk, self.cs, self.dom = D, D.L, params, pk, pk.cs, pk.domain
        self.n, self.bf = self.dom.n, self.cs.blinding_factors()
        self.last_rot, self.usable = -(self.bf + 1), self.n - (self.bf + 1)
        self.chunk = self.cs.degree() - 2                       # permutation columns per product
        self.nsets = (len(self.cs.perm_columns) + self.chunk - 1) // self.chunk
        self.lo, self.hi = D.row_range(self.n)                  # the rows this rank computes in the phases dealt by rows
        # The blinding rows are 16-bit values whatever the column holds (prover.rs:281-289), so the bound the reference
        # computes over the whole column is never below 16 bits -- a column of booleans or of a few tiny values then runs
        # as ONE window of 2^16 buckets with everything in its first partition.  A commitment is a sum: the usable rows
        # are committed under THEIR bound (the narrow-column shapes of the MSM) and the bf + 1 blinding rows as one more
        # (fused, few-point) MSM per group; the two points are added (_commit_lagrange_with_tail).
        self.split_tail = not (D.group_size > 1 or D.force_collective) and self.usable >= (1 << 12)
        self.transcript, self.rng = Blake2bWrite(), rng
        self.theta = self.beta = self.gamma = self.y = self.x = None   # challenges, as they are squeezed
        self.coset_tabs = pk.coset                              # the key's coset tables, or those built for a multi-instance proof
        self.circuits = []                                      # [_Circuit], from the instance phase on
        self.random_poly = self.random_commitment = None        # from the advice phase on
        self.whole_advice_rows = None       # several ranks: every rank holds every row of the advice columns (advice phase on)
        self.side_parts = []                # advice groups transformed on the side stream: advice phase -> _begin_advice_transforms
        self.side_intt = None               # (coefficients, extended or None, event): _begin_advice_transforms -> quotient
        self.advice_coeffs = self.advice_arrival = None         # several ranks: _begin_advice_transforms -> quotient
        self.z_arrival = self.m_arrival = None                  # several ranks: grand products -> quotient
        self.y_step = None                                      # y^(terms per circuit): inside the quotient phase
        self.timings, self.marks = timings, [("start", time.perf_counter())]
        self.host_trace = [] if os.environ.get("H2_PROVER_HOST_TRACE") else None

    def htrace(self, name):                   # host-side timestamps without any synchronisation (H2_PROVER_HOST_TRACE=1)
        if self.host_trace is not None:
            self.host_trace.append((name, time.perf_counter()))

    def mark(self, name):
        D = self.D
        self.htrace("mark " + name)
        if self.timings is not None:
            D.sync()
            self.marks.append((name, time.perf_counter()))
            if D.group_size > 1:
                _par.comm_trace_phase(name)
        if TRACE_TRANSCRIPT:                 # where two runs (or two ranks) of one proof part ways: the transcript after a phase
            sys.stderr.write("h2 trace: rank %d after %s: %s (%d bytes)\n" % (
                D.group_rank, name, hashlib.sha256(bytes(self.transcript.writer)).hexdigest()[:12], len(self.transcript.writer)))


def create_proof_ext(device, params, pk, advice, rng, use_gwc, timings=None, instances=(), montgomery=False,
                     first_unassigned=None, range_checks_on_device=False, strict_rationals=False):
    """plonk/prover.rs:206-850.  advice: list of (n, 4) u64 columns, canonical integers (or Montgomery residues with
    montgomery=True); rows past the usable range are overwritten with blinding values; instances: one list of
    canonical integers per instance column; rng: a rng.ProverRng.  Returns the proof bytes.
    A column may also be COMPACT -- a 1-D u64 array of n values below 2^64 (booleans, bytes, limbs: 8 bytes per cell over
    PCIe instead of 32, widened on the device) -- or a device tensor of canonical scalars (a witness already resident) --
    or a `Rational`, a column of fractions (an inverse column, a division, a slope) that is resolved on the device before
    anything else, in the form `montgomery` names; `strict_rationals`: a zero denominator is a ValueError, not the cell 0
    (in ANY row, the unused and the blinding rows included: give those the denominator 1, or list the assigned rows, `rows`).

    Several circuit instances in one proof (`circuits: &[ConcreteCircuit]`, prover.rs:206-232): pass `advice` as a list
    of such column lists and `instances` as the matching list of instance-column lists.  Every phase then runs circuit
    by circuit in the reference's order (instance commitments, advice commitments, theta, lookup multiplicities, beta /
    gamma, permutation / lookup / shuffle products, y, ONE quotient over all circuits, x, evaluations, openings).

    `first_unassigned`: {advice column index: first row synthesis left unassigned} (one dict, or one per circuit instance) for
    the range-checked columns -- what the reference's assignment tracking records (prover.rs:1706-1731); without it the
    cells the range is planted in must be zero.

    Range-checked columns are completed where they live: host columns of canonical integers on the host, in place
    (complete_range_check_witness); a pair with a device tensor in it, or Montgomery residues, on the device
    (complete_range_check_witness_device: tensors in place, host columns of the pair uploaded and left unwritten).
    `range_checks_on_device`: host columns too go up first and are completed there by one call per circuit instance, followed
    by one download of its status -- the caller's arrays are not written and the host does no per-row work (DESIGN.md,
    "Completing range-check witnesses", has the measured proof times).  A circuit instance with a range of 2^24 values or
    more, which the device refuses, is completed on the host instead, on copies of its columns.

    A proof that raises (a witness that does not satisfy a lookup, say) releases what it retained on the device."""
    D = device
    ps = _Proof(D, params, pk, rng, timings)
    transcript = ps.transcript
    if timings is not None and D.group_size > 1:
        _par.comm_trace_begin()              # this (untimed) proof records what its collectives cost, phase by phase
    transcript.common_scalar(pk.transcript_repr)
    D.release_retained()                     # (a caller may have retained by hand)
    try:
        if D.group_size > 1:
            ps.rng = rng.shared(D.group)      # every rank of one proof draws the same blinding values
        advice_sets, instance_sets = _witness_sets(ps.cs, ps.n, advice, instances, montgomery, first_unassigned, device=D,
                                                   range_checks_on_device=range_checks_on_device,
                                                   strict_rationals=strict_rationals)
        # The residency of the key was decided at keygen for ONE circuit instance; advice, product and lookup polynomials scale
        # with the number of instances.  A key judged 'extended' whose multi-instance proof does not fit runs this proof by the
        # coset route, from tables built on demand out of the key's coefficient forms (same bytes).
        if len(advice_sets) > 1 and pk.coset is None and D.group_size <= 1 and getattr(pk, "coset_builder", None) is not None:
            mode, keep_ = D.residency(ps.cs, ps.dom, len(advice_sets))
            if mode == "cosets":
                hit = pk.__dict__.get("_multi_coset")
                if hit is None or hit.keep != keep_:
                    hit = pk._multi_coset = CosetTables(pk.coset_builder, range(ps.dom.quotient_poly_degree), keep_)
                ps.coset_tabs = hit
        _commit_instances(ps, instance_sets)
        _commit_advice(ps, advice_sets, montgomery)
        ps.mark("advice commit")
        ps.theta = transcript.squeeze_challenge_scalar()
        _begin_advice_transforms(ps)
        _lookup_multiplicities(ps)
        ps.mark("lookups compress")
        ps.beta = transcript.squeeze_challenge_scalar()
        ps.gamma = transcript.squeeze_challenge_scalar()
        _grand_products(ps)
        ps.mark("permutation")
        ps.htrace("before random_commitment.result")
        transcript.write_point(ps.random_commitment.result())
        ps.y = transcript.squeeze_challenge_scalar()
        ps.htrace("y squeezed")
        pieces = _quotient(ps)
        ps.mark("vanishing transforms")
        for P in D.msm_batch(pieces, params.g, ps.n, 254):
            transcript.write_point(P)
        ps.x = transcript.squeeze_challenge_scalar()
        ps.mark("vanishing construct")
        h_poly, evals = _evaluations(ps, pieces)
        ps.mark("evaluations")
        queries, polys = _multiopen_queries(ps, h_poly, evals)
        (_gwc if use_gwc else _shplonk)(D, params, transcript, queries, polys, ps.n)
    finally:
        D.release_retained()                 # also of a proof that raised half way: its vectors are about to be freed
    ps.mark("multiopen")
    if ps.host_trace:
        base = ps.host_trace[0][1]
        sys.stderr.write("host trace (ms): " + ", ".join("%s %.2f" % (nm, (t - base) * 1e3) for nm, t in ps.host_trace) + "\n")
    if timings is not None:
        for (_, t0), (name, t1) in zip(ps.marks, ps.marks[1:]):
            timings[name] = timings.get(name, 0.0) + (t1 - t0)
        if D.group_size > 1:
            # per phase: seconds / bytes / calls of this rank's collectives (parallel.COMM_TRACE), next to `timings`
            D.last_comm = _par.comm_trace_end()
    return transcript.finalize()


def _commit_instances(ps, instance_sets):
    """instance columns (prover.rs:85-162): zero-padded, committed, hashed but not written"""
    D = ps.D
    dev_sets = [_instance_columns(D, ps.cs, ps.n, ps.usable, inst) for inst in instance_sets]
    for P in D.msm_batch([t for cols in dev_sets for t in cols], ps.params.g_lagrange, ps.n, 254):
        ps.transcript.common_point(P)
    ps.circuits = [_Circuit(cols, [D.intt(D.clone(t), ps.dom) for t in cols]) for cols in dev_sets]


def _commit_lagrange_with_tail(ps, cols_, bits_):
    """commit_lagrange of columns whose USABLE rows are bounded by bits_[i] and whose bf + 1 blinding rows are 16-bit
    values (advice columns, the lookups' multiplicities).  Under `ps.split_tail` a column whose usable rows are narrower than the
    blinding rows (and large enough for the narrow shapes of the MSM to matter) is committed as two sums -- the usable
    rows under THEIR bound, the blinding rows as one more (fused, few-point) MSM -- and the two points are added; the
    others are committed whole, under the bound of the whole column."""
    D, n, usable, bases, split_tail = ps.D, ps.n, ps.usable, ps.params.g_lagrange, ps.split_tail
    narrow_ = [i for i, b in enumerate(bits_) if split_tail and b <= 12 and n >= (1 << 20)]
    whole_ = [i for i in range(len(cols_)) if i not in narrow_]
    points_ = [None] * len(cols_)
    if whole_:
        wb = [max(bits_[i], 16) if split_tail else bits_[i] for i in whole_]
        for i, P in zip(whole_, D.msm_batch([cols_[i] for i in whole_], bases, n, wb)):
            points_[i] = P
    if narrow_:
        main_ = D.msm_batch([cols_[i] for i in narrow_], bases, usable, [bits_[i] for i in narrow_])
        tail_ = D.msm_batch([cols_[i][usable:] for i in narrow_], bases[usable:], n - usable, 16)
        for i, a_, b_ in zip(narrow_, main_, tail_):
            points_[i] = g1_add_affine(a_, b_)
    return points_


def _commit_advice(ps, advice_sets, montgomery):
    """advice columns: blinding rows, bounded commitments (prover.rs:255-312); the random polynomial next to them"""
    D, L, cs, dom, n, bf, usable, rng, transcript = ps.D, ps.L, ps.cs, ps.dom, ps.n, ps.bf, ps.usable, ps.rng, ps.transcript
    nadv = len(advice_sets[0])
    advice = [col for a in advice_sets for col in a]          # circuit-major: the order every phase walks them in
    # Every column is queued for upload on the copy stream first (DMA when it lives in pinned memory); the columns are
    # then blinded, measured (per-column max_bits, as the reference) and committed in small groups -- one pipelined
    # batch per group -- while the later groups are still in flight.
    # One proof over several ranks (n divisible by the group size): a rank uploads only ITS rows [lo, hi) of every
    # column over PCIe -- exactly the range its share of the commitment needs -- and the ranks complete each other's
    # columns over xGMI afterwards (parallel.allgather_rows): 1 / P of the witness per PCIe link instead of all of it.
    sharded_upload = D.group_size > 1 and n % D.group_size == 0 and n // D.group_size > bf + 1
    # ... every rank needs every row of an advice column only where something reads whole Lagrange columns: the
    # theta-compressions of lookups and shuffles (replicated).  Without them (mini-PLONK) a rank keeps its own rows -- all the
    # permutation terms of its range read -- and a column's rows follow their OWNER for the inverse transform
    # (Device.intt_columns_begin with complete = False): 1 / P of the all-gather's traffic.
    whole_advice_rows = ps.whole_advice_rows = bool(cs.lookups or cs.shuffles) or not sharded_upload
    lo_r, hi_r = 0, n
    if sharded_upload:
        lo_r, hi_r = msm_split_range(n, D.group_size, D.group_rank)
        uploads = []
        for col in advice:
            t = D.empty(n)
            with D.torch.cuda.stream(D.tstream):
                t[lo_r:hi_r] = col[lo_r:hi_r] if D.torch.is_tensor(col) else D.upload(np.ascontiguousarray(col[lo_r:hi_r]))
            uploads.append((t, None))
    else:
        # queued a few commitment groups ahead of the group being committed (queue_uploads below), not all at once: with
        # every column of a wide witness in the copy queue the FIRST group's commitment returned only when the LAST column
        # had crossed PCIe (k = 22, 64 compact columns: the GPU idle for 34 of the phase's 125 ms; tools/experiments/busy.sh)
        uploads = [None] * len(advice)
    queued = len(uploads) if sharded_upload else 0

    def queue_uploads(queued, upto):
        for i in range(queued, min(upto, len(uploads))):
            uploads[i] = D.upload_async(advice[i])
        return max(queued, min(upto, len(uploads)))

    # columns are blinded, measured and committed in groups while later uploads are still in flight; small witnesses
    # (<= 256 MiB: already on the device by the time the random polynomial is committed) go as one group -- one
    # synchronisation and one pipelined / fused batch instead of several
    # A WIDE witness (dozens of narrow columns) wants large groups: the columns of a group that share a bound are committed
    # as one fused MSM -- one sort, finish and reduce for all of them, and those latency-bound tails cost a narrow column
    # more than its accumulation -- so a group takes as many columns as cross PCIe in ~5 ms (256 MiB: 8 columns of 32-byte
    # cells at 2^20 rows, 32 compact ones), while the later groups are still in flight.
    group = len(uploads) if len(uploads) * n * 32 <= (256 << 20) else max(1, min(4, len(uploads) // 3))
    if len(uploads) >= 12:
        cell = max((8 if (not D.torch.is_tensor(c) and c.ndim == 1) else 32) for c in advice)
        group = max(group, min(len(uploads), (256 << 20) // (cell * n)))
    if os.environ.get("H2_ADVICE_GROUP"):
        group = int(os.environ["H2_ADVICE_GROUP"])
    group = max(group, 1)
    ahead = max(1, int(os.environ.get("H2_ADVICE_AHEAD", "2"))) * group
    queued = queue_uploads(queued, len(uploads) if len(uploads) <= group else group + ahead)
    # The vanishing argument's random polynomial (vanishing/prover.rs:40-67) and its commitment depend on nothing the
    # transcript has hashed: generated and committed NOW, while the witness columns cross PCIe on the copy stream (k = 24:
    # a 22 ms MSM under a 29 ms transfer) -- on a side stream, so that the columns that have already arrived are
    # blinded and committed next to it instead of behind it (k = 22: advice phase 10.7 -> 9.8 ms).  The commitment is
    # written where the protocol puts it, after the z's.
    # (Small witnesses too: folding it into the advice columns' batch instead was measured slower, k = 18 lookup circuit
    # 28.6 -> 30.2 ms -- the early MSM runs under the host's preparation of the blinding rows.)
    ps.htrace("uploads queued")
    ps.random_poly = D.empty(n)
    check(L.h2_dev_random_fr(rng.random_poly_key(), n, ps.random_poly.data_ptr(), D.stream), "h2_dev_random_fr")
    ps.random_commitment = D.msm_async(ps.random_poly, ps.params.g, n)   # collected where the transcript needs it
    D.retain([ps.random_poly])
    # the blinding rows of every column (drawn column by column, as the reference does) go up in one copy
    blind = np.zeros((max(len(uploads), 1), n - usable, 4), dtype=np.int64)
    for ci in range(len(uploads)):
        blind[ci, :, 0] = [rng.u16() for _ in range(usable, n)]
    with D.torch.cuda.stream(D.tstream):
        blind_dev = D.torch.from_numpy(blind).to(D.dev)
    advice_dev = []
    # A witness that crosses PCIe in SEVERAL groups (the wide circuit at k = 22: 64 columns of 32-byte cells, 8 GiB, 157 ms on the
    # link against ~80 ms of narrow commitments) leaves the GPU idle half of this phase: the columns of a group are final once they
    # are blinded, so their coefficient forms and extended cosets -- needed from the quotient on -- are computed on the SIDE stream
    # group by group, under the later groups' transfers, instead of after the whole phase (H2_SIDE_GROUPS=0: as before).  Measured
    # (profiles/r6_side_groups_ab.txt): wide k = 22 447 -> 352 ms (344 from a compact witness, was 369), wide k = 20 122 -> 113,
    # mini-PLONK k = 24 185 -> 177, k = 22 51.5 -> 50.6.  A witness that fits ONE group keeps the whole-phase form further down.
    side_groups = (os.environ.get("H2_SIDE_GROUPS", "1") != "0" and os.environ.get("H2_SIDE_INTT", "1") != "0" and
                   not sharded_upload and D.group_size <= 1 and not D.force_collective and len(uploads) > group)
    for g0 in range(0, len(uploads), group):
        queued = queue_uploads(queued, g0 + group + ahead)
        cols_ = []
        for ci, (t, arrived) in enumerate(uploads[g0:g0 + group], start=g0):
            if arrived is not None:
                D.tstream.wait_event(arrived)
            if montgomery:                                       # find_max_scalar_bits needs the canonical values
                check(L.h2_dev_batch_unmont(t[lo_r:hi_r].data_ptr(), hi_r - lo_r, D.stream), "h2_dev_batch_unmont")
            if hi_r > usable:                                    # the blinding rows live in the last rank's range
                with D.torch.cuda.stream(D.tstream):
                    t[usable:] = blind_dev[ci]
            cols_.append(t)
        m_rows = usable if ps.split_tail else hi_r - lo_r
        ps.htrace("advice group %d queued" % g0)
        bits_ = D.max_scalar_bits_many([t[lo_r:lo_r + m_rows] for t in cols_], m_rows)
        ps.htrace("advice group %d bits" % g0)
        if sharded_upload:
            bits_ = allreduce_max(bits_, group=D.group, device=D.dev)       # find_max_scalar_bits over the whole column
        bits_ = [max(b, 1) for b in bits_]
        for t in cols_:
            check(L.h2_dev_batch_mont(t[lo_r:hi_r].data_ptr(), hi_r - lo_r, D.stream), "h2_dev_batch_mont")
        for P in _commit_lagrange_with_tail(ps, cols_, bits_):
            transcript.write_point(P)
        ps.htrace("advice group %d committed" % g0)
        if sharded_upload and whole_advice_rows:
            for t in cols_:
                allgather_rows(t, lo_r, hi_r, group=D.group, stream=D.tstream)
        if side_groups:
            ps.side_parts.append(D.intt_on_side_stream(cols_, dom, extend=D.coset_plan(dom) is None and ps.coset_tabs is None))
        advice_dev += cols_
    for ci, C in enumerate(ps.circuits):
        C.advice = advice_dev[ci * nadv:(ci + 1) * nadv]


def _begin_advice_transforms(ps):
    D, dom = ps.D, ps.dom
    advice_dev = [t for C in ps.circuits for t in C.advice]
    # the advice columns are final: their coefficient forms (needed from the quotient on) are computed on the side stream
    # while the lookup / permutation phases run on the compute stream -- up to k = 20, where those phases are chains of
    # small latency-bound kernels (k = 18 lookup circuit 28.9 -> 27.6 ms); at k = 22 / 24 they fill the chip themselves and
    # the transforms only take their time away (60.1 vs 60.2 ms, 210 vs 211)
    if ps.side_parts:
        # (group by group above; the events of one stream are ordered: the last one covers them all)
        exts_ = [e for _, ext_g, _ in ps.side_parts for e in (ext_g or [])]
        ps.side_intt = ([p_ for polys_g, _, _ in ps.side_parts for p_ in polys_g],
                       exts_ if all(ext_g is not None for _, ext_g, _ in ps.side_parts) else None, ps.side_parts[-1][2])
        ps.side_parts = []
    elif (os.environ.get("H2_SIDE_INTT", "1") != "0" and dom.k <= int(os.environ.get("H2_SIDE_INTT_MAX_K", "20"))
            and D.group_size <= 1 and not D.force_collective):
        ps.side_intt = D.intt_on_side_stream(advice_dev, dom, extend=D.coset_plan(dom) is None and ps.coset_tabs is None)
    # one proof over several ranks: the advice columns' inverse transforms are dealt by column now (a rank transforms every
    # P-th column) and the coefficient vectors cross xGMI under the lookup / permutation phases that follow
    if D.group_size > 1:
        ps.advice_coeffs, ps.advice_arrival = D.intt_columns_begin(advice_dev, dom, complete=ps.whole_advice_rows, keep=True)


def _compress_of(ps, C, program, rows=None):
    return _compress(ps.D, ps.dom, program, ps.theta, ps.pk.fixed_values, C.advice, C.instance, rows)


def _lookup_multiplicities(ps):
    """lookups: theta-compressed inputs / table, multiplicities (logup/prover.rs:63-240); the shuffles' compressed expressions"""
    D, L, pk, n, usable, rng = ps.D, ps.L, ps.pk, ps.n, ps.usable, ps.rng
    # One proof over several ranks with the rows dealt (Device.row_range): the compressed INPUT expressions are needed on this
    # rank's rows only (the grand sums below read them there), and the multiplicities are integer counts -- an RCCL reduction:
    # every rank counts the hits of its own input rows in the (whole, replicated) compressed table, the counters are summed by
    # ONE all-reduce per lookup and become field elements afterwards.  The shuffles' expressions likewise: rows only.
    lo_c, hi_c = ps.lo, ps.hi
    rows_c = None if (lo_c, hi_c) == (0, n) else (lo_c, hi_c - lo_c)
    for C in ps.circuits:
        for table_prog, set_progs in pk.lookup_programs:
            st = _Lookup(_compress_of(ps, C, table_prog), [[_compress_of(ps, C, pr, rows_c) for pr in progs] for progs in set_progs])
            flat = [c for cols_ in st.inputs for c in cols_]
            m = D.empty(n)
            nbytes = L.h2_logup_scratch_bytes(n)
            ptrs = (_vp * len(flat))(*[c.data_ptr() for c in flat])
            # (hasattr: OracleLib, the CPU library of tests/oracle_prover.py, has only the plain h2_dev_logup_multiplicity)
            if rows_c is None and hasattr(L, "h2_dev_logup_multiplicity_bits") and os.environ.get("H2_M_BITS", "1") != "0":
                # ... and the width of the largest multiplicity: a range lookup's counts are a few bits wide, nowhere near
                # the log2(rows x inputs) their sum allows -- m's commitment then takes the narrow-column shapes of the MSM
                got_bits = ctypes.c_uint32(0)
                check(L.h2_dev_logup_multiplicity_bits(st.table.data_ptr(), ptrs, len(flat), usable, n, m.data_ptr(),
                                                       D.scratch(nbytes).data_ptr(), nbytes, ctypes.byref(got_bits), D.stream),
                      "h2_dev_logup_multiplicity_bits")
                st.m_usable_bits = max(int(got_bits.value), 1)
            elif rows_c is None:
                check(L.h2_dev_logup_multiplicity(st.table.data_ptr(), ptrs, len(flat), usable, n, m.data_ptr(),
                                                  D.scratch(nbytes).data_ptr(), nbytes, D.stream), "h2_dev_logup_multiplicity")
            else:
                with D.torch.cuda.stream(D.tstream):
                    counts = D.torch.empty(n + 1, dtype=D.torch.int32, device=D.dev)
                check(L.h2_dev_logup_counts(st.table.data_ptr(), ptrs, len(flat), usable, n, lo_c, hi_c, counts.data_ptr(),
                                            D.scratch(nbytes).data_ptr(), nbytes, D.stream), "h2_dev_logup_counts")
                missing = allreduce_counts(counts, group=D.group, stream=D.tstream)
                if missing:
                    raise ValueError("logup: %d input value(s) are missing from the table" % missing)
                check(L.h2_dev_logup_emit(counts.data_ptr(), usable, n, m.data_ptr(), D.stream), "h2_dev_logup_emit")
            D.set_rows(m, usable, [rng.u16() for _ in range(usable, n)])
            st.m, st.m_bits = m, max(16, (usable * len(flat)).bit_length())
            C.lookups.append(st)
        # ---- shuffles: compressed expressions (shuffle/prover.rs:40-80) ------------------------------------------
        C.shuffles = [[(_compress_of(ps, C, ip, rows_c), _compress_of(ps, C, sp, rows_c)) for ip, sp in group]
                      for group in pk.shuffle_programs]
    all_lookups = [st for C in ps.circuits for st in C.lookups]
    if all_lookups and all(st.m_usable_bits is not None for st in all_lookups):
        # (committed whole, a column's bound covers its 16-bit blinding rows too)
        m_bits_ = [st.m_usable_bits if ps.split_tail else max(st.m_usable_bits, 16) for st in all_lookups]
        for P in _commit_lagrange_with_tail(ps, [st.m for st in all_lookups], m_bits_):
            ps.transcript.write_point(P)
    elif all_lookups:
        for P in D.msm_batch([st.m for st in all_lookups], ps.params.g_lagrange, n, max(st.m_bits for st in all_lookups)):
            ps.transcript.write_point(P)


def _blind_product_column(ps, blinding, z):
    """the bf blinding rows of a product / sum column (prover.rs:446-465, :512-530): drawn now, written with the others"""
    blinding.append((z, ps.n - ps.bf, [ps.rng.fr() for _ in range(ps.bf)]))
    return z


def _grand_products(ps):
    """permutation grand products (permutation/prover.rs:47-165), lookup grand sums, shuffle products: the columns, their
    commitments and the start of their inverse transforms"""
    D, L, pk, cs, dom, n, usable, params = ps.D, ps.L, ps.pk, ps.cs, ps.dom, ps.n, ps.usable, ps.params
    beta, gamma, chunk, nsets, circuits = ps.beta, ps.gamma, ps.chunk, ps.nsets, ps.circuits
    cols = cs.perm_columns
    # Everything that has to be inverted before the grand products / sums can run -- the permutation denominators of
    # every set, (beta + f) of every lookup input and table, the shuffle products -- depends only on beta and gamma: it
    # is laid out in ONE buffer (per circuit instance) and inverted by ONE batch inversion, so the inversion's serial
    # a^(r-2) chain (~0.3 ms of pure latency per call) is paid once per proof instead of once per column.
    # One proof over several ranks: every pass of this phase -- the numerator / denominator terms, the batch inversion, the
    # products, the scans -- runs on this rank's rows [lo_s, hi_s) only (a prefix scan exchanges one field element per rank,
    # Device.prefix_scan); the range is exactly what the rank's share of the z commitments consumes, and the ranks complete
    # each other's z columns over xGMI before the inverse transforms (Device.gather_rows).
    lo_s, hi_s = ps.lo, ps.hi
    m_s = hi_s - lo_s
    rows = lambda t: t[lo_s:hi_s]  # noqa: E731
    omega_lo = pow(dom.omega, lo_s, R_MOD)
    fused_perm = D.permutation_product if (lo_s, hi_s) == (0, n) else None
    fused_lookup = D.logup_grand_sum if (lo_s, hi_s) == (0, n) else None
    colvals = [{"advice": C.advice, "fixed": pk.fixed_values, "instance": C.instance} for C in circuits]
    for C, vals in zip(circuits, colvals):
        lookups, shuffles = C.lookups, C.shuffles
        # a device whose vectors live on the HOST makes one call per set instead (h2_permutation_product: terms, inversion,
        # product and scan without num / den crossing PCIe around every step): its sets take no slot here
        pslots = 0 if fused_perm else nsets
        lslots = 0 if fused_lookup else sum(len(cols_in) for st in lookups for cols_in in st.inputs) + len(lookups)
        slots = pslots + lslots + len(shuffles)
        nums = D.empty(max(pslots, 1) * m_s)
        inv = D.empty(max(slots, 1) * m_s)
        slot = lambda i, inv=inv: inv[i * m_s:(i + 1) * m_s]  # noqa: E731
        for k_, si in enumerate(range(0, len(cols) if pslots else 0, chunk)):
            for ci in range(si, min(si + chunk, len(cols))):
                values = vals[cols[ci][0]][cols[ci][1]]
                check(L.h2_dev_permutation_terms(nums[k_ * m_s:].data_ptr(), slot(k_).data_ptr(), rows(values).data_ptr(),
                                                 rows(pk.sigma_values[ci]).data_ptr(), m_s, _fr(beta), _fr(gamma),
                                                 _fr(pow(DELTA, ci, R_MOD) * omega_lo), _fr(dom.omega), 1 if ci == si else 0,
                                                 D.stream), "h2_dev_permutation_terms")
        at = pslots
        for st in lookups:
            if fused_lookup:            # (host vectors: h2_logup_grand_sum inverts on the device, set by set, further down)
                continue
            st.inv_inputs = []
            for cols_in in st.inputs:
                st.inv_inputs.append([])
                for col in cols_in:                                     # beta + f_i
                    st.inv_inputs[-1].append(D.eval_op(OP_SUM_C, slot(at), rows(col), c=beta, size=m_s))
                    at += 1
            st.inv_table = D.eval_op(OP_SUM_C, slot(at), rows(st.table), c=beta, size=m_s)  # beta + t
            at += 1
        C.shuffle_inv = []
        for group in shuffles:                                          # prod_i (beta^(i+1) + shuffle_i)
            dst = slot(at)
            for i, (_, shf) in enumerate(group):
                if i == 0:
                    D.eval_op(OP_SUM_C, dst, rows(shf), c=beta, size=m_s)
                else:
                    D.eval_op(OP_LCBETA, dst, rows(shf), dst, c=pow(beta, i + 1, R_MOD), size=m_s)       # (l + c) * r
            C.shuffle_inv.append(dst)
            at += 1
        assert at == slots
        if slots:
            check(L.h2_dev_batch_invert(inv.data_ptr(), D.empty(slots * m_s).data_ptr(), slots * m_s, D.stream), "h2_dev_batch_invert")
        if pslots:
            D.eval_op(OP_MUL, nums, nums, inv[:nsets * m_s])                                # over all sets
        C.nums, C.inv = nums, inv
    del nums, inv, slot

    # ---- permutation grand products (permutation/prover.rs:89-165), circuit by circuit -------------------------
    blinding = []         # (z, first blinding row, values): drawn in the reference's order, written in one copy below
    for C, vals in zip(circuits, colvals):
        last_z = 1
        for k_ in range(nsets):
            if fused_perm:
                cis = range(k_ * chunk, min((k_ + 1) * chunk, len(cols)))
                z, last_z = fused_perm([vals[cols[ci][0]][cols[ci][1]] for ci in cis], [pk.sigma_values[ci] for ci in cis], n,
                                       beta, gamma, pow(DELTA, k_ * chunk, R_MOD), dom.omega, last_z, usable)
            else:
                z, last_z = D.prefix_scan(C.nums[k_ * m_s:(k_ + 1) * m_s], n, last_z, True, usable)
            C.z.append(_blind_product_column(ps, blinding, z))
        C.nums = None
    num = D.empty(m_s)
    # ---- lookup grand sums (logup/prover.rs:243-415; blinding prover.rs:446-465) -------------------------------
    for C in circuits:
        for st in C.lookups:
            last = 0
            for si, cols_in in enumerate(st.inputs):
                if fused_lookup:
                    z, last = fused_lookup(cols_in, st.table if si == 0 else None, st.m if si == 0 else None, n, beta, last, usable)
                else:
                    src = st.inv_inputs[si][0]                              # sum_i 1 / (beta + f_i)
                    for other in st.inv_inputs[si][1:]:
                        src = D.eval_op(OP_SUM, num, src, other, size=m_s)
                    if si == 0:                                             # - m / (beta + t)
                        D.eval_op(OP_MUL, st.inv_table, st.inv_table, rows(st.m), size=m_s)
                        src = D.eval_op(OP_SUB, num, src, st.inv_table, size=m_s)
                    z, last = D.prefix_scan(src, n, last, False, usable)
                st.z.append(_blind_product_column(ps, blinding, z))
            if last != 0:
                raise ValueError("lookup grand sum does not return to zero")   # sanity-checks feature of the reference
            st.inv_inputs = st.inv_table = None
    # ---- shuffle products (shuffle/prover.rs:82-150; blinding prover.rs:512-530) -------------------------------
    for C in circuits:
        for group, inverted in zip(C.shuffles, C.shuffle_inv):
            for i, (inp, _) in enumerate(group):
                D.eval_op(OP_LCBETA, inverted, rows(inp), inverted, c=pow(beta, i + 1, R_MOD), size=m_s)
            z, closing = D.prefix_scan(inverted, n, 1, True, usable)
            if closing != 1:
                raise ValueError("shuffle product does not return to one")
            C.shuffle_z.append(_blind_product_column(ps, blinding, z))
        C.inv = C.shuffle_inv = None
    del num
    D.set_rows_many(blinding)
    # commit_lagrange_and_ifft (poly/commitment.rs:144-197) for every z, in the transcript's order: the permutation
    # products of every circuit, then the lookup sums of every circuit, then the shuffle products (prover.rs:595-625)
    all_z = ([z for C in circuits for z in C.z] + [z for C in circuits for st in C.lookups for z in st.z] +
             [z for C in circuits for z in C.shuffle_z])
    # (a device whose vectors live on the HOST does both in one call per column, sharing the one upload:
    # gpu_multiexp_bound_and_fft, arithmetic.rs:375-410)
    commit_ifft = D.commit_lagrange_and_ifft if (lo_s, hi_s) == (0, n) and not D.force_collective else None
    z_commitments = commit_ifft(all_z, params.g_lagrange, dom) if commit_ifft else D.msm_batch(all_z, params.g_lagrange, n, 254)
    for P in z_commitments:
        ps.transcript.write_point(P)
    # (one proof over several ranks: every rank computed its own rows of the product columns; a column's rows go to the
    # rank that transforms it, and the coefficient vectors travel while the advice columns are taken to their cosets)
    # The product columns and the multiplicities are transformed in place, sixteen to a launch: coefficients from here on.
    if not commit_ifft:
        _, ps.z_arrival = D.intt_columns_begin(all_z, dom, complete=False)
    _, ps.m_arrival = D.intt_columns_begin([st.m for C in circuits for st in C.lookups], dom, complete=True)
    for C in circuits:
        for st in C.lookups:
            st.table = st.inputs = None
        C.shuffles = None


def _circuit_polys(C):
    """the coefficient vectors of one circuit instance that the quotient, the evaluations and the openings read, in the
    evaluator's groups: advice, instance, permutation z, lookup z, lookup m, shuffle z"""
    return [list(C.advice_polys), list(C.instance_polys), list(C.z), [t for st in C.lookups for t in st.z],
            [st.m for st in C.lookups], list(C.shuffle_z)]


def _evalh_desc(ps, tables, advice, instance, perm_z, lookup_z, lookup_m, shuffle_z, k_domain, zeta_, omega_, rows=None):
    """the h2_evalh_desc of one circuit instance over one evaluation domain: `tables` has the key's vectors there and the
    other lists this circuit's -- coefficient forms (h2_evaluate_h_coeff) or values on the domain (h2_dev_evaluate_h)"""
    pk, g = ps.pk, ps.pk.graph
    return ev.Builder().build(
        k=ps.dom.k, extended_k=k_domain, blinding_factors=ps.bf, chunk_len=ps.chunk,
        constants=np.array([fr_to_mont_limbs(c) for c in g.constants], dtype=np.uint64), rotations=g.rotations,
        calculations=g.calculations, value_parts=pk.value_parts, lookups=pk.lookup_calcs, shuffles=pk.shuffle_calcs,
        fixed=[t.data_ptr() for t in tables["fixed"]], advice=[t.data_ptr() for t in advice],
        instance=[t.data_ptr() for t in instance],
        l0=tables["l0"].data_ptr(), l_last=tables["l_last"].data_ptr(), l_active_row=tables["l_active_row"].data_ptr(),
        perm_z=[t.data_ptr() for t in perm_z], perm_columns=[(_ANY[kd], i) for kd, i in ps.cs.perm_columns],
        perm_sigma=[t.data_ptr() for t in tables["sigma"]],
        lookup_z=[t.data_ptr() for t in lookup_z], lookup_m=[t.data_ptr() for t in lookup_m],
        shuffle_z=[t.data_ptr() for t in shuffle_z],
        y=fr_to_mont_limbs(ps.y), beta=fr_to_mont_limbs(ps.beta), gamma=fr_to_mont_limbs(ps.gamma), theta=fr_to_mont_limbs(ps.theta),
        delta=fr_to_mont_limbs(DELTA), zeta=fr_to_mont_limbs(zeta_), extended_omega=fr_to_mont_limbs(omega_),
        flags=0 if pk.evalh_stats else ev.EVALH_INTERPRET,
        row_begin=rows[0] if rows is not None else 0, row_count=rows[1] if rows is not None else 0)


def _quotient_numerator(ps, points_of, tables, k_domain, zeta_, omega_, size, rows=None, fused=None):
    """the numerator of h over one evaluation domain, every circuit folded in.
    `rows` = (first, count): only these rows of the domain are evaluated (and valid in the result).  `fused` (host
    vectors, one circuit instance): the device's h2_quotient_poly_coeff -- the result is h(X) in COEFFICIENT form"""
    total = None
    lo_, cnt_ = rows if rows is not None else (0, size)
    for C in ps.circuits:
        h_c = _quotient_numerator_of(ps, C, points_of, tables, k_domain, zeta_, omega_, size, rows, fused)
        if total is None:
            total = h_c
        else:                                                                               # l * c + r
            ps.D.eval_op(OP_LCTHETA, total[lo_:lo_ + cnt_], total[lo_:lo_ + cnt_], h_c[lo_:lo_ + cnt_], c=ps.y_step, size=cnt_)
    return total


def _quotient_numerator_of(ps, C, points_of, tables, k_domain, zeta_, omega_, size, rows=None, fused=None):
    """the fused evaluator over one evaluation domain: `points_of` maps a list of coefficient vectors to their values there"""
    D, L, pk, groups = ps.D, ps.L, ps.pk, _circuit_polys(C)
    if points_of is None:
        # the cuda shape of Evaluator::evaluate_h (plonk/evaluation.rs:1229-1241): COEFFICIENT forms in, the extended
        # values of the numerator out, one h2_evaluate_h_coeff call (host slices: halo2-gpu-specific_amd/host_api.py)
        coeff_tables = {"fixed": pk.fixed_polys, "sigma": pk.sigma_polys, "l0": pk.l0_poly, "l_last": pk.l_last_poly,
                        "l_active_row": tables["l_active_row"]}
        b = _evalh_desc(ps, coeff_tables, *groups, k_domain, zeta_, omega_)
        if fused:           # ... divided by the vanishing polynomial and taken back to coefficients in the same call
            out = fused(b.desc, ps.dom, pk.t_evaluations)
        else:
            out = D.empty(size)
            check(L.h2_evaluate_h_coeff(ctypes.byref(b.desc), out.data_ptr()), "h2_evaluate_h_coeff")
        ps.mark("evaluate_h")
        return out
    pre = C.advice_extended if size == ps.dom.extended_n else None    # already extended on the side stream (small proofs)
    if pre is not None:
        groups[0] = []
    # every coefficient vector of this circuit instance that the evaluator reads, taken to the evaluation domain as ONE
    # list (the coset route transforms them sixteen to a launch)
    if ps.advice_arrival is not None:
        # the advice columns' coefficients have been travelling since the commit phase; the product columns' are still on
        # their way: the advice columns go to the evaluation domain first
        ps.advice_arrival.wait()
        first = points_of(groups[0])
        for arrival in (ps.z_arrival, ps.m_arrival):
            if arrival is not None:
                arrival.wait()
        flat = first + points_of([t for grp in groups[1:] for t in grp])
    else:
        flat = points_of([t for grp in groups for t in grp])
    it = iter(flat)
    cosets = [[next(it) for _ in grp] for grp in groups]             # the values, in the evaluator's groups again
    if pre is not None:
        cosets[0] = pre
    del flat, it
    ps.htrace("points_of done (launched)")
    ps.mark("cosets")
    b = _evalh_desc(ps, tables, *cosets, k_domain, zeta_, omega_, rows)
    ps.htrace("descriptor built")
    out = D.empty(size)
    ps.htrace("output allocated")
    check(L.h2_dev_evaluate_h(ctypes.byref(b.desc), out.data_ptr(), D.stream), "h2_dev_evaluate_h")
    ps.htrace("h2_dev_evaluate_h returned")
    ps.mark("evaluate_h")
    return out


def _quotient(ps):
    """h(X): advice to coefficient form, extended cosets, the fused evaluator -> the pieces of h, n coefficients each"""
    D, dom, circuits = ps.D, ps.dom, ps.circuits
    nadv = len(circuits[0].advice)
    if ps.side_intt is not None:
        polys_, ext_, done_ = ps.side_intt
        D.tstream.wait_event(done_)
        for ci, C in enumerate(circuits):
            C.advice_polys = polys_[ci * nadv:(ci + 1) * nadv]
            C.advice_extended = ext_[ci * nadv:(ci + 1) * nadv] if ext_ is not None else None
            C.advice = None                                          # the Lagrange values are not needed again
        ps.side_intt = None
        del polys_, ext_
    elif ps.advice_arrival is not None:
        for ci, C in enumerate(circuits):
            C.advice_polys = ps.advice_coeffs[ci * nadv:(ci + 1) * nadv]
            C.advice = None
        ps.advice_coeffs = None
    else:
        for C in circuits:
            C.advice_polys = D.intt_many(C.advice, dom)                 # in place: the Lagrange values are not needed again
    # the coefficient forms of the witness and of the product columns are final: evaluator, evaluations and openings read them
    D.retain([t for C in circuits for grp in _circuit_polys(C) for t in grp])
    plan = D.coset_plan(dom)
    if D.group_size <= 1:                      # on one device the proving key decides which tables exist
        if ps.coset_tabs is None:
            plan = None
        else:
            plan = (dom.quotient_poly_degree, 1, sorted(ps.coset_tabs))
    # Several circuits share one quotient: the reference keeps folding `value = value * y + term` from one circuit into
    # the next (plonk/evaluation.rs:839-1100), i.e. h = sum_i y^(T (N - 1 - i)) h_i with T terms per circuit and h_i the
    # fold of circuit i alone -- each circuit runs through the evaluator on its own and the results are combined.
    terms_per_circuit = (len(ps.pk.value_parts) + (2 * ps.nsets + 1 if ps.nsets else 0) +
                         sum(2 * len(st.z) + 1 for st in circuits[0].lookups) + 3 * len(circuits[0].shuffle_z))
    ps.y_step = pow(ps.y, terms_per_circuit, R_MOD)
    return _quotient_extended(ps) if plan is None else _quotient_by_cosets(ps, plan)


def _quotient_extended(ps):
    """one device: the whole extended domain at once"""
    D, L, pk, dom, n = ps.D, ps.L, ps.pk, ps.dom, ps.n
    en = dom.extended_n
    tables = {"fixed": pk.fixed_cosets, "sigma": pk.sigma_cosets, "l0": pk.l0, "l_last": pk.l_last,
              "l_active_row": pk.l_active_row}
    from_coeffs = D.quotient_from_coeffs
    # (host vectors, one circuit instance: the three steps in one call, the 2^extended_k values never leave the device)
    fused = D.quotient_poly_coeff if from_coeffs and len(ps.circuits) == 1 else None
    h = _quotient_numerator(ps, None if from_coeffs else (lambda ts: D.coeffs_to_extended(ts, dom)), tables, dom.extended_k, ZETA,
                            dom.extended_omega, en, fused=fused)
    if not fused:
        # vanishing construct: divide, back to coefficients (vanishing/prover.rs:69-112)
        check(L.h2_dev_divide_by_vanishing_poly(h.data_ptr(), en, pk.t_evaluations.data_ptr(), len(dom.t_evaluations),
                                                D.stream), "h2_dev_divide_by_vanishing_poly")
        D.extended_to_coeff(h, dom)
    return [h[i * n:(i + 1) * n] for i in range(dom.quotient_poly_degree)]


def _quotient_by_cosets(ps, plan):
    """one proof over several ranks: the extended domain by coset.  On coset j (points
    g_j w^i, extended indices c i + j) every rotation stays inside the coset, the vanishing polynomial is the
    constant gamma_j - 1 (gamma_j = g_j^n) and h(X) = sum_m X^(n m) h_m(X) reads P_j(X) = sum_m gamma_j^m h_m(X): the
    evaluator runs on n points per coset with zeta := g_j, extended_omega := omega, extended_k := k; the inverse
    coset transform gives P_j; one n-vector per coset is exchanged; the pieces are h_m = sum_j Vinv[m][j] P_j."""
    D, dom, n, circuits, coset_tabs = ps.D, ps.dom, ps.n, ps.circuits, ps.coset_tabs
    c, shards, owned = plan
    mine = {}
    # More ranks than cosets (a multiple G of them): the G ranks of a coset share its work instead of repeating it --
    # every G-th column's coset transform each, row slices exchanged, the evaluator on n / G rows each, the quotient's
    # rows all-gathered inside the group (parallel.exchange_row_slices)
    sub = D.coset_rank_group(c)
    used_rots = list(ps.pk.graph.rotations) + ([0, 1, ps.last_rot] if (ps.nsets or circuits[0].lookups or circuits[0].shuffle_z) else [0])
    halo = (max(0, -min(used_rots)), max(0, max(used_rots)))
    if sub is not None and (n % sub[1] or n // sub[1] <= halo[0] + halo[1] + 1):
        sub = None
    for j in owned:
        g_j = ZETA * pow(dom.extended_omega, j, R_MOD) % R_MOD
        if sub is None:
            lo_g, m_g = 0, n
            h_j = _quotient_numerator(ps, lambda ts, j=j: D.coeffs_to_coset(ts, dom, j), coset_tabs[j], dom.k, g_j, dom.omega, n)
        else:
            m_g = n // sub[1]
            lo_g = sub[2] * m_g
            h_j = _quotient_numerator(ps, lambda ts, j=j: D.coeffs_to_coset_rows(ts, dom, j, sub, halo), coset_tabs[j], dom.k, g_j,
                                      dom.omega, n, rows=(lo_g, m_g))
        D.eval_op(OP_MUL_C, h_j[lo_g:lo_g + m_g], h_j[lo_g:lo_g + m_g], c=dom.t_evaluations[j % len(dom.t_evaluations)],
                  size=m_g)                                                                   # / (gamma_j - 1)
        if sub is not None:
            allgather_rows(h_j, lo_g, lo_g + m_g, group=sub[0], stream=D.tstream)
        mine[j] = D.coset_to_coeff(h_j, dom, j)
    # Everything after the quotient -- the un-mixing, the h pieces' commitments, the evaluations, the multiopen argument --
    # works on coefficient RANGES (Device.row_range): a rank needs only its own n / P coefficients of every coset
    # polynomial, so their owners scatter slices (c x n / P x 32 B per rank) instead of broadcasting whole vectors.
    if D.group_size > 1 and (ps.lo, ps.hi) != (0, n):
        polys_j = scatter_cosets(mine, c, shards, ps.lo, ps.hi, group=D.group, stream=D.tstream)
    elif D.group_size > 1:
        polys_j = exchange_cosets(mine, c, shards, group=D.group, stream=D.tstream)
    else:
        polys_j = [mine[j] for j in range(c)]
    gammas = [pow(ZETA * pow(dom.extended_omega, j, R_MOD) % R_MOD, n, R_MOD) for j in range(c)]
    unmix = coset_unmix_matrix(gammas, dom.quotient_poly_degree)
    pieces = [D.lincomb_range(D.empty(n), polys_j, row, n) for row in unmix]
    del polys_j, mine
    coset_tabs.trim()
    return pieces


def _evaluations(ps, pieces):
    """evaluations (prover.rs:700-790): every (polynomial, point) pair of the proof in one batched launch
    -> (h(X), {(key, rotation): value})"""
    D, pk, cs, dom, n, x, last_rot, circuits = ps.D, ps.pk, ps.cs, ps.dom, ps.n, ps.x, ps.last_rot, ps.circuits
    xn = pow(x, n, R_MOD)
    # h(X) = sum_i x^(n i) piece_i (vanishing/prover.rs:120-124)
    D.retain(pieces)
    h_poly = D.lincomb_range(D.empty(n), pieces, [pow(xn, i, R_MOD) for i in range(len(pieces))], n)
    D.retain([h_poly])
    wanted, written = [], []            # (key, poly, rotation); the subset the transcript receives, in its order

    def want(key, poly, rot, write=True):
        if (key, rot) not in [(k_, r_) for k_, _, r_ in wanted]:
            wanted.append((key, poly, rot))
        if write:
            written.append((key, rot))

    def want_set_evals(name, polys_):
        for i, p in enumerate(polys_):
            want((name, i), p, 0)
            want((name, i), p, 1)
            if i + 1 < len(polys_):
                want((name, i), p, last_rot)

    # evaluations in the transcript's order (prover.rs:704-790): instance columns of every circuit, advice columns of
    # every circuit, fixed, the random polynomial, sigma, then per circuit the permutation / lookup / shuffle products
    for ci, C in enumerate(circuits):
        for c, rot in cs.instance_queries:
            want(("instance", ci, c), C.instance_polys[c], rot)
    for ci, C in enumerate(circuits):
        for c, rot in cs.advice_queries:
            want(("advice", ci, c), C.advice_polys[c], rot)
    for c, rot in cs.fixed_queries:
        want(("fixed", c), pk.fixed_polys[c], rot)
    want(("random",), ps.random_poly, 0)
    for i, p in enumerate(pk.sigma_polys):
        want(("sigma", i), p, 0)
    for ci, C in enumerate(circuits):
        want_set_evals("z%d" % ci, C.z)
    for ci, C in enumerate(circuits):
        for li, st in enumerate(C.lookups):                            # logup/prover.rs:419-446
            want(("lookup_m", ci, li), st.m, 0)
            want_set_evals("lookup_z%d_%d" % (ci, li), st.z)
    for ci, C in enumerate(circuits):
        for i, p in enumerate(C.shuffle_z):                            # shuffle/prover.rs:196-212
            want(("shuffle_z", ci, i), p, 0)
            want(("shuffle_z", ci, i), p, 1)
    want(("h",), h_poly, 0, write=False)                               # opened, not written (vanishing/prover.rs:140-155)
    values = D.eval_polynomial_ranges([p for _, p, _ in wanted], n, [dom.rotate_omega(x, r) for _, _, r in wanted])
    evals = {(key, rot): v for (key, _, rot), v in zip(wanted, values)}
    for key, rot in written:
        ps.transcript.write_scalar(evals[(key, rot)])
    return h_poly, evals


def _multiopen_queries(ps, h_poly, evals):
    """multiopen query list in the reference's order (prover.rs:792-840): per circuit its instance, advice,
    permutation, lookup and shuffle openings; then fixed, sigma, h and the random polynomial -> (queries, polys)"""
    pk, cs, dom, x, last_rot = ps.pk, ps.cs, ps.dom, ps.x, ps.last_rot
    polys, queries = {}, []

    def query(key, poly, rot):
        polys[key] = poly
        queries.append((key, rot, dom.rotate_omega(x, rot), evals[(key, rot)]))

    def open_sets(name, polys_):
        for i, p in enumerate(polys_):
            query((name, i), p, 0)
            query((name, i), p, 1)
        for i in reversed(range(len(polys_) - 1)):
            query((name, i), polys_[i], last_rot)

    for ci, C in enumerate(ps.circuits):
        for c, rot in cs.instance_queries:
            query(("instance", ci, c), C.instance_polys[c], rot)
        for c, rot in cs.advice_queries:
            query(("advice", ci, c), C.advice_polys[c], rot)
        open_sets("z%d" % ci, C.z)
        for li, st in enumerate(C.lookups):
            query(("lookup_m", ci, li), st.m, 0)
            open_sets("lookup_z%d_%d" % (ci, li), st.z)
        for i, p in enumerate(C.shuffle_z):
            query(("shuffle_z", ci, i), p, 0)
            query(("shuffle_z", ci, i), p, 1)
    for c, rot in cs.fixed_queries:
        query(("fixed", c), pk.fixed_polys[c], rot)
    for i, p in enumerate(pk.sigma_polys):
        query(("sigma", i), p, 0)
    query(("h",), h_poly, 0)
    query(("random",), ps.random_poly, 0)
    return queries, polys
