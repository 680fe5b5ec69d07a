"""Device: the buffers (torch), the streams and thin typed wrappers over the h2_dev_* entry points, with the memory planning
(`footprint`, `CosetTables`) of the extended-domain phase.  There is no CPU path: without the library or a GPU it raises."""
import concurrent.futures
import contextlib
import ctypes
import os
import warnings

import numpy as np

from ._lib import check, lib
from .arithmetic import OP_CONSTANT, OP_MUL_C, OP_SUM, OP_SUM_C
from .assigned import ASSIGNED_STATUS_WORDS, resolve_rational
from .domain import _FR, _fr, _inv, _vp
from .parallel import (allgather_fold_many, allgather_rows, allgather_scalars, broadcast_columns_begin, combine_range_evals, coset_plan,
                       exchange_row_slices, gather_rows_to, kate_carries, msm_split_range, scan_carries)
from .transcript import R_MOD, fr_from_mont_limbs, fr_to_mont_limbs, jacobian_to_affine, jacobians_to_affine


# H2_POISON_EMPTY=1 (tests): every "uninitialised" vector starts as all-ones words -- not even a field element -- so a pass
# that reads rows nobody wrote (a partially valid vector of the multi-rank paths: only a row range, a row slice and its halo)
# changes the proof on every run instead of only when the allocator hands back dirty memory
POISON_EMPTY = os.environ.get("H2_POISON_EMPTY") == "1"


def parse_bytes(text):
    """'12G', '512M', '4096' -> bytes; None / '' -> None"""
    if text is None or str(text).strip() == "":
        return None
    t = str(text).strip()
    mult = {"K": 1 << 10, "M": 1 << 20, "G": 1 << 30, "T": 1 << 40}.get(t[-1].upper())
    return int(float(t[:-1]) * mult) if mult else int(float(t))


def footprint(cs, dom, cached_cosets=None, instances=1):
    """Device bytes of polynomial data a proof of this circuit holds at its peak, by residency mode:
    'extended' = every extended coset resident (the proving key's fixed / sigma / l tables for the life of the key, the
    witness-dependent ones during the quotient phase); 'cosets' = coefficient forms only, the extended domain visited
    one coset of the n-th roots of unity at a time with `cached_cosets` sets of proving-key tables retained.
    `instances`: circuit instances proved together (plonk/prover.rs:206-232): every witness-dependent polynomial exists once
    per instance, the proving key's once.
    A planning estimate (it decides the mode against H2_DEVICE_MEM_BUDGET), not an allocator."""
    n, en = dom.n, dom.extended_n
    chunk = max(cs.degree() - 2, 1)
    nsets = (len(cs.perm_columns) + chunk - 1) // chunk
    F, A, I, P = cs.num_fixed, cs.num_advice, cs.num_instance, len(cs.perm_columns)
    lk_sets = sum(len(sets) for _, _, sets in cs.lookups)
    witness_polys = (A + I + nsets + lk_sets + len(cs.lookups) + len(cs.shuffles)) * max(1, instances)
    key_polys = 2 * (F + P)                                   # Lagrange values and coefficient forms
    c = dom.quotient_poly_degree
    cached = c if cached_cosets is None else max(1, min(c, cached_cosets))
    # + random / h / scratch vectors, the c per-coset quotients, and the scratch of two commitments in flight (sorted digit
    # entries, slice partials, buckets: ~370 B per point each = 23 n-vectors' worth; k = 25 measured: 97 GiB at the peak)
    base = 32 * n * (key_polys + 2 * witness_polys + 4 + c + 23)
    # (the extended cosets of the witness exist for one instance at a time: the quotient is evaluated circuit by circuit)
    return {"extended": base + 32 * en * ((F + P + 3) + witness_polys // max(1, instances) + 2),
            "cosets": base + 32 * n * ((F + P + 3) * cached + witness_polys // max(1, instances) + 3)}


class CosetTables:
    """The proving key's tables on single cosets of the extended domain (fixed / sigma columns, l0, l_last,
    l_active_row: n values each), built on demand from the coefficient forms and retained least-recently-used up to
    `keep` cosets -- this build's counterpart of the reference's extended-FFT cache (plonk/evaluation_gpu.rs:335-468,
    HALO2_PROOF_GPU_EVAL_CACHE): a miss costs (fixed + sigma + 3) n-point coset transforms (1.8 ms each at 2^24)."""

    def __init__(self, build, cosets, keep=None):
        self.build, self.cosets, self.keep = build, list(cosets), keep
        self.tabs, self.tick, self.hits, self.misses = {}, 0, 0, 0

    def __iter__(self):
        return iter(self.cosets)

    def __getitem__(self, j):
        hit = self.tabs.get(j)
        if hit is None:
            self.misses += 1
            if self.keep is not None:
                while self.tabs and len(self.tabs) >= max(self.keep, 1):
                    del self.tabs[min(self.tabs, key=lambda i: self.tabs[i][1])]
            hit = self.tabs[j] = [self.build(j), 0]
        else:
            self.hits += 1
        self.tick += 1
        hit[1] = self.tick
        return hit[0]

    def trim(self):
        """after a proof: keep = 0 retains nothing between proofs"""
        if self.keep is not None:
            while len(self.tabs) > self.keep:
                del self.tabs[min(self.tabs, key=lambda i: self.tabs[i][1])]


_PROCESS_GROUPS = {}


def _process_group_cache(key, make):
    """communicators made once per process (a Device per bench leg / per fuzzed circuit used to call
    dist.new_group() each, piling up RCCL communicators and turning Device() into an implicit collective every time); dropped
    when the default group they were made under is gone"""
    import torch.distributed as dist

    world = dist.get_world_size()
    alive = _PROCESS_GROUPS.get("_default")
    if alive is None or alive is not dist.group.WORLD:
        _PROCESS_GROUPS.clear()
        _PROCESS_GROUPS["_default"] = dist.group.WORLD
    if (key, world) not in _PROCESS_GROUPS:
        _PROCESS_GROUPS[(key, world)] = make()
    return _PROCESS_GROUPS[(key, world)]


_DEVICE_STREAMS = {}        # (GPU index, stream priorities) -> {"compute", "copy", "side"}: see Device.__init__


class Device:
    """Buffers (torch) + stream + thin typed wrappers over the h2_dev_* entry points.

    Optional fused steps: a device whose vectors live on the host (host_api.HostApiDevice) does in ONE call what the proof
    flow otherwise does step by step; None = step by step.
      permutation_product       one permutation grand product: terms, batch inversion, product and scan
      logup_grand_sum           one lookup grand sum: beta + f, the inversions, the table's term and the scan
      commit_lagrange_and_ifft  the product columns' commitments and their inverse transforms
      quotient_poly_coeff       evaluate_h, the division by the vanishing polynomial and the way back to coefficients
                                (with `quotient_from_coeffs`: the evaluator is handed COEFFICIENT forms)
      quotient_sum              a multiopen quotient: the fold, the subtraction of the low terms and the division"""
    permutation_product = logup_grand_sum = commit_lagrange_and_ifft = quotient_poly_coeff = quotient_sum = None
    quotient_from_coeffs = False
    _side = _side_scratch = None            # (side stream, its helper thread) and the side MSM's scratch: made on first use

    def __init__(self, device=0, group=None, force_collective=False, force_cosets=False, mem_budget=None, eval_cache=None):
        """`mem_budget` (bytes; default H2_DEVICE_MEM_BUDGET, K / M / G suffixes; None = the device's memory): what the
        polynomial data of keygen + one proof may occupy.  A circuit whose extended cosets do not fit runs the
        extended-domain phase coset by coset from coefficient forms (`footprint`, `CosetTables`) -- the same proof bytes;
        `eval_cache` (default HALO2_PROOF_GPU_EVAL_CACHE, the reference's name) = how many cosets' worth of proving-key
        tables stay resident in that mode (setting it selects the mode; unset = as many as the budget holds).
        `group`: a torch.distributed process group (None = the default group when one is initialised) over which
        one proof is spread: every MSM is range-split over the ranks and the extended-domain phase is split by coset
        (DESIGN.md section 6); all ranks must then run the same proof on the same inputs.  `force_cosets` runs the
        coset path on a single device (all cosets locally): the same proof bytes by another route, for tests."""
        import torch  # plumbing only: device memory and the stream

        if not torch.cuda.is_available():
            raise RuntimeError("create_proof needs a HIP device: there is no CPU path")
        self.torch = torch
        self.dev = torch.device("cuda", device)
        torch.cuda.set_device(self.dev)
        self.L = lib()
        # H2_STREAM_PRIORITY = "<compute>,<side>" (torch / HIP stream priorities: lower = more urgent): experiment knob
        pr = os.environ.get("H2_STREAM_PRIORITY", "")
        self._prio = tuple(int(x) for x in pr.split(",")) if pr else (0, 0)
        # The streams belong to the PROCESS, not to the Device object: HIP multiplexes streams onto a few hardware queues
        # (GPU_MAX_HW_QUEUES) in creation order, and streams that share a queue serialise.  A process that made a Device per
        # workload kept drawing new streams, and which of them ended up sharing a queue depended on how many had been made before:
        # the 64-column proof at k = 22 ran 0.344 s as a process's first workload and 0.386 s after the k = 20 legs (its uploads
        # and commitments no longer overlapped: `advice commit` 170 -> 220 ms).  One set per (GPU, priorities), made once.
        streams = _DEVICE_STREAMS.setdefault((self.dev.index, self._prio), {})
        if not streams:
            streams["compute"] = torch.cuda.Stream(device=self.dev, priority=self._prio[0])
            streams["copy"] = torch.cuda.Stream(device=self.dev)
        self._streams = streams
        self.tstream, self.copy_stream = streams["compute"], streams["copy"]
        self.stream = _vp(self.tstream.cuda_stream)
        self._scratch = None
        self._pinned = {}
        self.group, self.group_size, self.group_rank, self.force_collective = group, 1, 0, force_collective
        self.force_cosets = force_cosets or os.environ.get("H2_FORCE_COSETS") == "1"   # experiment knob
        self.mem_budget = mem_budget if mem_budget is not None else parse_bytes(os.environ.get("H2_DEVICE_MEM_BUDGET"))
        if mem_budget is None and self.mem_budget is not None and not os.environ.get("H2_NTT_TABLE_BUDGET"):
            # a process-wide budget from the environment also bounds what the library keeps for itself (the optional
            # last-pass twiddle tables of the transforms): a sixteenth of it
            self.L.h2_set_table_budget(self.mem_budget // 16)
        env_cache = os.environ.get("HALO2_PROOF_GPU_EVAL_CACHE")
        self.eval_cache = eval_cache if eval_cache is not None else (int(env_cache) if env_cache not in (None, "") else None)
        import torch.distributed as dist

        self.bulk_group = group
        if dist.is_available() and dist.is_initialized():
            self.group_size, self.group_rank = dist.get_world_size(group), dist.get_rank(group)
            if self.group_size > 1 and group is None:
                # a second communicator for the bulk column traffic (parallel.broadcast_columns_begin): collectives of one
                # communicator run in issue order, and the 96-byte all-gathers of the commitments must not wait behind
                # half a gigabyte of coefficients.  ONE per process, made by the first Device of a multi-rank process
                # (collective: every rank constructs its first Device at the same point) and reused by every later one --
                # bench.py and the fuzzers build a Device per leg / per circuit, and communicators are never freed by torch
                # before destroy_process_group.
                self.bulk_group = _process_group_cache("bulk", dist.new_group)

    @classmethod
    def replica(cls, device=0, **kw):
        """a Device that proves ALONE inside a multi-rank process group -- one proof per GPU, no collective on the data path
        (the throughput form of N GPUs; `Device()` in such a process spreads ONE proof over the ranks).  Collective the first
        time: every rank builds the singleton groups of all ranks, in order."""
        import torch.distributed as dist

        if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size() == 1:
            return cls(device, **kw)
        groups = _process_group_cache("singletons", lambda: [dist.new_group(ranks=[r]) for r in range(dist.get_world_size())])
        return cls(device, group=groups[dist.get_rank()], **kw)

    # -- memory -----------------------------------------------------------------------------------------
    def empty(self, n):
        with self.torch.cuda.stream(self.tstream):
            t = self.torch.empty((n, 4), dtype=self.torch.int64, device=self.dev)
            if POISON_EMPTY:
                t.fill_(-1)
            return t

    def zeros(self, n):
        with self.torch.cuda.stream(self.tstream):
            return self.torch.zeros((n, 4), dtype=self.torch.int64, device=self.dev)

    def upload(self, a, widen=True):
        a = np.ascontiguousarray(a)
        with self.torch.cuda.stream(self.tstream):
            src = self._pinned.get(a.ctypes.data)
            if src is not None and src.numel() == a.size:
                t = src.to(self.dev, non_blocking=True)
            else:
                with warnings.catch_warnings():      # read-only sources (a memory-mapped witness file) are only read
                    warnings.simplefilter("ignore", UserWarning)
                    t = self.torch.from_numpy(a.view(np.int64)).to(self.dev)
        return self.widen(t) if a.ndim == 1 and widen else t

    def widen(self, small, stream=None):
        """a compact column (n u64 values on the device, 8 B per cell over PCIe) -> canonical (n, 4) scalars"""
        n = small.shape[0]
        out = self.empty(n)
        check(self.L.h2_dev_widen_u64(small.data_ptr(), n, out.data_ptr(), self.stream if stream is None else stream),
              "h2_dev_widen_u64")
        small.record_stream(self.tstream)
        return out

    def resolve_rational(self, columns, n, montgomery, strict=False, input_montgomery=None, names=None):
        """Rational columns -> device vectors (see assigned.resolve_rational)"""
        return resolve_rational(self, columns, n, montgomery, strict, input_montgomery, names)

    def _assigned_operand(self, a):
        """an operand of resolve_rational as it crosses PCIe: compact cells stay 8 bytes, row indices 4"""
        if self.torch.is_tensor(a):
            return a
        if a.dtype == np.uint32:
            with self.torch.cuda.stream(self.tstream):
                return self.torch.from_numpy(a.view(np.int32)).to(self.dev)
        return self.upload(a, widen=False)

    def _assigned_call(self, num, nforms, den, dforms, rows, counts, outs, count, n, out_form):
        with self.torch.cuda.stream(self.tstream):
            status = self.torch.empty(count * ASSIGNED_STATUS_WORDS, dtype=self.torch.int32, device=self.dev)
        check(self.L.h2_dev_assigned_resolve(num, nforms, den, dforms, rows, counts, outs, count, n, out_form,
                                             status.data_ptr(), self.stream), "h2_dev_assigned_resolve")
        with self.torch.cuda.stream(self.tstream):
            return status.cpu().numpy().view(np.uint32)

    def upload_async(self, a):
        """-> (device tensor, event or None): a pinned source is copied by DMA on the copy stream and the event marks
        its arrival; anything else goes through the synchronous path.  `a`: a canonical (n, 4) u64 column, a COMPACT column
        (1-D u64: every value below 2^64 -- 8 bytes per cell cross PCIe and the device widens them), or a device tensor
        (a witness that is already resident: copied, since the prover blinds and converts its columns in place)."""
        if self.torch.is_tensor(a):
            return self.clone(a), None
        a = np.ascontiguousarray(a)
        src = self._pinned.get(a.ctypes.data)
        if src is None or src.numel() != a.size:
            return self.upload(a), None
        torch = self.torch
        with torch.cuda.stream(self.copy_stream):
            t = src.to(self.dev, non_blocking=True)
            if a.ndim == 1:                    # widened on the copy stream too: behind its own arrival, ahead of nothing
                small, t = t, torch.empty((a.shape[0], 4), dtype=torch.int64, device=self.dev)
                check(self.L.h2_dev_widen_u64(small.data_ptr(), a.shape[0], t.data_ptr(), _vp(self.copy_stream.cuda_stream)),
                      "h2_dev_widen_u64")
            ev = torch.cuda.Event()
            ev.record(self.copy_stream)
        t.record_stream(self.tstream)          # allocated under the copy stream, consumed on the compute stream
        return t, ev

    def download(self, t):
        with self.torch.cuda.stream(self.tstream):
            return t.cpu().numpy().view(np.uint64)

    def clone(self, t):
        with self.torch.cuda.stream(self.tstream):
            return t.clone()

    def set_rows(self, t, start, values):
        """t[start : start + len(values)] <- canonical integers (stored Montgomery)"""
        if not len(values):                      # (an instance column without public inputs)
            return
        a = np.array([fr_to_mont_limbs(v) for v in values], dtype=np.uint64)
        with self.torch.cuda.stream(self.tstream):
            t[start:start + len(values)] = self.torch.from_numpy(a.view(np.int64)).to(self.dev)

    def set_rows_many(self, items):
        """[(t, start, values)]: set_rows for several vectors with ONE host-to-device copy (the blinding rows of every
        product column of a phase: a copy from pageable memory synchronises, ~50 us each)"""
        items = [it for it in items if len(it[2])]
        if not items:
            return
        flat = np.array([fr_to_mont_limbs(v) for _, _, vals in items for v in vals], dtype=np.uint64)
        with self.torch.cuda.stream(self.tstream):
            blob = self.torch.from_numpy(flat.view(np.int64)).to(self.dev)
            at = 0
            for t, start, vals in items:
                t[start:start + len(vals)] = blob[at:at + len(vals)]
                at += len(vals)

    def max_scalar_bits_many(self, cols, n):
        """find_max_scalar_bits of several canonical columns resident on the device: one launch, one synchronisation"""
        count = len(cols)
        if not count:
            return []
        ptrs = (ctypes.c_void_p * count)(*[c.data_ptr() for c in cols])
        out = (ctypes.c_uint32 * count)()
        with self.torch.cuda.stream(self.tstream):
            words = self.torch.empty((count, 8), dtype=self.torch.int32, device=self.dev)
        check(self.L.h2_dev_max_scalar_bits(ptrs, count, n, words.data_ptr(), out, self.stream), "h2_dev_max_scalar_bits")
        return list(out)

    def pinned_columns(self, count, n, compact=False):
        """`count` zeroed (n, 4) u64 numpy columns in page-locked host memory: a witness synthesised into them
        reaches the device by DMA instead of through the driver's staging copies.  `compact`: 1-D columns of n u64 values
        (a quarter of the bytes over PCIe) for columns whose values all fit 64 bits."""
        out = []
        for _ in range(count):
            t = self.torch.zeros((n,) if compact else (n, 4), dtype=self.torch.int64).pin_memory()
            a = t.numpy().view(np.uint64)
            self._pinned[a.ctypes.data] = t
            out.append(a)
        return out

    def get_rows(self, t, start, count):
        with self.torch.cuda.stream(self.tstream):
            a = t[start:start + count].cpu().numpy().view(np.uint64)
        return [fr_from_mont_limbs(r) for r in a]

    def sync(self):
        self.tstream.synchronize()

    # -- vectors that will not change any more (hooks for the host-slice data flow; nothing to do for resident vectors) ----------
    def retain(self, vectors, owner=None):
        """`vectors` are final from here on -- the proving key's coefficient forms (owner = the key), or a proof's advice /
        product / quotient polynomials (until `release_retained`).  On this device they already live in HBM; the literal
        drop-in (host_api.HostApiDevice) registers them with the library (h2_poly_register) so that later calls that read them
        find a device copy instead of uploading them again."""

    def release_retained(self):
        """end of a proof: the per-proof registrations of `retain` go"""

    def scratch(self, nbytes):
        if self._scratch is None or self._scratch.numel() < nbytes:
            self._scratch = None
            with self.torch.cuda.stream(self.tstream):
                self._scratch = self.torch.empty(nbytes, dtype=self.torch.uint8, device=self.dev)
        return self._scratch

    # -- coset sharding of the extended domain (one proof over several ranks) --------------------------
    def coset_plan(self, dom):
        """None = the quotient is evaluated on the whole extended domain; else (c, shards, owned): it is evaluated coset
        by coset.  The extended domain is the union of 2^(extended_k - k) cosets g_j H (g_j = zeta extended_omega^j, H =
        the n-th roots of unity; extended index 2^(extended_k - k) i + j is point i of coset j), but the quotient has
        only quotient_poly_degree = degree - 1 pieces h_t of n coefficients, and on coset j it reads
        P_j(X) = sum_t gamma_j^t h_t(X) (gamma_j = g_j^n): its values on the FIRST c = quotient_poly_degree cosets
        determine it (a c x c Vandermonde system per coefficient).  This rank evaluates the cosets in `owned`.

        Used when one proof is spread over several ranks.  On a single device the fused extended-domain transforms win
        (2^(extended_k - k) is the next power of two above degree - 1, so at best 5 of 8 cosets are saved, and the
        per-coset launches cost more than that below k = 22: profiles/r2_coset_path_vs_extended.txt); `force_cosets` /
        H2_COSETS=1 runs the coset route there -- the same proof bytes -- for tests."""
        c = dom.quotient_poly_degree
        if self.group_size <= 1 and not self.force_cosets and os.environ.get("H2_COSETS") != "1":
            return None
        shards, owned = coset_plan(c, self.group_size, self.group_rank)
        return c, shards, owned

    def residency(self, cs, dom, instances=1):
        """('extended', None) or ('cosets', keep): how the extended-domain phase of this circuit runs on ONE device under
        the memory budget.  `keep` = cosets' worth of proving-key tables retained between uses.  `instances`: circuit
        instances in one proof (decided at keygen for one; create_proof_ext asks again when it is handed several)."""
        c = dom.quotient_poly_degree
        if self.eval_cache is not None:
            return "cosets", max(0, min(c, self.eval_cache))
        budget = self.mem_budget
        if budget is None:
            # what the device has left NOW -- behind the SRS and its shifted-base tables (96 GiB at k = 26), other keys --
            # plus what torch's allocator holds but does not use; a fifth of it stays free for library tables and slack
            torch = self.torch
            free, _ = torch.cuda.mem_get_info(self.dev)
            held = self._scratch.numel() if self._scratch is not None else 0     # commitment scratch: reused, and counted
            budget = int(0.8 * (free + torch.cuda.memory_reserved(self.dev) - torch.cuda.memory_allocated(self.dev) + held))
            if footprint(cs, dom, None, instances)["extended"] <= budget:
                return "extended", None
        elif footprint(cs, dom, None, instances)["extended"] <= budget:
            return "extended", None
        for keep in range(c, 0, -1):
            if footprint(cs, dom, keep, instances)["cosets"] <= budget:
                return "cosets", keep
        if footprint(cs, dom, 1, instances)["cosets"] > budget * 1.5:
            raise MemoryError("this circuit needs ~%.1f GiB of device memory even coset by coset; the budget is %.1f GiB"
                              % (footprint(cs, dom, 1, instances)["cosets"] / 2**30, budget / 2**30))
        return "cosets", 0

    def coeff_to_coset(self, poly, dom, j):
        """values of a coefficient vector (n entries) on coset j: a[t] *= g_j^t, then the n-point NTT -- coeff_to_extended
        (poly/domain.rs:270-287) restricted to the extended indices c i + j.  One fused transform (h2_dev_coset_ntt: the
        powers of g_j are applied on the first pass's load): `poly` is read, not copied"""
        out = self.empty(dom.n)
        g = dom.g_coset * pow(dom.extended_omega, j, R_MOD) % R_MOD
        tmp = self.empty(dom.n)
        check(self.L.h2_dev_coset_ntt(poly.data_ptr(), out.data_ptr(), tmp.data_ptr(), dom.k, _fr(g), _fr(dom.omega),
                                      self.stream), "h2_dev_coset_ntt")
        return out

    @staticmethod
    def _batch_width(points, cap_bytes=1 << 30):
        """vectors per batched-transform call: up to 16, fewer when their scratch (one vector each) would pass `cap_bytes` --
        large transforms fill the chip on their own, and the scratch must stay small next to a memory budget"""
        return max(1, min(16, cap_bytes // (32 * points)))

    def coeffs_to_coset(self, polys, dom, j):
        """coeff_to_coset of several coefficient vectors: up to 16 transforms per launch (h2_dev_coset_ntt_batch) -- the
        tiles of one 2^20-point pass do not fill the chip for long enough to hide their own latencies, those of a
        dozen vectors do"""
        count = len(polys)
        if count == 0:
            return []
        if count == 1:
            return [self.coeff_to_coset(polys[0], dom, j)]
        outs = [self.empty(dom.n) for _ in polys]
        width = self._batch_width(dom.n)
        tmp = self.empty(min(count, width) * dom.n)
        g = dom.g_coset * pow(dom.extended_omega, j, R_MOD) % R_MOD
        for at in range(0, count, width):
            part = min(width, count - at)
            src = (_vp * part)(*[p.data_ptr() for p in polys[at:at + part]])
            dst = (_vp * part)(*[o.data_ptr() for o in outs[at:at + part]])
            check(self.L.h2_dev_coset_ntt_batch(src, dst, part, tmp.data_ptr(), dom.k, _fr(g), _fr(dom.omega), self.stream),
                  "h2_dev_coset_ntt_batch")
        return outs

    def intt_many(self, ts, dom):
        """lagrange_to_coeff in place on several vectors, up to 16 per launch (h2_dev_intt_batch)"""
        count = len(ts)
        if count == 0:
            return ts
        if count == 1:
            return [self.intt(t, dom) for t in ts]
        width = self._batch_width(dom.n)
        tmp = self.empty(min(count, width) * dom.n)
        for at in range(0, count, width):
            part = min(width, count - at)
            ptrs = (_vp * part)(*[t.data_ptr() for t in ts[at:at + part]])
            check(self.L.h2_dev_intt_batch(ptrs, part, tmp.data_ptr(), _fr(dom.omega_inv), _fr(dom.ifft_divisor), dom.k,
                                           self.stream), "h2_dev_intt_batch")
        return ts

    def column_owner(self, i):
        return i % self.group_size

    def coset_rank_group(self, c):
        """(group, members G, this rank's member index) of the ranks that share this rank's coset when the P ranks are a
        multiple G >= 2 of the c cosets (rank r evaluates coset r mod c; its group is {j, j + c, j + 2 c, ...}), else None.
        Creating the groups is collective: every rank creates all c of them, in order, the first time a circuit with c
        cosets is proved (cached)."""
        P = self.group_size
        if P <= 1 or c < 1 or P % c or P // c < 2 or self.group is not None or os.environ.get("H2_COSET_GROUPS") == "0":
            return None
        import torch.distributed as dist

        G = P // c
        # (per process, not per Device: the same c groups serve every Device of this world size)
        groups = _process_group_cache(("coset", P, c), lambda: [dist.new_group(ranks=[j + c * m for m in range(G)]) for j in range(c)])
        sub = (groups[self.group_rank % c], G, self.group_rank // c)
        self.__dict__.setdefault("_coset_groups", {})[c] = sub      # (what this Device used: the multi-rank tests look)
        return sub

    def coeffs_to_coset_rows(self, polys, dom, j, sub, halo):
        """the values of `polys` on coset j where THIS member of the coset's rank group needs them: member g transforms
        every G-th column (batched coset transforms) and the members exchange row slices (parallel.exchange_row_slices);
        returns full-size vectors valid on this member's rows and their halo"""
        group, G, g = sub
        count = len(polys)
        if count == 0:
            return []
        owners = [i % G for i in range(count)]
        done = self.coeffs_to_coset([p for p, o in zip(polys, owners) if o == g], dom, j)
        it = iter(done)
        cols = [next(it) if o == g else self.empty(dom.n) for o in owners]
        exchange_row_slices(cols, owners, dom.n, G, g, halo[0], halo[1], group=group, stream=self.tstream)
        return cols

    def intt_columns_begin(self, cols, dom, complete=True, keep=False):
        """lagrange_to_coeff of whole columns dealt round-robin over the ranks -- north_star's per-column NTT sharding
        (plonk/prover.rs:643-646 runs them as a par_iter) -- instead of every rank transforming every column: rank
        i mod P transforms column i and the coefficient vectors travel to the other ranks on the side stream
        (parallel.broadcast_columns_begin).  `complete` False: every rank holds only its row range of the columns (they
        were computed by ranges): the rows are gathered to the owner, not to everybody.  `keep`: the columns' Lagrange
        values stay as they are and the result is a new list.  Returns (coefficient columns, arrival): `arrival.wait()`
        before the compute stream reads them.  One device: plain transforms, arrival None."""
        n = dom.n
        if self.group_size <= 1:
            out = [self.clone(t) for t in cols] if keep else list(cols)
            return self.intt_many(out, dom), None
        owners = [self.column_owner(i) for i in range(len(cols))]
        lo, hi = self.row_range(n)
        if not complete and (lo, hi) != (0, n):
            for t, owner in zip(cols, owners):
                gather_rows_to(t, lo, hi, owner, group=self.group, stream=self.tstream)
        if keep:
            out = [self.clone(t) if owner == self.group_rank else self.empty(n) for t, owner in zip(cols, owners)]
        else:
            out = list(cols)
        self.intt_many([t for t, owner in zip(out, owners) if owner == self.group_rank], dom)
        arrival = broadcast_columns_begin(out, owners, group=self.bulk_group, stream=self.tstream, side=self.copy_stream)
        return out, arrival

    def coset_to_coeff(self, vals, dom, j):
        """in place: the polynomial of degree < n that takes the values `vals` on coset j (the inverse transform with
        1 / n and the powers of 1 / g_j fused into its last pass)"""
        tmp = self.empty(dom.n)
        g_inv = _inv(dom.g_coset * pow(dom.extended_omega, j, R_MOD) % R_MOD)
        check(self.L.h2_dev_coset_intt(vals.data_ptr(), tmp.data_ptr(), dom.k, _fr(g_inv), _fr(dom.omega_inv),
                                       _fr(dom.ifft_divisor), self.stream), "h2_dev_coset_intt")
        return vals

    # -- transforms -------------------------------------------------------------------------------------
    def intt(self, t, dom):
        """lagrange_to_coeff in place (poly/domain.rs:233-266)"""
        tmp = self.empty(dom.n)
        check(self.L.h2_dev_intt(t.data_ptr(), tmp.data_ptr(), _fr(dom.omega_inv), _fr(dom.ifft_divisor), dom.k,
                                 self.stream), "h2_dev_intt")
        return t

    def _side_stream(self):
        """the process's side stream of this GPU (see the streams' note in __init__)"""
        if "side" not in self._streams:
            self._streams["side"] = self.torch.cuda.Stream(device=self.dev, priority=self._prio[1])
        return self._streams["side"]

    def intt_on_side_stream(self, cols, dom, extend=False):
        """coefficient forms of `cols` (left untouched) -- and with `extend` their values on the extended domain --
        computed on the side stream, behind what is queued on the compute stream now; returns (copies, extended or None,
        event): the compute stream must wait for the event before it reads them.  The transforms then fill the issue
        slots that the latency-bound tails of the commitments in between leave."""
        if self._side is None:
            self._side = (self._side_stream(), concurrent.futures.ThreadPoolExecutor(max_workers=1))
        side = self._side[0]
        ready = self.torch.cuda.Event()
        ready.record(self.tstream)
        side.wait_event(ready)
        out = []
        with self.torch.cuda.stream(side):
            sptr = _vp(side.cuda_stream)
            out = [t.clone() for t in cols]
            if len(out) >= 2:
                width = self._batch_width(dom.n)
                tmp = self.torch.empty((min(len(out), width) * dom.n, 4), dtype=self.torch.int64, device=self.dev)
                for at in range(0, len(out), width):
                    part = out[at:at + width]
                    ptrs = (_vp * len(part))(*[c.data_ptr() for c in part])
                    check(self.L.h2_dev_intt_batch(ptrs, len(part), tmp.data_ptr(), _fr(dom.omega_inv), _fr(dom.ifft_divisor),
                                                   dom.k, sptr), "h2_dev_intt_batch")
                tmp.record_stream(self.tstream)
            else:
                for c in out:
                    tmp = self.torch.empty_like(c)
                    check(self.L.h2_dev_intt(c.data_ptr(), tmp.data_ptr(), _fr(dom.omega_inv), _fr(dom.ifft_divisor), dom.k,
                                             sptr), "h2_dev_intt")
            for c in out:
                c.record_stream(self.tstream)
            ext = None
            if extend:
                ext = self.coeffs_to_extended(out, dom, stream=sptr)
                for e in ext:
                    e.record_stream(self.tstream)
            done = self.torch.cuda.Event()
            done.record(side)
        return out, ext, done

    def coeff_to_extended(self, t, dom, out=None, stream=None):
        """`stream`: a caller's side stream (a raw handle; the caller is inside its torch.cuda.stream context, so the buffers
        made here belong to it) -- the launch must be on the stream the input was produced on, not on the compute stream"""
        if stream is None:
            out = out if out is not None else self.empty(dom.extended_n)
            tmp = self.empty(dom.extended_n)
        else:
            out = out if out is not None else self.torch.empty((dom.extended_n, 4), dtype=self.torch.int64, device=self.dev)
            tmp = self.torch.empty((dom.extended_n, 4), dtype=self.torch.int64, device=self.dev)
        check(self.L.h2_dev_coeff_to_extended(t.data_ptr(), out.data_ptr(), tmp.data_ptr(), dom.k, dom.extended_k,
                                              _fr(dom.g_coset), _fr(dom.g_coset_inv), _fr(dom.extended_omega),
                                              self.stream if stream is None else stream), "h2_dev_coeff_to_extended")
        return out

    def coeffs_to_extended(self, ts, dom, stream=None):
        """coeff_to_extended of several coefficient vectors: up to 16 per launch while the extended domain is small enough
        for that to matter (<= 2^23 points: a pass over one vector does not keep the chip busy; the scratch is 16 extended
        vectors), one by one above"""
        count = len(ts)
        if count < 2 or dom.extended_k > 23:
            return [self.coeff_to_extended(t, dom, stream=stream) for t in ts]
        torch = self.torch
        # (allocations belong to the stream they are made under: the caller's side stream, or the compute stream)
        width = self._batch_width(dom.extended_n, 2 << 30)
        with (torch.cuda.stream(self.tstream) if stream is None else contextlib.nullcontext()):
            outs = [torch.empty((dom.extended_n, 4), dtype=torch.int64, device=self.dev) for _ in ts]
            tmp = torch.empty((min(count, width) * dom.extended_n, 4), dtype=torch.int64, device=self.dev)
        for at in range(0, count, width):
            part = min(width, count - at)
            src = (_vp * part)(*[t.data_ptr() for t in ts[at:at + part]])
            dst = (_vp * part)(*[o.data_ptr() for o in outs[at:at + part]])
            check(self.L.h2_dev_coeff_to_extended_batch(src, dst, part, tmp.data_ptr(), dom.k, dom.extended_k, _fr(dom.g_coset),
                                                        _fr(dom.g_coset_inv), _fr(dom.extended_omega),
                                                        self.stream if stream is None else stream), "h2_dev_coeff_to_extended_batch")
        return outs

    def extended_to_coeff(self, t, dom):
        tmp = self.empty(dom.extended_n)
        check(self.L.h2_dev_extended_to_coeff(t.data_ptr(), tmp.data_ptr(), dom.extended_k, _fr(dom.g_coset),
                                              _fr(dom.g_coset_inv), _fr(dom.extended_omega_inv),
                                              _fr(dom.extended_ifft_divisor), self.stream), "h2_dev_extended_to_coeff")
        return t

    # -- commitments ------------------------------------------------------------------------------------
    def msm(self, scalars, bases, n, max_bits=254):
        """[Params::commit / commit_lagrange(_with_bound)] over device-resident bases -> affine point"""
        return self.msm_batch([scalars], bases, n, max_bits)[0]

    def msm_async(self, scalars, bases, n, max_bits=254):
        """One commitment on a SIDE stream, driven by a helper thread (the C call blocks until its result is back): the
        caller's stream goes on with other work and collects the point with `.result()`.  Only what is already queued
        on the compute stream is waited for.  One device only: a process group keeps its collectives in program order."""
        if self.group_size > 1 or self.force_collective:
            point = self.msm(scalars, bases, n, max_bits)
            fut = concurrent.futures.Future()
            fut.set_result(point)
            return fut
        if self._side is None:
            self._side = (self._side_stream(), concurrent.futures.ThreadPoolExecutor(max_workers=1))
        side, pool = self._side
        ready = self.torch.cuda.Event()
        ready.record(self.tstream)
        side.wait_event(ready)
        nbytes = self.L.h2_msm_scratch_bytes(n, max_bits)
        if self._side_scratch is None or self._side_scratch.numel() < nbytes:
            self._side_scratch = self.torch.empty(nbytes, dtype=self.torch.uint8, device=self.dev)
        scratch = self._side_scratch

        def run():
            self.torch.cuda.set_device(self.dev)
            out = np.zeros(12, dtype=np.uint64)
            check(self.L.h2_dev_msm(scalars.data_ptr(), bases.data_ptr(), n, max_bits, scratch.data_ptr(), nbytes,
                                    out.ctypes.data, _vp(side.cuda_stream)), "h2_dev_msm")
            return jacobian_to_affine(out)

        return pool.submit(run)

    def msm_batch(self, columns, bases, n, max_bits=254, also=None):
        """one MSM per column over the same bases (max_bits: one bound or one per column), pipelined inside the
        library; `also` = (scalars, other bases) is one more MSM over a different table in the same pipeline.  With a process group (one process per GPU, every rank holding the same
        polynomials) each MSM is split into contiguous ranges over the ranks -- gpu_multiexp_bound's split
        (arithmetic.rs:413-440) -- and the partial points are all-gathered and folded (parallel.py)."""
        if not columns and not also:
            return []
        lo, hi = 0, n
        collective = self.group_size > 1 or self.force_collective
        if collective:
            lo, hi = msm_split_range(n, self.group_size, self.group_rank)
        out = self.msm_partial(columns, bases, lo, hi, max_bits, also)
        if collective:
            out = allgather_fold_many(out, group=self.group, device=self.dev, stream=self.tstream)
        return jacobians_to_affine(out)

    def msm_partial(self, columns, bases, lo, hi, max_bits=254, also=None):
        """the MSMs restricted to the index range [lo, hi): raw Jacobian results, (count (+1), 12) u64.
        max_bits: one bound for every column or a list with one bound per column."""
        items = [(c, bases, b) for c, b in zip(columns, max_bits if isinstance(max_bits, (list, tuple)) else
                                               [max_bits] * len(columns))]
        if also:
            items.append((also[0], also[1], 254))
        count, m = len(items), hi - lo
        per = max((self.L.h2_msm_scratch_bytes(m, b) + 255) // 256 * 256 for b in {b for _, _, b in items})
        groups = {}
        for _, bs, b in items:                      # columns over one table with one bound can be fused by the library
            groups[(bs.data_ptr(), b)] = groups.get((bs.data_ptr(), b), 0) + 1
        nbytes = max([2 * per] + [self.L.h2_msm_batch_scratch_bytes(m, b, cnt) for (_, b), cnt in groups.items()])
        scratch = self.scratch(nbytes)
        out = np.zeros((count, 12), dtype=np.uint64)
        if count == 1:
            c, bs, b = items[0]
            check(self.L.h2_dev_msm(c.data_ptr() + 32 * lo, bs.data_ptr() + 64 * lo, m, b, scratch.data_ptr(), per,
                                    out.ctypes.data, self.stream), "h2_dev_msm")
        elif count > 1:
            sp = (_vp * count)(*[c.data_ptr() + 32 * lo for c, _, _ in items])
            bp = (_vp * count)(*[bs.data_ptr() + 64 * lo for _, bs, _ in items])
            bits = (ctypes.c_uint32 * count)(*[b for _, _, b in items])
            check(self.L.h2_dev_msm_batch_ex(sp, bp, bits, count, m, scratch.data_ptr(), nbytes, out.ctypes.data,
                                             self.stream), "h2_dev_msm_batch_ex")
        return out

    # -- elementwise / scans ----------------------------------------------------------------------------
    def eval_op(self, op, res, l=None, r=None, c=None, size=None):
        size = size if size is not None else res.shape[0]
        check(self.L.h2_dev_eval_op(op, res.data_ptr(), l.data_ptr() if l is not None else None,
                                    r.data_ptr() if r is not None else None, 0, 0, size,
                                    _fr(c) if c is not None else None, self.stream), "h2_dev_eval_op")
        return res

    def eval_polynomial(self, t, n, x):
        out = _FR()
        check(self.L.h2_dev_eval_polynomial(t.data_ptr(), n, _fr(x), out, self.stream), "h2_dev_eval_polynomial")
        return fr_from_mont_limbs(out)

    def eval_polynomial_batch(self, polys, n, points):
        """[poly_j(point_j)]: enqueued back to back, one read-back (the par_iter of plonk/prover.rs:731-737)"""
        count = len(polys)
        if count == 0:
            return []
        ptrs = (_vp * count)(*[p.data_ptr() for p in polys])
        pts = np.array([fr_to_mont_limbs(x % R_MOD) for x in points], dtype=np.uint64)
        out = np.zeros((count, 4), dtype=np.uint64)
        check(self.L.h2_dev_eval_polynomial_batch(ptrs, count, n, pts.ctypes.data, out.ctypes.data, self.stream),
              "h2_dev_eval_polynomial_batch")
        return [fr_from_mont_limbs(r) for r in out]

    def lincomb(self, res, polys, coeffs, size):
        ptrs = (_vp * len(polys))(*[p.data_ptr() for p in polys])
        cf = np.array([fr_to_mont_limbs(c % R_MOD) for c in coeffs], dtype=np.uint64)
        check(self.L.h2_dev_lincomb(res.data_ptr(), ptrs, cf.ctypes.data, len(polys), size, self.stream),
              "h2_dev_lincomb")
        return res

    def kate_division(self, a, n, b, out):
        """out[0 : n-1] = a / (X - b); out[n-1] = 0  (arithmetic.rs:754-773, resized as shplonk/prover.rs:112)"""
        check(self.L.h2_dev_kate_division(a.data_ptr(), n, _fr(b), out.data_ptr(), self.stream), "h2_dev_kate_division")
        with self.torch.cuda.stream(self.tstream):
            out[n - 1:n] = 0
        return out

    def sub_low(self, t, low):
        """t[i] -= low[i] for the first few coefficients"""
        if not low:
            return
        cur = self.get_rows(t, 0, len(low))
        self.set_rows(t, 0, [(c - l) % R_MOD for c, l in zip(cur, low)])

    # -- index-range sharding of the O(n) passes (one proof over several ranks) ------------------
    def row_range(self, n):
        """[lo, hi): the rows / coefficients of an n-vector this rank works on -- the contiguous range its share of every
        range-split MSM consumes (arithmetic.rs:425-435) -- or the whole vector on one device.  Vectors stay full-size
        allocations; a rank only ever computes and reads its own range of the ones that are sharded."""
        if self.group_size > 1 and n % self.group_size == 0 and n // self.group_size >= 8:
            return msm_split_range(n, self.group_size, self.group_rank)
        return 0, n

    def _exchange(self, values):
        return allgather_scalars(values, group=self.group, device=self.dev)

    def prefix_scan(self, f, n, init, product, probe):
        """z[0] = init, z[i] = z[i-1] * f[i-1] (product) / + f[i-1]: the grand-product / grand-sum columns
        (permutation/prover.rs:151-160, logup/prover.rs:353-367, shuffle/prover.rs).  Returns (z, z[probe]).
        Sharded: `f` is this rank's rows [lo, hi) of the factors / terms (hi - lo elements); the local scan starts from the
        neutral element, the totals of the ranges cross in ONE all-gather of a field element per rank and the range is
        corrected by the value entering it.  z is a full-size vector valid on [lo, hi) (`gather_rows` completes it)."""
        lo, hi = self.row_range(n)
        kernel = self.L.h2_dev_prefix_product if product else self.L.h2_dev_prefix_sum
        z = self.empty(n)
        if (lo, hi) == (0, n):
            check(kernel(f.data_ptr(), n, _fr(init), z.data_ptr(), self.stream), "h2_dev_prefix_scan")
            return z, self.get_rows(z, probe, 1)[0]
        m = hi - lo
        tmp = self.empty(m + 1)                      # tmp[t] = f[lo] .. f[lo + t - 1] folded; tmp[m] = this range's total
        check(kernel(f.data_ptr(), m + 1, _fr(1 if product else 0), tmp.data_ptr(), self.stream), "h2_dev_prefix_scan")
        total = self.get_rows(tmp, m, 1)[0]
        at = self.get_rows(tmp, probe - lo, 1)[0] if lo <= probe < hi else 0
        gathered = self._exchange([total, at])
        carries = scan_carries([g[0] for g in gathered], init, product)
        self.eval_op(OP_MUL_C if product else OP_SUM_C, z[lo:hi], tmp[:m], c=carries[self.group_rank], size=m)
        owner = probe // m
        value = carries[owner] * gathered[owner][1] % R_MOD if product else (carries[owner] + gathered[owner][1]) % R_MOD
        return z, value

    def gather_rows(self, t, n):
        """complete a vector of which every rank computed its own range (all-gather over xGMI)"""
        lo, hi = self.row_range(n)
        if (lo, hi) != (0, n):
            allgather_rows(t[:n], lo, hi, group=self.group, stream=self.tstream)
        return t

    def eval_polynomial_ranges(self, polys, n, points):
        """[poly_j(point_j)] with every polynomial cut into the ranks' coefficient ranges: p(x) = sum_r x^(lo_r) p_r(x);
        the partial values cross in one all-gather of len(polys) field elements per rank.  `polys` need only be valid on
        this rank's range."""
        lo, hi = self.row_range(n)
        if (lo, hi) == (0, n):
            return self.eval_polynomial_batch(polys, n, points)
        m = hi - lo
        parts = self.eval_polynomial_batch([p[lo:hi] for p in polys], m, points)
        gathered = self._exchange(parts)
        return [combine_range_evals([g[j] for g in gathered], points[j] % R_MOD, m) for j in range(len(polys))]

    def lincomb_range(self, res, polys, coeffs, n):
        """res[lo:hi) = sum_j coeffs[j] * polys[j][lo:hi) over this rank's range (the whole vector on one device)"""
        lo, hi = self.row_range(n)
        self.lincomb(res[lo:hi], [p[lo:hi] for p in polys], coeffs, hi - lo)
        return res

    def sub_low_range(self, t, low, n):
        """t[i] -= low[i] for the first few coefficients: they live in the first rank's range"""
        lo, hi = self.row_range(n)
        assert len(low) <= hi - lo
        if lo == 0:
            self.sub_low(t, low)

    def kate_division_ranges(self, a, n, b, out):
        """out = a / (X - b) (arithmetic.rs:754-773; out[n-1] = 0), `a` valid on this rank's range, `out` filled on it:
        out[j] = sum_{t > j} a[t] b^(t - j - 1).  The part of the sum inside the range is the same kernel on the range; the
        part above it is C b^(hi - 1 - j) with C = the recurrence value entering the range from above -- the local Horner
        values of the ranges at b cross in one all-gather, C follows on the host (parallel.kate_carries)."""
        lo, hi = self.row_range(n)
        if (lo, hi) == (0, n):
            return self.kate_division(a, n, b, out)
        m = hi - lo
        self.kate_division(a[lo:hi], m, b, out[lo:hi])               # the last coefficient of the range is zeroed
        part = self.eval_polynomial(a[lo:hi], m, b)
        carry = kate_carries([g[0] for g in self._exchange([part])], b % R_MOD, m)[self.group_rank]
        if carry:
            b %= R_MOD
            if b == 0:                                                # only out[hi - 1] = C
                self.set_rows(out, hi - 1, [carry])
            else:
                corr = self.eval_op(OP_CONSTANT, self.empty(m), c=carry * pow(b, m - 1, R_MOD) % R_MOD)
                check(self.L.h2_dev_distribute_powers(corr.data_ptr(), m, _fr(_inv(b)), self.stream), "h2_dev_distribute_powers")
                self.eval_op(OP_SUM, out[lo:hi], out[lo:hi], corr, size=m)
        return out


def sharding_description(device):
    """how one proof is spread over the ranks of `device`'s process group (bench.py reports it)"""
    if device.group_size <= 1 and not device.force_collective:
        return "one proof on one device"
    return ("one proof over %d rank(s): every MSM range-split over the ranks (partial points: one all-gather per batch, folded "
            "on the device); extended-domain phase (coset NTTs, evaluate_h, vanishing division, inverse transform) split by "
            "coset of the n-th roots of unity, the per-coset quotients scattered as coefficient ranges; the O(n) passes of the "
            "permutation / lookup / shuffle products (terms, batch inversion, prefix scans), the evaluations and the multiopen "
            "argument (linear combinations, Kate divisions) on the rank's row / coefficient range, one field element per rank "
            "exchanged per scan / division / evaluation batch; witness-dependent inverse transforms dealt by column (rows to "
            "the owner, coefficient vectors broadcast on a second communicator and a side stream); with more ranks than cosets "
            "the ranks of a coset deal its columns for the coset transforms, exchange row slices and evaluate the quotient by "
            "row range; lookup inputs compressed by rows, multiplicities all-reduced as integer counts" % device.group_size)


def g1_ntt(device, points, k, inverse):
    """h2_dev_g1_ntt on a (2^k, 8) device tensor of affine Montgomery points -> a new tensor: inverse = True gives
    n^-1 sum_j w^(-ij) points[j] (the Lagrange basis from the powers), False sum_j w^(ij) points[j]; w = Domain(k, _).omega"""
    D, torch = device, device.torch
    n = 1 << k
    with torch.cuda.stream(D.tstream):
        out = torch.empty((n, 8), dtype=torch.int64, device=D.dev)
        scratch = torch.empty(D.L.h2_g1_ntt_scratch_bytes(k), dtype=torch.uint8, device=D.dev)
    check(D.L.h2_dev_g1_ntt(points.data_ptr(), out.data_ptr(), k, int(bool(inverse)), scratch.data_ptr(), scratch.numel(),
                            D.stream), "h2_dev_g1_ntt")
    return out


def max_scalar_bits(col):
    """find_max_scalar_bits (plonk/prover.rs:237-254) on a canonical (n, 4) u64 column"""
    for limb in (3, 2, 1, 0):
        m = int(col[:, limb].max())
        if m:
            return 64 * limb + m.bit_length()
    return 0
