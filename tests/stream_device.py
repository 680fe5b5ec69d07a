"""Device plumbing of the stream-contract tests (tests/test_gpu_stream_contract.py and its worker process): the tensors of a
stream_cases.py case on the device, one call of its adapter on a stream, and two threads that run calls on streams of their own.

Every tensor is allocated when a Bound is made -- nothing is allocated while work is queued -- and kept until the Bound goes.
Outputs are compared ON the device, bit for bit (a mismatch reports how many elements differ); the adapters whose bytes are not
determined (unordered records, a Jacobian point) come down and are normalised first."""
import threading
import time

import numpy as np
import torch

_TORCH = {np.dtype(np.uint64): np.int64, np.dtype(np.uint32): np.int32, np.dtype(np.uint8): np.uint8}


def to_device(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(np.array(a, order="C").view(_TORCH[a.dtype])).cuda()


class Bound:
    """one case of one adapter with its tensors: `t` what the calls read and write, `pristine` the inputs as built, `want`
    the expected outputs, `snaps[r]` where the outputs of call r are kept"""

    def __init__(self, adapter, case, L, snapshots=1):
        self.adapter, self.case, self.L = adapter, case, L
        self.pristine = {k: to_device(v) for k, v in case.inputs.items()}
        self.t = {k: v.clone() for k, v in self.pristine.items()}
        for k, (shape, dtype) in case.like.items():
            self.t[k] = torch.zeros(shape, dtype=getattr(torch, np.dtype(_TORCH[np.dtype(dtype)]).name), device="cuda")
        for k, nbytes in case.scratch.items():
            self.t[k] = torch.zeros(max(int(nbytes(L)), 8), dtype=torch.uint8, device="cuda")
        self.ptr = {k: v.data_ptr() for k, v in self.t.items()}
        self.want = {k: to_device(case.expect[k]) for k in adapter.outputs}
        self.snaps = [{k: torch.zeros_like(self.t[k]) for k in adapter.outputs} for _ in range(snapshots)]
        self.in_place = any(k in case.inputs for k in adapter.outputs)

    def load(self, source):
        """queue copies of `source` (name -> device tensor: this case's pristine inputs, or a decoy's) over the inputs"""
        for k, v in source.items():
            self.t[k].copy_(v, non_blocking=True)

    def call(self, stream):
        return self.adapter.call(self.L, stream.cuda_stream, self.ptr, self.case)

    def snapshot(self, r=0):
        for k, v in self.snaps[r].items():
            v.copy_(self.t[k], non_blocking=True)

    def mismatches(self, r=0, host=None):
        """after a synchronisation: [] or what differs in the outputs kept by snapshot r (and in the host results `host`)"""
        a, case, bad = self.adapter, self.case, []
        if a.normalised:
            got = a.normalise(case, {k: v.cpu().numpy().view(case.expect[k].dtype) for k, v in self.snaps[r].items()})
            exp = a.normalise(case, dict(case.expect))
            bad += ["%s differs" % k for k in got if not np.array_equal(np.asarray(got[k]).reshape(-1), np.asarray(exp[k]).reshape(-1))]
        else:
            for k, v in self.snaps[r].items():
                differ = int((v != self.want[k]).sum())
                if differ:
                    bad.append("%s: %d of %d words differ" % (k, differ, v.numel()))
        if host is not None:
            got, exp = a.normalise(case, dict(host)), a.normalise(case, dict(case.host))
            bad += ["host result %s: %s, expected %s" % (k, got[k], exp[k]) for k in exp if not np.array_equal(got[k], exp[k])]
        return bad


def warm(bound, stream):
    """one call with the whole device synchronised on either side of it, checked: plans are published, programs compiled and
    the library's buffers grown to this size.  No test of stream order: whatever stream the call used, its inputs were ready
    and its work has run."""
    with torch.cuda.stream(stream):
        bound.load(bound.pristine)
        torch.cuda.synchronize()
        rc, host = bound.call(stream)
        torch.cuda.synchronize()
        bound.snapshot(0)
        bound.load(bound.pristine)
    stream.synchronize()
    assert rc == 0, (bound.adapter.name, rc, bound.L.h2_last_error())
    assert bound.mismatches(0) == [], bound.adapter.name       # (host results are (a)'s to judge: they are read as the call returns)


def run_side(bound, stream, rounds, results, errors, go):
    """`rounds` back-to-back calls on `stream` (inputs restored in between only where a call works in place)"""
    try:
        go.wait()
        with torch.cuda.stream(stream):
            for r in range(rounds):
                if bound.in_place and r:
                    bound.load(bound.pristine)
                rc, host = bound.call(stream)
                results.append((rc, host))
                bound.snapshot(r)
        stream.synchronize()
    except Exception as exc:  # noqa: BLE001
        errors.append(repr(exc))


def run_pair(sides, rounds):
    """sides: two (Bound made with snapshots >= rounds, stream).  Both threads start together.  -> per side the list of
    (round, what differed) -- empty when every one of its `rounds` results is its reference's"""
    go = threading.Event()
    results, errors = [[], []], []
    threads = [threading.Thread(target=run_side, args=(b, s, rounds, results[i], errors, go)) for i, (b, s) in enumerate(sides)]
    for t in threads:
        t.start()
    go.set()
    for t in threads:
        t.join()
    torch.cuda.synchronize()
    assert not errors, errors
    failed = []
    for i, (b, _) in enumerate(sides):
        bad = []
        assert len(results[i]) == rounds
        for r, (rc, host) in enumerate(results[i]):
            what = (["status %d: %s" % (rc, b.L.h2_last_error())] if rc else []) + (b.mismatches(r, host) if rc == 0 else [])
            if what:
                bad.append((r, what))
        if b.in_place:
            with torch.cuda.stream(sides[i][1]):
                b.load(b.pristine)
            sides[i][1].synchronize()
        failed.append(bad)
    return failed


class Delay:
    """a bounded stretch of plain torch work on a stream: matrix products, calibrated once to last about `ms`"""

    def __init__(self, ms, stream):
        self.a = torch.rand((4096, 4096), dtype=torch.float32, device="cuda")
        self.b = torch.empty_like(self.a)
        begin, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(stream):
            self.queue(8)                                   # (the first product loads its kernel)
            begin.record(stream)
            self.queue(32)
            end.record(stream)
        stream.synchronize()
        self.unit_ms = begin.elapsed_time(end) / 32
        self.reps = max(1, int(ms / max(self.unit_ms, 1e-4)) + 1)
        self.ms = self.reps * self.unit_ms

    def queue(self, reps=None):
        for _ in range(self.reps if reps is None else reps):
            torch.mm(self.a, self.a, out=self.b)


def timed(f):
    t0 = time.perf_counter()
    out = f()
    return out, (time.perf_counter() - t0) * 1e3
