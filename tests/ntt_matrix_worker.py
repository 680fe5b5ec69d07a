"""Runs rows of the NTT matrix (tests/ntt_matrix_cases.py) on the device and compares every output vector with its expected
one, bit for bit.  tests/test_gpu_ntt_matrix.py imports the Runner; run as a script (one knob setting per child process:
the H2_NTT_* knobs are read once per process) it runs the thinned rows of every knob setting, compares them with the oracle
inside this process and prints the kernel ids h2_ntt_shape reported for them."""
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402  (before the library: both bind to one HIP runtime)

if torch.cuda.is_available():
    torch.cuda.init()

import halo2_gpu_specific_amd as h2  # noqa: E402
from halo2_gpu_specific_amd._lib import check  # noqa: E402
from h2util import fr_mont  # noqa: E402

import ntt_matrix_cases as mc  # noqa: E402


def _vp(a):
    return a.ctypes.data_as(ctypes.c_void_p)


class Runner:
    """the rows of one size: expected vectors are computed once (CPU), kept on the device and shared by every variant"""

    def __init__(self, oracle, log_n):
        self.L = h2.lib()
        self.log_n, self.n = log_n, 1 << log_n
        self.ref = mc.Reference(oracle, log_n)
        self.dev = torch.device("cuda", 0)
        self.tmp = None
        self.cache = {}
        self.kernels = set()
        r = self.ref
        self.fr = {k: fr_mont(v) for k, v in (("w", r.w), ("w_inv", r.w_inv), ("d", r.d), ("g", r.g), ("g_inv", r.g_inv))}

    def sync(self):
        # the library's default stream is not torch's: both, around every call
        torch.cuda.synchronize()
        check(self.L.h2_synchronize(), "h2_synchronize")

    def upload(self, a):
        return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).to(self.dev)

    def scratch(self, vectors=1):
        if self.tmp is None or self.tmp.shape[0] < vectors * self.n:
            self.tmp = None
            self.tmp = torch.empty((vectors * self.n, 4), dtype=torch.int64, device=self.dev)
        return self.tmp

    def prepare(self, case):
        """(input, expected) on the device"""
        if case not in self.cache:
            x, want = self.ref.expected(case)
            self.cache[case] = (self.upload(x), self.upload(want))
        self.kernels |= mc.kernel_ids(self.L, self.log_n, case.z)
        return self.cache[case]

    def constants(self, case):
        a, b = self.ref.constants(case)
        return fr_mont(a), fr_mont(b)

    def run(self, case, place):
        """one call of the entry point; returns the output vector (device)"""
        L, f, log_n, n = self.L, self.fr, self.log_n, self.n
        x, _ = self.prepare(case)
        tmp = self.scratch().data_ptr()
        if place == "in":
            buf = torch.full((n, 4), -1, dtype=torch.int64, device=self.dev)  # (what lies behind a short input is not read)
            buf[: len(x)] = x
            src = out = buf
        else:
            src = x.clone()
            out = torch.full((n, 4), -1, dtype=torch.int64, device=self.dev)
        self.sync()
        op = case.op
        if op == "ntt":
            rc = L.h2_dev_ntt(out.data_ptr(), tmp, _vp(f["w"]), log_n, None)
        elif op == "intt":
            rc = L.h2_dev_intt(out.data_ptr(), tmp, _vp(f["w_inv"]), _vp(f["d"]), log_n, None)
        elif op == "coeff_to_extended":
            a, b = self.constants(case)
            rc = L.h2_dev_coeff_to_extended(src.data_ptr(), out.data_ptr(), tmp, log_n - case.z, log_n, _vp(a), _vp(b), _vp(f["w"]), None)
        elif op == "extended_to_coeff":
            a, b = self.constants(case)
            rc = L.h2_dev_extended_to_coeff(out.data_ptr(), tmp, log_n, _vp(a), _vp(b), _vp(f["w_inv"]), _vp(f["d"]), None)
        elif op == "coset_ntt":
            rc = L.h2_dev_coset_ntt(src.data_ptr(), out.data_ptr(), tmp, log_n, _vp(f["g"]), _vp(f["w"]), None)
        elif op == "coset_intt":
            rc = L.h2_dev_coset_intt(out.data_ptr(), tmp, log_n, _vp(f["g_inv"]), _vp(f["w_inv"]), _vp(f["d"]), None)
        else:
            raise AssertionError(op)
        check(rc, "h2_dev_" + op)
        self.sync()
        if place == "out":
            assert torch.equal(src, x), ("an out-of-place transform wrote its source", log_n, case)
        return out

    def compare(self, got, want, what):
        if torch.equal(got, want):
            return
        bad = torch.nonzero((got != want).any(dim=1)).flatten()
        i = int(bad[0])
        raise AssertionError("%s: %d of %d outputs differ, the first at %d: got %s, expected %s" % (
            what, len(bad), len(want), i, got[i].cpu().numpy().view(np.uint64), want[i].cpu().numpy().view(np.uint64)))

    def run_cases(self, cases, calls=1, tag=""):
        for case in cases:
            _, want = self.prepare(case)
            for place in mc.PLACES[case.op]:
                for call in range(calls):
                    self.compare(self.run(case, place), want, "2^%d %s %s call %d%s" % (self.log_n, case, place, call, tag))

    def run_batch(self, bop, count, z=0):
        """`count` vectors, the input kinds in turn, through one batched call"""
        L, f, log_n, n = self.L, self.fr, self.log_n, self.n
        op = bop[: -len("_batch")]
        arbitrary = next(c.arbitrary for c in mc.matrix_cases(L, log_n) if c.op == op and c.z == z)
        cases = [mc.Case(op, z, mc.INPUTS[i % len(mc.INPUTS)], arbitrary) for i in range(count)]
        pairs = [self.prepare(c) for c in cases]
        tmp = self.scratch(min(count, 16)).data_ptr()
        srcs = [x.clone() for x, _ in pairs]
        in_place = bop in ("ntt_batch", "intt_batch")
        outs = srcs if in_place else [torch.full((n, 4), -1, dtype=torch.int64, device=self.dev) for _ in range(count)]
        sp = (ctypes.c_void_p * count)(*[t.data_ptr() for t in srcs])
        dp = (ctypes.c_void_p * count)(*[t.data_ptr() for t in outs])
        self.sync()
        if bop == "ntt_batch":
            rc = L.h2_dev_ntt_batch(dp, count, tmp, _vp(f["w"]), log_n, None)
        elif bop == "intt_batch":
            rc = L.h2_dev_intt_batch(dp, count, tmp, _vp(f["w_inv"]), _vp(f["d"]), log_n, None)
        elif bop == "coset_ntt_batch":
            rc = L.h2_dev_coset_ntt_batch(sp, dp, count, tmp, log_n, _vp(f["g"]), _vp(f["w"]), None)
        elif bop == "coeff_to_extended_batch":
            a, b = self.constants(cases[0])
            rc = L.h2_dev_coeff_to_extended_batch(sp, dp, count, tmp, log_n - z, log_n, _vp(a), _vp(b), _vp(f["w"]), None)
        else:
            raise AssertionError(bop)
        check(rc, "h2_dev_" + bop)
        self.sync()
        for i, (got, (x, want)) in enumerate(zip(outs, pairs)):
            self.compare(got, want, "2^%d %s of %d, z = %d, vector %d (%s)" % (log_n, bop, count, z, i, cases[i].inp))
            if not in_place:
                assert torch.equal(srcs[i], x), ("an out-of-place batch wrote its source", log_n, bop, count, i)


def main():
    from h2util import Oracle

    oracle = Oracle.get()
    L = h2.lib()
    kernels = set()
    for log_n in mc.CHILD_SIZES:
        r = Runner(oracle, log_n)
        r.run_cases(mc.child_cases(L, log_n), calls=2 if log_n >= 18 else 1)
        kernels |= r.kernels
        print("SHAPE %d %s" % (log_n, [(p["bits"], p["kernel"]) for p in mc.ntt_shape(L, log_n, log_n)]), flush=True)
        del r
        check(L.h2_release_plans(), "h2_release_plans")
    print("KERNELS %s" % " ".join(str(k) for k in sorted(kernels)), flush=True)
    print("CHILD OK", flush=True)


if __name__ == "__main__":
    main()
