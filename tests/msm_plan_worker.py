"""Runs rows of the MSM plan matrix (tests/msm_plan_cases.py) on the device: every row against the oracle's best_multiexp
(and, for n <= 256, the sum in Python integers), its launch record against what the row expects, and -- for rows that are one
launch -- the partition bases, bucket starts, heavy count and sorted entries the launch left in the scratch against the
digits recoded on the host.  tests/test_gpu_msm_plans.py imports the Runner; run as a script with the name of one of
msm_plan_cases.CHILDREN (one knob setting per child process, set before the library is loaded) it runs that setting's rows,
compares their records with the recorded ones and prints the branches they show."""
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
from h2util import arr_to_points, to_mont  # noqa: E402

import msm_plan_cases as mc  # noqa: E402

_NAMED = {"form": mc.FORMS, "partition": mc.PARTS, "finish": mc.FINISH, "reduce": mc.REDUCE}


class Runner:
    """points, tables and references are built once per (size, seed) and shared by the rows that use them"""

    def __init__(self, oracle):
        self.L = h2.lib()
        self.oracle = oracle
        self.dev = torch.device("cuda", 0)
        self.points = {}     # n -> (host array, device tensor)
        self.table = None    # (device pointer, digits) of the one table that exists at a time
        self.branches = set()
        self.classes = set()
        self.threads = min(16, os.cpu_count() or 1)

    # ---- plumbing
    def sync(self):
        torch.cuda.synchronize()
        check(self.L.h2_synchronize(), "h2_synchronize")

    def upload(self, a):
        return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).to(self.dev)

    def bases(self, n):
        if n not in self.points:
            pts = mc.build_points(self.oracle, 0x5EED + n, n)
            self.points[n] = (pts, self.upload(pts))
        return self.points[n]

    def use_table(self, d_pts, n, digits):
        want = (d_pts.data_ptr(), digits) if digits else None
        if self.table == want:
            return
        self.forget()
        if want:
            assert self.L.h2_dev_bases_precompute(d_pts.data_ptr(), n, digits, None) == 0, self.L.h2_last_error()
            self.table = want

    def forget(self):
        if self.table:
            assert self.L.h2_dev_bases_forget(self.table[0]) == 0
            self.table = None

    def affine(self, jac):
        return arr_to_points(self.oracle.to_affine(np.asarray(jac, dtype=np.uint64)))[0]

    def widths(self, row, bits):
        if row.digits:
            return mc.digit_widths(bits, digits=row.digits)
        c, W, nb = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32()
        assert self.L.h2_msm_shape(row.n, bits, ctypes.byref(c), ctypes.byref(W), ctypes.byref(nb)) == 0
        return mc.digit_widths(bits, W=W.value)

    # ---- one row
    def run(self, row):
        try:
            return self._run(row)
        except AssertionError as e:
            raise AssertionError("row '%s': %s" % (row.name, e)) from e

    def _run(self, row):
        L, n = self.L, row.n
        table_n = row.table_n or n
        pts_all, d_all = self.bases(table_n)
        pts = pts_all[row.lo:row.lo + n]
        d_bases = d_all.data_ptr() + 64 * row.lo
        dists = [row.dist] if row.kind == "single" else list(row.dist)
        bits = [row.bits - j if row.kind == "batch_ex" else row.bits for j in range(len(dists))]   # batch_ex: no two columns fuse
        cols = [mc.build_scalars(d, n, b, 0xC01 + 977 * j + n, self.widths(row, b)) for j, (d, b) in enumerate(zip(dists, bits))]
        scalars = [to_mont(v) for v in cols]
        d_cols = [self.upload(s) for s in scalars]
        old_min_n = os.environ.get("H2_MSM_TABLE_MIN_N")
        os.environ["H2_MSM_TABLE_MIN_N"] = "1"   # (read per call) tables are used from 2^15 rows on; the rows are smaller
        try:
            self.use_table(d_all, table_n, row.digits)
            count = len(cols)
            out = np.zeros((count, 12), dtype=np.uint64)
            self.sync()
            if row.kind == "single":
                nbytes = L.h2_msm_scratch_bytes(n, row.bits)
                scratch = torch.empty(max(nbytes, 256), dtype=torch.uint8, device=self.dev)
                rc = L.h2_dev_msm(d_cols[0].data_ptr(), d_bases, n, row.bits, scratch.data_ptr(), nbytes, out.ctypes.data, None)
            elif row.kind == "batch":
                nbytes = L.h2_msm_batch_scratch_bytes(n, row.bits, count)
                scratch = torch.empty(max(nbytes, 256), dtype=torch.uint8, device=self.dev)
                sp = (ctypes.c_void_p * count)(*[t.data_ptr() for t in d_cols])
                rc = L.h2_dev_msm_batch(sp, count, d_bases, n, row.bits, scratch.data_ptr(), nbytes, out.ctypes.data, None)
            else:
                lanes = row.expect.get("scratch_slices", 2)
                nbytes = lanes * max((L.h2_msm_scratch_bytes(n, b) + 255) // 256 * 256 for b in bits)
                scratch = torch.empty(nbytes, dtype=torch.uint8, device=self.dev)
                sp = (ctypes.c_void_p * count)(*[t.data_ptr() for t in d_cols])
                bp = (ctypes.c_void_p * count)(*[d_bases] * count)
                bb = (ctypes.c_uint32 * count)(*bits)
                rc = L.h2_dev_msm_batch_ex(sp, bp, bb, count, n, scratch.data_ptr(), nbytes, out.ctypes.data, None)
            assert rc == 0, L.h2_last_error()
            recs = mc.last_launches(L)
            self.sync()
        finally:
            if old_min_n is None:
                del os.environ["H2_MSM_TABLE_MIN_N"]
            else:
                os.environ["H2_MSM_TABLE_MIN_N"] = old_min_n
        # the group element, against the oracle and (small rows) against Python integers
        for j in range(count):
            got = self.affine(out[j])
            want = self.affine(self.oracle.best_multiexp(scalars[j], pts, threads=self.threads))
            assert got == want, "column %d (%s): the device gives %s, the oracle %s; records %s" % (j, dists[j], got, want, recs)
            if n <= mc.INT_CHECK_MAX_N:
                assert got == mc.int_msm(cols[j], arr_to_points(pts)), "column %d (%s) differs from the sum in Python integers" % (j, dists[j])
        self.expectations(row, recs, scratch)
        found = set()
        for rec in recs:
            self.branches |= mc.branches(rec)
        if len(recs) == 1:
            found = self.scratch_evidence(row, recs[0], scratch, cols, table_n)
            self.classes |= found
        missing = row.classes - found
        assert not missing, "the scratch shows no %s (it shows %s); record %s" % (sorted(missing), sorted(found), recs)
        return recs, found

    def expectations(self, row, recs, scratch):
        assert recs, "no launch was recorded"
        rec = recs[0]
        lo, hi = scratch.data_ptr(), scratch.data_ptr() + scratch.numel()
        for r in recs:
            assert lo <= r["scratch"] and r["scratch"] + r["total"] <= hi, "a launch's scratch slice lies outside the buffer: %s" % r
        for key, want in row.expect.items():
            if key == "launches":
                got = len(recs)
            elif key == "scratch_slices":
                got = len({r["scratch"] for r in recs})
            elif key == "hot_mask_bit":
                got, want = (rec["hot_mask"] >> want) & 1, 1
            elif key == "staged":
                got = rec["stage_cap"] != 0
            elif key == "RG>1":
                got = rec["RG"] > 1
            elif key == "R>1":
                got = rec["R"] > 1
            elif key in _NAMED:
                got = _NAMED[key][rec[key]]
            else:
                got = rec[key]
            assert got == want, "the record has %s = %s, the row exists for %s; records %s" % (key, got, want, recs)

    def scratch_evidence(self, row, rec, scratch, cols, table_n):
        """parts 3 (b) and (c): the call has synchronised and the buffer is this test's"""
        def words(off, count):
            base = rec["scratch"] - scratch.data_ptr() + off
            return scratch[base:base + 4 * count].cpu().numpy().view(np.uint32)

        pbase = words(rec["off_pbase"], rec["np"] + 1)
        starts = words(rec["off_starts"], rec["nbt"] + 1)
        heavy = int(words(rec["off_heavy"], 1)[0])
        assert int(starts[rec["nbt"]]) <= rec["entries"], "starts[nbt] = %d exceeds the %d entries" % (starts[rec["nbt"]], rec["entries"])
        found = mc.scratch_classes(rec, pbase, starts, heavy)
        if row.n <= mc.SORT_CHECK_MAX_N:
            entries = words(rec["off_sorted"], int(starts[rec["nbt"]]))
            mc.check_sort(rec, starts, entries, mc.recode(cols, rec, table_n if rec["form"] == 1 else 0))
        return found

    def run_rows(self, rows, child=None):
        for row in rows:
            recs, found = self.run(row)
            mc.check_golden(child, row, recs)
            print("ROW %s: %s %s" % (row.name, sorted(set().union(*[mc.branches(r) for r in recs])), sorted(found)), flush=True)
        self.forget()


def main():
    from h2util import Oracle

    name = sys.argv[1]
    _, env, rows, _ = next(c for c in mc.CHILDREN if c[0] == name)
    for k, v in env.items():
        assert os.environ.get(k) == v, "start this child with %s=%s" % (k, v)
    r = Runner(Oracle.get())
    try:
        r.run_rows(rows, child=name)
    finally:
        r.forget()
    print("BRANCHES %s" % " ".join(sorted(r.branches | {"class:" + c for c in r.classes})), flush=True)
    print("CHILD OK", flush=True)


if __name__ == "__main__":
    main()
