"""Device plumbing shared by tests/test_gpu_hash_tables.py and tests/test_gpu_check_kernels.py: columns on the device and the
caller-owned block of the h2_dev_check_* entry points (a caller-zeroed u64 count, then `cap` h2_check_records), filled with a
sentinel so that a record written where none belongs shows."""
import numpy as np
import torch

SENTINEL = 0x5A5A5A5A
SLACK = 8                   # records' worth of sentinel kept behind the `cap` the library is told about
H2_CHECK_GATE, H2_CHECK_LOOKUP, H2_CHECK_SHUFFLE, H2_CHECK_COPY = 0, 1, 2, 3
CIRCUIT = 3


def dev(a):
    """(n, 4) uint64 -> device tensor (of a copy: a case's arrays are read-only); ready when this returns"""
    t = torch.from_numpy(np.array(a, dtype=np.uint64, order="C").view(np.int64)).cuda()
    torch.cuda.synchronize()
    return t


def dev_u32(a):
    t = torch.from_numpy(np.array(a, dtype=np.uint32, order="C").view(np.int32)).cuda()
    torch.cuda.synchronize()
    return t


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy().view(np.uint64)


def host_u32(t):
    torch.cuda.synchronize()
    return t.cpu().numpy().view(np.uint32)


class Records:
    """[u64 count = 0, 8 B pad][(cap + SLACK) x 16 B of SENTINEL]"""

    def __init__(self, cap):
        self.cap = cap
        self.blob = torch.full((4 + 4 * (cap + SLACK),), SENTINEL, dtype=torch.int32, device="cuda")
        self.blob[:4] = 0
        torch.cuda.synchronize()
        self.count_ptr = self.blob.data_ptr()
        self.ptr = self.blob.data_ptr() + 16
        self.out = (self.count_ptr, self.ptr, cap)

    def read(self):
        """(count, the whole record area as an (cap + SLACK, 4) uint32 array)"""
        words = host_u32(self.blob)
        return int(words[:2].copy().view(np.uint64)[0]), words[4:].reshape(-1, 4).copy()

    def check(self, want, kind):
        """the block after ONE call that should have appended the records `want` ((index, sub, row) tuples, all of `kind`):
        the count is exact whatever cap is; the first min(cap, total) slots hold distinct members of `want`, all of them when
        cap allows; every slot behind them still holds the sentinel"""
        total, recs = self.read()
        assert total == len(want), (total, len(want))
        kept = min(self.cap, total)
        got = [tuple(int(x) for x in r) for r in recs[:kept]]
        assert all(g[0] == kind for g in got), got[:4]
        body = [g[1:] for g in got]
        assert len(set(body)) == kept and set(body) <= set(want)
        if self.cap >= total:
            assert sorted(body) == sorted(want)
        assert (recs[kept:] == SENTINEL).all()
        return sorted(body)
