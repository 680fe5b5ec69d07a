"""Run in a child process (tests/test_gpu_stream_contract.py): two threads, each ROUNDS back-to-back calls of one
stream_cases.py adapter on a stream of its own, every result compared with its reference after a final synchronisation.

    stream_pair_worker.py ROOT LEFT RIGHT ROUNDS

LEFT / RIGHT: adapter names; RIGHT may be `host_kate_division`: the host-slice h2_kate_division over RIGHT's numpy arrays, which
the parent starts with H2_HOST_SLOTS=1 so that slot 0 -- whose scratch the h2_dev_* calls borrow -- serves it.  A process of its
own because the slot count is read once.  Prints `PAIR {"left": [...], "right": [...]}`: per side the rounds that differed."""
import json
import sys

import numpy as np

sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")

import torch  # noqa: E402

import halo2_gpu_specific_amd as h2  # noqa: E402
import stream_cases as S  # noqa: E402
import stream_device as D  # noqa: E402

left, right, rounds = sys.argv[2], sys.argv[3], int(sys.argv[4])
L = h2.lib()
streams = [torch.cuda.Stream(), torch.cuda.Stream()]


class HostKate:
    """h2_kate_division over host vectors, shaped like a Bound for run_pair"""

    in_place = False

    def __init__(self, case):
        self.adapter, self.case, self.L = S.BY_NAME["kate_division"], case, L
        self.a = np.array(case.inputs["a"], order="C")
        self.q = [np.zeros_like(case.expect["q"]) for _ in range(rounds)]
        self.r = 0

    def call(self, stream):
        q = self.q[self.r]
        self.r += 1
        return L.h2_kate_division(self.a.ctypes.data, self.case.dims["n"], self.case.p["b"].ctypes.data, q.ctypes.data), {}

    def snapshot(self, r):
        pass

    def mismatches(self, r, host=None):
        differ = int((self.q[r] != self.case.expect["q"]).any(axis=1).sum())
        return ["q: %d of %d elements differ" % (differ, len(self.q[r]))] if differ else []


def bound(name, seed):
    if name == "host_kate_division":
        b = HostKate(S.built("kate_division", seed))
        assert b.call(None)[0] == 0 and b.mismatches(0) == []           # warm: the slot's buffers have this size now
        b.r = 0
        return b
    b = D.Bound(S.BY_NAME[name], S.built(name, seed), L, snapshots=rounds)
    D.warm(b, streams[seed - 1])
    return b


sides = [(bound(left, 1), streams[0]), (bound(right, 2), streams[1])]
torch.cuda.synchronize()
failed = D.run_pair(sides, rounds)
print("PAIR " + json.dumps({"left": failed[0], "right": failed[1]}))
