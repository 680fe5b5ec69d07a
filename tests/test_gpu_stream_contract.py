"""The h2_dev_* entry points on caller streams, as include/halo2_hip.h promises them: the stream argument is honoured, the
entry points that the header lists as waiting do wait and the others do not, and two threads on two streams get their own results.
Cases and references: tests/stream_cases.py (pinned to integer definitions by tests/test_stream_cases_host.py).

(a) test_stream_argument_is_honoured, one per adapter, deterministic.  On a stream S that is neither the library's nor torch's
    default: the inputs hold a DECOY (the adapter built from another seed: same shapes, other values); a bounded delay is queued;
    event E; copies of the real inputs; the call; copies of the outputs into snapshots; the decoy back.  A call that reads its
    inputs before its stream position, launches elsewhere, or whose outputs its stream position does not cover computes the
    decoy's answer.  E.query() when the call returns says whether it waited: Adapter.waits, the header's list.
(b) test_two_streams_at_once, a detector: two threads, ROUNDS back-to-back calls each on a stream of its own.

Measured on an MI355X: the delay is DELAY_MS = 80 ms of 4096^3 float matrix products, calibrated when the module starts (87
products of 0.92 ms: 80.1 ms); the enqueue of an entry point that does not wait, the copies of its inputs included, took
0.012 ms (random_fr) to 0.30 ms (evaluate_h on generated kernels, whose descriptor Python rebuilds per call; next: check_gates
0.13 ms, lincomb 0.10 ms), so the delay is more than 250 times the slowest and a sixth of half a second.  The calls that wait
returned 77 - 79 ms after the event was recorded.  ROUNDS = 16 a side; the whole module takes 7.5 s.

Safety: both sides of a pair and every decoy are valid inputs of identical shapes (the host test), so a mix-up gives wrong
values, never an index out of range; every tensor is allocated and every adapter warmed, synchronised, at its one size before
the first test, so no library buffer grows while work is queued; two threads, one process, plus one worker process."""
import json
import os
import subprocess
import sys

import pytest
import torch

import halo2_gpu_specific_amd as h2
import stream_cases as S
import stream_device as D
from h2util import ROOT

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]

DELAY_MS = 80
ROUNDS = 16
NAMES = [a.name for a in S.ADAPTERS]
PAIRS = [("kate_division", "kate_division"), ("kate_division", "eval_polynomial"), ("kate_division", "prefix_sum"),
         ("kate_division", "points_decompress"), ("evaluate_h_interpreter", "evaluate_h_interpreter"),
         ("evaluate_h_interpreter", "check_gates"),
         ("eval_op", "lincomb"), ("coset_ntt", "coset_ntt")]          # the last two are controls: they share nothing / one plan
PAIRED = {name for pair in PAIRS for name in pair}


class World:
    def __init__(self, L):
        self.L = L
        self.streams = [torch.cuda.Stream(), torch.cuda.Stream()]
        self.bounds, self.decoy = {}, {}
        for a in S.ADAPTERS:
            for seed in (1, 2) if a.name in PAIRED else (1,):
                self.bounds[(a.name, seed)] = D.Bound(a, S.built(a.name, seed), L, snapshots=ROUNDS if a.name in PAIRED else 1)
            self.decoy[a.name] = {k: D.to_device(v) for k, v in S.built(a.name, 2).inputs.items()}
        self.delay = D.Delay(DELAY_MS, self.streams[0])
        torch.cuda.synchronize()
        for (name, seed), b in self.bounds.items():
            D.warm(b, self.streams[seed - 1])
        torch.cuda.synchronize()


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    mp = pytest.MonkeyPatch()
    mp.setenv("H2_JIT_CACHE", str(tmp_path_factory.mktemp("jit")))
    w = World(h2.lib())
    yield w
    torch.cuda.synchronize()
    mp.undo()


@pytest.mark.parametrize("name", NAMES)
def test_stream_argument_is_honoured(world, name):
    a, b, decoy, stream = S.BY_NAME[name], world.bounds[(name, 1)], world.decoy[name], world.streams[0]
    reached = torch.cuda.Event()
    with torch.cuda.stream(stream):
        b.load(decoy)                                    # 1
        stream.synchronize()
        world.delay.queue()                              # 2
        reached.record(stream)                           # 3

        def enqueue():
            b.load(b.pristine)                           # 4
            return b.call(stream)                        # 5

        (rc, host), ms = D.timed(enqueue)
        delay_over = reached.query()
        b.snapshot(0)                                    # 6
        b.load(decoy)                                    # 7
    stream.synchronize()                                 # 8
    print("%s: enqueue %.3f ms, delay %.1f ms (%d products of %.3f ms), the delay was %s when the call returned"
          % (name, ms, world.delay.ms, world.delay.reps, world.delay.unit_ms, "over" if delay_over else "running"))
    with torch.cuda.stream(stream):
        b.load(b.pristine)
    stream.synchronize()
    assert rc == 0, world.L.h2_last_error()
    assert b.mismatches(0, host) == [], "the call did not compute from what its stream position holds"
    assert 2 * world.delay.ms < 500
    if a.waits:
        assert delay_over, "the header lists %s among the calls that wait for their stream; it returned while the delay was running" % a.entry
    else:
        assert not delay_over, ("%s returned after the delay: it waited for its stream, which the header says it does not -- or the "
                                "delay of %.1f ms is too short for an enqueue that took %.3f ms" % (a.entry, world.delay.ms, ms))


@pytest.mark.parametrize("left,right", PAIRS)
def test_two_streams_at_once(world, left, right):
    sides = [(world.bounds[(left, 1)], world.streams[0]), (world.bounds[(right, 2)], world.streams[1])]
    failed = D.run_pair(sides, ROUNDS)
    print("%s / %s: %d and %d of %d results differ" % (left, right, len(failed[0]), len(failed[1]), ROUNDS))
    assert failed == [[], []], "%d of %d results differ: %s" % (len(failed[0]) + len(failed[1]), 2 * ROUNDS, [f[:2] for f in failed])


def test_caller_stream_against_a_host_call_on_slot_0():
    """h2_dev_kate_division on a caller's stream while h2_kate_division runs on slot 0 (H2_HOST_SLOTS=1, read once: a process
    of its own, as tests/pool_split_worker.py)"""
    env = dict(os.environ, H2_HOST_SLOTS="1")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "stream_pair_worker.py"), ROOT, "kate_division",
                          "host_kate_division", str(ROUNDS)], env=env, capture_output=True, text=True, timeout=240)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    failed = json.loads(next(line for line in out.stdout.splitlines() if line.startswith("PAIR "))[5:])
    print("kate_division / host h2_kate_division: %d and %d of %d results differ" % (len(failed["left"]), len(failed["right"]), ROUNDS))
    assert failed == {"left": [], "right": []}
