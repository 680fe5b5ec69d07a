"""h2_dev_g1_fold (k_g1_fold, csrc/g1util.hip) called directly on a (world, count, 12) tensor of Jacobian partial points, on one GPU.

Under RCCL the fold runs only behind an all-gather, and with one GPU that is world = 1, where every fold is identity + P and
xyzz_add hands its operand back.  Here the partials are made in Python -- affine multiples of the generator under a generic z --
with the cases a fold can meet planted in the columns: an identity partial in the first, a middle and the last rank, a column of
identities only, one point in two ranks under different z (P + P: the doubling branch of xyzz_add, also as A, B, A + B), and a
point with its negative next to it and with another point between them (also as P, Q, -(P + Q)).  The sum of every column is
compared as a group element with the affine sum in Python integers (ref_plonk.g1_add), and its 96 bytes with the host twin
h2_g1_sum: both compile the same ec.hpp, and parallel.allgather_fold_many relies on every rank deriving one representation.
"""
import functools
import random

import numpy as np
import pytest

from ref_plonk import G1, Q, R as R_MOD, g1_add, g1_mul, g1_neg

RM = 1 << 256
SEED = 0xF01D
WORLDS = [1, 2, 3, 8]
COUNTS = [1, 63, 64, 65, 130]            # the kernel's block is 64 lanes, one lane per column
PLANS = ["generic", "identity-first", "identity-middle", "identity-last", "all-identity", "same-point", "sum-of-two",
         "negative-adjacent", "negative-apart", "negative-of-two"]


@functools.lru_cache(maxsize=None)
def point_pool():
    rnd = random.Random(SEED)
    return [G1] + [g1_mul(G1, rnd.randrange(1, R_MOD)) for _ in range(31)]


def jacobian(P, z):
    """the affine point P as (x z^2, y z^3, z) in Montgomery form; None, the identity, as z = 0 under leftover coordinates"""
    c = (5, 7, 0) if P is None else (P[0] * z * z % Q, P[1] * z * z * z % Q, z)
    return np.array([(v * RM % Q) >> (64 * i) & 0xFFFFFFFFFFFFFFFF for v in c for i in range(4)], dtype=np.uint64)


def column(plan, world, rnd):
    """the partial points of one column, rank by rank, as affine points (None: the identity)"""
    pool = point_pool()
    pts = rnd.sample(pool, world)
    P = pts[0]
    if plan == "identity-first":
        pts[0] = None
    elif plan == "identity-middle":
        pts[world // 2] = None
    elif plan == "identity-last":
        pts[-1] = None
    elif plan == "all-identity":
        pts = [None] * world
    elif plan == "same-point" and world >= 2:            # acc = P meets P under another z
        pts[1] = P
    elif plan == "sum-of-two" and world >= 3:            # acc = A + B meets the point A + B
        pts[2] = g1_add(pts[0], pts[1])
    elif plan == "negative-adjacent" and world >= 2:     # acc = P meets -P: the identity, and the fold goes on from it
        pts[1] = g1_neg(P)
    elif plan == "negative-apart" and world >= 3:
        pts[2] = g1_neg(P)
    elif plan == "negative-of-two" and world >= 3:       # acc = A + B meets -(A + B)
        pts[2] = g1_neg(g1_add(pts[0], pts[1]))
    return pts


@functools.lru_cache(maxsize=None)
def build_shape(world, count):
    """-> ((world, count, 12) uint64, the plans of the columns, their affine sums); made once, shared and left unchanged"""
    rnd = random.Random(SEED * 1000 + world * 131 + count)
    arr = np.zeros((world, count, 12), dtype=np.uint64)
    plans, sums = [], []
    for j in range(count):
        plan = PLANS[(j + world + count) % len(PLANS)]
        pts = column(plan, world, rnd)
        acc = None
        for r, P in enumerate(pts):
            arr[r, j] = jacobian(P, 1 if rnd.random() < 0.1 else rnd.randrange(2, Q))
            acc = g1_add(acc, P)
        plans.append(plan)
        sums.append(acc)
    return arr, plans, sums


def to_affine(rec):
    """12 x u64 (Jacobian, Montgomery form) -> the affine point, None for z = 0; the coordinates must be canonical"""
    c = [sum(int(rec[4 * i + k]) << (64 * k) for k in range(4)) for i in range(3)]
    assert all(v < Q for v in c)
    x, y, z = (v * pow(RM, -1, Q) % Q for v in c)
    if z == 0:
        return None
    return x * pow(z, -2, Q) % Q, y * pow(z, -3, Q) % Q


def test_every_plan_is_planted_where_there_is_room():
    """the tables the GPU test below folds hold what they are said to hold (this one needs no GPU)"""
    seen = set()
    for world in WORLDS:
        for count in COUNTS:
            arr, plans, sums = build_shape(world, count)
            z = arr[:, :, 8:].any(axis=2)                                   # (world, count): the partial is no identity
            for j, plan in enumerate(plans):
                col = arr[:, j, :]
                if plan == "all-identity":
                    assert not z[:, j].any() and sums[j] is None
                elif plan.startswith("identity-"):
                    r = {"identity-first": 0, "identity-middle": world // 2, "identity-last": world - 1}[plan]
                    assert not z[r, j] and (world == 1 or z[:, j].sum() == world - 1)
                elif world >= 3 or (world == 2 and plan in ("same-point", "negative-adjacent")):
                    pts = [to_affine(col[r]) for r in range(world)]
                    if plan == "same-point":
                        assert pts[0] == pts[1] and (col[0] != col[1]).any()
                    elif plan == "sum-of-two":
                        assert g1_add(pts[0], pts[1]) == pts[2]
                    elif plan == "negative-adjacent":
                        assert pts[1] == g1_neg(pts[0]) and (world > 2 or sums[j] is None)
                    elif plan == "negative-apart":
                        assert pts[2] == g1_neg(pts[0]) and pts[1] not in (pts[0], pts[2])
                    elif plan == "negative-of-two":
                        assert g1_add(g1_add(pts[0], pts[1]), pts[2]) is None
                seen.add((world, plan))
            if count >= len(PLANS):
                assert set(plans) == set(PLANS)
    assert seen == {(w, p) for w in WORLDS for p in PLANS}


@pytest.mark.parametrize("world", WORLDS)
def test_host_fold_matches_integer_sum(world):
    """the host twin the device is compared with, against the same integers (no GPU)"""
    from halo2_gpu_specific_amd import parallel

    arr, plans, sums = build_shape(world, 65)
    for j in range(65):
        assert to_affine(parallel.g1_sum(arr[:, j, :])) == sums[j], "world %d, column %d (%s)" % (world, j, plans[j])


@pytest.fixture(scope="module")
def device():
    from halo2_gpu_specific_amd import prover

    return prover.Device()


@pytest.mark.gpu
@pytest.mark.parametrize("count", COUNTS)
@pytest.mark.parametrize("world", WORLDS)
def test_fold_matches_integer_sum_and_host_twin(device, world, count):
    import torch

    from halo2_gpu_specific_amd import parallel
    from halo2_gpu_specific_amd._lib import check, lib

    arr, plans, sums = build_shape(world, count)
    with torch.cuda.stream(device.tstream):
        points = torch.from_numpy(arr.view(np.int64)).to(device.dev)
        out = torch.full((count, 12), -1, dtype=torch.int64, device=device.dev)      # a column never written stays this pattern
        check(lib().h2_dev_g1_fold(points.data_ptr(), world, count, out.data_ptr(), device.stream), "h2_dev_g1_fold")
        got = out.cpu().numpy().view(np.uint64)
    for j in range(count):
        what = "world %d, count %d, column %d (%s)" % (world, count, j, plans[j])
        assert to_affine(got[j]) == sums[j], what
        twin = parallel.g1_sum(arr[:, j, :])
        assert got[j].tobytes() == twin.tobytes(), what + ": the device's 96 bytes are not the host fold's"
