"""Params.from_powers -- the G1 NTT h2_dev_g1_ntt (inverse) of 2^k points -- timed on the device, with the Fq products its
kernels issue and the share of the multiplier's measured rate (1.60e11 products/s, README).  One JSON line per k.
usage: python tools/g1_ntt_bench.py K [K ...] [--reps N]

The products are counted here from the formulas csrc/g1ntt.hip uses (ec.hpp: doubling 9, XYZZ addition 14, mixed addition
10; a^(q-2) 254 squarings + popcount(q-2) products) and the twiddles' bits, which the tool computes on the device (powers of
w^-1 by a prefix product, taken out of Montgomery form).  A wave issues a doubling while any of its lanes has bits left and an
addition at every bit position where any lane has a set bit below its top one: in the uniform stages that is the count of
the one twiddle the wave holds, in the last min(6, k) stages the union over its lanes ("as issued")."""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")  # before HIP initialises (halo2-gpu-specific_amd/__init__.py says why)
import numpy as np  # noqa: E402

MULTIPLIER_RATE = 1.60e11                 # 254-bit Montgomery products/s, measured in round 5 (README)
DBL, ADD, MADD = 9, 14, 10
WAVE, WAVE_LOG, TW_LO_BITS = 64, 6, 12
R_MOD = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001
Q_MOD = 0x30644E72E131A029B85045B68181585D97816A916871CA8D3C208C16D87CFD47
ROOT_OF_UNITY = 0x03DDB9F5166D18B798865EA93DD31F743215CF6DD39329C8D34F1ED960C37C9C


def bitlen64(x):
    x = x.copy()
    n = np.zeros(x.shape, dtype=np.int64)
    for sh in (32, 16, 8, 4, 2, 1):
        m = (x >> np.uint64(sh)) != 0
        n += m * sh
        x = np.where(m, x >> np.uint64(sh), x)
    return n + (x != 0)


def bitlen256(w):
    """w: (m, 4) u64 little-endian limbs -> bit lengths"""
    bl = np.zeros(w.shape[0], dtype=np.int64)
    for j in range(4):
        blj = bitlen64(w[:, j])
        bl = np.where(blj > 0, 64 * j + blj, bl)
    return bl


def scalar_cost(bits, pops, add):
    return np.where(bits > 0, DBL * (bits - 1) + add * (pops - 1), 0)


def count_products(k, twiddles):
    """products issued by one inverse transform of 2^k points; twiddles: (n/2, 4) u64 canonical w^-e, e < n/2.
    -> dict of the phases' counts"""
    n = 1 << k
    ninv = pow(n, -1, R_MOD)
    out = {"load": n * int(DBL * (ninv.bit_length() - 1) + MADD * (bin(ninv).count("1") - 1)) if k else 0,
           "uniform_stages": 0, "divergent_stages": 0,
           "normalize": n * (254 + bin(Q_MOD - 2).count("1") + 4)}
    if k == 0:
        return out
    half = n >> 1
    lookup = 1 + (1 if k > TW_LO_BITS else 0)
    bl = bitlen256(twiddles)
    pc = np.bitwise_count(twiddles).sum(axis=1).astype(np.int64)
    bl[0], pc[0] = 0, 0                                      # e = 0: w = 1, no multiplication
    top = np.zeros_like(twiddles)                            # each twiddle without its top bit
    for j in range(4):
        sel = (bl - 1) // 64 == j
        top[:, j] = np.where(sel, np.uint64(1) << ((np.maximum(bl, 1) - 1) % 64).astype(np.uint64), np.uint64(0))
    stripped = twiddles & ~top
    stripped[0] = 0
    t = np.arange(half, dtype=np.int64)
    for s in range(k):
        nb_log = k - 1 - s
        e = t & ~((1 << nb_log) - 1)
        if nb_log >= WAVE_LOG:
            # one twiddle per wave: per butterfly its own count
            cost = scalar_cost(bl[e], pc[e], ADD) + np.where(e != 0, lookup, 0) + 2 * ADD
            out["uniform_stages"] += int(cost.sum())
        else:
            lanes = min(WAVE, half)
            ew = e.reshape(-1, lanes)
            dbl = np.maximum(bl[ew].max(axis=1) - 1, 0)
            adds = np.bitwise_count(np.bitwise_or.reduce(stripped[ew], axis=1)).sum(axis=1).astype(np.int64)
            issued = DBL * dbl + ADD * adds + np.where((ew != 0).any(axis=1), lookup, 0) + 2 * ADD
            out["divergent_stages"] += int(issued.sum()) * lanes
    return out


def device_twiddles(D, k):
    """w^-e canonical, e < 2^(k-1), as (n/2, 4) u64 (w = the domain's omega)"""
    from halo2_gpu_specific_amd._lib import check
    from halo2_gpu_specific_amd.domain import _fr

    half = 1 << (k - 1)
    w_inv = pow(pow(ROOT_OF_UNITY, 1 << (28 - k), R_MOD), -1, R_MOD)
    f = D.eval_op(8, D.empty(half), c=w_inv)                                   # H2_OP_CONSTANT
    out = D.empty(half)
    check(D.L.h2_dev_prefix_product(f.data_ptr(), half, _fr(1), out.data_ptr(), D.stream), "h2_dev_prefix_product")
    check(D.L.h2_dev_batch_unmont(out.data_ptr(), half, D.stream), "h2_dev_batch_unmont")
    return np.ascontiguousarray(D.download(out).reshape(-1, 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("k", type=int, nargs="+")
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    import torch

    torch.cuda.init()
    from halo2_gpu_specific_amd import prover
    from halo2_gpu_specific_amd._lib import check

    D = prover.Device()
    L = D.L
    for k in args.k:
        n = 1 << k
        with torch.cuda.stream(D.tstream):
            g = torch.empty((n, 8), dtype=torch.int64, device=D.dev)
        check(L.h2_dev_random_points(0x6731 + k, n, g.data_ptr(), D.stream), "h2_dev_random_points")
        prover.Params.from_powers(D, k, g, tables=False)                          # warm-up: plan, code objects
        times = []
        for _ in range(args.reps):
            ms = ctypes.c_float()
            check(L.h2_timer_start(D.stream), "h2_timer_start")
            P = prover.Params.from_powers(D, k, g, tables=False)
            check(L.h2_timer_stop(D.stream, ctypes.byref(ms)), "h2_timer_stop")
            times.append(ms.value * 1e-3)
            del P
        counts = count_products(k, device_twiddles(D, k) if k else np.zeros((0, 4), dtype=np.uint64))
        products = sum(counts.values())
        best = min(times)
        print(json.dumps({
            "k": k, "reps": args.reps, "from_powers_s_min": round(best, 5),
            "from_powers_s_median": round(statistics.median(times), 5),
            "products": products, "products_by_phase": counts,
            "products_per_s": float("%.4g" % (products / best)),
            "fraction_of_multiplier_rate": round(products / best / MULTIPLIER_RATE, 3),
            "divergent_share_of_products": round(counts["divergent_stages"] / products, 3),
        }), flush=True)
        del g
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
