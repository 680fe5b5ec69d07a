"""Params.update from the command line: one contribution to an SRS file, the check of one, or the update timed by phase.
usage: python tools/params_update.py IN OUT [--k K] [--contribution FILE] [--seed N]
       python tools/params_update.py --check OLD NEW CONTRIBUTION [--seed N]
       python tools/params_update.py --bench K [K ...] [--reps N]

IN OUT: the SRS file IN is read (formats.params_read, with --k the parameters of 2^K rows derived from it) with the [s]G2 of its
additional_data, updated with a tau drawn from os.urandom (Params.update), checked against the file it came from
(params_update.assert_valid_update) and written to OUT with the new [s tau]G2 as additional_data; the contribution -- the 64
compressed bytes of [tau]G2 -- goes to --contribution (default OUT.contribution).  The process does nothing else and ends: tau
is a Python integer and cannot be wiped.  --seed N takes tau from N instead (params_update.tau_from_seed): deterministic, FOR
TESTS ONLY -- whoever knows N knows tau -- and the tool says so on stderr.

--check: prints params_update.describe of the report of NEW as an update of OLD by CONTRIBUTION (--seed: the seed of the
check's randomness).  The exit status is 0 for an update that is ok, 1 otherwise.

--bench: on Params.unsafe_setup parameters of each K, one JSON line: the milliseconds of each phase of the update (powers
column, point scaling, G1 NTT, G2 multiplication, total; a synchronisation between phases; the best of --reps by total after
a warm-up, tables off), `from_powers` of the same K from the same run, and the Fq products the scaling kernel issues per
point.  The products are counted here from the digit schedule of csrc/g1mul.hip over the scalars tau^i of the run (ec.hpp:
doubling 9, XYZZ addition 14; a^(q-2) 254 squarings + 127 products), as tools/g1_ntt_bench.py counts: a wave of 64 lanes
issues a doubling while any of its lanes has a point in its accumulator and an addition at every digit where any such lane
has a digit other than zero.  The plain MSB-first double-and-add (doubling 9, mixed addition 10) is counted over the same
scalars the same way, beside it."""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")  # before HIP initialises (halo2-gpu-specific_amd/__init__.py says why)
import numpy as np  # noqa: E402

PHASES = ("powers", "scale", "g1_ntt", "g2_mul", "total")
BENCH_TRAPDOOR = 0x1D0C5F0A3B7E91C2A4D6F8091B2C3D4E5F60718293A4B5C6D7E8F9010203
BENCH_TAU = 0x2B7E151628AED2A6ABF7158809CF4F3C762E7160F38B4DA56A784D9045190CFE % (
    0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001)
DBL, ADD, MADD = 9, 14, 10
WAVE = 64
WINDOW, DIGITS = 3, 85                    # G1MUL_WINDOW, G1MUL_DIGITS (csrc/g1mul.hpp)
NORMALIZE = 254 + 127 + 4                 # a^(q-2) and the four products around it
TABLE = DBL + ADD + DBL                   # 2P, 3P, 4P


# ---- the products the scaling kernel issues ---------------------------------------------------------------------------------
def biased(scalars):
    """k + C over 256 bits for (n, 4) u64 canonical scalars, C = 4 (1 + 8 + ... + 8^84): bits 2, 5, ..., 254"""
    c = sum(1 << b for b in range(2, 255, 3))
    out = np.empty_like(scalars)
    carry = np.zeros(scalars.shape[0], dtype=np.uint64)
    for j in range(4):
        cj = np.uint64((c >> (64 * j)) & (2**64 - 1))
        s = scalars[:, j] + cj
        c1 = s < cj
        s2 = s + carry
        c2 = s2 < carry
        out[:, j] = s2
        carry = (c1 | c2).astype(np.uint64)
    assert not carry.any()
    return out


def bits_at(limbs, pos, width):
    """`width` bits of the (n, 4) u64 little-endian numbers from bit `pos`"""
    j, off = divmod(pos, 64)
    v = limbs[:, j] >> np.uint64(off)
    if off + width > 64 and j < 3:
        v = v | (limbs[:, j + 1] << np.uint64(64 - off))
    return (v & np.uint64((1 << width) - 1)).astype(np.int64)


def waves(a, fill):
    """a per-lane array as (waves, 64), the last wave padded with `fill`"""
    pad = (-a.shape[0]) % WAVE
    if pad:
        a = np.concatenate([a, np.full(pad, fill, dtype=a.dtype)])
    return a.reshape(-1, WAVE)


def count_products(scalars):
    """-> (products the signed-digit kernel issues per point, scaling only; the same for the plain double-and-add), both
    averaged over the points of full waves; scalars: (n, 4) u64 canonical"""
    n = scalars.shape[0]
    kb = biased(scalars)
    started = waves(bits_at(kb, 255, 1) != 0, False)                # lanes whose accumulator holds a point
    issued = np.zeros(started.shape[0], dtype=np.int64)
    for digit in range(DIGITS - 1, -1, -1):
        nonzero = waves(bits_at(kb, WINDOW * digit, WINDOW) != 4, False)
        issued += WINDOW * DBL * started.any(axis=1)
        issued += ADD * (started & nonzero).any(axis=1)
        started = started | nonzero
    digits = 1 + TABLE + issued                                      # + the scalar out of Montgomery form
    # the plain MSB-first double-and-add over the same scalars
    started = np.zeros_like(started)
    plain = np.zeros(started.shape[0], dtype=np.int64)
    for bit in range(255, -1, -1):
        one = waves(bits_at(scalars, bit, 1) != 0, False)
        plain += DBL * started.any(axis=1)
        plain += MADD * (started & one).any(axis=1)
        started = started | one
    lanes = started.shape[0] * WAVE
    return float(digits.sum() * WAVE / lanes), float(plain.sum() * WAVE / lanes), n


def device_powers(D, tau, n):
    """tau^i canonical, i < n, as (n, 4) u64"""
    from halo2_gpu_specific_amd.domain import _fr
    from halo2_gpu_specific_amd.prover import OP_CONSTANT, check

    f = D.eval_op(OP_CONSTANT, D.empty(n), c=tau)
    out = D.empty(n)
    check(D.L.h2_dev_prefix_product(f.data_ptr(), n, _fr(1), out.data_ptr(), D.stream), "h2_dev_prefix_product")
    check(D.L.h2_dev_batch_unmont(out.data_ptr(), n, D.stream), "h2_dev_batch_unmont")
    return np.ascontiguousarray(D.download(out).reshape(-1, 4))


# ---- the three modes ----------------------------------------------------------------------------------------------------------
def s_g2_of(path, additional):
    if len(additional) != 64:
        sys.exit("%s: additional_data is %d bytes, not the 64 of a compressed [s]G2" % (path, len(additional)))
    return additional


def update_file(args):
    from halo2_gpu_specific_amd import formats, params_update as pu, prover
    from halo2_gpu_specific_amd.pairing import g2_compress

    src, dst = args.files
    D = prover.Device()
    old, additional = formats.params_read(D, src, k=args.k)
    s_g2 = s_g2_of(src, additional)
    tau = None
    if args.seed is not None:
        print("params_update: --seed: tau is derived from the seed -- deterministic, FOR TESTS ONLY, not a contribution",
              file=sys.stderr)
        tau = pu.tau_from_seed(args.seed)
    new, contribution = old.update(D, tau=tau, s_g2=s_g2)
    del tau
    pu.assert_valid_update(D, old, new, contribution, s_g2=new.s_g2, seed=args.seed)
    formats.params_write(D, new, dst, g2_compress(new.s_g2))
    cpath = args.contribution or dst + ".contribution"
    with open(cpath, "wb") as f:
        f.write(contribution)
    print("%s: k = %d updated and checked -> %s, contribution [tau]G2 -> %s" % (src, new.k, dst, cpath))
    return 0


def check_files(args):
    from halo2_gpu_specific_amd import formats, params_update as pu, prover

    old_path, new_path, cpath = args.check
    D = prover.Device()
    old, _ = formats.params_read(D, old_path, k=args.k)
    new, additional = formats.params_read(D, new_path, k=args.k)
    with open(cpath, "rb") as f:
        contribution = f.read()
    report = pu.verify_update(D, old, new, contribution, s_g2=additional if len(additional) == 64 else None, seed=args.seed)
    print(pu.describe(report))
    return 0 if report.ok else 1


def timed(D, fn):
    """device milliseconds of fn() on the compute stream (h2_timer_*)"""
    from halo2_gpu_specific_amd._lib import check

    ms = ctypes.c_float()
    check(D.L.h2_timer_start(D.stream), "h2_timer_start")
    out = fn()
    check(D.L.h2_timer_stop(D.stream, ctypes.byref(ms)), "h2_timer_stop")
    return ms.value, out


def bench(args):
    import gc

    import torch

    from halo2_gpu_specific_amd import params_update as pu, prover

    D = prover.Device()
    for k in args.bench:
        n = 1 << k
        P = prover.Params.unsafe_setup(D, k, BENCH_TRAPDOOR)
        runs = []
        for _ in range(args.reps + 1):                                                # the first is the warm-up
            timings = {}
            new, _ = pu.update_params(D, P, tau=BENCH_TAU, tables=False, timings=timings)
            runs.append(timings)
            del new
        best = min(runs[1:], key=lambda t: t["total"])
        prover.Params.from_powers(D, k, P.g, tables=False)                           # warm-up: plan, code objects
        from_powers_ms = min(timed(D, lambda: prover.Params.from_powers(D, k, P.g, tables=False))[0] for _ in range(args.reps))
        digits, plain, _ = count_products(device_powers(D, BENCH_TAU, n))
        print(json.dumps({
            "k": k, "reps": args.reps,
            "update_ms": {name: round(best[name], 3) for name in PHASES},
            "update_total_ms_all": [round(t["total"], 3) for t in runs[1:]],
            "from_powers_ms": round(from_powers_ms, 3),
            "scale_over_from_powers": round(best["scale"] / from_powers_ms, 3),
            "scale_products_per_point": round(digits, 1),
            "double_and_add_products_per_point": round(plain, 1),
            "normalize_products_per_point": NORMALIZE,
            "scale_products_per_s": float("%.4g" % ((digits + NORMALIZE) * n / (best["scale"] * 1e-3))),
        }), flush=True)
        del P, runs
        gc.collect()
        torch.cuda.empty_cache()
    return 0


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("files", nargs="*", metavar="FILE", help="IN OUT")
    ap.add_argument("--k", type=int, default=None)
    ap.add_argument("--contribution", default=None)
    ap.add_argument("--seed", type=int, default=None)
    ap.add_argument("--check", nargs=3, metavar=("OLD", "NEW", "CONTRIBUTION"))
    ap.add_argument("--bench", type=int, nargs="+", metavar="K")
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    modes = [bool(args.files), args.check is not None, args.bench is not None]
    if sum(modes) != 1 or (args.files and len(args.files) != 2):
        ap.error("give IN OUT, --check OLD NEW CONTRIBUTION or --bench K ...")
    import torch

    torch.cuda.init()
    if args.bench:
        return bench(args)
    return check_files(args) if args.check else update_file(args)


if __name__ == "__main__":
    sys.exit(main())
