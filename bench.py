#!/usr/bin/env python3
"""bench.py -- halo2 prover hot path on MI355X.

One step = one forward + one inverse 2^24-point BN254 Fr NTT (BASELINE.json configs[2], the
k = 24 size the metric is quoted on), data resident in HBM.  `value` = NTT Fr-ops/s with
Fr-ops = 3 * (n/2) * log2(n) per transform.  The MSM leg (2^20 random
scalars/points, configs[1]) is timed separately with `--full` and reported under "msm".

    python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR] [--full]

A plain run measures the headline only: set-up, warm-up, the K timed NTT steps, the result line.  `--full` adds everything
else this file measures (the from-idle repeat of the K steps, the MSM legs, the create_proof legs, the C++ host, the
multi-rank replicas, the CPU baselines).  `--dump-outputs DIR` writes what the last timed step computed to DIR/*.npy (a
fixed, seeded sample of rows; every 254-bit element as its eight 32-bit Montgomery limb halves in float64, exact).

N > 1: one process per GPU (torchrun), every rank runs the same per-column workload on its own
device (independent polynomials: no data-path collective) -> "scaling": "weak"; the timing is
the max over ranks.  torch is used for device memory, streams and the rank barrier only.
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

R_MOD = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001
ROOT_OF_UNITY = 0x03DDB9F5166D18B798865EA93DD31F743215CF6DD39329C8D34F1ED960C37C9C
HBM_PEAK_GBS = 8000.0  # /opt/skills/guides/MI355X_MICROARCH.md: 8 TB/s spec
# Integer-ALU bound of the 254-bit Montgomery product, from HARDWARE rates (tools/mulbench.hip, profiles/r2_mulbench.txt):
# v_mad_u64_u32 issues at 3.046e13 lane-ops/s on the whole chip; a product needs 136 of them (64 + 64 + 8); nothing
# else credited.  The multiplier itself reaches 1.60e11/s (0.71 of this bound: the add-with-carry after the
# multiply-adds that can carry, and the final conditional subtraction, share the same issue port).
MAD_RATE = 3.046e13
MUL_HW_BOUND = MAD_RATE / 136.0   # 2.24e11 products/s
MUL_MEASURED = 1.60e11            # the multiplier in a loop, >= 2 waves/SIMD


def fr_limbs(v):
    v = v * (1 << 256) % R_MOD  # Montgomery form
    return np.array([(v >> (64 * i)) & ((1 << 64) - 1) for i in range(4)], dtype=np.uint64)


def vp(a):
    return a.ctypes.data_as(ctypes.c_void_p)


Q_MOD = 0x30644E72E131A029B85045B68181585D97816A916871CA8D3C208C16D87CFD47


def jac_eq(p, q):
    """projective equality of two Jacobian points (12 x u64, Montgomery limbs): the representation
    depends on the (atomic-ordered) summation order, the group element does not."""
    def limbs(a, i):
        return sum(int(a[4 * i + k]) << (64 * k) for k in range(4))
    x1, y1, z1, x2, y2, z2 = limbs(p, 0), limbs(p, 1), limbs(p, 2), limbs(q, 0), limbs(q, 1), limbs(q, 2)
    if z1 == 0 or z2 == 0:
        return z1 == z2
    return (x1 * z2 * z2 - x2 * z1 * z1) % Q_MOD == 0 and (y1 * z2 ** 3 - y2 * z1 ** 3) % Q_MOD == 0


def launch_ranks(n, argv):
    """`python3 bench.py --gpus N` with no launcher around it: this process -- which has NOT imported torch and never
    touches the GPU -- starts N fresh rank processes (one per GPU, RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* set as
    torch.distributed.run would), relays rank 0's JSON line as its own last stdout line and exits non-zero if any rank
    does.  The reference splits over N_GPU devices inside one call (arithmetic.rs:413-440, plonk/prover.rs:56-74); here
    that is one process per device.  Nothing is re-executed from a process that has initialised the GPU."""
    import socket
    import subprocess
    import threading

    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    procs, lines = [], []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")      # dmabuf IPC: RCCL across processes needs it on this driver
        env.setdefault("OMP_NUM_THREADS", "1")                 # as torch.distributed.run does
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + list(argv), env=env,
                                      stdout=subprocess.PIPE if r == 0 else sys.stderr, text=(r == 0)))

    def pump():
        for line in procs[0].stdout:
            lines.append(line.rstrip("\n"))

    reader = threading.Thread(target=pump, daemon=True)
    reader.start()
    grace = float(os.environ.get("H2_BENCH_RANK_GRACE_S", "30"))
    failed_at, rc = None, 0
    while any(p.poll() is None for p in procs):
        codes = [p.poll() for p in procs]
        if failed_at is None and any(c not in (None, 0) for c in codes):
            failed_at = time.perf_counter()                    # a rank died: the others are waiting for it in a collective
        if failed_at is not None and time.perf_counter() - failed_at > grace:
            # SIGTERM first: rank 0's signal thread (main: `partial_line_on_sigterm`) prints what it has measured -- the
            # primary NTT metric is complete long before the proof legs -- and exits; SIGKILL for what is left 5 s later
            for p in procs:                                    # exactly the processes started above
                if p.poll() is None:
                    p.terminate()
            t_end = time.perf_counter() + 5.0
            while time.perf_counter() < t_end and any(p.poll() is None for p in procs):
                time.sleep(0.05)
            for p in procs:
                if p.poll() is None:
                    p.kill()
        time.sleep(0.05)
    reader.join(timeout=5)
    for r, p in enumerate(procs):
        if p.returncode != 0:
            print("bench.py: rank %d exited with code %s" % (r, p.returncode), file=sys.stderr)
            rc = rc or (p.returncode if p.returncode and p.returncode > 0 else 1)
    for line in lines[:-1]:
        print(line, file=sys.stderr)                           # anything rank 0 printed before its result line
    if lines:
        print(lines[-1], flush=True)
    elif rc == 0:
        rc = 1
    return rc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--log-n", type=int, default=24)
    ap.add_argument("--msm-log-n", type=int, default=20)
    ap.add_argument("--msm-steps", type=int, default=5)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-msm", action="store_true")
    ap.add_argument("--prove-k", type=int, default=22, help="create_proof leg: mini-PLONK with 2^k rows (0 = skip)")
    ap.add_argument("--prove-steps", type=int, default=3)
    ap.add_argument("--wide-k", type=int, default=20, help="create_proof_wide leg: circuits.wide with 2^k rows (0 = skip)")
    ap.add_argument("--wide-quads", type=int, default=16, help="create_proof_wide: quads of advice columns (16 -> 64 columns)")
    ap.add_argument("--wide-k22", type=int, default=1, help="1: also run the wide circuit at 2^22 rows (the zkWasm size), resident mode only")
    ap.add_argument("--cpu-prove-k", type=int, default=22, help="CPU create_proof baseline: mini-PLONK with 2^k rows on the host cores (0 = skip)")
    ap.add_argument("--k24", type=int, default=1, help="1: also run the k = 24 legs (MSM 2^24, create_proof k = 24) the metric is quoted at")
    ap.add_argument("--full", action="store_true",
                    help="also run every secondary leg (from-idle NTT, MSM, create_proof, C++ host, replicas, CPU baselines); "
                         "the options above that select those legs apply only with --full")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last step computed to DIR/<name>.npy (float64)")
    args = ap.parse_args()

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # no launcher around this process: become one (before torch is imported or the GPU is touched)
        sys.exit(launch_ranks(args.gpus, sys.argv[1:]))

    world_env = int(os.environ.get("WORLD_SIZE", "1"))
    if world_env > 1:
        # SIGTERM (our launcher or torchrun stopping the ranks after another rank failed) is taken by a dedicated thread:
        # blocked here, before any other thread exists, so that every thread inherits the mask; the main thread may be
        # inside an RCCL call that never returns and could not run a Python signal handler
        import signal

        signal.pthread_sigmask(signal.SIG_BLOCK, {signal.SIGTERM})
    # the CPU baseline's OpenMP teams sleep at their barriers instead of spinning (read when libgomp is loaded, i.e. before
    # torch is imported): rayon's idle workers park; a spinning team of 256 on a box whose cgroup grants fewer CPUs took 4.7 s
    # for a 2^20 transform in round 4's line
    os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")   # before HIP initialises: streams that share a hardware queue serialise (package __init__)
    os.environ.setdefault("OMP_WAIT_POLICY", "PASSIVE")
    os.environ.setdefault("GOMP_SPINCOUNT", "0")
    import torch

    import halo2_gpu_specific_amd as h2
    from halo2_gpu_specific_amd._lib import check

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    # H2_BENCH_BACKEND=gloo: a dry run of the multi-rank flow on ONE GPU (every rank on cuda:0; RCCL refuses two ranks on one
    # device) -- the barriers, the reductions of the timings and one proof over the ranks, not a measurement
    backend = os.environ.get("H2_BENCH_BACKEND", "nccl")
    if backend != "nccl":
        local_rank = 0
    elif torch.cuda.device_count() < max(world, local_rank + 1):
        # one rank per GPU under RCCL: fail loudly instead of piling ranks onto one device or hanging in the rendezvous
        sys.exit("bench.py: %d ranks under RCCL need %d GPUs, this node shows %d (H2_BENCH_BACKEND=gloo dry-runs the "
                 "multi-rank flow on one GPU)" % (world, world, torch.cuda.device_count()))
    torch.cuda.set_device(local_rank)
    dist = None
    if world > 1 or os.environ.get("H2_BENCH_FORCE_DIST"):  # the env knob exercises the RCCL path with one rank
        import torch.distributed as dist

        if backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
        else:
            dist.init_process_group(backend)
    L = h2.lib()  # raises loudly if libhalo2_hip.so is missing: no fallback path
    dev = torch.device("cuda", local_rank)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def leg_failed(key, e):
        """a secondary leg raised: recorded in the line (the primary NTT metric is still printed) and reported on stderr with
        the rank.  With N > 1 the legs are sequences of collectives that every rank must walk in step -- a rank that left one
        early would pair its next barrier with the others' current one -- so there the run ends here, non-zero (the launcher
        stops the other ranks and reports which one failed)."""
        import traceback

        sys.stderr.write("bench.py: rank %d: leg %s failed: %s: %s\n%s" % (rank, key, type(e).__name__, e, traceback.format_exc()))
        sys.stderr.flush()
        if world > 1:
            if rank == 0:
                out[key] = {"error": "%s: %s" % (type(e).__name__, e)}
                print(json.dumps(out), flush=True)
            os._exit(3)
        return {"error": "%s: %s" % (type(e).__name__, e)}

    partial = {}                                  # rank 0's result line so far, for the SIGTERM thread below

    def partial_line_on_sigterm():
        import signal

        signal.sigwait({signal.SIGTERM})
        if rank == 0 and partial.get("out") is not None:
            line = dict(partial["out"])
            line["error"] = "stopped by SIGTERM before the run was complete (another rank failed or stalled): the legs present were measured"
            try:
                print(json.dumps(line), flush=True)
            except Exception:  # noqa: BLE001 - a leg being written by the main thread at this instant
                pass
        os._exit(4)

    if world > 1:
        import threading

        threading.Thread(target=partial_line_on_sigterm, daemon=True).start()

    def barrier():
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
            torch.cuda.synchronize()

    # ---------------------------------------------------------------- NTT leg (primary metric)
    log_n, n = args.log_n, 1 << args.log_n
    omega = pow(ROOT_OF_UNITY, 1 << (28 - log_n), R_MOD)
    w_f, w_i, n_inv = fr_limbs(omega), fr_limbs(pow(omega, -1, R_MOD)), fr_limbs(pow(n, -1, R_MOD))
    g = torch.Generator(device=dev)
    g.manual_seed(0x48414C4F32 + 1 + rank)
    a = torch.randint(-(2**63), 2**63 - 1, (n, 4), dtype=torch.int64, device=dev, generator=g)
    a[:, 3] &= 0x1FFFFFFFFFFFFFFF  # top limb < 2^61 < r's top limb: every row is a valid residue
    tmp = torch.empty_like(a)

    def ntt_step():
        check(L.h2_dev_ntt(a.data_ptr(), tmp.data_ptr(), vp(w_f), log_n, stream), "h2_dev_ntt")
        check(L.h2_dev_intt(a.data_ptr(), tmp.data_ptr(), vp(w_i), vp(n_inv), log_n, stream), "h2_dev_intt")

    # The device needs ~30 ms of load to reach its steady clock (after an idle second the first 6-8 steps run 4.7 .. 3.8 ms,
    # the rest 3.65: tools/experiments/ntt_ramp.py).  Every timed loop of this file is preceded by SPIN_S seconds of the
    # same step, untimed, on top of the W warmup steps; the line says so ("spin_up_s").
    SPIN_S = float(os.environ.get("H2_BENCH_SPIN_S", "0.15"))

    def spin(fn):
        t_end = time.perf_counter() + SPIN_S
        while time.perf_counter() < t_end:
            fn()
            torch.cuda.synchronize()

    ref_head = a[:64].clone()
    # torch generated `a` on ITS current stream; the library runs on the stream it is handed (NULL = its own, non-blocking:
    # not ordered with torch's default stream): everything above is complete before the first transform starts
    torch.cuda.synchronize()
    spin(ntt_step)
    for _ in range(args.warmup):
        ntt_step()
    # --dump-outputs: the timed steps' input (every step maps x to itself), kept to recompute the forward half of a step
    x_in = a.clone() if args.dump_outputs and rank == 0 else None
    barrier()
    t0 = time.perf_counter()
    check(L.h2_timer_start(stream), "timer")
    for _ in range(args.steps):
        ntt_step()
    ev_ms = ctypes.c_float(0)
    check(L.h2_timer_stop(stream, ctypes.byref(ev_ms)), "timer")
    barrier()
    t1 = time.perf_counter()
    assert torch.equal(a[:64], ref_head), "inverse(forward(x)) != x"  # round-trip property at full size
    elapsed = t1 - t0
    if dist is not None:
        t = torch.tensor([elapsed], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    fr_ops_per_transform = 3 * (n // 2) * log_n
    value = world * args.steps * 2 * fr_ops_per_transform / elapsed
    if x_in is not None:
        # ntt_roundtrip: the array the last timed step returned, inverse(forward(x)); ntt_forward: the forward half of a
        # step, h2_dev_ntt of the same input recomputed once here (the transform is deterministic).  The same 2^17 rows
        # (or all of them) from a fixed seed; each Montgomery limb as two exact 32-bit halves, low first
        os.makedirs(args.dump_outputs, exist_ok=True)
        rows = np.sort(np.random.default_rng(0x48414C4F32).choice(n, min(n, 1 << 17), replace=False))
        rows_t = torch.from_numpy(rows).to(dev)

        def dump(name, t):
            u = t.index_select(0, rows_t).cpu().numpy().view(np.uint64)
            halves = np.stack([u & np.uint64(0xFFFFFFFF), u >> np.uint64(32)], axis=-1).reshape(len(rows), 8)
            np.save(os.path.join(args.dump_outputs, name + ".npy"), halves.astype(np.float64))

        dump("ntt_roundtrip", a)
        check(L.h2_dev_ntt(x_in.data_ptr(), tmp.data_ptr(), vp(w_f), log_n, stream), "h2_dev_ntt")
        torch.cuda.synchronize()
        dump("ntt_forward", x_in)
        del x_in, rows_t
    idle_elapsed = None
    if args.full:
        # ... and the same K steps FROM IDLE (a prover is called from idle): one second of sleep, no spin-up, no warm-up
        time.sleep(1.0)
        barrier()
        i0 = time.perf_counter()
        for _ in range(args.steps):
            ntt_step()
        barrier()
        idle_elapsed = time.perf_counter() - i0
        if dist is not None:
            t = torch.tensor([idle_elapsed], dtype=torch.float64, device=dev)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            idle_elapsed = float(t.item())

    # roofline of the dominant kernel (k_ntt_pass): algorithmic bytes per SURVEY.md 8(d) =
    # 64 * n * ceil(log_n / 12) per transform, spread over the passes this build launches per transform
    # csrc/ntt.hip ntt_split: 8-bit passes, the remainder first -- or folded into 9-bit passes at the end (one-bit remainders)
    q8, rem8 = divmod(log_n, 8)
    passes = (q8 if (q8 >= rem8 and (rem8 == 1 or (rem8 == 2 and log_n <= 18))) else q8 + (1 if rem8 else 0)) if log_n else 1
    alg_bytes_per_transform = 64 * n * ((log_n + 11) // 12)
    launches = args.steps * 2 * passes
    avg_launch_ms = ev_ms.value / launches
    achieved_gbs = (alg_bytes_per_transform / passes) / (avg_launch_ms * 1e-3) / 1e9

    # HBM bytes per k_ntt_pass launch from the PMC passes committed under profiles/ (separate rocprofv3
    # --pmc FETCH_SIZE / WRITE_SIZE runs, gfx950 correction applied); null when the file is absent
    traffic, traffic_source = None, None
    for prof in ("r6_hbm_traffic.json", "r5_hbm_traffic.json", "r4_hbm_traffic.json", "r3_hbm_traffic.json", "r2_hbm_traffic.json"):
        try:
            with open(os.path.join(ROOT, "profiles", prof)) as f:
                if log_n == 24:
                    kern = json.load(f)["kernels"]
                    # every instantiation of the pass kernel (since round 6 the last pass is one of its own), launch-weighted
                    passes_ = [v for k, v in kern.items() if "k_ntt_pass" in k]
                    traffic = (sum(v["hbm_bytes_per_launch_corrected"] * v["launches"] for v in passes_) /
                               sum(v["launches"] for v in passes_))
                    traffic_source = ("profiles/%s: separate rocprofv3 --pmc passes of this kernel (tools/hbm_traffic.py), "
                                      "NOT measured in this run" % prof)
                    break
        except (OSError, KeyError, ValueError, IndexError):
            traffic = None

    # products per transform (csrc/ntt.hip k_ntt_pass): (n/2) log2 n butterflies minus the twiddle-1 ones the early stages
    # skip (stage 0 of every pass; the r = 0 waves of stages 1-3), one tabulated inter-pass twiddle per element in the
    # middle passes and one in the last (a complete table for 2^18 .. 2^26 points; lo x hi and the product otherwise)
    last_tw = 1 if 18 <= log_n <= 26 else 2   # the last pass reads its twiddle from a complete table at these sizes
    mults_per_transform = n * (passes * 3.06 + max(passes - 2, 0) + (last_tw if passes > 1 else 0)) if log_n >= 8 else (log_n / 2.0 + passes) * n
    # multiply-adds per product: the twiddles read from tables (butterflies, the middle passes' inter-pass twiddles) are
    # (plain value, quotient) pairs multiplied in 115 multiply-adds (field.hpp fp_mul_const; transforms >= 2^18, H2_NTT_CONSTW=0:
    # off); the last pass's table product stays a Montgomery product (136): the bound below is priced with the mix
    constw = log_n >= 18 and os.environ.get("H2_NTT_CONSTW", "1") != "0"
    const_products = n * (passes * 3.06 + max(passes - 2, 0)) if log_n >= 8 else 0.0
    mads_per_product = ((115.0 * const_products + 136.0 * (mults_per_transform - const_products)) / mults_per_transform) if constw else 136.0
    ntt_mul_bound = MAD_RATE / mads_per_product
    out = {
        "metric": "NTT Fr-ops/s @ k=24 (forward+inverse 2^24 BN254 Fr NTT; MSM G1-adds/s under 'msm')",
        "value": value,
        "unit": "Fr-ops/s",
        "n_gpus": world,
        "steps": args.steps,
        "warmup": args.warmup,
        "spin_up_s": SPIN_S,
        "ms_per_step": elapsed / args.steps * 1e3,
        "ms_per_step_from_idle": idle_elapsed / args.steps * 1e3 if idle_elapsed is not None else None,
        "clock_note": "`value` / `ms_per_step`: the K timed steps at the device's steady clock (spin_up_s of the same step, untimed, "
                      "before the W warm-up steps); `ms_per_step_from_idle` (--full): the same K steps after one idle second, nothing "
                      "before them",
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        "dtype": "u32x8 (254-bit Montgomery, integer)",
        "data": "synthetic",
        "runtime": {"GPU_MAX_HW_QUEUES": os.environ.get("GPU_MAX_HW_QUEUES"),
                    "note": "HIP hardware queues the process's streams are multiplexed onto (the runtime's default is 4; streams "
                            "that share a queue serialise: DESIGN.md section 0)"},
        "config": {
            "workload": "BASELINE configs[2]: 2^%d-point BN254 Fr forward+inverse NTT per step, resident in HBM" % log_n,
            "log_n": log_n,
            "per_rank": "one independent polynomial per GPU (per-column sharding, no collective)",
        },
        "roofline": {
            "bound": "hbm",
            "kernel": "k_ntt_pass",
            "achieved": achieved_gbs,
            "peak": HBM_PEAK_GBS,
            "unit": "GB/s",
            "frac": achieved_gbs / HBM_PEAK_GBS,
            "traffic": traffic,
            "traffic_source": traffic_source,
            "algorithmic_bytes_per_launch": alg_bytes_per_transform / passes,
            "avg_launch_ms": avg_launch_ms,
            "launches_per_transform": passes,
            "limiter": "integer VALU (254-bit modular multiplication), not HBM: the HBM figure above is the contract's "
            "definition; the ALU accounting follows",
            "alu": {
                "bound": "v_mad_u64_u32 issue rate / multiply-adds per product (hardware rates, tools/mulbench.hip): 115 for a product "
                         "by a tabulated twiddle (constant-operand form), 136 for a Montgomery product",
                "multiply_adds_per_product": mads_per_product,
                "achieved_mul_per_s": mults_per_transform / (passes * avg_launch_ms * 1e-3),
                "peak_mul_per_s": ntt_mul_bound,
                "frac": mults_per_transform / (passes * avg_launch_ms * 1e-3) / ntt_mul_bound,
                "frac_at_136_multiply_adds": mults_per_transform / (passes * avg_launch_ms * 1e-3) / MUL_HW_BOUND,
                "multiplier_in_a_loop_per_s": MUL_MEASURED,
                "note": "products per transform: 3.06 per element per 8-bit pass (4 butterflies, the twiddle-1 ones of the early "
                "stages skipped) + one tabulated inter-pass twiddle product per element in the middle passes and in the last",
            },
        },
    }

    # ---------------------------------------------------------------- MSM legs: 2^20 (configs[1]) and 2^24 (the k = 24 size)
    def msm_leg(mlog, steps, batch):
        mn = 1 << mlog
        bases = torch.empty((mn, 8), dtype=torch.int64, device=dev)
        check(L.h2_dev_random_points(0x48414C4F32, mn, bases.data_ptr(), stream), "h2_dev_random_points")
        cols = []
        for j in range(max(batch, 1)):          # DISTINCT uniform columns (a batch of one repeated column is cache-friendly)
            sc = torch.randint(-(2**63), 2**63 - 1, (mn, 4), dtype=torch.int64, device=dev, generator=g)
            sc[:, 3] &= 0x1FFFFFFFFFFFFFFF
            cols.append(sc)
        torch.cuda.synchronize()                # torch's stream produced the columns; the library's streams consume them
        sbytes = L.h2_msm_scratch_bytes(mn, 254)
        scratch = torch.empty(sbytes, dtype=torch.uint8, device=dev)
        res = np.zeros(12, dtype=np.uint64)
        c, W, nb = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32()
        L.h2_msm_shape(mn, 254, ctypes.byref(c), ctypes.byref(W), ctypes.byref(nb))

        def msm_step(j=0):
            check(L.h2_dev_msm(cols[j].data_ptr(), bases.data_ptr(), mn, 254, scratch.data_ptr(), sbytes, vp(res), stream), "h2_dev_msm")

        singles = []
        for j in range(len(cols)):
            msm_step(j)
            singles.append(res.copy())
        spin(msm_step)
        barrier()
        m0 = time.perf_counter()
        for i in range(steps):
            msm_step(i % len(cols))
        barrier()
        melapsed = time.perf_counter() - m0
        assert jac_eq(singles[(steps - 1) % len(cols)], res), "MSM result changed between runs"
        adds = mn * W.value + 2 * nb.value * W.value + W.value * c.value
        leg = {
            "single_msm": {"ms_per_msm": None, "g1_adds_per_s": None, "pairs_per_s": None},
            "window_bits": c.value, "windows": W.value, "buckets_per_window": nb.value, "g1_adds_per_msm": adds,
            "g1_adds_formula": "n*W + 2*2^(c-1)*W + W*c (bucket accumulate + running-sum reduce + window doublings)",
            "steps": steps,
        }
        belapsed = None
        if batch > 1:
            # batch leg: `batch` distinct columns committed against the same bases (the prover's shape,
            # plonk/prover.rs:293-299), pipelined by the library on two internal streams
            per = (sbytes + 255) // 256 * 256
            del scratch
            scratch2 = torch.empty(2 * per, dtype=torch.uint8, device=dev)
            ptrs = (ctypes.c_void_p * batch)(*[t.data_ptr() for t in cols])
            bres = np.zeros((batch, 12), dtype=np.uint64)

            def batch_step():
                check(L.h2_dev_msm_batch(ptrs, batch, bases.data_ptr(), mn, 254, scratch2.data_ptr(), 2 * per, vp(bres), stream), "h2_dev_msm_batch")

            batch_step()
            assert all(jac_eq(singles[i], bres[i]) for i in range(batch)), "batched MSM differs from the single MSMs"
            spin(batch_step)
            barrier()
            b0 = time.perf_counter()
            for _ in range(steps):
                batch_step()
            barrier()
            belapsed = time.perf_counter() - b0
            del scratch2
        if dist is not None:
            t = torch.tensor([melapsed, belapsed or 0.0], dtype=torch.float64, device=dev)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            melapsed, belapsed = float(t[0].item()), (float(t[1].item()) if belapsed is not None else None)
        leg["single_msm"] = {"ms_per_msm": melapsed / steps * 1e3, "g1_adds_per_s": world * steps * adds / melapsed,
                             "pairs_per_s": world * steps * mn / melapsed}
        if belapsed is not None:
            leg.update({
                "g1_adds_per_s": world * steps * batch * adds / belapsed,
                "pairs_per_s": world * steps * batch * mn / belapsed,
                "ms_per_msm_batched": belapsed / (steps * batch) * 1e3,
                "batch": "%d DISTINCT uniform columns over shared bases per call (h2_dev_msm_batch, two streams)" % batch,
            })
        # the same MSMs over a shifted-base table of the bases (h2_dev_bases_precompute): how the prover holds its SRS
        t0 = time.perf_counter()
        check(L.h2_dev_bases_precompute(bases.data_ptr(), mn, 0, stream), "h2_dev_bases_precompute")
        build_s = time.perf_counter() - t0
        sbytes_t = L.h2_msm_scratch_bytes(mn, 254)
        per_t = (sbytes_t + 255) // 256 * 256
        scratch_t = torch.empty(2 * per_t, dtype=torch.uint8, device=dev)

        def table_step(j=0):
            check(L.h2_dev_msm(cols[j].data_ptr(), bases.data_ptr(), mn, 254, scratch_t.data_ptr(), sbytes_t, vp(res), stream), "h2_dev_msm")

        for j in range(len(cols)):
            table_step(j)
            assert jac_eq(singles[j], res), "MSM over the table differs from the windowed MSM"
        spin(table_step)
        barrier()
        t0 = time.perf_counter()
        for i in range(steps):
            table_step(i % len(cols))
        barrier()
        telapsed = time.perf_counter() - t0
        tb = None
        if batch > 1:
            def tbatch_step():
                check(L.h2_dev_msm_batch(ptrs, batch, bases.data_ptr(), mn, 254, scratch_t.data_ptr(), 2 * per_t, vp(bres), stream), "h2_dev_msm_batch")

            tbatch_step()
            assert all(jac_eq(singles[i], bres[i]) for i in range(batch)), "batched MSM over the table differs"
            spin(tbatch_step)
            barrier()
            t0 = time.perf_counter()
            for _ in range(steps):
                tbatch_step()
            barrier()
            tb = time.perf_counter() - t0
        if dist is not None:
            t = torch.tensor([telapsed, tb or 0.0], dtype=torch.float64, device=dev)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            telapsed, tb = float(t[0].item()), (float(t[1].item()) if tb is not None else None)
        leg["over_shifted_base_table"] = {
            "what": "bases expanded once into [2^(o_j)] P_i for the digit offsets o_j; all digits of a scalar share one bucket set "
                    "(same group element; `g1_adds` keeps the windowed formula so the rates compare by time)",
            "table_bytes": int(L.h2_dev_bases_precompute_bytes(mn, 0)), "build_ms": build_s * 1e3,
            "ms_per_msm": telapsed / steps * 1e3, "g1_adds_per_s_single": world * steps * adds / telapsed,
        }
        if tb is not None:
            leg["over_shifted_base_table"].update({"ms_per_msm_batched": tb / (steps * batch) * 1e3,
                                                   "g1_adds_per_s": world * steps * batch * adds / tb})
        check(L.h2_dev_bases_forget(bases.data_ptr()), "h2_dev_bases_forget")
        del scratch_t
        # additions actually EXECUTED per MSM: the windowed formula for the windowed pipeline; over a table D digits per
        # scalar into ONE shared bucket set of 2^(c_t - 1) buckets (c_t = ceil(255 / D) bits per digit) and one reduction
        digits = int(L.h2_dev_bases_precompute_bytes(mn, 0)) // (64 * mn)
        c_t = (255 + digits - 1) // digits
        adds_table = mn * digits + 2 * (1 << (c_t - 1)) + c_t
        tab = leg["over_shifted_base_table"]
        tab["digits"], tab["digit_bits"], tab["g1_adds_executed_per_msm"] = digits, c_t, adds_table
        rates = [leg["single_msm"]["g1_adds_per_s"], leg.get("g1_adds_per_s") or 0.0,
                 adds_table / (tab["ms_per_msm"] * 1e-3) * world,
                 (adds_table / (tab["ms_per_msm_batched"] * 1e-3) * world) if tab.get("ms_per_msm_batched") else 0.0]
        tab["g1_adds_executed_per_s"] = max(rates[2], rates[3])
        leg["alu_roofline"] = {
            "bound": "integer VALU (not HBM: 96 B per pair): v_mad_u64_u32 issue rate / 136 per product / 10 products per mixed XYZZ addition",
            "peak_adds_per_s": world * MUL_HW_BOUND / 10.0,
            "frac": max(rates) / (world * MUL_HW_BOUND / 10.0),
            "note": "additions actually executed per second (windowed: n*W + 2*2^(c-1)*W + W*c; over a table: n*D + 2*2^(c_t-1) + c_t), "
                    "best of single / batched, windowed / table; field additions, sorting and the bucket reduction are not credited. "
                    "`g1_adds_per_s` elsewhere in this leg keeps the windowed formula so that the rates compare by time",
        }
        return leg

    partial["out"] = out
    # BASELINE.json's metric has three parts (create_proof seconds, MSM G1-adds/s, NTT Fr-ops/s, all at k = 24): `value` is the
    # third; the other two, and the zkWasm-shaped legs, are repeated here inside `config` -- the part of the line every summary keeps
    headline = out["config"].setdefault("headline", {"ntt_fr_ops_per_s_k%d" % log_n: value, "ntt_hbm_roofline_frac": achieved_gbs / HBM_PEAK_GBS})

    def seconds_of(leg, *path):
        for name in path:
            leg = leg.get(name) if isinstance(leg, dict) else None
        return leg

    if args.full and not args.no_msm:
        for key, mlog, msteps, mbatch, what in (
                ("msm", args.msm_log_n, args.msm_steps, 8, "BASELINE configs[1]: 2^%d BN254 G1 MSM, uniform 254-bit scalars, resident in HBM" % args.msm_log_n),
                ("msm_k24", 24 if (args.k24 and args.msm_log_n != 24) else 0, 3, 0,
                 "the metric's k = 24 size: 2^24 BN254 G1 MSM, uniform 254-bit scalars, resident in HBM")):
            if not mlog:
                continue
            try:
                out[key] = dict(workload=what, **msm_leg(mlog, msteps, mbatch))
            except Exception as e:  # noqa: BLE001 - the primary (NTT) line must still be printed
                out[key] = leg_failed(key, e)
            torch.cuda.empty_cache()
            headline["%s_g1_adds_per_s" % key] = seconds_of(out[key], "over_shifted_base_table", "g1_adds_executed_per_s")
            headline["%s_ms" % key] = seconds_of(out[key], "over_shifted_base_table", "ms_per_msm")
            headline["%s_alu_roofline_frac" % key] = seconds_of(out[key], "alu_roofline", "frac")

    def evalh_roofline(pk, phases_s):
        """evaluate_h against both of its rooflines (algorithmic bytes = 32 * (distinct columns read + 1) *
        2^extended_k; products per row from the generated program): the phase's synchronised wall time, descriptor staging
        included"""
        st = getattr(pk, "evalh_stats", None)
        if not st or not phases_s.get("evaluate_h") or pk.coset is not None:
            return None
        size, t = pk.domain.extended_n, phases_s["evaluate_h"]
        alg = 32 * (st["vectors_read"] + 1) * size
        muls = st["products_per_row"] * size / t
        return {"bound": "hbm", "achieved": alg / t / 1e9, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": alg / t / 1e9 / HBM_PEAK_GBS,
                "algorithmic_bytes": alg, "distinct_vectors_read": st["vectors_read"], "seconds": t,
                "kernel": "h2_evalh_gen x %d (gates + permutation / lookup / shuffle terms, generated by the library: csrc/evalh_gen.cpp)" % st["stages"],
                "alu": {"products_per_row": st["products_per_row"], "products_per_row_as_written": st["reference_products_per_row"],
                        "max_registers": st["max_registers"], "achieved_mul_per_s": muls, "peak_mul_per_s": MUL_HW_BOUND,
                        "frac": muls / MUL_HW_BOUND, "frac_of_multiplier_in_a_loop": muls / MUL_MEASURED},
                "limiter": "integer VALU: the field products of the gate and argument terms, not HBM"}

    def comm_summary(D, phases_s):
        """N > 1: what rank 0's collectives cost in the phase-split proof (prover.Device.last_comm: every collective bracketed by
        stream synchronisations, the asynchronous broadcasts measured serialised), next to the phase's whole time -- the part of
        a scaling curve that is links, not kernels.  MAX over ranks of the per-phase communication seconds."""
        comm = getattr(D, "last_comm", None)
        if dist is None or not comm:
            return None
        names = list(phases_s)
        t = torch.tensor([comm.get(n, {}).get("seconds", 0.0) for n in names], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        worst = [float(v) for v in t.tolist()]
        return {
            "what": "per phase: seconds inside collectives (max over ranks; measured serialised in the phase-split proof -- the timed "
                    "proofs overlap the bulk broadcasts with compute), the phase's whole time, payload bytes and calls of rank 0",
            "phases": {n: {"comm_ms": round(w * 1e3, 3), "phase_ms": round(phases_s[n] * 1e3, 2),
                           "bytes": comm.get(n, {}).get("bytes", 0), "calls": comm.get(n, {}).get("calls", 0),
                           "by_collective_ms": {c: round(v * 1e3, 3) for c, v in comm.get(n, {}).get("by_collective", {}).items()}}
                       for n, w in zip(names, worst)},
            "comm_ms_total": round(sum(worst) * 1e3, 2), "phases_ms_total": round(sum(phases_s.values()) * 1e3, 2),
        }

    # ---------------------------------------------------------------- create_proof legs (configs[3] k = 22; configs[4]'s k = 24)
    def prove_leg(pk_k, steps, verify):
        from halo2_gpu_specific_amd import circuits, prover
        from halo2_gpu_specific_amd.rng import ProverRng

        trapdoor = 0x1D0C5F0A3B7E91C2A4D6F8091B2C3D4E5F60718293A4B5C6D7E8F9010203
        # N > 1: ONE proof over all ranks (config 5): prover.Device splits the work over the process group
        D = prover.Device(local_rank, force_collective=dist is not None)
        # Params::unsafe_setup on the device with a fixed toxic scalar: a real (insecure, test-only) SRS, so the timed
        # proofs are valid proofs
        params = prover.Params.unsafe_setup(D, pk_k, trapdoor)
        s0 = time.perf_counter()
        adv, fixed, copies = circuits.mini_plonk_synthesize(pk_k, alloc=D.pinned_columns)
        synth_s = time.perf_counter() - s0
        k0 = time.perf_counter()
        pk = prover.keygen(D, params, circuits.mini_plonk(), fixed, copies)
        D.sync()
        keygen_s = time.perf_counter() - k0
        proof = prover.create_proof_with_shplonk(D, params, pk, adv, ProverRng(1))  # warm-up (arena growth, plan caches)
        assert proof == prover.create_proof_with_shplonk(D, params, pk, adv, ProverRng(1)), "create_proof is not deterministic"
        verified = None
        if verify and rank == 0:
            # outside the timed region: the warm-up proof is accepted by the big-integer verifier of the tests (gate and
            # permutation identities at x, opening equation through the trapdoor)
            import ref_plonk as rp

            vk = rp.Keys()
            vk.cs, vk.dom, vk.s = rp.MiniPlonk, rp.Domain(pk_k, 3), trapdoor
            vk.fixed_commitments, vk.perm_commitments, vk.transcript_repr = pk.fixed_commitments, pk.perm_commitments, pk.transcript_repr
            verified = bool(rp.verify_proof(vk, proof))
            assert verified, "the bench proof was rejected by the verifier"
        phases = {}
        barrier()
        p0 = time.perf_counter()
        for i in range(steps):
            prover.create_proof_with_shplonk(D, params, pk, adv, ProverRng(2 + i))
        D.sync()
        barrier()
        pelapsed = time.perf_counter() - p0
        prover.create_proof_with_shplonk(D, params, pk, adv, ProverRng(1), timings=phases)  # per-phase split (adds syncs: untimed)
        if dist is not None:
            t = torch.tensor([pelapsed], dtype=torch.float64, device=dev)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            pelapsed = float(t[0].item())
        peak_gib = torch.cuda.max_memory_allocated(dev) / 2**30
        # the same witness handed over COMPACT (every cell of this circuit fits 64 bits: 8 bytes per cell over PCIe instead of
        # 32, widened on the device) -- the 32-byte form above is the reference's `Vec<Fr>`; same proof bytes
        compact = None
        if dist is None:
            cadv = D.pinned_columns(len(adv), 1 << pk_k, compact=True)
            for dst, src in zip(cadv, adv):
                dst[:] = src[:, 0]
            cproof = prover.create_proof_with_shplonk(D, params, pk, cadv, ProverRng(1))
            D.sync()
            c0 = time.perf_counter()
            for i in range(steps):
                prover.create_proof_with_shplonk(D, params, pk, cadv, ProverRng(2 + i))
            D.sync()
            compact = {"seconds": (time.perf_counter() - c0) / steps, "same_proof_bytes": bool(cproof == proof)}
            assert cproof == proof, "the compact witness changed the proof"
            del cadv
        host_api = None
        if dist is None and pk_k <= 22 and not os.environ.get("H2_BENCH_NO_HOST_API"):
            # the LITERAL drop-in's data flow, measured: every polynomial a host vector, every vector operation one
            # host-slice entry point (the calls integration/hip.rs binds; halo2-gpu-specific_amd/host_api.py), the SRS
            # registered once -- a PCIe round trip per call.  Same SRS / witness / randomness: the same proof bytes.
            from halo2_gpu_specific_amd import host_api as ha

            host_api = {"what": "host vectors + one host-slice C-ABI call per vector operation (h2_ntt, h2_intt, h2_msm over the "
                                "registered SRS, h2_evaluate_h_coeff, h2_extended_to_coeff, h2_lincomb, ...): what `--features hip` as "
                                "patched executes; the passes the reference leaves to rayon run through host-slice entry points too "
                                "(no CPU arithmetic here).  `pageable`: the vectors in ordinary memory (a Rust Vec); `pinned`: in "
                                "page-locked memory (an allocator over h2_host_alloc_pinned): the same calls, DMA transfers"}
            for mode in ("pageable", "pinned"):
                import gc

                gc.collect()
                H = ha.HostApiDevice(local_rank, pinned=(mode == "pinned"))
                hparams = ha.params_like(H, params)
                hpk = prover.keygen(H, hparams, circuits.mini_plonk(), fixed, copies)
                hproof = prover.create_proof_with_shplonk(H, hparams, hpk, adv, ProverRng(1))      # warm-up (device copies, tables)
                # three timed proofs, the MEDIAN one reported with its own call times (the host side of this leg allocates and
                # frees ~30 blocks of 128 MiB per proof: single proofs vary by 10-20 % from run to run)
                runs = []
                for _ in range(3):
                    H.L.calls.clear()
                    H.L.R.reset()
                    h0 = time.perf_counter()
                    hproof = prover.create_proof_with_shplonk(H, hparams, hpk, adv, ProverRng(1))
                    hsec = time.perf_counter() - h0
                    runs.append((hsec, H.L.R.busy_seconds, {n: round(v * 1e3, 2) for n, v in sorted(H.L.R.by_call.items())},
                                 dict(sorted(H.L.calls.items()))))
                    assert hproof == proof, "the host-slice data flow changed the proof"
                hsec, in_lib, by_call, calls = sorted(runs, key=lambda r: r[0])[1]
                hphases = {}
                H.L.R.reset()
                prover.create_proof_with_shplonk(H, hparams, hpk, adv, ProverRng(1), timings=hphases)
                if os.environ.get("H2_BENCH_DEBUG"):
                    sys.stderr.write("%s phases run, library ms by call: %s\n" % (mode, {n: round(v * 1e3, 1) for n, v in sorted(H.L.R.by_call.items())}))
                host_api[mode] = {
                    "seconds": hsec, "seconds_each": [round(r[0], 4) for r in runs], "proof_bytes_equal": bool(hproof == proof),
                    "ratio_to_resident": hsec / (pelapsed / steps),
                    # wall time with at least one C-ABI call executing; the rest is the host's own handling of its vectors
                    # (allocating, first-touching, freeing 128 MiB blocks: what the reference's Vecs cost it too)
                    "seconds_inside_library_calls": in_lib, "seconds_host_vector_handling": hsec - in_lib,
                    "library_ms_by_call_summed_over_threads": by_call,
                    "phases_ms": {n: round(v * 1e3, 2) for n, v in hphases.items()}, "calls_per_proof": calls,
                }
                assert hproof == proof, "the host-slice data flow changed the proof"
                del hpk, hparams, H
                # (the leg's objects sit in reference cycles: collected NOW -- their finalizers unregister and free ~40 host and
                # device vectors -- not in the middle of the next leg's proofs)
                import gc

                gc.collect()
        return {
            "k": pk_k,
            "compact_witness": compact,
            "host_slice_api": host_api,
            "seconds": pelapsed / steps,
            # the reference times witness synthesis INSIDE create_proof (plonk/prover.rs:1525-1781); here it is a host
            # (numpy) pass outside `seconds`, reported next to it; keygen likewise
            "witness_synthesis_seconds": synth_s,
            "keygen_seconds": keygen_s,
            "seconds_with_synthesis": pelapsed / steps + synth_s,
            "scaling": "strong" if world > 1 else "n/a",
            "sharding": prover.sharding_description(D),
            "proof_bytes": len(proof),
            "verified": verified,
            "phases_ms": {n: round(v * 1e3, 2) for n, v in phases.items()},
            "communication": comm_summary(D, phases),
            "evaluate_h": {"roofline": evalh_roofline(pk, phases)},
            "steps": steps,
            "peak_device_memory_gib": round(peak_gib, 1),
            "srs_shifted_base_tables_gib": round(params.table_bytes / 2**30, 1),   # library memory, not in the peak above
            "srs": "Params::unsafe_setup on the device with a fixed trapdoor (g[i] = [s^i]G, g_lagrange[i] = [l_i(s)]G)",
        }

    # ---------------------------------------------------------------- wide circuit (zkWasm-shaped): 64 advice columns, degree 5,
    # 8 logup range lookups -- with every extended coset resident, and under a memory budget that forces the coset-by-coset
    # route with the proving key's coset tables evicted and rebuilt (same proof bytes)
    def wide_leg(pk_k, quads, steps, only_resident=False):
        import hashlib

        from halo2_gpu_specific_amd import circuits, prover
        from halo2_gpu_specific_amd.rng import ProverRng

        trapdoor = 0x1D0C5F0A3B7E91C2A4D6F8091B2C3D4E5F60718293A4B5C6D7E8F9010203
        cs = circuits.wide(quads)
        res = {"k": pk_k, "advice_columns": 4 * quads, "fixed_columns": 2, "lookups": quads // 2, "degree": cs.degree(),
               "workload": "circuits.wide(%d): %d advice columns, q * (a b c - d) per quad, %d logup range lookups of two columns each "
                           "into a 2^16-row table, equality on two columns, 2^%d rows, KZG/SHPLONK" % (quads, 4 * quads, quads // 2, pk_k)}
        proofs = {}
        # N > 1: ONE proof over all ranks (degree 5 -> 4 cosets over the ranks, every MSM range-split): a single "sharded" mode
        modes = ("resident", "budgeted") if dist is None else ("sharded",)
        if only_resident and dist is None:
            modes = ("resident",)
        for mode in modes:
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats(dev)
            D0 = prover.Device(local_rank, force_collective=dist is not None)
            if mode != "budgeted":
                D = D0
            else:
                dom = prover.Domain(pk_k, cs.degree())
                budget = prover.footprint(cs, dom, 1)["cosets"]
                D = prover.Device(local_rank, mem_budget=budget)
                res[mode + "_budget_gib"] = round(budget / 2**30, 2)
            params = prover.Params.unsafe_setup(D, pk_k, trapdoor)
            s0 = time.perf_counter()
            adv, fixed, copies = circuits.wide_synthesize(pk_k, quads, alloc=D.pinned_columns)
            synth_s = time.perf_counter() - s0
            k0 = time.perf_counter()
            pk = prover.keygen(D, params, cs, fixed, copies)
            D.sync()
            keygen_s = time.perf_counter() - k0
            proof = prover.create_proof_with_shplonk(D, params, pk, adv, ProverRng(1))      # warm-up
            proofs[mode] = proof
            D.sync()
            barrier()
            p0 = time.perf_counter()
            for i in range(steps):
                prover.create_proof_with_shplonk(D, params, pk, adv, ProverRng(2 + i))
            D.sync()
            barrier()
            sec = time.perf_counter() - p0
            if dist is not None:
                t = torch.tensor([sec], dtype=torch.float64, device=dev)
                dist.all_reduce(t, op=dist.ReduceOp.MAX)
                sec = float(t[0].item())
            sec /= steps
            phases = {}
            prover.create_proof_with_shplonk(D, params, pk, adv, ProverRng(1), timings=phases)
            # up to k = 20 the advice columns' inverse transforms and extensions run on a SIDE stream under the lookup and
            # permutation phases (prover.Device.intt_on_side_stream): whichever phase they happen to overlap is charged with
            # them above.  The same proof with that work kept on the compute stream attributes every kernel to its own phase
            serial_phases = None
            if pk_k <= 20 and dist is None:
                side_before = os.environ.get("H2_SIDE_INTT")     # (the caller's own setting comes back afterwards)
                os.environ["H2_SIDE_INTT"] = "0"
                try:
                    serial_phases = {}
                    prover.create_proof_with_shplonk(D, params, pk, adv, ProverRng(1), timings=serial_phases)
                finally:
                    if side_before is None:
                        del os.environ["H2_SIDE_INTT"]
                    else:
                        os.environ["H2_SIDE_INTT"] = side_before
            res[mode] = {
                "residency": pk.residency, "seconds": sec, "witness_synthesis_seconds": synth_s, "keygen_seconds": keygen_s,
                "phases_ms": {n: round(v * 1e3, 2) for n, v in phases.items()},
                "phases_ms_without_side_stream_overlap": ({n: round(v * 1e3, 2) for n, v in serial_phases.items()}
                                                          if serial_phases else None),
                "peak_device_memory_gib": round(torch.cuda.max_memory_allocated(dev) / 2**30, 2),
                "library_memory_gib": round(L.h2_library_memory_bytes() / 2**30, 2),
                "proof_sha256": hashlib.sha256(proof).hexdigest(), "proof_bytes": len(proof),
                "evaluate_h": {"roofline": evalh_roofline(pk, phases)},
                "communication": comm_summary(D, phases),
            }
            if dist is not None:
                res[mode]["sharding"] = prover.sharding_description(D)
                res[mode]["scaling"] = "strong"
            if mode == "resident":
                # the same proof with the columns that fit 64 bits handed over COMPACT (8 bytes per cell over PCIe instead of
                # 32, widened on the device: h2_dev_widen_u64) -- the same proof bytes
                cadv = [np.ascontiguousarray(a[:, 0]) if not a[:, 1:].any() else a for a in adv]
                ncompact = sum(1 for a in cadv if a.ndim == 1)
                pinned = D.pinned_columns(ncompact, 1 << pk_k, compact=True)
                it = iter(pinned)
                for i, a in enumerate(cadv):
                    if a.ndim == 1:
                        dst = next(it)
                        dst[:] = a
                        cadv[i] = dst
                cproof = prover.create_proof_with_shplonk(D, params, pk, cadv, ProverRng(1))
                D.sync()
                c0 = time.perf_counter()
                for i in range(steps):
                    prover.create_proof_with_shplonk(D, params, pk, cadv, ProverRng(2 + i))
                D.sync()
                cphases = {}
                csec = (time.perf_counter() - c0) / steps
                prover.create_proof_with_shplonk(D, params, pk, cadv, ProverRng(1), timings=cphases)
                res["resident_compact_witness"] = {
                    "seconds": csec, "compact_columns": ncompact, "same_proof_bytes": bool(cproof == proof),
                    "phases_ms": {n: round(v * 1e3, 2) for n, v in cphases.items()},
                    "what": "columns whose cells all fit 64 bits cross PCIe as 8 bytes per cell and are widened on the device",
                }
                assert cproof == proof, "the compact witness changed the proof"
                del cadv, pinned
            if pk.coset is not None:
                res[mode]["coset_table_rebuilds"] = pk.coset.misses
            if mode != "budgeted" and rank == 0:
                import ref_plonk as rp

                vk = rp.Keys()
                vk.cs, vk.dom, vk.s = rp.wide_class(quads), rp.Domain(pk_k, cs.degree()), trapdoor
                vk.fixed_commitments, vk.perm_commitments, vk.transcript_repr = pk.fixed_commitments, pk.perm_commitments, pk.transcript_repr
                res["verified"] = bool(rp.verify_proof(vk, proof))
                assert res["verified"], "the wide-circuit proof was rejected by the verifier"
            del pk, params, adv, fixed, D, D0
            L.h2_release_plans()
        if dist is None and "budgeted" in proofs:
            res["same_proof_bytes"] = proofs["resident"] == proofs["budgeted"]
            assert res["same_proof_bytes"], "the memory-budgeted route changed the proof"
        return res

    # N > 1: the proof legs are ONE proof over all ranks -- collectives on the data path.  A rank that fails or stalls
    # there would leave the others waiting inside RCCL for good, and the line above would never be printed: a watchdog
    # thread prints what has been measured and ends the process when a leg overruns its budget.
    watchdog_done = None
    if world > 1 and args.full:
        import threading

        watchdog_done = threading.Event()
        budget = float(os.environ.get("H2_BENCH_PROOF_BUDGET_S", "360"))

        def watchdog():
            if watchdog_done.wait(budget):
                return
            if rank == 0:
                out.setdefault("create_proof", {"error": "the multi-rank proof legs did not finish within %.0f s" % budget})
                print(json.dumps(out), flush=True)
            # a stalled collective is a FAILED run: every rank ends non-zero so that torchrun / the harness see it
            # (no restart or re-exec from a process that has initialised the GPU)
            os._exit(2)

        threading.Thread(target=watchdog, daemon=True).start()

    if args.full and args.wide_k:
        try:
            out["create_proof_wide"] = wide_leg(args.wide_k, args.wide_quads, 2)
        except Exception as e:  # noqa: BLE001 - the primary (NTT) line must still be printed
            out["create_proof_wide"] = leg_failed("create_proof_wide", e)
        torch.cuda.empty_cache()
        headline["create_proof_wide_k%d_seconds" % args.wide_k] = seconds_of(out["create_proof_wide"], "resident" if dist is None else "sharded", "seconds")
        headline["create_proof_wide_k%d_compact_witness_seconds" % args.wide_k] = seconds_of(out["create_proof_wide"], "resident_compact_witness", "seconds")
    if args.full and args.wide_k22 and args.wide_k != 22 and dist is None:      # (N = 1 only: 8 GiB of witness per rank and a fifth proof leg
        #                                                              would eat the multi-rank legs' time budget for no new information)
        # the zkWasm-sized leg: 64 advice columns x 2^22 rows (8 GiB of 32-byte cells; 2 GiB handed over compact)
        try:
            out["create_proof_wide_k22"] = wide_leg(22, args.wide_quads, 2, only_resident=True)
        except Exception as e:  # noqa: BLE001
            out["create_proof_wide_k22"] = leg_failed("create_proof_wide_k22", e)
        torch.cuda.empty_cache()
        headline["create_proof_wide_k22_seconds"] = seconds_of(out["create_proof_wide_k22"], "resident" if dist is None else "sharded", "seconds")
        headline["create_proof_wide_k22_compact_witness_seconds"] = seconds_of(out["create_proof_wide_k22"], "resident_compact_witness", "seconds")

    for key, kk, steps in (("create_proof", args.prove_k, args.prove_steps), ("create_proof_k24", 24 if args.k24 else 0, 2)):
        if not args.full or not kk or (key == "create_proof_k24" and args.prove_k == 24):
            continue
        try:
            leg = prove_leg(kk, steps, verify=True)
            leg["workload"] = ("BASELINE configs[%d]: mini-PLONK (examples/simple-example-2.rs) with 2^%d rows, KZG/SHPLONK, "
                               "witness in pinned host memory, SRS / proving key resident in HBM" % (3 if kk != 24 else 4, kk))
            out[key] = leg
        except Exception as e:  # noqa: BLE001 - the primary (NTT) line must still be printed
            out[key] = leg_failed(key, e)
        torch.cuda.empty_cache()
        headline["create_proof_k%d_seconds" % kk] = seconds_of(out[key], "seconds")
        headline["create_proof_k%d_evaluate_h_alu_frac" % kk] = seconds_of(out[key], "evaluate_h", "roofline", "alu", "frac")
    # the same k = 22 proof from a host that is not Python: tools/h2prove (plain C++ over the C ABI alone, a process of its own;
    # its bytes are pinned by tests/test_gpu_h2prove.py) -- seconds next to prover.py's
    if args.full and world == 1 and args.prove_k and "error" not in out.get("create_proof", {"error": 1}):
        try:
            import subprocess

            tool = os.path.join(ROOT, "tools", "h2prove")
            if not os.path.exists(tool):
                subprocess.check_call(["make", "-C", os.path.join(ROOT, "tools"), "h2prove"], stdout=subprocess.DEVNULL)
            torch.cuda.synchronize()
            res = subprocess.run([tool, str(args.prove_k), "1", "--reps", "3"], capture_output=True, text=True, timeout=600)
            fields = [ln for ln in res.stdout.splitlines() if ln.startswith("k ")][0].split()
            stats = dict(zip(fields[0::2], fields[1::2]))
            out["create_proof"]["h2prove_cxx"] = {
                "what": "tools/h2prove.cpp: keygen + create_proof (SHPLONK) in plain C++ over include/halo2_hip.h alone -- no Python, no "
                        "torch, no HIP headers; one stream, recycled h2_dev_alloc blocks",
                "seconds": float(stats["create_proof_s"]), "keygen_seconds": float(stats["keygen_s"]), "proof_bytes": int(stats["proof_bytes"])}
        except Exception as e:  # noqa: BLE001 - a side figure: the line is printed without it
            out["create_proof"]["h2prove_cxx"] = {"error": "%s: %s" % (type(e).__name__, e)}
    # N > 1: the same circuit as INDEPENDENT proofs, one per GPU (prover.Device.replica: a singleton group, no collective on
    # the data path) -- the throughput a node reaches when there are at least N proofs to make, next to the latency form above
    if args.full and world > 1 and args.prove_k and "error" not in out.get("create_proof", {"error": 1}):
        try:
            from halo2_gpu_specific_amd import circuits, prover
            from halo2_gpu_specific_amd.rng import ProverRng

            kk = args.prove_k
            D = prover.Device.replica(local_rank)
            params = prover.Params.unsafe_setup(D, kk, 0x1D0C5F0A3B7E91C2A4D6F8091B2C3D4E5F60718293A4B5C6D7E8F9010203)
            adv, fixed, copies = circuits.mini_plonk_synthesize(kk, alloc=D.pinned_columns)
            pk = prover.keygen(D, params, circuits.mini_plonk(), fixed, copies)
            proof = prover.create_proof_with_shplonk(D, params, pk, adv, ProverRng(1))
            D.sync()
            barrier()
            r0 = time.perf_counter()
            for i in range(args.prove_steps):
                prover.create_proof_with_shplonk(D, params, pk, adv, ProverRng(2 + i))
            D.sync()
            barrier()
            rsec = time.perf_counter() - r0
            t = torch.tensor([rsec], dtype=torch.float64, device=dev)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            rsec = float(t[0].item())
            one = out["create_proof"].get("seconds")
            out["create_proof_replicas"] = {
                "what": "one independent mini-PLONK proof per GPU at k = %d, no collective on the data path: N x K proofs between two "
                        "barriers, max over ranks" % kk,
                "k": kk, "proofs_per_s": world * args.prove_steps / rsec, "seconds_per_proof_per_gpu": rsec / args.prove_steps,
                "scaling": "weak", "proof_bytes": len(proof),
                "one_proof_over_all_ranks_seconds": one,
                "one_proof_over_all_ranks_proofs_per_s": (1.0 / one) if one else None,
            }
            headline["create_proof_k%d_replicas_proofs_per_s" % kk] = out["create_proof_replicas"]["proofs_per_s"]
            del pk, params, adv, D
        except Exception as e:  # noqa: BLE001
            out["create_proof_replicas"] = leg_failed("create_proof_replicas", e)
        torch.cuda.empty_cache()
    if watchdog_done is not None:
        watchdog_done.set()

    # ---------------------------------------------------------------- CPU baseline (rank 0, N = 1 only)
    if args.full and world == 1 and not args.no_cpu_baseline:
        try:
            from h2util import Oracle  # the oracle is only the timed CPU baseline here, never the product path

            oracle = Oracle.get()
            cores = os.cpu_count() or 1
            # what this process may actually run on: its affinity mask and the cgroup's CPU quota (a container that shows
            # 256 CPUs may be granted far fewer)
            try:
                affinity = len(os.sched_getaffinity(0))
            except (AttributeError, OSError):
                affinity = cores
            quota = None
            try:
                with open("/sys/fs/cgroup/cpu.max") as f:
                    q, per = f.read().split()[:2]
                    quota = None if q == "max" else float(q) / float(per)
            except (OSError, ValueError):
                pass
            cores = max(1, min(cores, affinity))
            clog = log_n                       # the GPU's own size (2^24)
            wc = fr_limbs(pow(ROOT_OF_UNITY, 1 << (28 - clog), R_MOD))
            # team size: probed on a 2^20 transform (a fraction of a second each), then the full size is timed with the best
            plog = min(clog, 20)
            xp = oracle.random_fr(8, 1 << plog)
            wp = fr_limbs(pow(ROOT_OF_UNITY, 1 << (28 - plog), R_MOD))
            best_t, best_th, probe = None, cores, {}
            for th in sorted({cores, max(cores // 2, 1), max(cores // 4, 1), min(cores, 32), min(cores, 16)}, reverse=True):
                oracle.best_fft(xp, wp, plog, threads=th)          # warm the team
                c0 = time.perf_counter()
                oracle.best_fft(xp, wp, plog, threads=th)
                dt = time.perf_counter() - c0
                probe[th] = dt
                if best_t is None or dt < best_t:
                    best_t, best_th = dt, th
            # one core: best_fft_cpu_st (arithmetic.rs:952-1009) on the probe size, median of 3 -- the per-core cost
            st = []
            for _ in range(3):
                c0 = time.perf_counter()
                oracle.best_fft_st(xp, wp, plog)
                st.append(time.perf_counter() - c0)
            st_t = sorted(st)[1]
            del xp
            x = oracle.random_fr(7, 1 << clog)
            oracle.best_fft(x, wc, clog, threads=best_th)          # 1 warm-up + median of >= 5
            times, c0 = [], time.perf_counter()
            while len(times) < 5 or (len(times) < 7 and time.perf_counter() - c0 < 10.0):
                r0 = time.perf_counter()
                oracle.best_fft(x, wc, clog, threads=best_th)
                times.append(time.perf_counter() - r0)
            ct = sorted(times)[len(times) // 2]
            reps = len(times)
            ops = lambda lg: 3 * ((1 << lg) // 2) * lg  # noqa: E731
            # every hardware thread, as BASELINE.md asks: at the full size when the probe says it finishes in seconds
            # (libgomp on 256 SMT threads can take a minute per transform), always at the probe size
            all_t = {"threads": cores, "log_n": plog, "seconds": probe[cores], "fr_ops_per_s": ops(plog) / probe[cores]}
            if best_th != cores and probe[cores] * (1 << (clog - plog)) * 1.3 < 8.0:
                r0 = time.perf_counter()
                oracle.best_fft(x, wc, clog, threads=cores)
                dt = time.perf_counter() - r0
                all_t = {"threads": cores, "log_n": clog, "seconds": dt, "fr_ops_per_s": ops(clog) / dt}
            elif best_th == cores:
                all_t = {"threads": cores, "log_n": clog, "seconds": ct, "fr_ops_per_s": ops(clog) / ct}
            out["cpu_baseline"] = {
                "value": ops(clog) / ct,
                "unit": "Fr-ops/s",
                "cores": best_th,
                "host_threads_available": cores,
                "cgroup_cpu_quota": quota,
                "omp_wait_policy": os.environ.get("OMP_WAIT_POLICY"),
                "kind": "port",
                "sample": "oracle best_fft (C restatement of arithmetic.rs:556-705: serial bit reversal as the reference, the "
                "butterflies of its recursion scheduled statically over the team) on one forward 2^%d NTT (the GPU's size), "
                "1 warm-up + median of %d reps, %.3f s each (includes the oracle wrapper's input copy); team size probed on 2^%d"
                % (clog, reps, ct, plog),
                "reps_seconds": [round(t, 4) for t in times],
                "team_probe_seconds_2p%d" % plog: {str(th): round(t, 4) for th, t in sorted(probe.items())},
                "all_threads": all_t,
                "single_thread": {"what": "best_fft_cpu_st (arithmetic.rs:952-1009) on 2^%d points, median of 3" % plog,
                                  "seconds": st_t, "fr_ops_per_s": ops(plog) / st_t},
            }
            del x

            # the MSM leg's CPU twin: best_multiexp (arithmetic.rs:465-492, c = ceil(ln n) per thread chunk) at the GPU's 2^20
            if "msm" in out:
                mlog_c = min(args.msm_log_n, 20)
                ms, mp = oracle.random_fr(11, 1 << mlog_c), oracle.random_g1(12, 1 << mlog_c)
                best_m, best_mth = None, cores
                for th in sorted({cores, min(cores, 128), min(cores, 64)}, reverse=True):
                    c0 = time.perf_counter()
                    oracle.best_multiexp(ms, mp, threads=th)
                    dt = time.perf_counter() - c0
                    if best_m is None or dt < best_m:
                        best_m, best_mth = dt, th
                out["msm"]["cpu_baseline"] = {
                    "pairs_per_s": (1 << mlog_c) / best_m,
                    "cores": best_mth,
                    "kind": "port",
                    "sample": "oracle best_multiexp on 2^%d uniform pairs (the GPU's size), best of 3 team sizes, %.3f s" % (mlog_c, best_m),
                }
            # create_proof's CPU twin: the same host orchestration with every kernel replaced by the oracle's restatement of
            # the reference's CPU loop (tests/oracle_prover.py), same SRS / witness / randomness: the bytes must be equal
            if "create_proof" in out and args.cpu_prove_k:
                import oracle_prover as op
                from halo2_gpu_specific_amd import circuits, prover
                from halo2_gpu_specific_amd.rng import ProverRng

                kc = args.cpu_prove_k
                D = prover.Device(local_rank)
                params = prover.Params.unsafe_setup(D, kc, 0x1D0C5F0A3B7E91C2A4D6F8091B2C3D4E5F60718293A4B5C6D7E8F9010203)
                adv, fixed, copies = circuits.mini_plonk_synthesize(kc)
                pk = prover.keygen(D, params, circuits.mini_plonk(), fixed, copies)
                prover.create_proof_with_shplonk(D, params, pk, adv, ProverRng(1))
                g0 = time.perf_counter()
                proof = prover.create_proof_with_shplonk(D, params, pk, adv, ProverRng(3))
                D.sync()
                gpu_s = time.perf_counter() - g0
                cpu = op.OracleDevice()
                cparams = op.params_like(cpu, params)
                c0 = time.perf_counter()
                cpk = op.keygen(cpu, cparams, circuits.mini_plonk(), fixed, copies)
                ck = time.perf_counter() - c0
                c0 = time.perf_counter()
                want = prover.create_proof_with_shplonk(cpu, cparams, cpk, adv, ProverRng(3))
                ct = time.perf_counter() - c0
                out["create_proof"]["cpu_baseline"] = {
                    "k": kc, "seconds": ct, "keygen_seconds": ck, "cores": cpu.L.threads, "host_threads_available": cores,
                    "kind": "port", "gpu_seconds_same_circuit": gpu_s, "proof_bytes_equal": bool(proof == want),
                    "sample": "one mini-PLONK create_proof (SHPLONK) at k = %d on the host cores: the host orchestration of prover.py "
                    "over the C oracle's loops (oracle/oracle.c; serial scans and Kate divisions as the reference), same SRS, "
                    "witness and randomness as the device proof next to it; at k = 24 the same comparison is "
                    "tests/test_gpu_cpu_prover.py (135 s of CPU on 32 threads)" % kc,
                }
        except Exception as e:  # noqa: BLE001 - the line must still be printed
            if "cpu_baseline" in out:
                out["cpu_baseline_error"] = "%s: %s" % (type(e).__name__, e)
            out.setdefault("cpu_baseline", {"error": "%s: %s" % (type(e).__name__, e)})

    # The other two parts of BASELINE's metric (MSM G1-adds/s, create_proof seconds) and the ALU accounting, once more as FLAT
    # scalar keys of `config` / `roofline`: a summary that keeps only the scalars of those two objects (the driver's `parsed`
    # does; round 5's record lost `config.headline` and `roofline.alu` that way) still answers the whole metric.
    def _num(x):
        return x if isinstance(x, (int, float)) and not isinstance(x, bool) else None

    cfg, roof = out["config"], out["roofline"]
    roof["alu_frac"] = roof["alu"]["frac"]
    roof["alu_achieved_mul_per_s"] = roof["alu"]["achieved_mul_per_s"]
    roof["alu_peak_mul_per_s"] = roof["alu"]["peak_mul_per_s"]
    for flat, leg, path in (
            ("msm_2p%d_ms" % args.msm_log_n, "msm", ("over_shifted_base_table", "ms_per_msm")),
            ("msm_2p%d_g1_adds_per_s" % args.msm_log_n, "msm", ("over_shifted_base_table", "g1_adds_executed_per_s")),
            ("msm_2p%d_alu_frac" % args.msm_log_n, "msm", ("alu_roofline", "frac")),
            ("msm_k24_ms", "msm_k24", ("over_shifted_base_table", "ms_per_msm")),
            ("msm_k24_g1_adds_per_s", "msm_k24", ("over_shifted_base_table", "g1_adds_executed_per_s")),
            ("msm_k24_alu_frac", "msm_k24", ("alu_roofline", "frac")),
            ("create_proof_k%d_s" % args.prove_k, "create_proof", ("seconds",)),
            ("create_proof_k%d_evalh_alu_frac" % args.prove_k, "create_proof", ("evaluate_h", "roofline", "alu", "frac")),
            ("create_proof_k%d_host_slice_pinned_s" % args.prove_k, "create_proof", ("host_slice_api", "pinned", "seconds")),
            ("create_proof_k%d_host_slice_pageable_s" % args.prove_k, "create_proof", ("host_slice_api", "pageable", "seconds")),
            ("create_proof_k%d_host_slice_pinned_in_library_s" % args.prove_k, "create_proof", ("host_slice_api", "pinned", "seconds_inside_library_calls")),
            ("create_proof_k%d_host_slice_pageable_in_library_s" % args.prove_k, "create_proof", ("host_slice_api", "pageable", "seconds_inside_library_calls")),
            ("create_proof_k%d_h2prove_cxx_s" % args.prove_k, "create_proof", ("h2prove_cxx", "seconds")),
            ("create_proof_k%d_cpu_s" % args.cpu_prove_k, "create_proof", ("cpu_baseline", "seconds")),
            ("create_proof_k24_s", "create_proof_k24", ("seconds",)),
            ("create_proof_k24_evalh_alu_frac", "create_proof_k24", ("evaluate_h", "roofline", "alu", "frac")),
            ("wide_k%d_s" % args.wide_k, "create_proof_wide", ("resident" if dist is None else "sharded", "seconds")),
            ("wide_k%d_compact_s" % args.wide_k, "create_proof_wide", ("resident_compact_witness", "seconds")),
            ("wide_k22_s", "create_proof_wide_k22", ("resident", "seconds")),
            ("wide_k22_compact_s", "create_proof_wide_k22", ("resident_compact_witness", "seconds")),
            ("replicas_proofs_per_s", "create_proof_replicas", ("proofs_per_s",))):
        v = _num(seconds_of(out.get(leg), *path))
        if v is not None:
            cfg[flat] = v
    if rank == 0:
        print(json.dumps(out))
    if dist is not None:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
