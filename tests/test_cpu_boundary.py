"""CPU-only checks of the drop-in boundary: the C-ABI library loads, exports every symbol that
include/halo2_hip.h declares, reports errors the documented way without a GPU, and the host-side
logic (device-pool env, sharding plan, host point fold) behaves.  No GPU compute is launched."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import halo2_gpu_specific_amd as h2
from halo2_gpu_specific_amd import parallel
from halo2_gpu_specific_amd._lib import SYMBOLS
from h2util import ROOT, Oracle, arr_to_points, to_mont


def declared_symbols():
    text = open(os.path.join(ROOT, "include", "halo2_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(h2_[a-z0-9_]+)\s*\(", text)))


def test_library_exports_every_declared_symbol():
    L = h2.lib()
    names = declared_symbols()
    assert len(names) >= 30
    for name in names:
        assert hasattr(L, name), "libhalo2_hip.so does not export %s" % name
        assert name in SYMBOLS, "python binding table misses %s" % name
    assert sorted(SYMBOLS) == names
    # ... and the names prover.py gives Device.eval_op's operations are the header's H2_OP_* values
    from halo2_gpu_specific_amd import prover

    ops = dict(re.findall(r"\bH2_(OP_[A-Z_]+)\s*=\s*(\d+)", open(os.path.join(ROOT, "include", "halo2_hip.h")).read()))
    assert len(ops) == 9 and all(getattr(prover, name) == int(value) for name, value in ops.items()), ops


def test_every_entry_point_cites_the_reference():
    text = open(os.path.join(ROOT, "include", "halo2_hip.h")).read()
    for needle in ("arithmetic.rs:546", "arithmetic.rs:515", "arithmetic.rs:334", "arithmetic.rs:375", "arithmetic.rs:413",
                   "poly/domain.rs:270", "poly/domain.rs:328", "poly/domain.rs:354"):
        assert needle in text


def test_no_gpu_means_loud_error_not_fallback():
    L = h2.lib()
    if L.h2_device_count() > 0:
        pytest.skip("a GPU is visible")
    a = np.zeros((4, 4), dtype=np.uint64)
    w = np.zeros(4, dtype=np.uint64)
    rc = L.h2_ntt(a.ctypes.data, w.ctypes.data, 2)
    assert rc != 0 and L.h2_last_error()
    with pytest.raises(h2.H2Error):
        h2.arithmetic.best_fft(a, w, 2)


def test_argument_validation_without_gpu():
    L = h2.lib()
    assert L.h2_ntt(None, None, 3) == 1  # H2_ERR_INVALID
    out = np.zeros(12, dtype=np.uint64)
    assert L.h2_msm(None, None, 5, 254, out.ctypes.data) == 1
    # n == 0 / max_bits == 0 -> identity without touching a device (arithmetic.rs:346, :421)
    assert L.h2_msm(None, None, 0, 254, out.ctypes.data) == 0
    assert not out[8:].any()  # z == 0
    assert h2.arithmetic.best_multiexp(np.zeros((0, 4), np.uint64), np.zeros((0, 8), np.uint64))[8:].sum() == 0
    with pytest.raises(AssertionError):  # arithmetic.rs:466 assert_eq!(coeffs.len(), bases.len())
        h2.arithmetic.best_multiexp(np.zeros((2, 4), np.uint64), np.zeros((3, 8), np.uint64))
    with pytest.raises(AssertionError):  # arithmetic.rs:569 assert_eq!(n, 1 << log_n)
        h2.arithmetic.best_fft(np.zeros((5, 4), np.uint64), np.zeros(4, np.uint64), 3)


def test_scans_refuse_overlapping_buffers_before_they_touch_a_device():
    """h2_dev_kate_division reads a[0, n) while other workgroups write q[0, n - 1); h2_dev_prefix_product / _sum read f[0, n - 1)
    and write z[0, n): any overlap of the two ranges is H2_ERR_INVALID with a message, checked in front of the device (the
    pointers here are never dereferenced).  Ranges that only touch, and n < 2, pass the check: without a device the call
    then ends as H2_ERR_NO_DEVICE; with one, tests/test_gpu_poly_kernels.py makes the same calls on live buffers."""
    L = h2.lib()
    no_device = L.h2_device_count() == 0
    scalar = np.zeros(4, dtype=np.uint64)
    base, n, fr = 1 << 40, 5000, 32
    kate = lambda a, q, n=n: L.h2_dev_kate_division(a, n, scalar.ctypes.data, q, None)
    scans = [lambda f, z, n=n, fn=fn: fn(f, n, scalar.ctypes.data, z, None) for fn in (L.h2_dev_prefix_product, L.h2_dev_prefix_sum)]

    def refused(rc):
        return rc == 1 and b"must not overlap" in L.h2_last_error()

    assert refused(kate(base, base))                           # equal pointers
    assert refused(kate(base, base + fr))                      # q = a + 32 bytes
    assert refused(kate(base, base - (n - 2) * fr))            # q's last element is a[0]
    assert refused(kate(base, base + (n - 1) * fr))            # q's first element is a[n - 1]
    assert refused(kate(base, base, n=2))
    for scan in scans:
        assert refused(scan(base, base))
        assert refused(scan(base, base + fr))
        assert refused(scan(base, base - (n - 1) * fr))        # z's last element is f[0]
        assert refused(scan(base, base + (n - 2) * fr))        # z's first element is f[n - 2], the last one read
        assert refused(scan(base, base, n=2))
    if no_device:                                              # accepted by the check: the next thing missing is the device
        passed = lambda rc: rc not in (0, 1) and b"overlap" not in L.h2_last_error()
        assert passed(kate(base, base + n * fr)) and passed(kate(base, base - (n - 1) * fr))       # the ranges only touch
        assert passed(kate(base, base, n=1)) and passed(kate(base, base, n=0))
        for scan in scans:
            assert passed(scan(base, base + (n - 1) * fr)) and passed(scan(base, base - n * fr))
            assert passed(scan(base, base, n=1))


def test_evaluate_h_validates_the_descriptor_before_it_touches_memory():
    """h2_evaluate_h / h2_evaluate_h_coeff with extended_k = 29 > 28 and with extended_k = 3 < k = 4 over a 4 KiB `values`:
    H2_ERR_INVALID and a message, with or without a GPU -- the sizes are checked before a slot is leased or a page of `values`
    touched (2^29 elements would be 16 GiB past the buffer).  In a child process: a library that touched them would take the
    process down, and that is to show as this assertion failing."""
    code = (
        "import ctypes, sys; sys.path.insert(0, %r)\n"
        "import numpy as np\n"
        "import halo2_gpu_specific_amd as h2\n"
        "from halo2_gpu_specific_amd import evaluation\n"
        "L = h2.lib()\n"
        "values = np.zeros(4096 // 8, dtype=np.uint64)\n"
        "for name in ('h2_evaluate_h', 'h2_evaluate_h_coeff'):\n"
        "    for k, ek in ((4, 29), (4, 3)):\n"
        "        desc = evaluation.EvalHDesc()\n"
        "        desc.k, desc.extended_k = k, ek\n"
        "        rc = getattr(L, name)(ctypes.byref(desc), values.ctypes.data)\n"
        "        print('CALL', name, ek, rc, bool(L.h2_last_error()), flush=True)\n"
        "print('DONE')\n"
    ) % ROOT
    res = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and "DONE" in res.stdout, res.stdout[-2000:] + res.stderr[-2000:]
    for name in ("h2_evaluate_h", "h2_evaluate_h_coeff"):
        for ek in (29, 3):
            assert "CALL %s %d 1 True" % (name, ek) in res.stdout, res.stdout


def test_missing_extension_fails_loudly(tmp_path):
    code = (
        "import sys; sys.path.insert(0, %r)\n"
        "import halo2_gpu_specific_amd as h2\n"
        "from halo2_gpu_specific_amd import _lib\n"
        "_lib.lib_path = lambda: %r\n"
        "try:\n    h2._lib.lib()\nexcept h2.H2Error as e:\n    print('LOUD', e)\n"
    ) % (ROOT, str(tmp_path / "nope.so"))
    out = subprocess.check_output([sys.executable, "-c", code], text=True)
    assert out.startswith("LOUD") and "no CPU fallback" in out


def test_h2_lib_names_another_build_and_nothing_else(tmp_path):
    """H2_LIB (tools/gen_sanitize.sh: a sanitizer build of the same ABI) replaces the in-tree path; a missing file is the same
    loud error, and the package sets its HIP hardware-queue default without overriding a caller's"""
    code = (
        "import os, sys; sys.path.insert(0, %r)\n"
        "os.environ['H2_LIB'] = %r\n"
        "import halo2_gpu_specific_amd as h2\n"
        "print('QUEUES', os.environ['GPU_MAX_HW_QUEUES'])\n"
        "try:\n    h2.lib()\nexcept h2.H2Error as e:\n    print('LOUD', e)\n"
    ) % (ROOT, str(tmp_path / "elsewhere.so"))
    env = {k: v for k, v in os.environ.items() if k != "GPU_MAX_HW_QUEUES"}
    out = subprocess.check_output([sys.executable, "-c", code], text=True, env=env)
    assert "QUEUES 8" in out and "LOUD" in out and "elsewhere.so" in out and "no CPU fallback" in out
    out = subprocess.check_output([sys.executable, "-c", code], text=True, env=dict(env, GPU_MAX_HW_QUEUES="3"))
    assert "QUEUES 3" in out


def test_library_sets_its_hardware_queue_default_when_loaded():
    """libhalo2_hip.so's load-time constructor: GPU_MAX_HW_QUEUES=8 for a host that reaches HIP only through the library (the
    runtime reads it at its first call), unless the caller has set it"""
    code = (
        "import ctypes, sys\n"
        "libc = ctypes.CDLL(None); libc.getenv.restype = ctypes.c_char_p; libc.getenv.argtypes = [ctypes.c_char_p]\n"
        "before = libc.getenv(b'GPU_MAX_HW_QUEUES')\n"
        "ctypes.CDLL(%r)\n"
        "print('BEFORE', before, 'AFTER', libc.getenv(b'GPU_MAX_HW_QUEUES'))\n"
    ) % h2.lib_path()
    env = {k: v for k, v in os.environ.items() if k != "GPU_MAX_HW_QUEUES"}
    out = subprocess.check_output([sys.executable, "-c", code], text=True, env=env)
    assert "BEFORE None AFTER b'8'" in out, out
    out = subprocess.check_output([sys.executable, "-c", code], text=True, env=dict(env, GPU_MAX_HW_QUEUES="5"))
    assert "BEFORE b'5' AFTER b'5'" in out, out
    out = subprocess.check_output([sys.executable, "-c", code], text=True, env=dict(env, H2_NO_RUNTIME_DEFAULTS="1"))
    assert "BEFORE None AFTER None" in out, out          # the opt-out: the host's environment is left alone


def test_msm_shape_and_scratch():
    L = h2.lib()
    c, W, nb = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32()
    for n, bits in ((1 << 20, 254), (1 << 24, 254), (1 << 14, 16), (3, 254), (1 << 22, 64)):
        assert L.h2_msm_shape(n, bits, ctypes.byref(c), ctypes.byref(W), ctypes.byref(nb)) == 0
        assert W.value * c.value >= bits + 1  # room for the signed-digit carry
        assert nb.value == 1 << (c.value - 1)
        assert L.h2_msm_scratch_bytes(n, bits) > n * W.value * 8


def test_msm_sizing_functions_match_the_recorded_sizes():
    """h2_msm_shape, h2_msm_scratch_bytes and h2_msm_batch_scratch_bytes over a grid of sizes, bounds and batch counts
    (windowed and fused shapes: what is reachable without a table) equal tests/golden/msm_scratch_sizes.json, recorded
    from the library before the shape / scratch-layout helpers were shared: callers size their scratch from these"""
    import json

    knobs = sorted(k for k in os.environ if k.startswith("H2_MSM_"))
    if knobs:
        pytest.skip("the recorded sizes hold for the default shapes; set in this environment: " + ", ".join(knobs))
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    try:
        import gen_msm_scratch_sizes as gen
    finally:
        sys.path.pop(0)
    with open(os.path.join(ROOT, "tests", "golden", "msm_scratch_sizes.json")) as f:
        want = json.load(f)
    assert want["n"] == [1, 255, 1 << 10, (1 << 15) - 1, 1 << 15, (1 << 18) + 3, 1 << 20, 1 << 22, 1 << 24, 1 << 26]
    assert want["max_bits"] == [1, 8, 16, 17, 64, 128, 254, 300] and want["count"] == [1, 2, 8, 64, 100]
    assert (gen.NS, gen.BITS, gen.COUNTS) == (want["n"], want["max_bits"], want["count"])
    got = gen.sizes(h2.lib())
    assert len(got) == len(want["rows"]) == 80
    for g, w in zip(got, want["rows"]):
        assert g == w, (g, w)


NTT_PASS_WIDTHS = {  # the comment in ntt_split: as many 8-bit passes as possible, the remainder first; a remainder of one
    0: [], 1: [1], 2: [2], 3: [3], 4: [4], 5: [5], 6: [6], 7: [7], 8: [8],  # bit (and of two bits up to 2^18) as 9-bit passes at the end
    9: [9], 10: [2, 8], 11: [3, 8], 12: [4, 8], 13: [5, 8], 14: [6, 8], 15: [7, 8], 16: [8, 8], 17: [8, 9], 18: [9, 9],
    19: [3, 8, 8], 20: [4, 8, 8], 21: [5, 8, 8], 22: [6, 8, 8], 23: [7, 8, 8], 24: [8, 8, 8], 25: [8, 8, 9],
    26: [2, 8, 8, 8], 27: [3, 8, 8, 8], 28: [4, 8, 8, 8],
}


def test_ntt_shape_reports_the_documented_plan():
    """h2_ntt_shape, log_n 0 .. 28 and every padding: the pass widths ntt_split documents, summing to log_n; zskip = min(z, B)
    on the first of several passes and 0 elsewhere; the fixed geometry is 8 bits, 4 columns, 256 lanes; radix-4 (and with it
    the constant-operand twiddles) from 2^18 only; a kernel id inside the enumeration"""
    import ntt_matrix_cases as mc

    L = h2.lib()
    assert sorted(NTT_PASS_WIDTHS) == list(range(29))
    for log_n, widths in NTT_PASS_WIDTHS.items():
        for in_log in range(log_n + 1):
            z = log_n - in_log
            passes = mc.ntt_shape(L, log_n, in_log)
            assert [p["bits"] for p in passes] == widths, (log_n, in_log)
            assert sum(p["bits"] for p in passes) == log_n
            for i, p in enumerate(passes):
                assert p["zskip"] == (min(z, p["bits"]) if i == 0 and len(passes) > 1 else 0), (log_n, in_log, i)
                if p["fixed"]:
                    assert (p["bits"], p["log_c"], p["threads"]) == (8, 2, 256) and p["radix4"]
                assert p["radix4"] == (1 if log_n >= 18 else 0), (log_n, p)
                assert p["fixed"] == (1 if log_n >= 18 and p["bits"] == 8 and p["log_c"] == 2 else 0), (log_n, p)
                assert 64 <= p["threads"] <= 512 and p["kernel"] in mc.ALL_KERNELS
                consumed = sum(q["bits"] for q in passes[:i])
                avail = consumed if i + 1 == len(passes) else log_n - consumed - p["bits"]
                assert p["log_c"] <= avail
                last = i + 1 == len(passes)
                if log_n < 18:
                    assert mc.KERNELS[p["kernel"]] == "k_ntt_pass<false>"
                elif p["fixed"] and p["zskip"] == 0:
                    assert mc.KERNELS[p["kernel"]] == ("k_ntt_pass8<false>" if last else "k_ntt_pass8<true>")
                else:
                    assert mc.KERNELS[p["kernel"]] == "k_ntt_pass<true, %s>" % ("false" if last else "true")


def test_ntt_shape_equals_the_recorded_table():
    """h2_ntt_shape for every log_n in 0 .. 28 and every in_log in 0 .. log_n, with default knobs, under H2_NTT_NINE=0 and
    under H2_NTT_NO_ZSKIP=1 (a child process each), equals tests/golden/ntt_shape_table.json row for row: the table was
    recorded from the library before the pass schedule moved into one function (ntt_schedule) that the plan builder, the
    launcher and h2_ntt_shape share"""
    import json

    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    try:
        import gen_ntt_shape_table as gen
    finally:
        sys.path.pop(0)
    with open(os.path.join(ROOT, "tests", "golden", "ntt_shape_table.json")) as f:
        want = json.load(f)["settings"]
    assert [s["knobs"] for s in want] == list(gen.SETTINGS) == [{}, {"H2_NTT_NINE": "0"}, {"H2_NTT_NO_ZSKIP": "1"}]
    for setting in want:
        got = gen.rows_under(setting["knobs"])
        assert len(got) == len(setting["rows"]) == 29 * 30 // 2
        assert [r[:2] for r in got] == [[log_n, in_log] for log_n in range(29) for in_log in range(log_n + 1)]
        for g, w in zip(got, setting["rows"]):
            assert g == w, (setting["knobs"], g, w)


def test_ntt_shape_bad_arguments():
    L = h2.lib()
    out = np.zeros((8, 7), dtype=np.uint32)
    count = ctypes.c_size_t(77)
    assert L.h2_ntt_shape(29, 0, out.ctypes.data, 8, ctypes.byref(count)) == 1     # H2_ERR_INVALID: beyond the 2-adicity
    assert L.h2_ntt_shape(20, 21, out.ctypes.data, 8, ctypes.byref(count)) == 1    # more live inputs than points
    assert L.h2_ntt_shape(20, 18, out.ctypes.data, 8, None) == 1
    assert L.h2_ntt_shape(20, 18, None, 8, ctypes.byref(count)) == 1
    assert count.value == 77 and not out.any() and L.h2_last_error()
    assert L.h2_ntt_shape(26, 26, out.ctypes.data, 3, ctypes.byref(count)) == 1    # four passes into room for three:
    assert count.value == 4 and not out[3:].any()                                  # the count is reported, nothing past cap
    assert L.h2_ntt_shape(26, 26, None, 0, ctypes.byref(count)) == 1 and count.value == 4
    assert L.h2_ntt_shape(0, 0, None, 0, ctypes.byref(count)) == 0 and count.value == 0
    assert L.h2_ntt_shape(26, 26, out.ctypes.data, 8, ctypes.byref(count)) == 0 and count.value == 4


def test_ntt_matrix_enumerates_without_a_gpu_and_reaches_every_default_kernel():
    """tests/ntt_matrix_cases.py, the rows of tests/test_gpu_ntt_matrix.py: enumerated here with h2_ntt_shape alone.  At least
    one row with default knobs maps to each of the five kernels of ntt_run_chunk, so a change of ntt_split or pass_shape that
    silently moves the coverage fails on any machine; the paddings sit around the first pass's width"""
    import ntt_matrix_cases as mc

    L = h2.lib()
    reach = mc.matrix_kernel_ids(L)
    assert set(reach) == set(mc.DEFAULT_KERNELS), {mc.KERNELS[k]: v[:3] for k, v in reach.items()}
    assert len(mc.KERNELS) == 5 and mc.DEFAULT_KERNELS == mc.ALL_KERNELS == frozenset(range(5))
    assert mc.MATRIX_SIZES == (9, 10, 16, 17) + tuple(range(18, 25))
    for log_n in mc.MATRIX_SIZES:
        cases = mc.matrix_cases(L, log_n)
        assert len(cases) == len(set(cases))
        B = mc.first_width(L, log_n)
        assert B == NTT_PASS_WIDTHS[log_n][0]
        zs = {c.z for c in cases if c.op == "coeff_to_extended"}
        if log_n <= 22:
            assert zs == {z for z in (0, 1, 2, 3, B - 1, B, B + 1, log_n - 1, log_n) if z <= log_n}
            assert {c.op for c in cases} == set(mc.OPS)
            assert {c.inp for c in cases} == (set(mc.INPUTS) if log_n <= 21 else {"random", "rm1", "delta_seeded"})
            assert {c.arbitrary for c in cases if c.op == "coeff_to_extended"} == {False, True}
        else:
            assert zs == {1, 2, 3, B} and {c.inp for c in cases} >= {"random", "rm1"}
        # z >= B: one live row, no stage in the first pass; an odd zskip under the radix-4 stage loop
        assert any(mc.ntt_shape(L, log_n, log_n - z)[0]["zskip"] == B for z in zs) or len(NTT_PASS_WIDTHS[log_n]) == 1
    for log_n in mc.CHILD_SIZES:
        cases = mc.child_cases(L, log_n)
        assert {c.op for c in cases} == set(mc.OPS) and {c.inp for c in cases} == {"random", "rm1"}
        assert {c.z for c in cases} == {0, 1, mc.first_width(L, log_n)}
    assert list(mc.KNOB_SETTINGS) == [{"H2_NTT_NINE": "0"}, {"H2_NTT_NO_ZSKIP": "1"}, {"H2_NTT_LAST_TABLE": "0"}]


def test_ntt_shape_under_every_knob_reaches_every_kernel():
    """the knob settings of the matrix's child processes, here with h2_ntt_shape alone (a child process each: the knobs are
    read once): each setting's rows run the kernels recorded here, all five of ntt_run_chunk between them"""
    import ntt_matrix_cases as mc

    code = (
        "import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
        "import halo2_gpu_specific_amd as h2, ntt_matrix_cases as mc\n"
        "L = h2.lib(); ids = set()\n"
        "for log_n in mc.CHILD_SIZES:\n"
        "    for c in mc.child_cases(L, log_n):\n"
        "        ids |= mc.kernel_ids(L, log_n, c.z)\n"
        "print('KERNELS', *sorted(ids))\n"
    ) % (ROOT, os.path.join(ROOT, "tests"))
    reached = set()
    # what each setting's rows run: the same kernels as the default rows, in other geometries and with other twiddle sources
    want = [{0, 1, 2, 4}, {0, 1, 2, 3, 4}, {0, 1, 2, 3, 4}]
    assert len(want) == len(mc.KNOB_SETTINGS)
    for knobs, want_ids in zip(mc.KNOB_SETTINGS, want):
        env = {k: v for k, v in os.environ.items() if k not in mc.KNOBS}
        env.update(knobs)
        out = subprocess.check_output([sys.executable, "-c", code], text=True, env=env, timeout=300)
        ids = {int(v) for v in out.split()[1:]}
        assert ids == want_ids, (knobs, sorted(ids))
        reached |= ids
    assert reached == set(mc.ALL_KERNELS), sorted(mc.ALL_KERNELS - reached)


def test_sharding_plan():
    cols = [parallel.shard_columns(11, 4, r) for r in range(4)]
    assert sorted(sum(cols, [])) == list(range(11))
    for n in (0, 1, 7, 1 << 20, (1 << 20) + 3):
        for world in (1, 2, 3, 8):
            spans = [parallel.msm_split_range(n, world, r) for r in range(world)]
            assert spans[0][0] == 0 and spans[-1][1] == n
            for (a0, a1), (b0, b1) in zip(spans, spans[1:]):
                assert a1 == b0 and a0 <= a1
            part = (n + world - 1) // world if n else 0
            assert all(hi - lo <= part for lo, hi in spans)


def test_host_point_fold_matches_oracle():
    oracle = Oracle.get()
    n = 96
    s, p = oracle.random_fr(31, n), oracle.random_g1(32, n)
    parts = np.stack([oracle.best_multiexp(s[i : i + 24], p[i : i + 24]) for i in range(0, n, 24)])
    ident = np.zeros((1, 12), dtype=np.uint64)
    ident[0, 4:8] = to_mont([1], 0x30644E72E131A029B85045B68181585D97816A916871CA8D3C208C16D87CFD47)[0]
    parts = np.concatenate([parts, ident, parts[:1], parts[:1]])  # identity + a repeated point (doubling branch)
    got = arr_to_points(oracle.to_affine(parallel.g1_sum(parts)))[0]
    want_j = oracle.best_multiexp(s, p)
    two = np.zeros(12, dtype=np.uint64)
    oracle.lib.oracle_g1_double(parts[0].ctypes.data, two.ctypes.data)
    full = np.zeros(12, dtype=np.uint64)
    oracle.lib.oracle_g1_add(want_j.ctypes.data, two.ctypes.data, full.ctypes.data)
    assert got == arr_to_points(oracle.to_affine(full))[0]
    assert parallel.g1_sum(np.zeros((0, 12), np.uint64))[8:].sum() == 0


def test_device_pool_env(tmp_path):
    code = (
        "import sys; sys.path.insert(0, %r)\n"
        "import halo2_gpu_specific_amd as h2\n"
        "print(h2.lib().h2_device_count())\n"
    ) % ROOT
    env = dict(os.environ, HALO2_PROOFS_N_GPU="3")
    out = subprocess.check_output([sys.executable, "-c", code], text=True, env=env)
    # no GPU here: the pool is empty whatever the variable says; on a GPU box it would print 3
    assert out.strip() in ("0", "3")
