"""The common NTT pass with its tile ends fused into the outer stage pairs (k_ntt_pass8, csrc/ntt.hip) computes what the pass
through LDS (H2_NTT_FUSE=0) computes, bit for bit.

The knob is read once per process, so every setting runs in a child process of its own, one after another; each child runs
the same seeded set of transforms and prints SHA-256 digests of the results.  H2_NTT_PERSIST and H2_NTT_PERSIST_SLOTS belonged
to a persistent-workgroup form of the kernel that measured slower and was removed: the library no longer reads
them, and the two settings that name them are kept as runs of the default path.

Which sizes reach k_ntt_pass8: 2^16 does not (no radix-4 passes below 2^18) and 2^18 does not (9 + 9 bits); they pin the
neighbouring paths.  2^20 (4 + 8 + 8) and 2^22 (6 + 8 + 8) run its middle and last passes, 2^24 (8 + 8 + 8) also its first
pass -- the form whose first stage pair follows the loads with no product in between.

The device ABI's h2_dev_ntt / h2_dev_intt are in place; the out-of-place forms of the same transforms are h2_dev_coset_ntt
(source and destination distinct) and the batched coset entry point."""
import os
import subprocess
import sys

import pytest

from h2util import ROOT as REPO

pytestmark = pytest.mark.gpu

CHILD = r"""
import ctypes, hashlib, os, sys
sys.path.insert(0, %(repo)r); sys.path.insert(0, os.path.join(%(repo)r, "tests"))
import numpy as np, torch
torch.cuda.init()
import halo2_gpu_specific_amd as h2
from halo2_gpu_specific_amd._lib import check
from h2util import R_MOD, Oracle, fr_mont

L = h2.lib()
oracle = Oracle.get()
CHECK_ORACLE = os.environ.get("H2_FUSED_TEST_ORACLE") == "1"
ROOT_W = 0x03DDB9F5166D18B798865EA93DD31F743215CF6DD39329C8D34F1ED960C37C9C
dev = torch.device("cuda", 0)
vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
rng = np.random.default_rng(20241)
LMAX = 24
host = rng.integers(0, 2**64, size=(1 << LMAX, 4), dtype=np.uint64)
host[:, 3] >>= np.uint64(4)            # below 2^252: canonical residues
base = torch.from_numpy(host.view(np.int64)).to(dev)

def sync():
    torch.cuda.synchronize()
    check(L.h2_synchronize(), "h2_synchronize")

def digest(name, size, tensors):
    sync()
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.cpu().numpy().tobytes())
    print("DIGEST %%s %%d %%s" %% (name, size, h.hexdigest()), flush=True)

def arr(t):
    sync()
    return t.cpu().numpy().view(np.uint64)

for log_n in (16, 18, 20, 22, 24):
    n = 1 << log_n
    full = log_n <= 22          # 2^24: forward, inverse and the out-of-place coset form only
    wi = pow(ROOT_W, 1 << (28 - log_n), R_MOD)
    w, w_inv, n_inv = fr_mont(wi), fr_mont(pow(wi, -1, R_MOD)), fr_mont(pow(n, -1, R_MOD))
    gi = 7 * pow(ROOT_W, 5, R_MOD) %% R_MOD
    g, g_inv = fr_mont(gi), fr_mont(pow(gi, -1, R_MOD))
    x = base[:n].clone()
    tmp = torch.empty(((16 if full else 1) * n, 4), dtype=torch.int64, device=dev)
    sync()
    # forward and inverse, in place
    a = x.clone(); sync()
    check(L.h2_dev_ntt(a.data_ptr(), tmp.data_ptr(), vp(w), log_n, None), "h2_dev_ntt")
    digest("ntt", log_n, [a])
    if CHECK_ORACLE and log_n in (18, 20):
        assert np.array_equal(arr(a), oracle.best_fft(host[:n], w, log_n, threads=8)), ("ntt vs oracle", log_n)
    check(L.h2_dev_intt(a.data_ptr(), tmp.data_ptr(), vp(w_inv), vp(n_inv), log_n, None), "h2_dev_intt")
    digest("intt", log_n, [a])
    if CHECK_ORACLE and log_n in (18, 20):
        assert torch.equal(a, x), ("intt(ntt(x)) != x", log_n)
    # out of place, then the same in place; the inverse with its scale in the last pass's store
    out = torch.empty_like(x); sync()
    check(L.h2_dev_coset_ntt(x.data_ptr(), out.data_ptr(), tmp.data_ptr(), log_n, vp(g), vp(w), None), "h2_dev_coset_ntt")
    digest("coset_ntt_out_of_place", log_n, [out])
    assert torch.equal(x, base[:n]), "an out-of-place transform wrote its source"
    if not full:
        check(L.h2_dev_coset_intt(out.data_ptr(), tmp.data_ptr(), log_n, vp(g_inv), vp(w_inv), vp(n_inv), None), "h2_dev_coset_intt")
        digest("coset_intt", log_n, [out])
        assert torch.equal(out, x), ("coset_intt(coset_ntt(x)) != x", log_n)
        del tmp, x, a, out
        continue
    b = x.clone(); sync()
    check(L.h2_dev_coset_ntt(b.data_ptr(), b.data_ptr(), tmp.data_ptr(), log_n, vp(g), vp(w), None), "h2_dev_coset_ntt")
    digest("coset_ntt_in_place", log_n, [b])
    check(L.h2_dev_coset_intt(b.data_ptr(), tmp.data_ptr(), log_n, vp(g_inv), vp(w_inv), vp(n_inv), None), "h2_dev_coset_intt")
    digest("coset_intt", log_n, [b])
    # batches: 3 and 16 vectors per launch
    for count in (3, 16):
        vs = [torch.roll(x, 97 * i + 1, 0).contiguous() for i in range(count)]
        ptrs = (ctypes.c_void_p * count)(*[t.data_ptr() for t in vs])
        sync()
        check(L.h2_dev_ntt_batch(ptrs, count, tmp.data_ptr(), vp(w), log_n, None), "h2_dev_ntt_batch")
        digest("ntt_batch%%d" %% count, log_n, vs)
        check(L.h2_dev_intt_batch(ptrs, count, tmp.data_ptr(), vp(w_inv), vp(n_inv), log_n, None), "h2_dev_intt_batch")
        digest("intt_batch%%d" %% count, log_n, vs)
        outs = [torch.empty_like(t) for t in vs]
        optrs = (ctypes.c_void_p * count)(*[t.data_ptr() for t in outs])
        sync()
        check(L.h2_dev_coset_ntt_batch(ptrs, optrs, count, tmp.data_ptr(), log_n, vp(g), vp(w), None), "h2_dev_coset_ntt_batch")
        digest("coset_ntt_batch%%d" %% count, log_n, outs)
        del vs, outs
    # the extended domain of size 2^log_n: zero padding, pre3 and the zeta scale on the way in, post3 on the way back
    d, _ = oracle.domain(5, log_n - 2)
    assert d.extended_k == log_n and d.k == log_n - 2
    coeffs = x[: n >> 2].clone()
    ext = torch.empty_like(x); sync()
    check(L.h2_dev_coeff_to_extended(coeffs.data_ptr(), ext.data_ptr(), tmp.data_ptr(), d.k, d.extended_k, vp(d.fr("g_coset")),
                                     vp(d.fr("g_coset_inv")), vp(d.fr("extended_omega")), None), "h2_dev_coeff_to_extended")
    digest("coeff_to_extended", log_n, [ext])
    if CHECK_ORACLE and log_n in (18, 20):
        want_ext = oracle.coeff_to_extended(host[: n >> 2], d)
        assert np.array_equal(arr(ext), want_ext), ("coeff_to_extended vs oracle", log_n)
    check(L.h2_dev_extended_to_coeff(ext.data_ptr(), tmp.data_ptr(), d.extended_k, vp(d.fr("g_coset")), vp(d.fr("g_coset_inv")),
                                     vp(d.fr("extended_omega_inv")), vp(d.fr("extended_ifft_divisor")), None), "h2_dev_extended_to_coeff")
    digest("extended_to_coeff", log_n, [ext])
    if CHECK_ORACLE and log_n in (18, 20):
        want = oracle.extended_to_coeff(want_ext, d)
        assert np.array_equal(arr(ext)[: len(want)], want), ("extended_to_coeff vs oracle", log_n)
    del tmp, x, a, b, out, ext, coeffs
print("CHILD OK", flush=True)
"""

SETTINGS = [
    ("default", {}),
    ("unfused", {"H2_NTT_FUSE": "0", "H2_NTT_PERSIST": "0"}),
    ("default, PERSIST_SLOTS=7", {"H2_NTT_PERSIST_SLOTS": "7"}),
    ("default, PERSIST_SLOTS=1024", {"H2_NTT_PERSIST_SLOTS": "1024"}),
]
KNOBS = ("H2_NTT_FUSE", "H2_NTT_PERSIST", "H2_NTT_PERSIST_SLOTS")


@pytest.mark.timeout(1500)
def test_fused_persistent_pass_equals_the_unfused_pass(tmp_path):
    """Digests of h2_dev_ntt / h2_dev_intt (in place), h2_dev_coset_ntt (out of place and in place), h2_dev_coset_intt, batches
    of 3 and 16 vectors, coeff_to_extended and extended_to_coeff (both scale modes, pre3 / post3, zero padding) at 2^16, 2^18,
    2^20 and 2^22, and of the forward, inverse and coset transforms at 2^24, are equal under: the defaults; H2_NTT_FUSE=0
    H2_NTT_PERSIST=0 (the pass as it was); H2_NTT_PERSIST_SLOTS=7 and =1024 (the default path: see the module's docstring).
    The default child also compares 2^18 and 2^20 with the oracle.  A child that fails ends the test there."""
    script = tmp_path / "fused_child.py"
    script.write_text(CHILD % {"repo": REPO})
    digests = {}
    for i, (name, knobs) in enumerate(SETTINGS):
        env = {k: v for k, v in os.environ.items() if k not in KNOBS}
        env.update(knobs)
        if i == 0:
            env["H2_FUSED_TEST_ORACLE"] = "1"
        res = subprocess.run([sys.executable, str(script)], env=env, capture_output=True, text=True, timeout=360, cwd=REPO)
        assert res.returncode == 0 and "CHILD OK" in res.stdout, (name, res.returncode, res.stdout[-2000:], res.stderr[-3000:])
        digests[name] = [ln for ln in res.stdout.splitlines() if ln.startswith("DIGEST ")]
        print(name, len(digests[name]), "digests")
    want = digests[SETTINGS[0][0]]
    assert len(want) == 4 * 13 + 4
    for name, got in digests.items():
        differing = [(a, b) for a, b in zip(want, got) if a != b]
        assert len(got) == len(want) and not differing, (name, differing[:4])
