"""Generates tests/golden/msm_scratch_sizes.json from the built library: what h2_msm_shape, h2_msm_scratch_bytes and
h2_msm_batch_scratch_bytes report over a grid of sizes, bounds and batch counts, with no H2_MSM_* variable set and no
shifted-base table registered (no device is needed).  Regenerate only when a sizing rule changes on purpose.

usage: python tests/golden/gen_msm_scratch_sizes.py"""
import ctypes
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import halo2_gpu_specific_amd as h2  # noqa: E402

NS = [1, 255, 1 << 10, (1 << 15) - 1, 1 << 15, (1 << 18) + 3, 1 << 20, 1 << 22, 1 << 24, 1 << 26]
BITS = [1, 8, 16, 17, 64, 128, 254, 300]
COUNTS = [1, 2, 8, 64, 100]


def sizes(L):
    """[n, max_bits, c, windows, buckets, scratch bytes, [batch scratch bytes per count]] per grid point"""
    c, W, nb = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32()
    rows = []
    for n in NS:
        for bits in BITS:
            assert L.h2_msm_shape(n, bits, ctypes.byref(c), ctypes.byref(W), ctypes.byref(nb)) == 0
            rows.append([n, bits, c.value, W.value, nb.value, L.h2_msm_scratch_bytes(n, bits),
                         [L.h2_msm_batch_scratch_bytes(n, bits, k) for k in COUNTS]])
    return rows


if __name__ == "__main__":
    assert not [k for k in os.environ if k.startswith("H2_MSM_")], "unset every H2_MSM_* variable first"
    doc = {"n": NS, "max_bits": BITS, "count": COUNTS, "rows": sizes(h2.lib())}
    with open(os.path.join(HERE, "msm_scratch_sizes.json"), "w") as f:
        f.write(json.dumps(doc).replace("], [", "],\n[") + "\n")
