"""Generates tests/golden/ntt_shape_table.json from the built library: what h2_ntt_shape reports for every log_n in 0 .. 28
and every in_log in 0 .. log_n -- per pass bits, log_c, threads, radix4, fixed, zskip, kernel id -- with no H2_NTT_* variable
set, under H2_NTT_NINE=0 and under H2_NTT_NO_ZSKIP=1 (a child process per setting: the knobs are read once; no device is
needed).  Regenerate only when the pass schedule changes on purpose.

usage: python tests/golden/gen_ntt_shape_table.py"""
import ctypes
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))

MAX_LOG = 28
SETTINGS = ({}, {"H2_NTT_NINE": "0"}, {"H2_NTT_NO_ZSKIP": "1"})


def rows(L):
    """[log_n, in_log, [seven words per pass]] under this process's knobs"""
    out = (ctypes.c_uint32 * (8 * 7))()
    count = ctypes.c_size_t()
    table = []
    for log_n in range(MAX_LOG + 1):
        for in_log in range(log_n + 1):
            assert L.h2_ntt_shape(log_n, in_log, out, 8, ctypes.byref(count)) == 0, (log_n, in_log)
            table.append([log_n, in_log, [list(out[7 * p : 7 * p + 7]) for p in range(count.value)]])
    return table


def rows_under(knobs):
    """rows() of a child process with exactly `knobs` of the H2_NTT_* variables set"""
    env = {k: v for k, v in os.environ.items() if not k.startswith("H2_NTT_")}
    env.update(knobs)
    return json.loads(subprocess.check_output([sys.executable, os.path.abspath(__file__), "--rows"], env=env, timeout=300))


if __name__ == "__main__":
    if sys.argv[1:] == ["--rows"]:
        sys.path.insert(0, ROOT)
        import halo2_gpu_specific_amd as h2

        print(json.dumps(rows(h2.lib())))
    else:
        doc = {"settings": [{"knobs": knobs, "rows": rows_under(knobs)} for knobs in SETTINGS]}
        with open(os.path.join(HERE, "ntt_shape_table.json"), "w") as f:
            f.write(json.dumps(doc).replace("]]], [", "]]],\n[") + "\n")
