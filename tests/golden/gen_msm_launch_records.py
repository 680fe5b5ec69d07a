"""Generates tests/golden/msm_launch_records.json on a GPU: every h2_msm_launch_info (h2_msm_last_launches) of every row of
tests/msm_plan_cases.py, run by tests/msm_plan_worker.py's Runner -- the default rows in this process, each of CHILDREN under
its knob setting in a child process of its own (one time limit per child).  Per row: the call's inputs and knobs, then one
launch record per line, without the `scratch` address (the only field that is not a function of the inputs).  Regenerate only
when a launch decision changes on purpose: the records are what tests/test_gpu_msm_plans.py (on the device) and
tests/test_msm_plan_host.py (the plan alone, without one) compare against.

usage: python tests/golden/gen_msm_launch_records.py            (no H2_MSM_* variable set)"""
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import msm_plan_cases as mc  # noqa: E402

CHILD_TIMEOUT = 60
OUT = os.path.join(HERE, "msm_launch_records.json")


def entry(child, knobs, row, recs):
    columns = [row.dist] if row.kind == "single" else list(row.dist)
    bits = [row.bits - j if row.kind == "batch_ex" else row.bits for j in range(len(columns))]   # as the worker bounds them
    return {"child": child, "knobs": knobs, "name": row.name, "kind": row.kind, "n": row.n, "bits": bits, "columns": columns,
            "digits": row.digits, "table_n": row.table_n or 0, "lo": row.lo,
            "launches": [{k: v for k, v in r.items() if k != "scratch"} for r in recs]}


def run_rows(child, knobs, rows):
    from h2util import Oracle
    from msm_plan_worker import Runner

    runner = Runner(Oracle.get())
    try:
        return [entry(child, knobs, row, runner.run(row)[0]) for row in rows]
    finally:
        runner.forget()


def dump(entries):
    """one row header per line, one launch record per line"""
    lines = []
    for e in entries:
        head = json.dumps({k: v for k, v in e.items() if k != "launches"}, sort_keys=True)
        recs = ",\n ".join(json.dumps(r, sort_keys=True) for r in e["launches"])
        lines.append(head[:-1] + ', "launches": [\n ' + recs + "]}")
    return '{"rows": [\n' + ",\n".join(lines) + "\n]}\n"


def main():
    if len(sys.argv) == 3 and sys.argv[1] == "--child":     # one knob setting: its entries as one JSON line on stdout
        name, knobs, rows, _ = next(c for c in mc.CHILDREN if c[0] == sys.argv[2])
        for k, v in knobs.items():
            assert os.environ.get(k) == v, "start this child with %s=%s" % (k, v)
        print("ENTRIES " + json.dumps(run_rows(name, knobs, rows)), flush=True)
        return
    assert not [k for k in os.environ if k.startswith("H2_MSM_")], "unset every H2_MSM_* variable first"
    entries = run_rows(None, {}, mc.WINDOWED_ROWS + mc.TABLE_ROWS + mc.FUSED_ROWS)
    for name, knobs, _, _ in mc.CHILDREN:
        env = dict(os.environ)
        env.update(knobs)
        res = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", name], env=env, capture_output=True, text=True,
                             timeout=CHILD_TIMEOUT, cwd=ROOT)
        assert res.returncode == 0, (name, res.returncode, res.stdout[-3000:], res.stderr[-3000:])
        entries += json.loads([ln for ln in res.stdout.splitlines() if ln.startswith("ENTRIES ")][-1][len("ENTRIES "):])
    with open(OUT, "w") as f:
        f.write(dump(entries))
    print("%d rows, %d launch records -> %s" % (len(entries), sum(len(e["launches"]) for e in entries), OUT))


if __name__ == "__main__":
    main()
