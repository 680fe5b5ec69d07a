# Per-pass durations and SQ counters of the common NTT pass at 2^24 (three 8-bit passes; launch order mod 3) with H2_NTT_FUSE=0
# (k_ntt_pass<true, true, 8, ...>, the pass before k_ntt_pass8) and =1 (k_ntt_pass8, the default).
# Two separate rocprofv3 runs per setting: --kernel-trace --stats for the durations, --pmc alone for the counters; each under
# its own time limit, the first failure ends the script.  The traces go to a directory of the script's own, removed at the end.
# usage: bash tools/experiments/ntt_fuse_pmc.sh     (from the repository root)
OUT=$(mktemp -d) || exit 1
R=$(pwd)
for F in 0 1; do
  set -- $F x
  export H2_NTT_FUSE=$1
  timeout -k 10 300 rocprofv3 --kernel-trace --stats -d "$OUT/t$1$2" -o p -f csv -- "$R/tools/h2bench" ntt 24 10 > /dev/null 2>&1 || exit 1
  timeout -k 10 300 rocprofv3 --pmc SQ_INSTS_VALU SQ_INSTS_LDS SQ_WAVE_CYCLES SQ_WAIT_ANY SQ_BUSY_CYCLES GRBM_GUI_ACTIVE -d "$OUT/c$1$2" -o p -f csv -- "$R/tools/h2bench" ntt 24 3 > /dev/null 2>&1 || exit 1
done
python3 - "$OUT" <<'PY'
import collections, csv, glob, sys
out = sys.argv[1]
for fuse, persist in ((0, "x"), (1, "x")):
    print("== H2_NTT_FUSE=%d" % fuse)
    for f in glob.glob('%s/t%d%s/**/*kernel_trace.csv' % (out, fuse, persist), recursive=True):
        rows = [r for r in csv.DictReader(open(f)) if 'k_ntt_pass' in r['Kernel_Name']]
        rows.sort(key=lambda r: int(r['Start_Timestamp']))
        rows = rows[len(rows) // 2 // 3 * 3:]                      # the second half: the steady clock
        acc = collections.defaultdict(list)
        for i, r in enumerate(rows):
            acc[i % 3].append((int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e3)
        r0 = rows[0]
        print('  %s  grid=%s lds=%s scratch=%s vgpr=%s' % (r0['Kernel_Name'][:64], r0.get('Grid_Size_X', r0.get('Grid_Size')), r0.get('LDS_Block_Size'),
                                                        r0.get('Scratch_Size'), r0.get('VGPR_Count')))
        for p in sorted(acc):
            v = sorted(acc[p])
            print('  pass %d: median %.1f us  mean %.1f us over %d launches' % (p, v[len(v) // 2], sum(v) / len(v), len(v)))
        print('  sum of medians: %.1f us per transform' % sum(sorted(acc[p])[len(acc[p]) // 2] for p in acc))
    for f in glob.glob('%s/c%d%s/**/*counter_collection.csv' % (out, fuse, persist), recursive=True):
        rows = [r for r in csv.DictReader(open(f)) if 'k_ntt_pass' in r['Kernel_Name']]
        ids = sorted({int(r['Dispatch_Id']) for r in rows})
        pos = {d_: i % 3 for i, d_ in enumerate(ids)}
        acc = collections.defaultdict(lambda: collections.defaultdict(float))
        for r in rows:
            acc[pos[int(r['Dispatch_Id'])]][r['Counter_Name']] += float(r['Counter_Value'])
        n = len(ids) // 3
        for p in sorted(acc):
            a = acc[p]
            # slot occupancy: SQ_WAVE_CYCLES read as quad-cycles over the 4096 wave slots of the chip (16 per CU) for the
            # kernel's GRBM_GUI_ACTIVE cycles per XCD (the counter is summed over the 8 XCDs)
            print('  pass %d: VALU instr/element %.0f  SQ_INSTS_LDS %.4g (%.1f per element)  cycles per VALU instr per SIMD %.2f  '
                  'SQ_WAIT_ANY / SQ_WAVE_CYCLES %.3f  slot occupancy %.3f' % (
                      p, a['SQ_INSTS_VALU'] / n * 64 / 2**24, a['SQ_INSTS_LDS'] / n, a['SQ_INSTS_LDS'] / n * 64 / 2**24,
                      a['GRBM_GUI_ACTIVE'] / n / 8 / (a['SQ_INSTS_VALU'] / n / 1024), a['SQ_WAIT_ANY'] / a['SQ_WAVE_CYCLES'],
                      a['SQ_WAVE_CYCLES'] * 4 / (4096 * a['GRBM_GUI_ACTIVE'] / 8)))
PY
rm -rf "$OUT"
