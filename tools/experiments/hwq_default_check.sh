cd "$GRAFT_REPO_ROOT"
unset GPU_MAX_HW_QUEUES
python3 tools/wide_bench.py 22 16 2>&1 | grep "rep 2" | cut -c1-40
python3 tools/wide_bench.py 22 16 - compact 2>&1 | grep "rep 2" | cut -c1-40
line=$(mktemp); python3 bench.py --full --steps 5 --warmup 2 --no-cpu-baseline > "$line" 2>/dev/null; python3 -c "
import json, sys; d=json.load(open(sys.argv[1])); print(json.dumps(d['config']['headline']))" "$line"; rm -f "$line"
GPU_MAX_HW_QUEUES=4 python3 tools/wide_bench.py 22 16 2>&1 | grep "rep 2" | cut -c1-40
