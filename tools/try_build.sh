#!/bin/bash
# round 6: GPU check of a work-in-progress build -- new tests first, then the whole suite, then a short headline run
cd "$(dirname "$0")/.."
LOG=${LOG:-build/try_build}   # logs of this check (build/ is not tracked)
mkdir -p "$LOG"
timeout 1500 python3 -m pytest tests/test_gpu_skew.py tests/test_gpu_operators.py tests/test_gpu_tables.py -m gpu -q -x > "$LOG/b_new.log" 2>&1; echo "new tests rc=$?"; tail -15 "$LOG/b_new.log"
timeout 2400 python3 -m pytest tests -m gpu -q -x --deselect tests/test_gpu_skew.py > "$LOG/b_all.log" 2>&1; echo "all rc=$?"; tail -8 "$LOG/b_all.log"
timeout 600 python3 bench.py --full --steps 5 --warmup 2 --no-cpu-baseline --no-other-configs --no-pcie > "$LOG/b_bench.json" 2> "$LOG/b_bench.err"; echo "bench rc=$?"
tail -3 "$LOG/b_bench.err"
LOG="$LOG" python3 - <<'P'
import json, os
try:
    b=json.loads(open(os.path.join(os.environ['LOG'], 'b_bench.json')).read().strip().splitlines()[-1])
    x=b['roofline']['exclusive']
    print('ms_per_step', b['ms_per_step'], 'median', b['median_ms'], 'verified', b['verified'])
    print('exclusive phases', x['phase_ms']); print('overlapped phases', b['phase_ms'])
except Exception as e: print('no bench line', e)
P
