#!/bin/bash
cd "$(dirname "$0")/.."
O=${1:?usage: r06_probe6.sh OUTPUT_DIR}
mkdir -p "$O"
( time python3 -m pytest tests/test_gpu_bench.py -q -m gpu -p no:cacheprovider -x ) > "$O/r06_p6_test.txt" 2>&1
tail -5 "$O/r06_p6_test.txt"
python3 bench.py --full --steps 20 --warmup 5 > "$O/r06_bench_line_v2.json" 2> "$O/r06_bench_v2.err"
python3 -c "
import json, sys
d=json.loads(open(sys.argv[1]).read().strip().splitlines()[-1])
print(d['ms_per_step'], d['roofline']['frac'], d['roofline_gather']['frac'], d['roofline']['traffic'])
print(json.dumps(d['parity_1m']['iter2_teacher_forced']))
print({k:d['parity_1m'][k] for k in ('rel','max_abs_dpos','max_abs_dnorm','mad_delta_deg','ok')})
" "$O/r06_bench_line_v2.json"
