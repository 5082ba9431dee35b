# round-end: full GPU suite, bench line + rocprof stats + PMC passes (tools/final.sh pmc), config lines
set -o pipefail
export CSM_OUT=${CSM_OUT:-bench_out}
OUT=$CSM_OUT
mkdir -p $OUT
timeout -k 10 900 python -u -m pytest tests -m gpu -x -q --timeout 300 --timeout-method thread > $OUT/full.log 2>&1 || { tail -30 $OUT/full.log; exit 1; }
tail -1 $OUT/full.log
bash tools/final.sh pmc > $OUT/final.log 2>&1 || { tail -20 $OUT/final.log; exit 1; }
head -1 $OUT/final_bench.json | python3 -c "import json,sys; d=json.load(sys.stdin); print('bench', d['value'], d['roofline']['avg_us'], d['roofline']['frac'])"
bash tools/configs.sh 4 5 3 10 8
