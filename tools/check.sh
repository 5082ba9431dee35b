# full GPU suite + bench line + eager kernel stats of the bench command ($CSM_OUT, default bench_out/)
OUT=${CSM_OUT:-bench_out}
mkdir -p $OUT
timeout -k 10 900 python -u -m pytest tests -m gpu -x -q --timeout 300 --timeout-method thread > $OUT/full.log 2>&1; tail -2 $OUT/full.log
timeout -k 10 300 python -u bench.py --full --no-cpu-baseline > $OUT/bench_r02.json 2> $OUT/bench_r02.err || { tail -5 $OUT/bench_r02.err; exit 1; }
python3 -c "import json; d=json.load(open('$OUT/bench_r02.json')); print(d['value'], d['roofline']['avg_us'])"
export TMPDIR=/tmp
CSM_GRAPH=0 timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/kp -o run -- python3 bench.py --steps 1 --warmup 1 > $OUT/kp.json 2>&1 || exit 1
python3 tools/kstats.py $(find $OUT/kp -name "*kernel_stats.csv" | head -1) 14
