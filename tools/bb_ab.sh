# bb_step variant A/B with stamps: test on the first variant, then bench + stamps per variant
OUT=${CSM_OUT:-bench_out}
mkdir -p $OUT
CSM_HIP_LIB=$PWD/lab/libcsm_hip_$1.so timeout -k 10 400 python -u -m pytest -x -q --timeout 240 --timeout-method thread tests/test_bb_step_gpu.py > $OUT/t_bbab.log 2>&1 || { tail -20 $OUT/t_bbab.log; exit 1; }
tail -1 $OUT/t_bbab.log
for v in "$@"; do
  CSM_HIP_LIB=$PWD/lab/libcsm_hip_$v.so timeout -k 10 200 python -u bench.py --steps 3 --warmup 1 --full --no-cpu-baseline > $OUT/bb_$v.json 2> $OUT/bb_$v.err || exit 1
  CSM_HIP_LIB=$PWD/lab/libcsm_hip_$v.so timeout -k 10 120 python -u tools/bb_stamps.py 4 > $OUT/bbst_$v.txt 2>&1 || exit 1
  python3 -c "import json; d=json.load(open('$OUT/bb_$v.json')); print('$v', d['value'], d['ms_per_step'], d['roofline_backbone']['avg_us'])"
  grep "WG \|per layer" $OUT/bbst_$v.txt
done
