# A/B of in-tree variants (lab/libcsm_hip_<v>.so): dec_frame stamps + a short bench line each
set -e
OUT=${CSM_OUT:-bench_out}
mkdir -p $OUT
for v in "$@"; do
  CSM_HIP_LIB=$PWD/lab/libcsm_hip_$v.so timeout -k 10 120 python -u tools/df_stamps.py 6 > $OUT/st_$v.log 2>&1
  CSM_HIP_LIB=$PWD/lab/libcsm_hip_$v.so timeout -k 10 200 python -u bench.py --batch 1 --steps 3 --warmup 1 --full --no-cpu-baseline > $OUT/b_$v.log 2>&1
  python3 -c "import json; d=json.load(open('$OUT/b_$v.log')); print('$v', d['value'], d['roofline']['avg_us'])"
done
