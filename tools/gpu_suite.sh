# full GPU suite + a bench line with its forward / encoder / roofline legs on one box: [OUT=<dir>] bash tools/gpu_suite.sh <tag>     (the suite is bounded: a hang must not eat the box's time limit)
T=${1:-run}
OUT=${OUT:-/tmp/p3_suite}
cd "$(dirname "$0")/.."
mkdir -p $OUT
timeout 1500 python -m pytest tests/ -x -q -m gpu > $OUT/suite_$T.txt 2>&1
echo "pytest exit $?" >> $OUT/suite_$T.txt
tail -40 $OUT/suite_$T.txt
python bench.py --full --no-cpu-baseline --no-fp32-leg --no-predict --no-host-feed --no-ffl 2>&1 | tail -1 > $OUT/bench_$T.json
python -c "import json; d=json.load(open('$OUT/bench_$T.json')); print('ms/step', d['ms_per_step'], 'fwd', d['fwd_ms_per_batch'], 'enc', d['encoder_fwd']['ms_per_batch'], d['encoder_fwd']['mfma_frac'], 'roof', d['roofline']['kernel'], d['roofline']['avg_launch_us'])"
