# Round artefacts on one box: rocprofv3 kernel stats of the train step, FETCH / WRITE PMC passes (separate runs), THEN the bench line (so that its
# roofline.traffic comes from this round's counters), SQ counters, the FFL line.
# usage: [OUT=<dir>] bash tools/final_prof.sh r03      (OUT: where the logs and artefacts go, default /tmp/p3_final)
set -x
R=${1:-r03}
OUT=${OUT:-/tmp/p3_final}
export TMPDIR=/tmp
cd "$(dirname "$0")/.."
mkdir -p $OUT
rocprofv3 --kernel-trace --stats --output-format csv -d /tmp/pf_stats -o st -- python bench.py --lean --steps 20 > $OUT/stats_run.log 2>&1
find /tmp/pf_stats -name "*kernel_stats.csv" -exec cp {} $OUT/${R}_train_step_graph_kernel_stats.csv \;
python tools/kstats.py $OUT/${R}_train_step_graph_kernel_stats.csv 25 60 > $OUT/${R}_train_step_graph_summary.txt
rocprofv3 --pmc FETCH_SIZE --kernel-trace --output-format csv -d /tmp/pf_fetch -o f -- python bench.py --lean --graph 0 --steps 4 --warmup 2 > $OUT/fetch_run.log 2>&1
rocprofv3 --pmc WRITE_SIZE --kernel-trace --output-format csv -d /tmp/pf_write -o w -- python bench.py --lean --graph 0 --steps 4 --warmup 2 > $OUT/write_run.log 2>&1
python tools/pmc_traffic.py /tmp/pf_fetch /tmp/pf_write $OUT/${R}_pmc_traffic.json 6 > $OUT/${R}_pmc_summary.txt 2>&1
cp $OUT/${R}_pmc_traffic.json profiles/${R}_pmc_traffic.json
python bench.py --full 2>&1 | tail -1 > $OUT/${R}_bench.json
python bench.py --full --workload ffl_fusion --steps 10 --no-cpu-baseline --no-fp32-leg --no-predict --no-host-feed 2>&1 | tail -1 > $OUT/${R}_bench_ffl.json
rocprofv3 --pmc SQ_WAVE_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_VALU_MFMA_BUSY_CYCLES SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE GRBM_GUI_ACTIVE --kernel-trace --output-format csv -d /tmp/pf_sq -o q -- python bench.py --lean --graph 0 --steps 3 --warmup 2 > $OUT/sq_run.log 2>&1
python tools/pmc_kernels.py /tmp/pf_sq > $OUT/${R}_sq_counters_summary.txt 2>&1
rocprofv3 --kernel-trace --stats --output-format csv -d /tmp/pf_fp32 -o st32 -- python bench.py --lean --precision fp32 --steps 6 --warmup 2 > $OUT/fp32_run.log 2>&1
find /tmp/pf_fp32 -name "*kernel_stats.csv" -exec cp {} $OUT/${R}_fp32_step_kernel_stats.csv \;
python tools/kstats.py $OUT/${R}_fp32_step_kernel_stats.csv 9 40 > $OUT/${R}_fp32_step_summary.txt
rocprofv3 --kernel-trace --stats --output-format csv -d /tmp/pf_x3 -o stx3 -- python bench.py --lean --precision fp32x3 --steps 6 --warmup 2 > $OUT/fp32x3_run.log 2>&1
find /tmp/pf_x3 -name "*kernel_stats.csv" -exec cp {} $OUT/${R}_fp32x3_step_kernel_stats.csv \;
python tools/kstats.py $OUT/${R}_fp32x3_step_kernel_stats.csv 9 40 > $OUT/${R}_fp32x3_step_summary.txt
P3_FORCE_COLLECTIVES=1 python bench.py --full --no-cpu-baseline --no-fp32-leg --no-predict --no-host-feed --no-ffl --no-fwd 2>&1 | tail -1 > $OUT/${R}_bench_rccl_single_rank.json
tail -3 $OUT/${R}_pmc_summary.txt
cut -c1-900 $OUT/${R}_bench.json
cut -c1-300 $OUT/${R}_bench_ffl.json
