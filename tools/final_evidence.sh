# The round-end evidence run: the --full bench line, the driver-flags line, tools/prof_all.sh (kernel stats + PMC), the L-BFGS
# passes' PMC bytes, the pass microbenchmark, k_skin3 against k_skin2 (times; every launch of eight fits in flight checked).
#   OUT=<results dir> bash tools/final_evidence.sh [round tag, default r4]   ->  <results dir>/<tag>/...
set -e
T=${1:-r4}
export OUT=${OUT:?set OUT to the results directory}
mkdir -p $OUT/$T
python bench.py --full > $OUT/$T/bench_default.json 2> $OUT/$T/bench_default.err
python bench.py --gpus 1 --steps 20 --warmup 5 > $OUT/$T/bench_driver_flags.json 2> $OUT/$T/bench_driver_flags.err
bash tools/prof_all.sh > $OUT/$T/prof_all.log 2>&1
bash tools/pmc_lbfgs.sh > $OUT/$T/pmc_lbfgs.log 2>&1
python tools/time_skin16.py > $OUT/$T/skin16_times.log 2>&1
python tools/skin16_stress.py > $OUT/$T/skin16_stress_full.log 2>&1; tail -1 $OUT/$T/skin16_stress_full.log > $OUT/$T/skin16_stress.log
for f in p_bench_kernel_stats.csv p_closure_kernel_stats.csv p_roof_kernel_stats.csv pmc_summary.json pmc_lbfgs_summary.json roof_plain.log; do cp $OUT/$f $OUT/$T/$f; done
ls $OUT/$T
