#!/bin/bash
# round-4 profiles after the pipeline groups 4 frames per sparse tensor (bench.py --group 4 = default).  Counters in their own passes.
R=$GRAFT_REPO_ROOT
export OUT=${OUT:-$R/profile_out}; mkdir -p $OUT
cd $R && python bench.py --full > $OUT/r4g_bench.json 2> $OUT/r4g_bench.err; echo "bench rc=$?"; tail -2 $OUT/r4g_bench.err
cd /tmp && export TMPDIR=/tmp
rm -rf $OUT/r4g_stats
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/r4g_stats -- python3 $R/bench.py --full --no-cpu-baseline --strong-frames 64 > $OUT/r4g_stats_bench.json 2> $OUT/r4g_stats_bench.err
echo "stats rc=$?"
cd $R
for f in $OUT/r4g_stats/*/*kernel_trace.csv; do python tools/kernel_by_grid.py $f > $OUT/r4g_bench_kernel_by_grid.txt 2>&1; done
cp $OUT/r4g_stats/*/*kernel_stats.csv $OUT/r4g_bench_kernel_stats.csv 2>/dev/null
rm -rf $OUT/r4g_stats/*/*kernel_trace.csv $OUT/traffic
bash tools/pmc_traffic.sh > $OUT/r4g_traffic_raw.txt 2>&1; echo "traffic rc=$?"
bash tools/pmc_conv.sh r4g_level0 --level 0 --split 9,18 --frames 4 > $OUT/r4g_pmc_level0.txt 2>&1; echo "pmc0 rc=$?"
tail -2 $OUT/r4g_pmc_level0.txt
