#!/bin/bash
# round-2 profiles at HEAD: kernel stats + trace of the default bench command, PMC traffic passes, PMC passes on the
# level-0 / level-1 conv, the bench line itself
R=$GRAFT_REPO_ROOT
export OUT=${OUT:-$R/profile_out}; mkdir -p $OUT
cd $R && python bench.py --full > $OUT/r2_bench_final.json 2> $OUT/r2_bench_final.err; echo "bench rc=$?"; tail -2 $OUT/r2_bench_final.err
cd /tmp && export TMPDIR=/tmp
rm -rf $OUT/r2_stats
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/r2_stats -- python3 $R/bench.py --full --no-cpu-baseline > $OUT/r2_stats_bench.json 2> $OUT/r2_stats_bench.err
echo "stats rc=$?"
cd $R
rm -rf $OUT/traffic
bash tools/pmc_traffic.sh > $OUT/r2_traffic_raw.txt 2>&1; echo "traffic rc=$?"
bash tools/pmc_conv.sh r2_level0 --level 0 > $OUT/r2_pmc_level0.txt 2>&1; echo "pmc0 rc=$?"
bash tools/pmc_conv.sh r2_level1 --level 1 > $OUT/r2_pmc_level1.txt 2>&1; echo "pmc1 rc=$?"
rm -f $OUT/r2_wg_final0.bin $OUT/r2_wg_final1.bin
SV_CONV_TRACE=$OUT/r2_wg_final0.bin python tools/conv_microbench.py --level 0 --iters 1 > /dev/null 2>&1
SV_CONV_TRACE=$OUT/r2_wg_final1.bin python tools/conv_microbench.py --level 1 --iters 1 > /dev/null 2>&1
python tools/wg_trace.py $OUT/r2_wg_final0.bin > $OUT/r2_wg_final0.txt; python tools/wg_trace.py $OUT/r2_wg_final1.bin > $OUT/r2_wg_final1.txt
python tools/cfg_timings.py > $OUT/r2_cfg_timings.txt 2>&1; tail -12 $OUT/r2_cfg_timings.txt
