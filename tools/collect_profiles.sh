#!/bin/bash
# Run on the GPU box (gpurun -- tools/collect_profiles.sh): regenerates the rocprofv3 evidence that is
# copied into profiles/.  Counter passes are separate runs with --kernel-trace only (gpurun refuses --pmc
# combined with the sys/hip/hsa trace domains).
R=$GRAFT_REPO_ROOT
OUT=$R/gpurun_out/prof
rm -rf $OUT; mkdir -p $OUT
W=$(mktemp -d) && cd "$W" && export TMPDIR="$W" || exit 1
# Every GPU step below runs once under its own time limit, and the first that fails ends the script.  The bench trace is
# the --quick run (the headline leg and the C-ABI legs: the same kernels in the same regime, a third of the dispatches):
# in round 6 the C++ API's worker threads under the profiler crashed the full run inside the runtime calls the profiler
# intercepts (hipEventQuery, hipStreamSynchronize, a launch), never without the profiler.
BENCH="--full --quick --steps 10 --warmup 2 --no-cpu-baseline --no-parity --no-host-ceiling"
fail() { echo "collect_profiles.sh: $1 failed (exit $2), see $OUT"; exit 1; }
timeout -k 10 600 rocprofv3 --kernel-trace --stats --output-format csv -d "$W/p1" -o b -- python $R/bench.py $BENCH > $OUT/bench.log 2>&1 || fail "bench trace" $?
echo "bench trace: bench.py $BENCH" > $OUT/bench_trace_command.txt
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$W/p2" -o s -- python $R/tools/single_stream.py 20 > $OUT/single.log 2>&1 || fail "single-stream trace" $?
timeout -k 10 300 rocprofv3 --pmc FETCH_SIZE --kernel-trace --output-format csv -d "$W/p3" -o f -- python $R/tools/single_stream.py 3 > $OUT/pmc_fetch.log 2>&1 || fail "FETCH_SIZE pass" $?
timeout -k 10 300 rocprofv3 --pmc WRITE_SIZE --kernel-trace --output-format csv -d "$W/p4" -o w -- python $R/tools/single_stream.py 3 > $OUT/pmc_write.log 2>&1 || fail "WRITE_SIZE pass" $?
cp $(find "$W/p1" -name "*kernel_stats.csv" | head -1) $OUT/bench_kernel_stats.csv
cp $(find "$W/p2" -name "*kernel_stats.csv" | head -1) $OUT/single_stream_kernel_stats.csv
python $R/tools/profiles_summarize.py $(find "$W/p1" -name "*kernel_trace.csv" | head -1) $(find "$W/p2" -name "*kernel_trace.csv" | head -1) \
       $(find "$W/p3" -name "*counter_collection.csv" | head -1) $(find "$W/p4" -name "*counter_collection.csv" | head -1) $OUT || exit 1
timeout -k 10 900 bash $R/tools/pmc_desc.sh > /dev/null 2>&1 || fail "tools/pmc_desc.sh" $?
# which file holds the shader clock on this box (bench.py sustained leg)
{ for f in /sys/class/drm/card*/device/pp_dpm_sclk; do echo "== $f"; cat $f; done; rocm-smi --showclocks 2>&1 | head -30; } > $OUT/sclk_probe.txt 2>&1
ls -la $OUT $R/gpurun_out/pmc_desc 2>/dev/null
