#!/bin/bash
# Round profile: bench line, rocprofv3 kernel-trace --stats of the same bench, and the two HBM PMC passes
# (FETCH_SIZE, WRITE_SIZE in separate runs, kernel-trace only) -> $PROFILE_OUT/*_$TAG (default profile_out/); then
# tools/profile_summary.py $TAG (same PROFILE_OUT) writes profiles/.  Every run is bench.py --full: the summaries read
# the isolated and labelled legs' launches beside the timed region's.
export TMPDIR=/tmp
TAG=${1:-r1}
STEPS=${STEPS:-40}
OUT=${PROFILE_OUT:-profile_out}
mkdir -p "$OUT"
# (the library is built in-tree on the CPU side before the call)
timeout -k 10 300 python bench.py --full > $OUT/bench_$TAG.log 2>&1 || { echo "bench failed"; tail -20 $OUT/bench_$TAG.log; exit 1; }
echo "bench: $(tail -1 $OUT/bench_$TAG.log | cut -c1-200)"
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $OUT/prof_$TAG -o run --output-format csv -- python3 bench.py --steps $STEPS --warmup 50 --full --no-cpu-baseline > $OUT/prof_bench_$TAG.log 2>&1 || { echo "rocprof stats failed"; exit 1; }
timeout -k 10 300 rocprofv3 --kernel-trace --pmc FETCH_SIZE -d $OUT/pmcf_$TAG -o run --output-format csv -- python3 bench.py --steps 5 --warmup 1 --full --no-cpu-baseline > $OUT/pmcf_$TAG.log 2>&1 || { echo "pmc fetch failed"; exit 1; }
timeout -k 10 300 rocprofv3 --kernel-trace --pmc WRITE_SIZE -d $OUT/pmcw_$TAG -o run --output-format csv -- python3 bench.py --steps 5 --warmup 1 --full --no-cpu-baseline > $OUT/pmcw_$TAG.log 2>&1 || { echo "pmc write failed"; exit 1; }
echo "profile done"
