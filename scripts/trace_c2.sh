#!/bin/bash
# Kernel trace of the pipelined C2 bench (rocprofv3 --kernel-trace --stats): trace_c2.sh TAG [bench args]
set -u
cd "${GRAFT_REPO_ROOT:-/root/repo}"
export TMPDIR=/tmp
TAG="$1"; shift
RES="${TMH_RESULTS:-bench_out}"   # where the trace and its summary go
mkdir -p "$RES/tr_$TAG"
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $RES/tr_$TAG -o run -- python3 bench.py --steps 10 --warmup 3 --full --no-cpu-baseline "$@" > $RES/tr_$TAG/bench.json 2> $RES/tr_$TAG/bench.err || exit $?
f=$(find $RES/tr_$TAG -name '*kernel_trace.csv' | head -1)
cp "$f" $RES/tr_$TAG/kernel_trace.csv
python3 scripts/timeline.py $RES/tr_$TAG/kernel_trace.csv > $RES/tr_$TAG/timeline.txt; rm -rf $RES/tr_$TAG/*/; cat $RES/tr_$TAG/timeline.txt
