#!/bin/bash
# Expansion time vs chains per batch (workgroup-round / tail effects): alone + pipelined
set -u
cd "${GRAFT_REPO_ROOT:-/root/repo}"
export TMPDIR=/tmp
RES="${TMH_RESULTS:-bench_out}"   # where the runs' lines and logs go
mkdir -p "$RES"
TAG="$1"; shift
for n in "$@"; do
  timeout -k 10 300 python bench.py --steps 8 --warmup 2 --full --no-cpu-baseline --chains $n > $RES/cs_${TAG}_$n.json 2> $RES/cs_${TAG}_$n.err || exit $?
  python3 -c "
import json; d=json.loads(open('$RES/cs_${TAG}_$n.json').read()); r=d['roofline']
print('chains $n value %.4g ms/step %.3f expand %.3f alone %.3f  alone ns/chain-day %.1f' % (d['value'], d['ms_per_step'], r['kernel_ms'], r['alone']['kernel_ms'], r['alone']['kernel_ms'] * 1e6 / $n))"
done
