#!/bin/bash
# one serial-order kernel trace of the bench step (run on the GPU box): tools/quick_trace.sh <tag> [bench args]
set -euo pipefail
: "${GRAFT_REPO_ROOT:?run on the GPU box}"
TAG=$1; shift
cd /tmp && export TMPDIR=/tmp && cd "$GRAFT_REPO_ROOT"
OUT=${OUT:-profile_out}  # where the traces, counters and logs go
mkdir -p "$OUT"
rocprofv3 --kernel-trace --stats -d $OUT/${TAG}_trace -o kt --output-format csv -- python3 bench.py --full --steps 10 --warmup 3 --no-extras --no-cpu-baseline --no-alone-pass --depth 0 "$@" > $OUT/${TAG}_trace.log 2>&1
python3 tools/step_timeline.py $OUT/${TAG}_trace $OUT/${TAG}_step_timeline.txt > /dev/null
find $OUT/${TAG}_trace -name "*kernel_stats.csv" -exec cp {} $OUT/${TAG}_kernel_stats.csv \;
rm -rf $OUT/${TAG}_trace
