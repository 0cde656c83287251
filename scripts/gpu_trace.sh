#!/bin/bash
# kernel trace of config C (eager launches: rocprofv3 tracing crashes on hipGraph replays) for
# scripts/level_profile.py / timeline.py
# Output under $VIBA_OUT_DIR (default: bench_out/ in the repository).
set -o pipefail
export TMPDIR=/tmp VIBA_NO_GRAPHS=1
R=$(cd "$(dirname "$0")/.." && pwd)
OUT=${VIBA_OUT_DIR:-$R/bench_out}
mkdir -p $OUT
TAG=${1:-trace}
cd /tmp && timeout -k 10 400 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/$TAG -o run -- python3 $R/bench.py --full --steps 2 --warmup 1 --no-cpu-baseline > $OUT/$TAG.json 2> $OUT/$TAG.log
