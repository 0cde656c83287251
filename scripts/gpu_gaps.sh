#!/bin/bash
# kernel + memory-copy trace of the full bench's timed loop and roofline pass (the profiled fan-in family
# runs eagerly there), then the device idle between kernels (scripts/gaps.py)
# Output under $VIBA_OUT_DIR (default: bench_out/ in the repository).
set -o pipefail
export TMPDIR=/tmp
R=$(cd "$(dirname "$0")/.." && pwd)
OUT=${VIBA_OUT_DIR:-$R/bench_out}
mkdir -p $OUT
TAG=${1:-gaps}
cd /tmp && timeout -k 10 400 rocprofv3 --kernel-trace --memory-copy-trace --output-format csv -d $OUT/$TAG -o run -- python3 $R/bench.py --full --steps 4 --warmup 1 --no-cpu-baseline --no-banded-count > $OUT/$TAG.json 2> $OUT/$TAG.log || exit $?
cd $R && python scripts/gaps.py $(find $OUT/$TAG -name '*kernel_trace.csv' | head -1) 3 16 > $OUT/${TAG}_gaps.txt
