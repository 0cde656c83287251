#!/bin/bash
# rocprofv3 kernel stats of a short full bench (graphs off: the profiled family runs eagerly anyway)
# Output under $VIBA_OUT_DIR (default: bench_out/ in the repository).
set -o pipefail
export TMPDIR=/tmp
R=$(cd "$(dirname "$0")/.." && pwd)
OUT=${VIBA_OUT_DIR:-$R/bench_out}
mkdir -p $OUT
TAG=${1:-ks}
cd /tmp
export VIBA_NO_GRAPHS=1
timeout -k 10 600 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_$TAG -o run -- python3 $R/bench.py --full --no-cpu-baseline --steps 3 --warmup 1 > $OUT/bench_${TAG}_prof.json 2> $OUT/bench_${TAG}_prof.log || exit $?
cd $R && python scripts/prof_summary.py $OUT/prof_$TAG 24
