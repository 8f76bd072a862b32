#!/bin/bash
# Round trip used during development: the GPU tests + a kernel-traced full bench (--full: every secondary leg).
# usage: tools/gpu_check.sh <tag> [bench args]    OUT = where the logs go (default build/bench_out)
TAG=${1:-x}; shift
R=$(cd "$(dirname "$0")/.." && pwd); O=${OUT:-$R/build/bench_out}
mkdir -p $O
timeout -k 10 480 python -m pytest $R/tests -m gpu -q > $O/tests_$TAG.log 2>&1
echo "pytest exit $?" >> $O/tests_$TAG.log
tail -3 $O/tests_$TAG.log
cd /tmp && export TMPDIR=/tmp
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $O/prof_$TAG -o trace -- python3 $R/bench.py --full --steps 10 --warmup 2 "$@" > $O/bench_$TAG.json 2>&1
echo "bench exit $?"
grep '^{' $O/bench_$TAG.json | cut -c1-400
