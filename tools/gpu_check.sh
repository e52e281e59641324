#!/bin/bash
# GPU check (MI355X host, repo root): the engine pin against the reference's own outputs first
# (fast feedback), then the whole -m gpu suite and smoke(), then the default bench line with
# every leg but the CPU baseline (--full).
# Outputs in $OUT/<tag>_* (default bench_out/).        [OUT=dir] tools/gpu_check.sh TAG
cd "$(dirname "$0")/.."
export TMPDIR=/tmp
TAG=${1:-r4}
OUT=${OUT:-bench_out}
mkdir -p $OUT
timeout -k 10 300 python -u -m pytest tests/test_engine_pin.py -m gpu -x -v -s --timeout 200 --timeout-method thread > $OUT/${TAG}_pin.log 2>&1 || { tail -30 $OUT/${TAG}_pin.log; exit 1; }
tail -3 $OUT/${TAG}_pin.log
timeout -k 10 900 python -u -m pytest tests -m gpu -x -v --timeout 300 --timeout-method thread > $OUT/${TAG}_tests.log 2>&1
rc=$?
tail -5 $OUT/${TAG}_tests.log
[ $rc -eq 0 ] || exit $rc
timeout -k 10 200 python -c "import __graft_entry__ as g; g.smoke()" > $OUT/${TAG}_smoke.log 2>&1 &&
timeout -k 10 300 python bench.py --full --no-cpu-baseline > $OUT/${TAG}_bench.json 2> $OUT/${TAG}_bench.err
