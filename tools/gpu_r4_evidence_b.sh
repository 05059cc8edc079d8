#!/bin/bash
# Round-4 evidence, part B: every -m gpu test, smoke(), then the full bench line (all legs,
# reading part A's profiles for the traffic / CU-weighted fields).
set -o pipefail
OUT=${OUT:-bench_out}
mkdir -p $OUT/r4ev
cd /tmp && export TMPDIR=/tmp && cd "$GRAFT_REPO_ROOT"
timeout -k 10 900 python -u -m pytest tests -q -m gpu --timeout 240 --timeout-method thread > $OUT/r4ev/pytest_gpu.log 2>&1 || { tail -40 $OUT/r4ev/pytest_gpu.log; exit 1; }
tail -2 $OUT/r4ev/pytest_gpu.log
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke(); print('smoke ok')" > $OUT/r4ev/smoke.log 2>&1 || { tail -20 $OUT/r4ev/smoke.log; exit 1; }
tail -1 $OUT/r4ev/smoke.log
timeout -k 10 600 python bench.py --full > $OUT/r4ev/bench_full.log 2>&1 || { tail -20 $OUT/r4ev/bench_full.log; exit 1; }
tail -1 $OUT/r4ev/bench_full.log > $OUT/r4ev/bench_full.json
echo evidence-b-done
