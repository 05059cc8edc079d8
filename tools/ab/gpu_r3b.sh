#!/bin/bash
# Every -m gpu test, smoke(), the full bench line, then a kernel trace of the graphed sampler.
set -o pipefail
OUT=${OUT:-bench_out}
mkdir -p $OUT
cd /tmp && export TMPDIR=/tmp && cd "$GRAFT_REPO_ROOT"
timeout -k 10 900 python -u -m pytest tests -q -m gpu --timeout 180 --timeout-method thread > $OUT/pytest_gpu.log 2>&1
rc=$?; tail -2 $OUT/pytest_gpu.log; [ $rc -eq 0 ] || exit $rc
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > $OUT/smoke.log 2>&1 || { tail -20 $OUT/smoke.log; exit 1; }
grep "smoke ok" $OUT/smoke.log
timeout -k 10 600 python bench.py --full > $OUT/bench_full.log 2>&1 || { tail -20 $OUT/bench_full.log; exit 1; }
tail -1 $OUT/bench_full.log > $OUT/bench_full.json
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_sg -o sg -- python tools/sampler_graph_prof.py 3 > $OUT/prof_sg.log 2>&1
echo "rocprof rc=$?"
