#!/bin/bash
# Round-3 evidence on one tree: every -m gpu test, smoke(), the full bench line, the step's
# kernel table / timeline, the roofline legs' PMC passes (LEG list), the sampler graph's
# kernel table.  Each GPU step time-limited; stops at the first failure.
set -o pipefail
OUT=${OUT:-bench_out}
mkdir -p $OUT
cd /tmp && export TMPDIR=/tmp && cd "$GRAFT_REPO_ROOT"
timeout -k 10 700 python -u -m pytest tests -q -m gpu --timeout 120 --timeout-method thread > $OUT/pytest_gpu.log 2>&1
rc=$?; tail -2 $OUT/pytest_gpu.log; [ $rc -eq 0 ] || exit $rc
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > $OUT/smoke.log 2>&1 || { tail -20 $OUT/smoke.log; exit 1; }
grep "smoke ok" $OUT/smoke.log
timeout -k 10 600 python bench.py --full > $OUT/bench_full.log 2>&1 || { tail -20 $OUT/bench_full.log; exit 1; }
tail -1 $OUT/bench_full.log > $OUT/bench_full.json
echo bench-done
bash tools/gpu_evidence.sh > $OUT/evidence.txt 2>&1 || { tail -20 $OUT/evidence.txt; exit 1; }
head -6 $OUT/evidence.txt
for L in ${LEGS:-linfwd}; do
  LEG=$L bash tools/gpu_roofline.sh > $OUT/roof_$L.txt 2>&1 || { tail -20 $OUT/roof_$L.txt; exit 1; }
done
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_sgraph -o sg -- python tools/sampler_graph_prof.py > $OUT/prof_sgraph.log 2>&1 || { tail -20 $OUT/prof_sgraph.log; exit 1; }
echo r3-final-done
