#!/bin/bash
# tests -> bench -> rocprof(kernel stats) ; each step time-limited; stop at first failure
OUT=${OUT:-bench_out}
mkdir -p $OUT
cd /tmp && export TMPDIR=/tmp && cd "$GRAFT_REPO_ROOT"
timeout -k 10 900 python -u -m pytest tests -v -m gpu -x --timeout 120 --timeout-method thread ${PYTEST_ARGS} > $OUT/pytest_gpu.log 2>&1
rc=$?; echo "pytest rc=$rc" >> $OUT/pytest_gpu.log; tail -40 $OUT/pytest_gpu.log
[ $rc -eq 0 ] || [ -n "$CONTINUE_ON_TEST_FAIL" ] || exit $rc
timeout -k 10 600 python bench.py --full --steps ${BENCH_STEPS:-20} --warmup 5 ${BENCH_ARGS} > $OUT/bench.log 2>&1
rc=$?; echo "bench rc=$rc"; tail -5 $OUT/bench.log
[ $rc -eq 0 ] || exit $rc
timeout -k 10 600 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof -o bench -- python bench.py --full --steps 5 --warmup 2 --no-cpu-baseline > $OUT/prof.log 2>&1
rc=$?; echo "rocprof rc=$rc"; find $OUT/prof -name "*stats*" | head
exit $rc
