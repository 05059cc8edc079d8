#!/bin/bash
# sampler A/B of two library builds on one box: in-tree (base) vs lib_ab (variant), alternated
# processes (bench sampler leg only)
set -o pipefail
OUT=${OUT:-bench_out}
mkdir -p $OUT/libab
cd /tmp && export TMPDIR=/tmp && cd "$GRAFT_REPO_ROOT"
show() { python -c "import json;d=json.loads(open('$1').read().strip().splitlines()[-1]);print(d['ms_per_step'],d['sampler']['ms_per_batch'])"; }
for rep in 1 2 3; do
  timeout -k 10 300 python bench.py --full --steps 10 --warmup 3 --no-roofline --no-config0 --no-cpu-baseline --no-stage-legs > $OUT/libab/base.log 2>&1 || { tail -5 $OUT/libab/base.log; exit 1; }
  echo "base $(show $OUT/libab/base.log)"
  TVQ_HIP_LIB=$PWD/lib_ab/libtvq_hip.so timeout -k 10 300 python bench.py --full --steps 10 --warmup 3 --no-roofline --no-config0 --no-cpu-baseline --no-stage-legs > $OUT/libab/new.log 2>&1 || { tail -5 $OUT/libab/new.log; exit 1; }
  echo "new  $(show $OUT/libab/new.log)"
done
