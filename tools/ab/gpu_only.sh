cd /tmp && export TMPDIR=/tmp && cd "$GRAFT_REPO_ROOT"
OUT=${OUT:-bench_out}
for o in stage1 stage2; do TVQ_BENCH_ONLY=$o timeout -k 10 300 python bench.py --full --steps 20 --warmup 5 --no-cpu-baseline --no-config0 --no-sampler --no-roofline > $OUT/only_$o.log 2>&1 || exit 1; echo $o; tail -1 $OUT/only_$o.log | cut -c1-200; done
for v in 0; do TVQ_RESBLOCK_FUSED=$v timeout -k 10 300 python bench.py --full --steps 20 --warmup 5 --no-cpu-baseline --no-config0 --no-sampler --no-roofline > $OUT/fused_$v.log 2>&1 || exit 1; echo fused=$v; tail -1 $OUT/fused_$v.log | cut -c1-200; done
for o in stage1; do TVQ_RESBLOCK_FUSED=0 TVQ_BENCH_ONLY=$o timeout -k 10 300 python bench.py --full --steps 20 --warmup 5 --no-cpu-baseline --no-config0 --no-sampler --no-roofline > $OUT/only0_$o.log 2>&1 || exit 1; echo unfused $o; tail -1 $OUT/only0_$o.log | cut -c1-200; done
