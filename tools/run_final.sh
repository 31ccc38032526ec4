#!/bin/bash
# GPU box: the round's judged artifacts (arg 1 = tag): default bench line (with the CPU baseline), rocprofv3 kernel stats of the
# bench, FETCH_SIZE / WRITE_SIZE PMC passes (separate runs, --kernel-trace only), and the other configurations' bench lines.
tag=${1:-r03}
R=$GRAFT_REPO_ROOT
OUT=${OUT:-$R/out}      # absolute: the profiled runs start from /tmp
mkdir -p $OUT
cd $R
step() {
  local lim=$1 log=$2; shift 2
  timeout -k 10 $lim "$@" > $log 2>&1
  local rc=$?
  echo "[$(date +%T)] rc=$rc  $*"
  if [ $rc -ge 124 ]; then echo "killed at its limit: stopping"; tail -5 $log; exit $rc; fi
  return $rc
}
step 500 $OUT/${tag}_bench_default.err python bench.py --full
tail -1 $OUT/${tag}_bench_default.err > $OUT/${tag}_bench1080p_bf16_unprofiled_bench_line.json; cut -c1-300 $OUT/${tag}_bench1080p_bf16_unprofiled_bench_line.json; echo
cd /tmp && export TMPDIR=/tmp
rm -rf $OUT/${tag}_prof
step 500 $OUT/${tag}_prof.err rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/${tag}_prof -o out -- python3 $R/bench.py --full --steps 5 --warmup 3 --cpu-baseline none
grep "\"metric\"" $OUT/${tag}_prof.err | tail -1 > $OUT/${tag}_bench1080p_bf16_bench_line.json
f=$(find $OUT/${tag}_prof -name "*kernel_stats.csv" | sort | tail -1)
[ -n "$f" ] && cp $f $OUT/${tag}_bench1080p_bf16_kernel_stats.csv && rm -rf $OUT/${tag}_prof
for ctr in FETCH_SIZE WRITE_SIZE; do
  rm -rf $OUT/${tag}_$ctr
  step 500 $OUT/${tag}_$ctr.err rocprofv3 --pmc $ctr --kernel-trace --output-format csv -d $OUT/${tag}_$ctr -o out -- python3 $R/bench.py --full --graph 0 --steps 2 --warmup 2 --cpu-baseline none
  f=$(find $OUT/${tag}_$ctr -name "*counter_collection.csv" | sort | tail -1)
  [ -n "$f" ] && python3 $R/tools/pmc_summary.py --reduce $f $ctr > $OUT/${tag}_$ctr.reduced.json
  rm -rf $OUT/${tag}_$ctr
done
python3 $R/tools/pmc_summary.py --merge $OUT/${tag}_FETCH_SIZE.reduced.json $OUT/${tag}_WRITE_SIZE.reduced.json > $OUT/${tag}_pmc_summary.json
cd $R
step 300 $OUT/${tag}_fp32.err python bench.py --full --precision fp32 --cpu-baseline none --steps 10
tail -1 $OUT/${tag}_fp32.err > $OUT/${tag}_bench1080p_fp32_unprofiled_bench_line.json
step 300 $OUT/${tag}_540.err python bench.py --full --height 540 --width 960 --cpu-baseline none
tail -1 $OUT/${tag}_540.err > $OUT/${tag}_bench540p_bf16_bench_line.json
step 400 $OUT/${tag}_4k.err python bench.py --full --height 2160 --width 3840 --dataset underwater --cpu-baseline none --steps 10 --frames 3
tail -1 $OUT/${tag}_4k.err > $OUT/${tag}_bench4k_underwater_bf16_bench_line.json
step 300 $OUT/${tag}_eager.err python bench.py --full --graph 0 --cpu-baseline none
tail -1 $OUT/${tag}_eager.err > $OUT/${tag}_bench1080p_bf16_eager_bench_line.json
for f in $OUT/${tag}_bench*bench_line.json; do echo "$f: $(cut -c1-200 $f)"; done
exit 0
