#!/bin/bash
# GPU box: HBM traffic of the bench's kernels from two separate PMC passes (never combined with tracing domains other than
# --kernel-trace).  arg 1 = output tag.  Summarise afterwards with tools/pmc_summary.py.
set -e
tag=${1:-pmc}
R=$GRAFT_REPO_ROOT
OUT=${OUT:-$R/out}      # absolute: the profiled runs start from /tmp
mkdir -p $OUT
cd /tmp && export TMPDIR=/tmp
for ctr in FETCH_SIZE WRITE_SIZE; do
  rm -rf $OUT/${tag}_$ctr
  timeout -k 10 500 rocprofv3 --pmc $ctr --kernel-trace --output-format csv -d $OUT/${tag}_$ctr -o out -- python3 $R/bench.py --full --steps 2 --warmup 2 --cpu-baseline none > $OUT/${tag}_$ctr.json 2> $OUT/${tag}_$ctr.err
  f=$(find $OUT/${tag}_$ctr -name "*counter_collection.csv" | sort | tail -1)
  python3 $R/tools/pmc_summary.py --reduce $f $ctr > $OUT/${tag}_$ctr.reduced.json
  rm -rf $OUT/${tag}_$ctr
  echo "$ctr done"
done
python3 $R/tools/pmc_summary.py --merge $OUT/${tag}_FETCH_SIZE.reduced.json $OUT/${tag}_WRITE_SIZE.reduced.json > $OUT/${tag}_summary.json
head -c 1500 $OUT/${tag}_summary.json
