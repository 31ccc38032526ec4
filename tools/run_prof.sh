#!/bin/bash
# GPU box: rocprofv3 kernel stats of the default bench (arg 1 = output tag)
set -e
tag=${1:-prof}
R=$GRAFT_REPO_ROOT
OUT=${OUT:-$R/out}      # absolute: the profiled runs start from /tmp
mkdir -p $OUT
rm -rf $OUT/$tag
cd /tmp && export TMPDIR=/tmp
timeout -k 10 500 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/$tag -o out -- python3 $R/bench.py --full --steps 3 --warmup 2 --cpu-baseline none > $OUT/${tag}_bench.json 2> $OUT/${tag}_bench.err
cd $R
f=$(find $OUT/$tag -name "*kernel_stats.csv" | sort | tail -1)
cp $f $OUT/${tag}_kernel_stats.csv
head -40 $OUT/${tag}_kernel_stats.csv | cut -c1-150
timeout -k 10 300 python bench.py --steps 20 --warmup 3 --cpu-baseline none > $OUT/${tag}_unprofiled.json 2>/dev/null
cat $OUT/${tag}_unprofiled.json | cut -c1-200
