#!/bin/bash
# usage: tools/kstats.sh <outname> [bench args...]  -> rocprofv3 kernel stats of one bench run (GPU box)
export TMPDIR=/tmp
R=$PWD; O=$1; shift; OUT=${PROF_OUT:-$R/prof_out}; mkdir -p $OUT
cd /tmp && timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/$O -- python3 $R/bench.py --full --steps 3 --warmup 1 --no-cpu-baseline --no-e2e "$@" > $OUT/$O.log 2>&1
echo "rc=$?"; cd $R
grep "^{" $OUT/$O.log | python3 -c "import json,sys; d=json.loads(sys.stdin.read()); print(d['value'], d['components'])"
cat $OUT/$O/*/*kernel_stats.csv | sed "s/(anonymous namespace):://; s/(unsigned[^\"]*\"/\"/; s/(float[^\"]*\"/\"/" | cut -c1-120 | head -${HEADN:-6}
