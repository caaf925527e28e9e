#!/bin/bash
# Runs on the GPU box: rocprofv3 evidence for TWO builds of the library on the headline (bench.py cfg2), before / after a kernel change.
#   per build: kernel trace + stats in one run; then counters only, each pass a run of its own with no trace beside it
#   (FETCH_SIZE | WRITE_SIZE | the SQ counters); the FIRST build's FETCH_SIZE / WRITE_SIZE passes run twice: the difference
#   between the two is what a difference in bytes between the builds has to exceed.
#   tools/profile_ab_summary.py turns the csv files into summary.txt and, for the SECOND build, traffic_cfg2.json.
# usage: tools/profile_ab.sh <out dir> <library A> <library B> [steps = 30]     (library B must be the build of the working tree)
# Every step has its own time limit and the chain stops at the first failure.
set -u
OUT=$1; LIBA=$(readlink -f $2); LIBB=$(readlink -f $3); STEPS=${4:-30}
REPO=$(cd "$(dirname "$0")/.." && pwd)
mkdir -p $OUT; OUT=$(readlink -f $OUT)
BENCH="python $REPO/bench.py --gpus 1 --profile --steps $STEPS --warmup 5"
SQ="SQ_WAVE_CYCLES SQ_WAIT_INST_ANY SQ_INSTS_VALU SQ_INSTS_LDS SQ_LDS_BANK_CONFLICT"
pass() {   # pass <tag> <library> <rocprofv3 options...>
  local tag=$1 lib=$2; shift 2
  timeout -k 10 300 env KGCN_HIP_LIB=$lib rocprofv3 "$@" --output-format csv -d $OUT/$tag -o bench -- $BENCH > $OUT/$tag.log 2>&1
  local rc=$?
  [ $rc -eq 0 ] || { echo "pass $tag failed rc=$rc"; tail -5 $OUT/$tag.log; }
  return $rc
}
pass A_stats $LIBA --kernel-trace --stats &&
pass B_stats $LIBB --kernel-trace --stats &&
pass A_fetch $LIBA --pmc FETCH_SIZE &&
pass B_fetch $LIBB --pmc FETCH_SIZE &&
pass A_write $LIBA --pmc WRITE_SIZE &&
pass B_write $LIBB --pmc WRITE_SIZE &&
pass A2_fetch $LIBA --pmc FETCH_SIZE &&
pass A2_write $LIBA --pmc WRITE_SIZE &&
pass A_sq $LIBA --pmc $SQ &&
pass B_sq $LIBB --pmc $SQ &&
python $REPO/tools/profile_ab_summary.py $OUT $STEPS > $OUT/summary.txt 2>&1
rc=$?
cat $OUT/summary.txt 2>/dev/null
[ $rc -eq 0 ] || find $OUT -name '*.csv' | head -20
# keep the summary, the traffic file and the logs; the per-dispatch csv files are large
for d in A_stats B_stats A_fetch B_fetch A_write B_write A2_fetch A2_write A_sq B_sq; do rm -rf $OUT/$d; done
exit $rc
