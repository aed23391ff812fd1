#!/bin/bash
# tools/ab_procs.sh [-r rounds] [-s steps] [-w "workload ..."] parent.so new.so   -- on the GPU box.
#   Two builds of the library against each other as profiles/r09_even_deal_ab.txt has them: separate processes, interleaved
#   (workload by workload, parent then new), kernel time by tools/ab_kernel.py, then plain bench.py's ms_per_step on the
#   default workload.  Every process runs under a time limit and the first one that fails ends the script.
ROUNDS=5; STEPS=200; WLS="survey3_65536 realistic_65536 dcs94_65536 mixed_16384 dcs93_4096"
while getopts "r:s:w:" o; do case $o in r) ROUNDS=$OPTARG;; s) STEPS=$OPTARG;; w) WLS=$OPTARG;; esac; done; shift $((OPTIND - 1))
PARENT=$(realpath "$1"); NEW=$(realpath "$2"); HERE=$(cd "$(dirname "$0")/.." && pwd)
for r in $(seq $ROUNDS); do for wl in $WLS; do for tag in parent new; do
  lib=$NEW; [ $tag = parent ] && lib=$PARENT
  DCS_TAG=$tag DCS_HIP_LIB=$lib timeout -k 10 120 python "$HERE/tools/ab_kernel.py" $wl $STEPS || { echo "round $r $wl $tag failed: stopping"; exit 1; }
done; done; done
for r in $(seq $ROUNDS); do for tag in parent new; do
  lib=$NEW; [ $tag = parent ] && lib=$PARENT
  DCS_HIP_LIB=$lib timeout -k 10 300 python "$HERE/bench.py" --gpus 1 --steps $STEPS --warmup 20 2>/dev/null | python -c "
import json,sys
d=json.loads(sys.stdin.read().strip().splitlines()[-1]); print('$tag ms_per_step %.6f value %.4e' % (d['ms_per_step'], d['value']))" || { echo "bench round $r $tag failed: stopping"; exit 1; }
done; done
