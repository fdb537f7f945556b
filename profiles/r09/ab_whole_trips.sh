#!/bin/bash
# Same-job A/B of production builds, arms alternating three times (the protocol of profiles/r08/ab_row_order.sh):
#   profiles/r09/ab_whole_trips.sh <parent libtrx.so> <tree libtrx.so> [name=<libtrx.so> ...]
# parent and tree: config 1 at --steps 20 --warmup 5 with --full, which adds the controls (2000 irregular stamps, 100 / 200
# points, the 64-TOI step: none of them runs the changed code); every further arm -- a build with one switch of the change
# alone -- config 1 only.  Every bench.py runs under its own time limit and a failure ends the job.
set -o pipefail
R=$(cd "$(dirname "$0")/../.." && pwd)
PARENT=$1; TREE=$2; shift 2
for rep in 1 2 3; do
  for arm in parent=$PARENT tree=$TREE "$@"; do
    name=${arm%%=*}; L=${arm#*=}; X=""
    if [ $name = parent ] || [ $name = tree ]; then X="--full"; fi
    TRX_LIB=$L timeout -k 10 300 python $R/bench.py --gpus 1 $X --steps 20 --warmup 5 --no-cpu-baseline --no-e2e --pmc off \
      | python $R/profiles/r08/ab_line.py $name $rep || exit 1
  done
done
