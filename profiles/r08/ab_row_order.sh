#!/bin/bash
# Same-job A/B of two production builds, arms alternating three times (the protocol of profiles/r07/ab_window_trips.txt):
#   profiles/r08/ab_row_order.sh <parent libtrx.so> <tree libtrx.so> [extra bench.py arguments]
# config 1 at --steps 20 --warmup 5; --full adds the shapes that are the controls (100 / 200 points: the batched variant)
# and the 2000 irregular stamps, which run the changed path.
set -o pipefail
R=$(cd "$(dirname "$0")/../.." && pwd)
PARENT=$1; TREE=$2; shift 2
for rep in 1 2 3; do
  for arm in parent tree; do
    if [ $arm = parent ]; then L=$PARENT; else L=$TREE; fi
    TRX_LIB=$L timeout -k 10 300 python $R/bench.py --gpus 1 --full --steps 20 --warmup 5 --no-cpu-baseline --no-e2e --pmc off "$@" \
      | python $R/profiles/r08/ab_line.py $arm $rep || exit 1
  done
done
