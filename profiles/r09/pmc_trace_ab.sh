#!/bin/bash
# Per build, each in a run of its own: a counters-only pass of profiles/r07/cells2000_once.py (one launch per family on
# config 1's grid), then a kernel trace with statistics of bench.py's config-1 loop.
#   profiles/r09/pmc_trace_ab.sh <parent libtrx.so> <tree libtrx.so> <output directory>
set -o pipefail
R=$(cd "$(dirname "$0")/../.." && pwd); cd $R
O=$3; mkdir -p $O
for arm in parent tree; do
  L=$1; [ $arm = tree ] && L=$2
  TRX_LIB=$L timeout -k 10 180 rocprofv3 --pmc SQ_INSTS_VALU SQ_ACTIVE_INST_VALU SQ_BUSY_CYCLES SQ_WAVE_CYCLES --output-format csv -d $O/pmc_$arm -- python3 profiles/r07/cells2000_once.py > $O/pmc_$arm.log 2>&1 || { echo "pmc pass failed: $arm"; tail -5 $O/pmc_$arm.log; exit 1; }
  python3 profiles/pmc_summary.py $O/pmc_$arm > $O/pmc_${arm}_summary.txt 2>&1 || exit 1
  rm -rf $O/pmc_$arm
  TRX_LIB=$L timeout -k 10 240 rocprofv3 --kernel-trace --stats --output-format csv -d $O/trace_$arm -- python3 bench.py --gpus 1 --steps 3 --warmup 1 --no-extras > $O/trace_$arm.log 2>&1 || { echo "trace failed: $arm"; tail -5 $O/trace_$arm.log; exit 1; }
  F=$(find $O/trace_$arm -name "*kernel_stats.csv" | head -1); [ -n "$F" ] && head -9 "$F" > $O/${arm}_kernel_stats.csv
  rm -rf $O/trace_$arm
done
for arm in parent tree; do echo "== $arm"; grep -A4 "cells_kernel <0" $O/pmc_${arm}_summary.txt; cat $O/${arm}_kernel_stats.csv; done
