#!/bin/bash
# Kernel trace of bench.py's config-1 loop per build (what rowc_kernel's filing and the 4 KB memset cost):
#   profiles/r08/trace_ab.sh <parent libtrx.so> <tree libtrx.so> <output directory>
set -o pipefail
R=$(cd "$(dirname "$0")/../.." && pwd)
O=$3; mkdir -p $O
for arm in parent tree; do
  if [ $arm = parent ]; then L=$1; else L=$2; fi
  TRX_LIB=$L timeout -k 10 240 rocprofv3 --kernel-trace --stats --output-format csv -d $O/trace_$arm -- python3 $R/bench.py --gpus 1 --steps 3 --warmup 1 --no-extras > $O/trace_${arm}.log 2>&1 || { echo "trace failed: $arm"; tail -5 $O/trace_${arm}.log; exit 1; }
  F=$(find $O/trace_$arm -name "*kernel_stats.csv" | head -1); [ -n "$F" ] && head -9 "$F" > $O/${arm}_kernel_stats.csv
  rm -rf $O/trace_$arm
  echo "== $arm"; cat $O/${arm}_kernel_stats.csv
done
