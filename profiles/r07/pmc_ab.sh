#!/bin/bash
# counters-only passes (no tracing beside them) of cells2000_once.py for two builds of the library, then a kernel trace of
# bench.py --no-extras for each:  bash profiles/r07/pmc_ab.sh <parent libtrx.so> <tree libtrx.so> [output directory]
set -o pipefail
R=$(cd "$(dirname "$0")/../.." && pwd); cd $R
O=${3:-$R/build/r07}; mkdir -p $O
for arm in parent tree; do
  L=$1; [ $arm = tree ] && L=$2
  i=0
  for PMC in "SQ_INSTS_VALU SQ_ACTIVE_INST_VALU SQ_THREAD_CYCLES_VALU SQ_WAIT_INST_ANY SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_WAVES" \
             "SQ_LDS_BANK_CONFLICT SQ_ACTIVE_INST_LDS SQ_INSTS_LDS SQ_INSTS_SALU SQ_INSTS_SMEM SQ_INSTS_VMEM_RD SQ_ACTIVE_INST_ANY"; do
    i=$((i+1))
    TRX_LIB=$L timeout -k 10 180 rocprofv3 --pmc $PMC --output-format csv -d $O/pmc_$arm/pass$i -- python3 profiles/r07/cells2000_once.py > $O/pmc_${arm}_pass$i.log 2>&1 || { echo "pmc pass failed: $arm $i"; tail -5 $O/pmc_${arm}_pass$i.log; exit 1; }
  done
  python3 profiles/pmc_summary.py $O/pmc_$arm > $O/pmc_${arm}_summary.txt 2>&1 || exit 1
  TRX_LIB=$L timeout -k 10 240 rocprofv3 --kernel-trace --stats --output-format csv -d $O/trace_$arm -- python3 bench.py --gpus 1 --steps 3 --warmup 1 --no-extras > $O/trace_${arm}.log 2>&1 || { echo "trace failed: $arm"; tail -5 $O/trace_${arm}.log; exit 1; }
  F=$(find $O/trace_$arm -name "*kernel_stats.csv" | head -1); [ -n "$F" ] && head -8 "$F" > $O/${arm}_kernel_stats.csv
done
for arm in parent tree; do echo "== $arm"; cat $O/pmc_${arm}_summary.txt; cat $O/${arm}_kernel_stats.csv; done
