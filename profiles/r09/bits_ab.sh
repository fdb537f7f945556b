#!/bin/bash
# What bench.py's last timed step computed, parent against tree, bit for bit:
#   profiles/r09/bits_ab.sh <parent libtrx.so> <tree libtrx.so> <scratch directory>
set -o pipefail
R=$(cd "$(dirname "$0")/../.." && pwd)
O=$3; mkdir -p $O
for arm in parent tree; do
  L=$1; [ $arm = tree ] && L=$2
  TRX_LIB=$L timeout -k 10 200 python $R/bench.py --gpus 1 --steps 2 --warmup 1 --no-cpu-baseline --dump-outputs $O/dump_$arm > $O/dump_$arm.json || exit 1
done
python - $O <<'PY'
import json, sys
import numpy as np
O = sys.argv[1]
for name in ("lnZ", "halfchi2"):
    a, b = (np.load("%s/dump_%s/%s.npy" % (O, arm, name)) for arm in ("parent", "tree"))
    print("%s.npy %s bit-identical: %s" % (name, a.shape, a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))))
ck = [json.loads(open("%s/dump_%s.json" % (O, arm)).read().strip().splitlines()[-1])["lnZ_checksum"] for arm in ("parent", "tree")]
print("lnZ_checksum parent %.17g tree %.17g equal: %s" % (ck[0], ck[1], ck[0] == ck[1]))
PY
