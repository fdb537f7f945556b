"""trx_grid_quantiles against np.quantile on the grid target.fit_bands reduces for a 75-scenario table with 1000 samples
per scenario and 100 model points: [75 * 1000][100] doubles (60 MB), one call per scenario on its 1000 rows, and one
model-average call of 4096 gathered, rescaled rows.  Prints the lines of results.txt.

    python profiles/bands/measure.py            device events and the host clock, np.quantile on the same grid
    python profiles/bands/measure.py --trace    the device calls only, a few passes: the run to put under
                                                rocprofv3 --kernel-trace --stats (kernel time of band_quantile_kernel)"""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from triceratops_amd import _lib  # noqa: E402

SCEN, DRAWS, POINTS, MIX = 75, 1000, 100, 4096
Q = (0.16, 0.5, 0.84)
REPS = int(os.environ.get("REPS", "20"))

_lib.require_gpu()
rng = np.random.default_rng(13)
grid = 1.0 - 0.01 * rng.random((SCEN * DRAWS, POINTS))
grid[rng.random(grid.shape) < 2.0 / 3.0] = 1.0           # out of transit: exact ties, as in model curves
rows = rng.integers(0, SCEN * DRAWS, MIX)
scale = 1.0 - 0.5 * rng.random(MIX)
g_d = _lib.dev(grid)
rows_d = torch.as_tensor(rows).to(g_d.device)
scale_d = _lib.dev(scale)
out = torch.empty((SCEN + 1, len(Q), POINTS), dtype=torch.float64, device=g_d.device)


def device_pass():
    for k in range(SCEN):
        out[k] = _lib.grid_quantiles(g_d[k * DRAWS:(k + 1) * DRAWS], Q)
    out[SCEN] = _lib.grid_quantiles(g_d, Q, rows_d=rows_d, scale_d=scale_d)


device_pass()
torch.cuda.synchronize()
if "--trace" in sys.argv:
    for _ in range(5):
        device_pass()
    torch.cuda.synchronize()
    print("traced 6 passes of %d + 1 calls" % SCEN)
    sys.exit(0)

ms = []
for _ in range(REPS):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    device_pass()
    e1.record()
    torch.cuda.synchronize()
    ms.append(e0.elapsed_time(e1))
ms = np.array(ms)
print("grid [%d x %d][%d] fp64 (%.0f MB), q = %r" % (SCEN, DRAWS, POINTS, grid.nbytes / 1e6, Q))
print("device, %d calls of %d rows + 1 gathered call of %d rows, events around the pass: median %.3f ms (min %.3f, max %.3f, "
      "%d passes)" % (SCEN, DRAWS, MIX, np.median(ms), ms.min(), ms.max(), REPS))

host = []
for _ in range(3):
    t0 = time.perf_counter()
    want = np.stack([np.quantile(grid[k * DRAWS:(k + 1) * DRAWS], Q, axis=0) for k in range(SCEN)]
                    + [np.quantile(1 - scale[:, None] * (1 - grid[rows]), Q, axis=0)])
    host.append((time.perf_counter() - t0) * 1e3)
print("np.quantile, the same %d + 1 reductions on the host copy: median %.1f ms (min %.1f, max %.1f, 3 passes, %d threads)"
      % (SCEN, np.median(host), min(host), max(host), torch.get_num_threads()))
print("largest |device - np.quantile|: %.3g" % np.abs(out.cpu().numpy() - want).max())
