"""The tail of cells_kernel's one-row launches on BASELINE config 1's grid (2000 uniform points, 10^5 rows per family, every
row evaluated), per family, with the rows as they come and dearest first:

    TRX_LIB=<a build with -DTRX_TESTING -DTRX_TAIL_TIMERS> python profiles/r08/tail_once.py [n_rows]

Per launch: span = latest finish - earliest start; tail = latest finish - latest start (the dispatcher ran out of rows
at the latest start); occupancy = busy wave time inside the tail / (tail x 4096 wave slots); idle = the share of the
span's slot time that the tail leaves unused, tail x (1 - occupancy) / span.  Times from the device's constant-rate
wall clock (100 MHz on this part: 10 ns a tick)."""
import ctypes, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np, torch
from triceratops_amd import _lib, synth

SLOTS, TICK_US = 4096, 0.01
n_time, n_rows = 2000, int(sys.argv[1]) if len(sys.argv) > 1 else 100000
L = _lib.lib()
rng = np.random.default_rng(synth.SEED)
t_d = _lib.dev(synth.time_grid(n_time))
curve, _ = _lib.flux_grid(0, 0, t_d, _lib.dev(synth.reference_tp_row()), synth.EXPTIME, synth.NSAMPLES, False)
f_d = _lib.dev(synth.noisy_light_curve(rng, curve[0].cpu().numpy()))
out = torch.empty(n_rows, dtype=torch.float64, device="cuda")
rows = [_lib.dev(synth.family_rows(rng, fam, n_rows)) for fam in synth.FAMILIES]
head = (ctypes.c_ulonglong * 4)()
finish = np.zeros(n_rows, dtype=np.uint64)


def launch(i):
    fam = synth.FAMILIES[i]
    flags = (_lib.FLAG_COMPANION_IS_HOST if fam[2] else 0) | _lib.FLAG_EVALUATE_EXCLUDED
    _lib.lnl_batch(fam[1], flags, t_d, f_d, synth.SIGMA, rows[i], synth.EXPTIME, synth.NSAMPLES, out=out)


launch(0)                                       # (scratch, memo, code objects)
_lib.check(L.trx_debug_tail(head, None, ctypes.c_long(0)))
results = {}
for order in (0, 1):
    _lib.check(L.trx_set_row_order(order))
    keep = []
    for i, fam in enumerate(synth.FAMILIES):
        launch(i)
        _lib.check(L.trx_debug_tail(head, finish.ctypes.data_as(ctypes.POINTER(ctypes.c_ulonglong)), ctypes.c_long(n_rows)))
        first, last_start, last_finish, busy = (int(x) for x in head)
        span, tail = last_finish - first, last_finish - last_start
        f = finish.astype(np.int64)
        in_tail = np.clip(f - last_start, 0, None).sum()
        occ = in_tail / (tail * SLOTS) if tail > 0 else 1.0
        keep.append((span * TICK_US, tail * TICK_US, occ, tail * (1.0 - occ) / span, busy / (span * SLOTS)))
        print("order %d  %-6s span %8.1f us  tail %7.1f us  occupancy in tail %.3f  idle share of the launch %.4f  "
              "occupancy overall %.3f" % ((order, fam[0]) + keep[-1]))
    results[order] = np.array(keep)
    m = results[order].mean(axis=0)
    print("order %d  mean   span %8.1f us  tail %7.1f us  occupancy in tail %.3f  idle share of the launch %.4f  "
          "occupancy overall %.3f" % ((order,) + tuple(m)))
d = results[0].mean(axis=0) - results[1].mean(axis=0)
print("as they come -> dearest first: span %+.1f us, tail %+.1f us" % (-d[0], -d[1]))
