"""DEV TOOL: the times of the emission map ("Emission maps"), one JSON line each.

usage: exp_origin_timing.py --kernel [events (100000)] [repeats (20)]
       exp_origin_timing.py --run [events (1000000)] [pairs (3)]

--kernel: one chunk's forests grown once, then between HIP events (the median of `repeats` calls after a warm-up, as
tools/exp_skymap_timing.py measures the sky map) Engine.event_origin against the yardsticks on the same forest:
  - 1 x 16 x 32, no observer (its table in LDS), against Engine.event_rows binning a 16 x 32 sky map (rows=False,
    no flux table);
  - 16 x 32 origin x 16 x 32 observer with groups = 32 (adds to HBM) against Engine.event_replicates with R = 32 and a
    sky map of as many bins, 512 x 512 (no flux table);
  - and either map in the other accumulation mode where it fits, with bin_out and power_out, and with a range of r.
--run: run_events(events, chunk=65536, rows=False) with and without origin_map={}, as interleaved pairs after a warm-up."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import adiabatic_raytracer_amd as A  # noqa: E402

mode, argv = sys.argv[1], sys.argv[2:]
arg = lambda i, d: int(float(argv[i])) if len(argv) > i else d  # noqa: E731
emit = lambda line: print(json.dumps(line), flush=True)  # noqa: E731
eng = A.Engine(A.Params(theta_m=0.2, mass_a=1e-5, flat=True))

if mode == "--run":
    n, pairs = arg(0, 1_000_000), arg(1, 3)
    kw = dict(chunk=65536, rows=False)
    eng.run_events(4096, origin_map={}, **kw)  # warm-up: library load, kernels, pools
    eng.run_events(4096, **kw)
    times = {"off": [], "on": []}
    for _ in range(pairs):
        for tag, extra in (("off", {}), ("on", {"origin_map": {}})):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = eng.run_events(n, **kw, **extra)
            torch.cuda.synchronize()
            times[tag].append(time.perf_counter() - t0)
            emit({"what": "run_events", "case": tag, "events": n, "wall_s": times[tag][-1], "f_inx": r["f_inx"]})
    emit({"what": "run_events medians", "events": n, "pairs": pairs, "off_s": float(np.median(times["off"])),
          "on_s": float(np.median(times["on"])), "added_s": float(np.median(times["on"]) - np.median(times["off"]))})
    sys.exit(0)

from dataclasses import replace  # noqa: E402

n, reps = arg(0, 100_000), arg(1, 20)
back_eng = A.Engine(replace(eng.params, B0=-eng.params.B0))
s = eng.sample(n, seed=1769)
w5 = eng.event_weight(s)
back = back_eng.grow_trees(s["x"], -s["k_init"], s["erg"], 0, num_cutoff=0, splittings_cutoff=100000, crossing_cap=256, seed=1769)
fwd = eng.grow_trees(s["x"], s["k_init"], s["erg"], 1, seed=1769)
parts = (s, w5, back, fwd)


def timed(what, fn, **info):
    fn()
    fn()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    emit({"what": what, "events": n, "records": int(fwd["n_nodes"]), "ms_median": float(np.median(ms)), "ms_min": min(ms),
          "ms_max": max(ms), **info})
    return float(np.median(ms))


def origin(origin_kw, observer=None, groups=None, **kw):
    hist = eng.event_origin(*parts, origin_kw, observer=observer, groups=groups)  # (the table made once, then added to)
    return lambda: eng.event_origin(*parts, hist["spec"], groups=groups, hist=hist, **kw)


# 1. the LDS path against event_rows' sky map
sky = dict(n_theta=16, n_phi=32)
sky_hist = torch.zeros(2, 16, 32, 1, dtype=torch.float64, device=eng.device)
tot = torch.zeros(6, dtype=torch.float64, device=eng.device)
t_rows = timed("event_rows, sky 16 x 32, no rows, no flux (yardstick)",
               lambda: eng.event_rows(*parts, nbins=0, sky=sky, sky_hist=sky_hist, totals=tot, rows=False))
t = timed("event_origin 1 x 16 x 32 (lds)", origin({}))
emit({"what": "ratio, LDS", "origin_over_yardstick": t / t_rows})
timed("event_origin 1 x 16 x 32 (global)", origin({"mode": 2}))
timed("event_origin 1 x 16 x 32 (lds), bin_out and power_out", origin({}, return_bins=True))
r = torch.linalg.norm(s["x"].view(3, -1), dim=0)
timed("event_origin 4 x 16 x 32 over a range of r (lds)",
      origin({"n_r": 4, "r_range": (float(r.quantile(0.02).item()), float(r.quantile(0.98).item()))}))
timed("event_origin 1 x 16 x 32 x observer 2 x 3 (lds, 6144 doubles)", origin({}, dict(n_theta=2, n_phi=3)))

# 2. the HBM path against event_replicates
big = dict(n_theta=512, n_phi=512)
rep = eng.event_replicates(*parts, 32, nbins=0, sky=big)
t_rep = timed("event_replicates R = 32, sky 512 x 512, no flux (yardstick)",
              lambda: eng.event_replicates(*parts, 32, nbins=0, sky=big, rep=rep))
t = timed("event_origin 16 x 32 x observer 16 x 32, groups = 32 (global)", origin({}, dict(n_theta=16, n_phi=32), 32))
emit({"what": "ratio, global", "origin_over_yardstick": t / t_rep})
timed("event_origin 16 x 32 x observer 16 x 32, no groups (global)", origin({}, dict(n_theta=16, n_phi=32)))
