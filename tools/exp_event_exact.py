"""The cost of run_events(exact=True) and what the order of the float adds costs ("Exact tables").

usage: exp_event_exact.py --case TAG [events (100000)] [runs (4)]
       exp_event_exact.py --kernel [events (100000)] [repeats (20)]
       exp_event_exact.py --deviation [events (100000)]

--case TAG: one fresh process that times run_events(events, rows=False, sky 32 x 64) `runs` times after a warm-up and
prints one JSON line per run and one with their median. TAG "parent" and "off": the unchanged call (run "parent" with
ART_TREE naming a checkout of the parent commit, whose package is then imported; default: this tree); TAG "on": with
exact=True; TAG "on-scan": with exact=True beside a coupling scan of 16 values, "off-scan" that scan without. Run the
cases in alternating processes.
--kernel: one chunk's forests grown once, then Engine.event_exact alone, in each mode, between HIP events
(`repeats` calls each after a warm-up call; the accumulators are zeroed outside the timed span), with a 32 x 64 sky
map, without one, and the normalisation's share (a call on a chunk without node records adds nothing and normalises).
--deviation: the run with rows and exact=True: per table the largest |float - exact| as a fraction of the bound
2 (cnt + 1) u S between two float sums of the bin's cnt rows, and how many entries differ at all."""
import json
import os
import sys
import time

sys.path.insert(0, os.environ.get("ART_TREE") or os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import adiabatic_raytracer_amd as A  # noqa: E402

argv = sys.argv[1:]
mode, tag = argv[0], None
if mode == "--case":
    tag, argv = argv[1], argv[2:]
else:
    argv = argv[1:]
arg = lambda i, d: int(argv[i]) if len(argv) > i else d  # noqa: E731
n, reps = arg(0, 100_000), arg(1, 4 if mode == "--case" else 20)
emit = lambda line: print(json.dumps(line), flush=True)  # noqa: E731

eng = A.Engine(A.Params(theta_m=0.2, mass_a=1e-5, flat=True))
sky = dict(n_theta=32, n_phi=64)
g0 = eng.params.g_agg
G16 = [float(g0 * 2.0 ** (q / 4.0 - 2.0)) for q in range(16)]

if mode == "--case":
    kw = dict(rows=False, sky_map=sky)
    if tag.startswith("on"):
        kw["exact"] = True
    if tag.endswith("-scan"):
        kw["couplings"] = G16
    eng.run_events(min(n, 4096), **kw)  # warm-up: library load, kernels, pools
    times = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = eng.run_events(n, **kw)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
        emit({"what": "run_events", "case": tag, "events": n, "wall_s": times[-1], "f_inx": r["f_inx"]})
    emit({"what": "run_events median", "case": tag, "events": n, "runs": reps, "wall_s_median": float(np.median(times)),
          "wall_s_min": min(times), "wall_s_max": max(times)})
    sys.exit(0)

if mode == "--kernel":
    from dataclasses import replace
    back_eng = A.Engine(replace(eng.params, B0=-eng.params.B0))
    s = eng.sample(n, seed=1769)
    w5 = eng.event_weight(s)
    back = back_eng.grow_trees(s["x"], -s["k_init"], s["erg"], 0, num_cutoff=0, splittings_cutoff=100000, crossing_cap=256, seed=1769)
    fwd = eng.grow_trees(s["x"], s["k_init"], s["erg"], 1, seed=1769)
    none = dict(fwd, n_nodes=0)  # no records: the call adds nothing and normalises every table

    def timed(what, forest, sky_map, how):
        acc = eng.event_exact(s, w5, back, forest, sky=sky_map, mode=how)  # warm-up
        ms = []
        for _ in range(reps):
            for k in ("flux", "sky", "totals"):
                if acc[k] is not None:
                    acc[k].zero_()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            eng.event_exact(s, w5, back, forest, sky=sky_map, mode=how, acc=acc)
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b))
        emit({"what": what, "mode": how, "sky": sky_map is not None, "events": n, "records": int(forest["n_nodes"]),
              "ms_median": float(np.median(ms)), "ms_min": min(ms), "ms_max": max(ms)})

    for how in ("lds", "global", "auto"):
        timed("event_exact alone", fwd, sky, how)
    for how in ("lds", "global"):
        timed("event_exact alone, no sky map", fwd, None, how)
    timed("the normalisation alone", none, sky, "lds")
    timed("the normalisation alone, no sky map", none, None, "lds")
    # the float kernels of the same chunk, for scale
    for what, fn in (("event_rows (bins only)", lambda: eng.event_rows(s, w5, back, fwd, sky=sky, rows=False)),
                     ("event_replicates R = 8", lambda: eng.event_replicates(s, w5, back, fwd, 8, sky=sky))):
        fn()
        ms = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b))
        emit({"what": what, "events": n, "ms_median": float(np.median(ms)), "ms_min": min(ms), "ms_max": max(ms)})
    sys.exit(0)

# --deviation
U = 2.0 ** -53
r = eng.run_events(n, sky_map=dict(sky, theta_axis="theta"), exact=True)
rows = r["rows_raw"].cpu().numpy()
unit = rows.copy()
unit[:, 7] = unit[:, 8] = 1.0
cnt = A.trees.rows_exact(unit, 50, dict(sky, theta_axis="theta"))
ex = r["exact"]
for name, flt, exact, c in (("flux", r["flux_raw"], ex["flux_raw"], cnt["flux_raw"]), ("sky", r["sky_raw"], ex["sky_raw"], cnt["sky_raw"]),
                            ("totals", r["totals"][2:4], ex["totals_raw"], cnt["totals_raw"])):
    flt, exact, c = (np.asarray(v.cpu().numpy() if torch.is_tensor(v) else v, np.float64).reshape(-1) for v in (flt, exact, c))
    err, bound = np.abs(flt - exact), 2 * (c + 1) * U * np.maximum(flt, exact)
    f = bound > 0
    ulp = np.spacing(exact[f])
    emit({"what": "float table against the exact one", "table": name, "events": n, "rows": int(len(rows)), "entries_filled": int(f.sum()),
          "entries_that_differ": int((flt != exact).sum()), "bound_ratio_max": float(np.max(err[f] / bound[f])),
          "bound_ratio_median": float(np.median(err[f] / bound[f])), "ulp_max": float(np.max(err[f] / ulp)),
          "rel_max": float(np.max(err[f] / exact[f])), "rows_per_entry_max": int(c.max())})
emit({"what": "exact run", "events": n, "f_inx": r["f_inx"], "nonfinite": float(ex["nonfinite"].item())})
