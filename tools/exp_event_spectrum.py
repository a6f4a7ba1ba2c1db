"""The cost of run_events(spectrum={}): the large-run case with and without the event power spectrum, in
interleaved pairs, alone and beside a coupling scan of 16 values (K sets), and what the spectrum says of the run.

usage: exp_event_spectrum.py [--session N] [events (1000000)] [chunk (65536)] [pairs (3)]
       exp_event_spectrum.py [--session N] --plain TAG [events] [chunk]
       exp_event_spectrum.py [--session N] --kernels [events] [chunk]
       exp_event_spectrum.py [--session N] --stats KERNEL_STATS.csv [events] [chunk]

Prints one JSON line per timed run ("spectrum": false / true, "couplings": 0 / 16, wall_s), one line per
configuration with the pairs' overhead, and one line with the tail index, n_eff and max_share of the run (and of
the scan's sets). --plain TAG: one fresh process that times the UNCHANGED call (no spectrum) once after a warm-up,
labelled "build": TAG -- run it in turns from this tree and from a checkout of the parent commit (ART_TREE names
the tree whose package is imported; default: this one) to see that the feature costs nothing when it is off.
--session N: every line also carries "session": N, to tell a repeated measurement from the first.
--kernels: a warm-up of one chunk and ONE run with the coupling scan of 16 and the spectrum, for a kernel trace taken
around it (rocprofv3 --kernel-trace --stats -- python exp_event_spectrum.py --kernels), and the time of the run's
last step on its own: the scan's 16 sets of tables brought to the host and turned into spectrum_result's dict.
--stats FILE: no GPU work; reads the kernel statistics of such a trace (a CSV with Name, Calls, TotalDurationNs) and
prints one line per event kernel, and the sums, per chunk of the run (the warm-up's chunk counted in)."""
import json
import os
import sys
import time

sys.path.insert(0, os.environ.get("ART_TREE") or os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import adiabatic_raytracer_amd as A  # noqa: E402

plain = stats = None
kernels_only = False
SESSION = {}
argv = sys.argv[1:]
if argv[:1] == ["--session"]:
    SESSION, argv = {"session": int(argv[1])}, argv[2:]
if argv[:1] == ["--plain"]:
    plain, argv = argv[1], argv[2:]
elif argv[:1] == ["--kernels"]:
    kernels_only, argv = True, argv[1:]
elif argv[:1] == ["--stats"]:
    stats, argv = argv[1], argv[2:]
arg = lambda i, d: int(argv[i]) if len(argv) > i else d  # noqa: E731
n, chunk, pairs = arg(0, 1_000_000), arg(1, 65536), arg(2, 3)


def emit(line):
    print(json.dumps({**line, **SESSION}), flush=True)


if stats is not None:
    import csv
    calls = -(-n // chunk) + 1  # the run's chunks and the warm-up's one
    rows = [r for r in csv.DictReader(open(stats)) if "event_" in r["Name"]]
    groups = {"spectrum": 0.0, "reweight": 0.0, "other event kernels": 0.0}
    for r in rows:
        name, ms = r["Name"].split("(")[0].replace("art::", ""), float(r["TotalDurationNs"]) * 1e-6
        key = "spectrum" if "spectrum" in name else "reweight" if "reweight" in name else "other event kernels"
        groups[key] += ms
        emit({"what": "kernel", "name": name, "calls": int(r["Calls"]), "total_ms": ms, "ms_per_chunk": ms / calls})
    emit({"what": "kernel sums", "chunks": calls, **{k + " ms_per_chunk": v / calls for k, v in groups.items()}})
    sys.exit(0)

eng = A.Engine(A.Params(theta_m=0.2, mass_a=1e-5, flat=True))
sky = dict(n_theta=32, n_phi=64)
g0 = eng.params.g_agg
G16 = [float(g0 * 2.0 ** (q / 4.0 - 2.0)) for q in range(16)]  # 0.25 g0 .. 3.4 g0; q = 8 is g0 itself


def timed(spectrum, couplings, **tag):
    kw = dict(chunk=chunk, rows=False, sky_map=sky)
    if couplings:
        kw["couplings"] = G16
    if spectrum:
        kw["spectrum"] = {}
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = eng.run_events(n, **kw)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    emit({"what": "run_events", "events": n, "chunk": chunk, "spectrum": bool(spectrum),
          "couplings": len(G16) if couplings else 0, "wall_s": dt, "f_inx": r["f_inx"], **tag})
    return dt, r


def figures(sp, s=1):
    pick = lambda v: np.asarray(v)[..., s].tolist()  # noqa: E731
    return {"alpha": pick(sp["alpha"]), "alpha_sigma": pick(sp["alpha_sigma"]), "n_eff": pick(sp["n_eff"]),
            "max_share": pick(sp["max_share"]), "positive": pick(sp["positive"]), "zeros": pick(sp["zeros"]),
            "bad": pick(sp["bad"]), "top_share_last": np.asarray(sp["top_share"])[..., s, -1].tolist(),
            "top": sp["top"], "bins": list(sp["bins"]) if sp["bins"] else None}


if plain is not None:
    eng.run_events(min(n, chunk), rows=False, sky_map=sky)  # warm-up: library load, kernels, pools
    timed(False, False, build=plain, what="run_events unchanged call")
    sys.exit(0)

eng.run_events(min(n, chunk), rows=False, sky_map=sky, spectrum={}, couplings=G16)  # warm-up
if kernels_only:
    timed(True, True, what="run_events under a kernel trace")
    spec = eng._zero_spectrum("coupling", len(G16), 3, 64)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    A.trees.spectrum_result(A.trees.spectrum_raw(spec), 1)
    emit({"what": "the last step alone: 16 sets of tables to the host and spectrum_result", "wall_s": time.perf_counter() - t0})
    sys.exit(0)
chunks = -(-n // chunk)
last = None
for couplings in (False, True):
    off, on = [], []
    for _ in range(pairs):
        off.append(timed(False, couplings)[0])
        dt, last_run = timed(True, couplings)
        on.append(dt)
        last = last_run if not couplings else last
        scan = last_run.get("coupling_scan")
    over = float(np.median(on) - np.median(off))
    emit({"what": "spectrum overhead", "events": n, "chunk": chunk, "couplings": len(G16) if couplings else 0,
          "off_s": off, "on_s": on, "off_spread_s": max(off) - min(off), "on_spread_s": max(on) - min(on),
          "overhead_s_median": over, "overhead_ms_per_chunk": 1e3 * over / chunks,
          "overhead_rel_median": float(np.median(on) / np.median(off) - 1.0)})
    if couplings:
        emit({"what": "spectrum of the coupling scan's sets (photons)", "g_over_g0": [g / g0 for g in G16],
              **figures(scan["spectrum"])})
sp = last["spectrum"]
emit({"what": "spectrum of the run (photons)", "events": n, "f_inx": last["f_inx"], **figures(sp),
      "top_event": np.asarray(sp["top_event"])[1, :8].tolist(),
      "hill_at_k": {str(k): float(sp["hill"][1, k - 2]) for k in (8, 16, 32, 63) if k - 2 < sp["hill"].shape[-1]}})
emit({"what": "spectrum of the run (axions)", "events": n, **figures(sp, 0)})
