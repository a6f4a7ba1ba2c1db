"""Event throughput of the full pipeline, §8(f) rank 1: main_runner_tree (MainRunner.jl:354-763)
batched on the GPU against the oracle's event-by-event restatement on one host thread. The
oracle follows the reference's own model of one event at a time per process.

Each event is one sampled conversion point (find_samples_new). It then gets its backtrace
tree (axion, -B0, every crossing) and its forward photon tree. The defaults are
num_cutoff = MC_nodes = 5 and max_nodes = 50.

usage: [ART_DONATE=lanes] [ART_DEVICE_TREES=0|1|ab|events|events-ab] [ART_EVENTS_BIG=n,chunk] exp_events.py [flat|gr]
       [gpu event counts, comma-separated] [cpu events] [repeats]
ART_DEVICE_TREES: 0 (the default) grows the trees with the host forest (art_grow_trees), 1 with the
device-resident driver (main_runner_tree(device_trees=True), art_grow_trees_device), ab runs both,
alternating, `repeats` times (default 1) for each event count. events runs
main_runner_tree(device_events=True) (Engine.run_events: rows, flux and sky map built in HBM),
events-ab alternates device trees and device events. ART_EVENTS_BIG=n,chunk adds one
Engine.run_events(n, chunk=chunk, rows=False) run with the default sky map after the counts (untimed
warm-up of one chunk first). Prints one JSON line per run; its "trees" key says which variant ran. After each event count's runs one more line ("forest shape",
untimed) gives the forward forest's rounds -- its batched propagate launches -- and the sum of their
batch sizes, from the trees' counts."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import adiabatic_raytracer_amd as A  # noqa: E402
from adiabatic_raytracer_amd import trees  # noqa: E402

CFG = {"flat": dict(theta_m=0.2, mass_a=1e-5, flat=True), "gr": dict(theta_m=0.0, mass_a=1e-6, flat=False)}
cfg = sys.argv[1] if len(sys.argv) > 1 else "flat"
counts = [int(c) for c in (sys.argv[2] if len(sys.argv) > 2 else "1000,10000").split(",")]
n_cpu = int(sys.argv[3]) if len(sys.argv) > 3 else 50
repeats = int(sys.argv[4]) if len(sys.argv) > 4 else 1
p = A.Params(**CFG[cfg])
DONATE = int(os.environ.get("ART_DONATE", "-1"))  # tail donation of the forest's launches (-1: the library default)
if DONATE >= 0:
    import ctypes as C
    A._lib.load().art_set_tail_donation(C.c_int32(DONATE))
SIDES = {"0": [False], "1": [True], "ab": [False, True], "events": ["events"],
         "events-ab": [True, "events"]}[os.environ.get("ART_DEVICE_TREES", "0")]
NAME = {False: "host", True: "device", "events": "device events"}


def run(n, dev, **kw):
    if dev == "events":
        return trees.main_runner_tree(p, n + 1, device_events=True, **kw)
    return trees.main_runner_tree(p, n + 1, device_trees=dev, **kw)


for dev in SIDES:
    run(64, dev)  # warm-up: library load, kernels, pools
for n in counts:
    for _ in range(repeats):
        for dev in SIDES:
            info = {}
            t0 = time.perf_counter()
            rows = run(n, dev, run_info=info)
            dt = time.perf_counter() - t0
            print(json.dumps({"config": cfg, "side": "gpu", "trees": NAME[dev], "donate": DONATE,
                              "events": n, "wall_s": dt, "events_per_s": n / dt, "rows": int(rows.shape[0]),
                              "f_inx": info["f_inx"]}), flush=True)
    # the forward forest's shape (untimed): a tree takes part in `count` rounds, one segment in each
    s = A.sample_conversion_points(p, n, seed=1769)
    _, cnt, _ = trees.grow_trees(p, s["x"], s["k_init"], s["erg"], 1, device=bool(SIDES[-1]))
    print(json.dumps({"config": cfg, "side": "forest shape", "trees": "device" if SIDES[-1] else "host", "events": n,
                      "rounds": int(cnt.max()) if n else 0, "batch_sum": int(cnt.sum())}), flush=True)

if os.environ.get("ART_EVENTS_BIG"):
    import torch
    n_big, chunk = (int(v) for v in os.environ["ART_EVENTS_BIG"].split(","))
    eng = A.Engine(p)
    eng.run_events(min(chunk, n_big), rows=False, sky_map={})
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.perf_counter()
    r = eng.run_events(n_big, chunk=chunk, rows=False, sky_map={})
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    print(json.dumps({"config": cfg, "side": "gpu", "trees": "device events, chunked, rows=False, sky map 32x64x1",
                      "events": n_big, "chunk": chunk, "wall_s": dt, "events_per_s": n_big / dt, "rows": r["n_rows"],
                      "f_inx": r["f_inx"], "torch_peak_bytes": int(torch.cuda.max_memory_allocated())}), flush=True)

if n_cpu > 0:
    import oracle as O
    from oracle.tree import main_runner_rows
    O.build()
    po = O.make_params(**CFG[cfg])
    t0 = time.perf_counter()
    rows = main_runner_rows(po, n_cpu + 1)
    dt = time.perf_counter() - t0
    print(json.dumps({"config": cfg, "side": "cpu (oracle, 1 thread, event by event)", "events": n_cpu, "wall_s": dt,
                      "events_per_s": n_cpu / dt, "rows": int(rows.shape[0])}), flush=True)
