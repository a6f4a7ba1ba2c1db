"""The cost of run_events(errors=True): the large-run case with and without the event moments, in
interleaved pairs, and the block-to-block scatter of the total photon power against its predicted σ.

usage: exp_event_moments.py [events (1000000)] [chunk (65536)] [pairs (3)] [blocks (16)] [block events (4096)]

Prints one JSON line per timed run ("errors": false / true, wall_s), one line with the pairs' overhead,
and one informational line: the standard deviation of sum_weight_sln_prob[photons] over `blocks`
disjoint blocks of `block events` events (run_events with event_offset), the mean of the blocks'
predicted σ, and their ratio. Heavy-tailed weights make that ratio noisy; no threshold is derived for it."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import adiabatic_raytracer_amd as A  # noqa: E402

arg = lambda i, d: int(sys.argv[i]) if len(sys.argv) > i else d  # noqa: E731
n, chunk, pairs, blocks, block_n = arg(1, 1_000_000), arg(2, 65536), arg(3, 3), arg(4, 16), arg(5, 4096)
eng = A.Engine(A.Params(theta_m=0.2, mass_a=1e-5, flat=True))
sky = dict(n_theta=32, n_phi=64)


def timed(errors):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = eng.run_events(n, chunk=chunk, rows=False, sky_map=sky, errors=errors)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    line = {"what": "run_events", "events": n, "chunk": chunk, "errors": errors, "wall_s": dt, "f_inx": r["f_inx"]}
    if errors:
        rel = (r["flux_sigma"][1] / r["flux"][1]).cpu().numpy()
        line.update(photon_flux_rel_sigma_median=float(np.nanmedian(rel)),
                    photon_total_rel_sigma=r["sum_weight_sln_prob_sigma"][1] / r["sum_weight_sln_prob"][1])
    print(json.dumps(line), flush=True)
    return dt


if pairs > 0:
    eng.run_events(min(n, chunk), rows=False, sky_map=sky, errors=True)  # warm-up: library load, kernels, pools
    off, on = [], []
    for _ in range(pairs):
        off.append(timed(False))
        on.append(timed(True))
    print(json.dumps({"what": "errors overhead", "events": n, "chunk": chunk, "off_s": off, "on_s": on,
                      "off_spread_s": max(off) - min(off), "overhead_s_median": float(np.median(on) - np.median(off)),
                      "overhead_rel_median": float(np.median(on) / np.median(off) - 1.0)}), flush=True)

if blocks > 1:
    tot, sig = [], []
    for b in range(blocks):
        r = eng.run_events(block_n, event_offset=b * block_n, rows=False, errors=True)
        tot.append(r["sum_weight_sln_prob"][1])
        sig.append(r["sum_weight_sln_prob_sigma"][1])
    scatter = float(np.std(tot, ddof=1))
    print(json.dumps({"what": "block scatter of the total photon power (information, no threshold)", "blocks": blocks,
                      "block_events": block_n, "scatter": scatter, "sigma_mean": float(np.mean(sig)),
                      "sigma_min": float(np.min(sig)), "sigma_max": float(np.max(sig)),
                      "scatter_over_sigma": scatter / float(np.mean(sig))}), flush=True)
