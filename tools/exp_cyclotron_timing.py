"""DEV TOOL: the cyclotron-observing launch against the plain device launch on the same batch
(Engine.propagate, art_last_kernel_ms: the integrator kernels between their HIP events), the two
alternating after a warm-up of each. One JSON line.

    python tools/exp_cyclotron_timing.py [RAYS] [CONFIG] [PAIRS] > profiles/NAME.jsonl"""
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import adiabatic_raytracer_amd as A  # noqa: E402

CONFIGS = {"flat": dict(theta_m=0.2, mass_a=1e-5, flat=True), "gr": dict(theta_m=0.0, mass_a=1e-6, flat=False),
           "gr_oblique": dict(theta_m=0.2, mass_a=1e-5, flat=False)}

if __name__ == "__main__":
    n = int(float(sys.argv[1])) if len(sys.argv) > 1 else 1_000_000
    cfg = sys.argv[2] if len(sys.argv) > 2 else "flat"
    pairs = int(sys.argv[3]) if len(sys.argv) > 3 else 3
    eng = A.Engine(A.Params(**CONFIGS[cfg]))
    inp = eng.forward_roots(n, seed=1769)
    outs = {False: None, True: None}
    ms = {False: [], True: []}
    for rep in range(pairs + 1):  # (pair 0 warms both up)
        for cyc in (False, True):
            outs[cyc] = eng.propagate(inp, out=outs[cyc], max_crossings=-1, cyclotron=cyc)
            t = eng.kernel_ms()
            if rep:
                ms[cyc].append(t)
    torch.cuda.synchronize()
    same = all(torch.equal(outs[False][k], outs[True][k]) for k in ("x_end", "k_end", "u7_end", "tau_end", "status",
                                                                    "n_accept", "n_reject", "n_cross"))
    cnt = outs[True]["cyc_count"].cpu().numpy()
    tau = outs[True]["cyc_tau"].cpu().numpy()
    st = outs[True]["status"].cpu().numpy()
    print(json.dumps({"rays": n, "config": cfg, "plain_ms": ms[False], "cyclotron_ms": ms[True],
                      "ratio_of_medians": float(np.median(ms[True]) / np.median(ms[False])),
                      "outputs_identical": bool(same), "rays_with_crossing": int((cnt > 0).sum()),
                      "escaping_rays": int((st == 0).sum()),
                      "exp_minus_tau_mean_over_escaping": float(np.exp(-tau[st == 0]).mean())}))
