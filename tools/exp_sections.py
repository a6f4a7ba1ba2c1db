"""Dev: where the integrator's time goes, per main-loop section, from the
ART_SECTION_TIMING build (s_memtime cycles summed over every wave's iterations; the
stats slots carry the 8 section sums). Usage: ART_LIB=.../libart_sect.so exp_sections.py [n] [--host]
--host: the streamed host call's integrator (DON = 3) instead of the device launch's; kernel_ms is then the
launch's span by its in-kernel clock stamps."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import adiabatic_raytracer_amd as A  # noqa: E402
from adiabatic_raytracer_amd import Engine  # noqa: E402

NAMES = ["refill + reload, events, finish, stores", "step size + stage slots", "error norm, controller, certificate, parking",
         "grid pass", "sign-code fast paths", "code walk", "cooperative pass", "per-lane fallback"]
if "slot" in os.environ.get("ART_LIB", ""):
    NAMES = ["refill etc", "slot combination", "slot RHS", "slot rest", "norm/controller/cert/park", "grid pass",
             "fast+walk+coop", "fallback"]
host = "--host" in sys.argv
args = [a for a in sys.argv[1:] if a != "--host"]
n = int(args[0]) if args else 10_000_000
eng = Engine(A.Params(theta_m=0.2, mass_a=1e-5, flat=True))
inp = eng.forward_roots(n, seed=1769)
if host:
    import numpy as np
    x0, k0, erg = (inp[k].cpu().numpy() for k in ("x0", "k0", "erg"))
    for _ in range(2):
        res = A.propagate_batch(eng.params, x0, k0, erg, -np.ones(n), np.full(n, -30.0), np.ones(n, np.int8), flux_nbins=50)
    ms = A.raytracer.recent_kernel_span_ms(1)[0]  # (the integrator's span by its own clock stamps)
    st = [res["stats"][k] for k in ("attempts", "accepted", "root_steps", "scan_evals", "interp_evals", "rays", "init_rhs",
                                    "cert_steps")]
else:
    out = eng.alloc_out(n)
    for _ in range(2):
        eng.propagate(inp, out)
    ms = eng.kernel_ms()
    st = list(A.raytracer.last_stats().values())[:8]
st[6] -= 2 * n  # init_kernel's RHS count shares slot 6
tot = sum(st)
print(json.dumps({"kernel_ms": ms, "sections": {k: round(v / tot, 4) for k, v in zip(NAMES, st)},
                  "cycles_total": tot}), flush=True)
