"""Converged-truth fixtures for the cyclotron-resonance optical depth (TEST INFRASTRUCTURE ONLY).

The reference keeps the cyclotron optical depth as dead code (cyclotronF / tau_cyc,
RayTracer.jl:792-851) and writes opticalDepth = 0 (MainRunner.jl:703-708), so the engine's
observation is pinned to a converged solution of the same equations, as make_truth_fixture.py does
for the segment itself:

* each ray is integrated as the engine integrates it: scipy's DOP853 on the oracle's RHS (rtol
  1e-13, atol 1e-15), ended at the first plasma-resonance crossing that affect! records, at
  1.01 rNS or at ln_t_end, exactly as make_truth_fixture.truth_ray ends it;
* g = ln ω_c - ln erg is evaluated at 50 points of every truth step's dense output up to the
  ray's end, with a dipole written here in numpy (Cartesian: B = B0 rNS³/2 [3 (m̂·r̂) r̂ - m̂] / r³,
  m̂ the rotating moment), not the engine's header;
* at each sign change brentq solves g = 0 on the dense output, oracle_back_transform gives the
  Cartesian x and k, and τ = π ωp² / |k̂·∇ω_c| / (c ħ) with a central-difference Cartesian
  gradient (Richardson-extrapolated) and oracle.omega_p.

Rays: the first 64 forward-tree roots of the restated find_samples_new (seed 1769) per case,
classified by oracle.propagate(max_crossings = -1). A ray whose truth has more than one
cyclotron crossing, or whose DOP853 run fails, is dropped (at most 2 % per case; the npz
records how many).

Regenerate (well under a minute):  python tests/golden/make_cyclotron_fixture.py
"""
import ctypes as C
import math
import os
import sys
import time
from multiprocessing import Pool

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import oracle as O  # noqa: E402

RTOL, ATOL = 1e-13, 1e-15
INTERP_POINTS = 50
MAX_TRUTH_STEPS = 400_000
N_RAYS = 64
MAX_DROP = 0.02

# make_truth_fixture.py's cases
CASES = {
    "flat": dict(theta_m=0.2, mass_a=1e-5, flat=True),
    "gr": dict(theta_m=0.0, mass_a=1e-6, flat=False),
    "gr_oblique": dict(theta_m=0.2, mass_a=1e-5, flat=False),
    "scan": dict(theta_m=0.2, mass_a=5e-6, B0=5e13, omega_pul=2.0 * math.pi / 0.5, flat=True),
}

C_KM, HBAR = 2.99792e5, 6.582119e-16  # Constants.jl:3-5
KAPPA = 0.3 / 5.11e5 * (1.95e-20 * 1e18)  # eV per gauss (RayTracer.jl:794)


def omega_c(p, x, t):
    """ω_c [eV] at Cartesian x [km] and time t [s]: κ |B| of the rotating dipole."""
    x = np.asarray(x, np.float64)
    r = np.linalg.norm(x)
    m = np.array([math.sin(p.theta_m) * math.cos(p.omega_pul * t), math.sin(p.theta_m) * math.sin(p.omega_pul * t),
                  math.cos(p.theta_m)])
    rh = x / r
    B = 0.5 * abs(p.B0) * (p.rNS / r) ** 3 * (3.0 * np.dot(m, rh) * rh - m)
    return KAPPA * np.linalg.norm(B)


def grad_omega_c(p, x, t):
    """Cartesian gradient at fixed t: central differences at h and h/2, Richardson-extrapolated."""
    x = np.asarray(x, np.float64)
    g = np.zeros(3)
    h = 1e-3 * np.linalg.norm(x)
    for c in range(3):
        e = np.zeros(3)
        e[c] = 1.0
        d1 = (omega_c(p, x + h * e, t) - omega_c(p, x - h * e, t)) / (2 * h)
        d2 = (omega_c(p, x + 0.5 * h * e, t) - omega_c(p, x - 0.5 * h * e, t)) / h
        g[c] = (4.0 * d2 - d1) / 3.0
    return g


def tau_cyc(p, x, k, t):
    r = np.linalg.norm(x)
    wp = O.omega_p(p, r, math.acos(x[2] / r), math.atan2(x[1], x[0]), t, False, -1.0)
    dl = abs(np.dot(k, grad_omega_c(p, x, t))) / np.linalg.norm(k)
    return math.pi * wp * wp / dl / (C_KM * HBAR)


def _back_transform(p, u, erg):
    x, k = np.zeros(3), np.zeros(3)
    pd = C.POINTER(C.c_double)
    O.lib().oracle_back_transform(C.byref(p), np.ascontiguousarray(u).ctypes.data_as(pd), erg,
                                  x.ctypes.data_as(pd), k.ctypes.data_as(pd))
    return x, k


def truth_ray(args):
    """One forward segment to convergence with its cyclotron crossings.
    Returns dict(ok, count, tau, pos, ln_t)."""
    from scipy.integrate import DOP853
    from scipy.optimize import brentq
    kw, x0, k0, erg = args
    p = O.make_params(**kw)
    u0 = O.initial_state(p, x0, k0, erg, -1.0)
    tau0, tend = -30.0, p.ln_t_end
    rcut = 1.01 * p.rNS
    out = dict(ok=False, count=0, tau=0.0, pos=np.full(3, np.nan), ln_t=np.nan)

    def fun(t, y):
        return O.rhs(p, 1, y.copy(), t, erg)

    def cond(t, y):
        return O.condition(p, y, t)

    def g_of(t, y):  # spherical (r, θ, φ) -> Cartesian for the numpy dipole
        x = y[0] * np.array([math.sin(y[1]) * math.cos(y[2]), math.sin(y[1]) * math.sin(y[2]), math.cos(y[1])])
        return math.log(omega_c(p, x, math.exp(t))) - math.log(erg)

    def cyclotron(dense, ta, tb):  # the crossings of g = 0 in (ta, tb] of this step's dense output
        nonlocal g_prev
        ts = np.linspace(ta, tb, INTERP_POINTS)[1:]
        t_prev = ta
        for t in ts:
            g = g_of(t, dense(t))
            if g_prev != 0.0 and g != 0.0 and (g < 0.0) != (g_prev < 0.0):
                tr = brentq(lambda tt: g_of(tt, dense(tt)), t_prev, t, xtol=1e-15, rtol=1e-15)
                xc, kc = _back_transform(p, dense(tr), erg)
                out["tau"] += tau_cyc(p, xc, kc, math.exp(tr))
                if out["count"] == 0:
                    out["pos"], out["ln_t"] = xc, tr
                out["count"] += 1
            g_prev, t_prev = g, t

    if u0[0] < rcut:  # starts inside 1.01 rNS: cb_r ends it at once
        out["ok"] = True
        return out
    sol = DOP853(fun, tau0, u0, tend, rtol=RTOL, atol=ATOL)
    g_prev = g_of(tau0, u0)
    c_prev = cond(tau0, u0)
    s_prev = 0 if math.isnan(c_prev) else int(np.sign(c_prev))
    count = 0
    steps = 0
    while sol.status == "running" and steps < MAX_TRUTH_STEPS:
        sol.step()
        steps += 1
        if sol.status == "failed":
            out["ok"] = bool(sol.y[0] <= rcut + 1e-8)  # the step size collapsed on the cut at 1.01 rNS: the ray hit the star
            return out
        dense = sol.dense_output()
        ts = np.linspace(sol.t_old, sol.t, INTERP_POINTS)[1:]
        t_prev = sol.t_old
        for t in ts:  # the ray's end inside this step, as make_truth_fixture.truth_ray finds it
            y = dense(t)
            if y[0] <= rcut:
                tr = brentq(lambda tt: dense(tt)[0] - rcut, t_prev, t, xtol=1e-15, rtol=1e-15)
                cyclotron(dense, sol.t_old, tr)
                out["ok"] = True
                return out
            c = cond(t, y)
            if math.isnan(c):
                s_prev = 0
                t_prev = t
                continue
            s = int(np.sign(c))
            if s_prev != 0 and s != 0 and s != s_prev:
                tr = brentq(lambda tt: cond(tt, dense(tt)), t_prev, t, xtol=1e-15, rtol=1e-15)
                xc, _ = _back_transform(p, dense(tr), erg)
                skip = False
                if count == 0:
                    skip = bool(np.all(np.abs(xc) < np.abs(x0) * 1.0001) and np.all(np.abs(xc) > np.abs(x0) / 1.0001))
                if not skip and np.linalg.norm(xc) < rcut:
                    skip = True
                if not skip:
                    cyclotron(dense, sol.t_old, tr)
                    out["ok"] = True
                    return out
            if s != 0:
                s_prev = s
            t_prev = t
        cyclotron(dense, sol.t_old, sol.t)
    out["ok"] = sol.status == "finished"
    return out


def make(name, kw, n=N_RAYS, procs=8):
    p = O.make_params(**kw)
    maxr = O.find_conversion_surface(p)
    s = O.sample(p, maxr, 1769, 0, n, nthreads=procs)
    x0, k0 = s["x"].reshape(3, n), s["k_init"].reshape(3, n)
    status = O.propagate(p, s["x"], s["k_init"], s["erg"], -1.0, -30.0, 1, max_crossings=-1, nthreads=procs)["status"]
    t = time.time()
    with Pool(procs) as pool:
        res = pool.map(truth_ray, [(kw, x0[:, i].copy(), k0[:, i].copy(), float(s["erg"][i])) for i in range(n)],
                       chunksize=1)
    keep = np.array([r["ok"] and r["count"] <= 1 for r in res])
    dropped = int(n - keep.sum())
    assert dropped <= MAX_DROP * n, f"{name}: {dropped} of {n} rays dropped"
    kr = [r for r, kp in zip(res, keep) if kp]
    np.savez_compressed(
        os.path.join(HERE, "cyclotron", name + ".npz"), x0=x0[:, keep].reshape(-1), k0=k0[:, keep].reshape(-1),
        erg=s["erg"][keep], status=status[keep].astype(np.int32), count=np.array([r["count"] for r in kr], np.int32),
        tau=np.array([r["tau"] for r in kr]), pos=np.stack([r["pos"] for r in kr], axis=-1).reshape(-1),
        ln_t=np.array([r["ln_t"] for r in kr]), dropped=dropped, drawn=n, rtol=RTOL, atol=ATOL,
        **{"params_" + k: v for k, v in kw.items()})
    cnt = np.array([r["count"] for r in kr])
    tau = np.array([r["tau"] for r in kr])
    print(f"{name}: {n} rays in {time.time() - t:.0f} s; dropped {dropped}; oracle status counts "
          f"{np.bincount(status, minlength=3)} (success, crossing, hit NS); cyclotron counts {np.bincount(cnt)}; "
          f"tau {tau[cnt == 1].min() if (cnt == 1).any() else 0:.4g} .. {tau.max():.4g}", flush=True)


if __name__ == "__main__":
    O.build()
    os.makedirs(os.path.join(HERE, "cyclotron"), exist_ok=True)
    for nm in sys.argv[1:] or list(CASES):
        make(nm, CASES[nm])
