"""Parity of the gfx950 segment integrator (RT.propagate, RayTracer.jl:171-452) with the
oracle on identical, seeded initial conditions (forward-tree roots from the restated
find_samples_new, seed 1769), for the reference's configurations and both integrators.

Tolerance, stated against the problem's own floating-point sensitivity. Both sides run the
same adaptive Vern6 + event algorithm and differ only by rounding (fused vs unfused
operations, analytic vs dual-number gradients). An adaptive solver at reltol 1e-7 turns a
last-bit difference into a different accept/reject sequence for some rays, after which
the trajectories differ at the solver's own error level. So every test also runs the
ORACLE three more times with its initial positions perturbed by one ulp (independent
draws), and requires the GPU-vs-oracle discrepancy to be no larger than the envelope (the
per-ray maximum) of those oracle-vs-oracle discrepancies:
  * segment status agreement >= min(0.99, perturbed agreement - 0.02);
  * final position and momentum, u7, ln t, the crossing's position, momentum, t, Δω and
    conversion probability: the 50th, 90th and 99th percentiles of the relative error are
    <= 2x, 4x and 6x the perturbed run's percentiles (+1e-12), and the fraction of rays off by
    more than 1e-3 exceeds the perturbed run's by at most 0.006 (chaotic rays, e.g. grazing a
    kink of |B_z|, exist in both). Round 3 measured at most 1.2x, 3.2x and 5.1x and 0.0047
    over every comparison (profiles/r03par_parity.jsonl); round 2 allowed 10x and 0.01;
  * the median accepted-step count differs by <= 1.
Measured (MI355X, 512 rays): median x_end error 5e-14 (flat) / 5e-11 (GR), p99 1-2e-5,
exactly the oracle's own 1-ulp sensitivity (p99 1.4-3e-5)."""
import json
import os

import numpy as np
import pytest

import launch_path
from conftest import CONFIGS

pytestmark = pytest.mark.gpu

N_PERTURB = 3  # independent 1-ulp perturbations of the oracle's start positions


def _run(kw, n, integrator="vern6", species=1, max_crossings=-1, cap=1, oracle_lib=None, seed=1769, sample_kw=None,
         with_sample=False, n_perturb=N_PERTURB):
    import adiabatic_raytracer_amd as A
    p = A.Params(integrator=integrator, **kw)
    po = oracle_lib.make_params(integrator=oracle_lib.ART_RK4 if integrator == "rk4" else 0, **kw)
    ps = po if sample_kw is None else oracle_lib.make_params(**sample_kw)
    s = oracle_lib.sample(ps, oracle_lib.find_conversion_surface(ps), seed, 0, n)
    k0 = s["k_init"] if species == 1 else -s["k_init"]  # backtrace: k -> -k (MainRunner.jl:581-585)
    sp = np.full(n, species, np.int8)
    g = A.propagate_batch(p, s["x"], k0, s["erg"], -np.ones(n), np.full(n, -30.0), sp,
                          max_crossings=max_crossings, capacity=cap)
    o = oracle_lib.propagate(po, s["x"], k0, s["erg"], -1.0, -30.0, sp, max_crossings=max_crossings, cap=cap)
    o2 = []
    for k in range(n_perturb):
        ulp = np.random.default_rng(seed + k).choice([-1.0, 1.0], s["x"].shape) * 2.2e-16
        o2.append(oracle_lib.propagate(po, s["x"] * (1.0 + ulp), k0, s["erg"], -1.0, -30.0, sp,
                                       max_crossings=max_crossings, cap=cap))
    return (g, o, o2, s) if with_sample else (g, o, o2)


def _rel_end(a, b, n, key="x_end"):
    xa, xb = a[key].reshape(3, n), b[key].reshape(3, n)
    return np.abs(xa - xb).max(0) / np.linalg.norm(xb, axis=0)


def _rel1(a, b, key):
    return np.abs(a[key] - b[key]) / np.maximum(np.abs(b[key]), 1e-300)


def _within(err, ref_err, what):
    qs = [50, 90, 99]
    e, r = np.percentile(err, qs), np.percentile(ref_err, qs)
    if os.environ.get("ART_PARITY_REPORT"):  # the measured margins, one JSON line per comparison
        with open(os.environ["ART_PARITY_REPORT"], "a") as fh:
            fh.write(json.dumps({"test": os.environ.get("PYTEST_CURRENT_TEST", "").split(" ")[0], "what": what,
                                 "gpu": e.tolist(), "oracle_1ulp": r.tolist(),
                                 "outliers": [float(np.mean(err > 1e-3)), float(np.mean(ref_err > 1e-3))]}) + "\n")
    # round 3 measured at most 1.2x / 3.2x / 5.1x the oracle's own 1-ulp envelope at the 50th /
    # 90th / 99th percentile over every comparison of this module and of test_gpu_saveat.py and
    # test_gpu_configs2_full.py (profiles/r03par_parity.jsonl); round 2 allowed 10x throughout
    assert np.all(e <= np.array([2.0, 4.0, 6.0]) * r + 1e-12), (what, "gpu", e, "oracle 1-ulp", r)
    # outliers (> 1e-3): chaotic rays exist in both; at most 0.6% of rays (3 of 512) more than the
    # oracle's own (measured: at most 0.47%; round 2 allowed 1%)
    bad, bad_ref = np.mean(err > 1e-3), np.mean(ref_err > 1e-3)
    assert bad <= bad_ref + 0.006, (what, bad, bad_ref, err.max())


def _crossings(a, b, n, mask):
    """Relative errors of the first recorded crossing of the rays in `mask`: position, momentum,
    tc = exp(τ), Δωc = u7/erg (affect!, RayTracer.jl:325-342) and P_nonAD."""
    def vec(key):
        pa, pb = a[key].reshape(3, -1)[:, :n][:, mask], b[key].reshape(3, -1)[:, :n][:, mask]
        return np.abs(pa - pb).max(0) / np.linalg.norm(pb, axis=0)

    def sc(key):
        x, y = a[key][:n][mask], b[key][:n][mask]
        with np.errstate(divide="ignore", invalid="ignore"):
            e = np.where(x == y, 0.0, np.abs(x - y) / np.abs(y))
        # P_nonAD is NaN where the reference's is undefined (e.g. v_loc of a crossing below
        # the axion shell): NaN on both sides agrees, NaN on one side only is a full miss
        # (capped at 1, so percentiles stay finite)
        return np.where(np.isnan(x) & np.isnan(y), 0.0, np.where(np.isnan(x) | np.isnan(y), 1.0, np.minimum(e, 1.0)))
    return {"crossing position": vec("xc_pos"), "crossing k": vec("xc_k"), "crossing t": sc("xc_t"),
            "crossing dw": sc("xc_dw"), "P_nonAD": sc("xc_p")}


def _compare(g, o, o2, n):
    """GPU run g against the oracle o, measured against the envelope (per-ray maximum) of the
    oracle's discrepancies under the N_PERTURB 1-ulp perturbations o2."""
    same = g["status"] == o["status"]
    same2 = np.all([q["status"] == o["status"] for q in o2], axis=0)
    agree2 = min(np.mean(q["status"] == o["status"]) for q in o2)
    assert same.mean() >= min(0.99, agree2 - 0.02), (
        np.bincount(g["status"], minlength=5), np.bincount(o["status"], minlength=5), agree2)
    both = same & same2

    def env(f):
        return np.max([f(q) for q in o2], axis=0)
    # every per-ray output of the 14-tuple (RayTracer.jl:448): final position and momentum,
    # u7 = erg Δω (feeds Δω, MainRunner.jl:709) and the final ln t
    for key in ("x_end", "k_end"):
        _within(_rel_end(g, o, n, key)[both], env(lambda q: _rel_end(q, o, n, key))[both], key)
    for key in ("u7_end", "tau_end"):
        _within(_rel1(g, o, key)[both], env(lambda q: _rel1(q, o, key))[both], key)
    c = both & (o["status"] == 1) & (g["n_cross"] == o["n_cross"])
    c &= np.all([q["n_cross"] == o["n_cross"] for q in o2], axis=0)
    if c.sum() >= 20:
        gx = _crossings(g, o, n, c)
        ox = [_crossings(q, o, n, c) for q in o2]
        for what in gx:
            _within(gx[what], np.max([x[what] for x in ox], axis=0), what)
    # accepted steps: within one of the oracle's, or (long chaotic segments, e.g. ~5e4 steps
    # with a boundary layer) no further off than the oracle's own 1-ulp runs
    d_g = np.median(np.abs(g["n_accept"][same] - o["n_accept"][same]))
    d_o = max(np.median(np.abs(q["n_accept"][same] - o["n_accept"][same])) for q in o2)
    assert d_g <= max(1.0, 3.0 * d_o), (d_g, d_o)


@pytest.mark.parametrize("cfg", sorted(CONFIGS))
def test_vern6_photon_forward_roots(cfg, oracle_lib):
    n = 512
    g, o, o2 = _run(CONFIGS[cfg], n, oracle_lib=oracle_lib)
    # Batches of at most one ray per SIMD (1024 on the MI355X) run on the tail kernel, so this module's Vern6
    # cases hold tail_kernel to the oracle; tests/test_gpu_launch_paths.py holds the persistent integrator's
    # builds to it. (The oracle's runs launch nothing: the record is still the GPU run's.)
    launch_path.small_tail(launch_path.last(), cfg, n)
    _compare(g, o, o2, n)


# BASELINE.json configs[4]: two grid points of the 32-point (m_a, B0, P) scan, neither at the
# headline's (m_a = 1e-5, B0 = 1e14, P = 2π)
@pytest.mark.parametrize("m_a,B0,period", [(1e-6, 2.5e13, 0.5), (1e-5, 2e14, 1.0)])
def test_vern6_scan_points(m_a, B0, period, oracle_lib):
    from adiabatic_raytracer_amd.scan import scan_grid
    kw = [g for g in scan_grid() if g["mass_a"] == m_a and g["B0"] == B0 and abs(g["omega_pul"] * period - 2 * np.pi) < 1e-12]
    assert len(kw) == 1
    n = 384
    g, o, o2 = _run(kw[0], n, oracle_lib=oracle_lib)
    _compare(g, o, o2, n)


# The non-default physics branches on the kernel (GEOM_ANY): the boundary layer of plasma
# (RayTracer.jl:1155-1162, --bndry_lyr) and the isotropic plasma (k∥ -> 0, :542-543, 1573-1575).
# Initial conditions are the default geometry's forward roots.
@pytest.mark.parametrize("cfg", ["flat", "gr"])
@pytest.mark.parametrize("branch", [dict(bndry_lyr=3.0), dict(isotropic=True)], ids=["bndry_lyr", "isotropic"])
def test_vern6_physics_branches(cfg, branch, oracle_lib):
    n = 256
    g, o, o2 = _run(dict(CONFIGS[cfg], **branch), n, oracle_lib=oracle_lib, sample_kw=CONFIGS[cfg])
    _compare(g, o, o2, n)


def test_rk4_fixed_step(oracle_lib):
    n = 256
    kw = dict(CONFIGS["flat"], n_fixed=3000)
    g, o, o2 = _run(kw, n, integrator="rk4", oracle_lib=oracle_lib)
    launch_path.persistent(launch_path.last(), "rk4", build_is=("rk4", "FLAT", False, 0, 2, False), cont=False, tail=False)
    _compare(g, o, o2, n)
    assert np.all(g["n_reject"] == 0)


def _within_entries(err, envs, what):
    """Per-entry form of _within for the crossing slots of all-crossings segments, where a few
    grazing rays are chaotic and a 3-draw percentile is too noisy a yardstick: `envs` are the
    errors of N independent 1-ulp perturbations of the oracle. The GPU's median and 90th
    percentile are <= 10x the envelope's (per-entry max over the draws, +1e-12); at least 97%
    of the entries are within 10x their own envelope + 1e-9 (an entry the oracle reproduces
    to the last bits under its own perturbations still carries the GPU's different rounding
    along thousands of steps and the root polish's own tolerance, |condition| <= 1e-12: with
    a 1e-12 floor 96.2% of the GR backtrace's slot positions passed, the worst at 2.4e-4 --
    a chaotic ray -- and the next at 2.5e-6); and entries off by more
    than 1e-3 are at most 2% more frequent than in the worst single draw."""
    env = np.max(envs, axis=0)
    e, r = np.percentile(err, [50, 90]), np.percentile(env, [50, 90])
    assert np.all(e <= 10.0 * r + 1e-12), (what, "gpu", e, "oracle 1-ulp envelope", r)
    ok = np.mean(err <= 10.0 * env + 1e-9)
    assert ok >= 0.97, (what, ok, np.sort(err)[-5:], np.sort(err / np.maximum(env, 1e-300))[-5:])
    bad, bad_ref = np.mean(err > 1e-3), max(np.mean(q > 1e-3) for q in envs)
    assert bad <= bad_ref + 0.02, (what, bad, bad_ref, err.max())


def _slots(a, n, cap, rays, slots):
    """Crossing slot j of ray i for the (ray, slot) pairs given: position and momentum (3, m)
    and t, Δω, P (m), from the [component][slot][ray] layout of the crossing buffer."""
    pos, k = a["xc_pos"].reshape(3, cap, n), a["xc_k"].reshape(3, cap, n)
    return {"xc_pos": pos[:, slots, rays], "xc_k": k[:, slots, rays],
            **{key: a[key].reshape(cap, n)[slots, rays] for key in ("xc_t", "xc_dw", "xc_p")}}


def _slot_errors(a, b):
    """Relative errors per (ray, slot) pair of every recorded crossing field; NaN on both sides
    agrees, NaN on one side is a full miss (as _crossings)."""
    out = {}
    for key in ("xc_pos", "xc_k"):
        out[key] = np.abs(a[key] - b[key]).max(0) / np.linalg.norm(b[key], axis=0)
    for key in ("xc_t", "xc_dw", "xc_p"):
        x, y = a[key], b[key]
        with np.errstate(divide="ignore", invalid="ignore"):
            e = np.where(x == y, 0.0, np.abs(x - y) / np.abs(y))
        out[key] = np.where(np.isnan(x) & np.isnan(y), 0.0, np.where(np.isnan(x) | np.isnan(y), 1.0, np.minimum(e, 1.0)))
    return out


def _grouped_p(xs, rays, counts, erg, prob):
    """get_Prob_nonAD of each backtrace's crossings as ONE call (MainRunner.jl:581-630 through
    get_tree :265): groups of Nc > 1 take the linear-index quirk of RayTracer.jl:1432-1443."""
    starts = np.concatenate([[0], np.cumsum(counts)])
    e = erg[rays] * np.abs(xs["xc_dw"])  # erg_inf_ini .* abs.(Δωc)
    return prob(xs["xc_pos"].T, xs["xc_k"].T, e, starts)


@pytest.mark.parametrize("cfg,flip_b0", [("gr", False), ("flat", True)], ids=["gr", "flat_minusB0"])
def test_axion_backtrace_all_crossings(cfg, flip_b0, oracle_lib):
    """Backtrace segments (axion, k -> -k, and -B0 as MainRunner.jl:581-591 passes it; every
    crossing recorded, splittings_cutoff = 100000). Beyond status, crossing count and end
    point, EVERY recorded slot j < min(n_cross, cap) -- position, momentum, t, Δω and the
    per-crossing P -- and the grouped P_nonAD of each backtrace (one get_Prob_nonAD call over
    all its crossings, the Nc > 1 quirk) are held to the oracle's 1-ulp envelope."""
    import adiabatic_raytracer_amd as A
    n, cap = 256, 8
    kw = dict(CONFIGS[cfg], B0=-1e14) if flip_b0 else CONFIGS[cfg]
    g, o, o2, s = _run(kw, n, species=0, max_crossings=100000, cap=cap, oracle_lib=oracle_lib,
                       sample_kw=CONFIGS[cfg] if flip_b0 else None, with_sample=True, n_perturb=6)
    same = g["status"] == o["status"]
    same2 = np.all([q["status"] == o["status"] for q in o2], axis=0)
    agree2 = min(np.mean(q["status"] == o["status"]) for q in o2)
    assert same.mean() >= min(0.99, agree2 - 0.03), (same.mean(), agree2)
    nc, nc2 = np.mean(g["n_cross"] == o["n_cross"]), min(np.mean(q["n_cross"] == o["n_cross"]) for q in o2)
    assert nc >= min(0.98, nc2 - 0.03), (nc, nc2)
    both = same & same2
    _within(_rel_end(g, o, n)[both], np.max([_rel_end(q, o, n) for q in o2], axis=0)[both], "x_end")
    assert np.all(g["status"] != 2)  # axions never stop at the star (cb_r is photon-only, :361-368)

    # every recorded slot of the rays whose crossing count agrees everywhere
    c = both & (g["n_cross"] == o["n_cross"]) & np.all([q["n_cross"] == o["n_cross"] for q in o2], axis=0)
    m = np.minimum(o["n_cross"], cap)
    rays = np.repeat(np.arange(n)[c], m[c])
    slots = np.concatenate([np.arange(k) for k in m[c]]) if c.any() else np.zeros(0, int)
    assert rays.size >= 40 and np.any(slots >= 1), (rays.size, np.bincount(m[c]))
    go, oo = _slots(g, n, cap, rays, slots), _slots(o, n, cap, rays, slots)
    qs = [_slots(q, n, cap, rays, slots) for q in o2]
    eg = _slot_errors(go, oo)
    eq = [_slot_errors(q, oo) for q in qs]
    later = slots >= 1  # the slots past the first, which no forward-tree test reaches
    for key in eg:
        _within_entries(eg[key], [e[key] for e in eq], f"slot {key}")
        _within_entries(eg[key][later], [e[key][later] for e in eq], f"slot>=1 {key}")

    # grouped P_nonAD of each complete backtrace (n_cross <= cap)
    full = c & (o["n_cross"] >= 1) & (o["n_cross"] <= cap)
    sel = np.isin(rays, np.arange(n)[full])
    cnt = m[full]
    erg = s["erg"]
    p = A.Params(**kw)
    po = oracle_lib.make_params(**kw)

    def gpu_prob(pos, kpos, e, gs):
        return A.get_Prob_nonAD(pos, kpos, p.mass_a, p.g_agg, p.theta_m, p.omega_pul, p.B0, p.rNS, e, 0.0, p.flat,
                                p.isotropic, p.bndry_lyr, group_start=gs)

    def ora_prob(pos, kpos, e, gs):
        return oracle_lib.get_prob_nonad(po, pos.T.reshape(-1), kpos.T.reshape(-1), e, group_start=gs)

    def sub(xs):
        return {k: (v[:, sel] if v.ndim == 2 else v[sel]) for k, v in xs.items()}
    pg = _grouped_p(sub(go), rays[sel], cnt, erg, gpu_prob)
    po_ = _grouped_p(sub(oo), rays[sel], cnt, erg, ora_prob)
    pq = [_grouped_p(sub(q), rays[sel], cnt, erg, ora_prob) for q in qs]
    # the GPU's grouped probability of the ORACLE's crossings equals the oracle's to rounding
    assert np.allclose(_grouped_p(sub(oo), rays[sel], cnt, erg, gpu_prob), po_, rtol=1e-9, atol=0, equal_nan=True)

    def rel(a, b):
        with np.errstate(divide="ignore", invalid="ignore"):
            e = np.where(a == b, 0.0, np.abs(a - b) / np.abs(b))
        return np.where(np.isnan(a) & np.isnan(b), 0.0, np.where(np.isnan(a) | np.isnan(b), 1.0, np.minimum(e, 1.0)))
    _within_entries(rel(pg, po_), [rel(q, po_) for q in pq], "grouped P_nonAD")


def test_golden_fixture_roundtrip(oracle_lib):
    """The committed golden fixture (tests/golden/segments_flat.npz, generated by the oracle
    with tests/golden/make_golden.py) is reproduced by the GPU."""
    import adiabatic_raytracer_amd as A
    path = os.path.join(os.path.dirname(__file__), "golden", "segments_flat.npz")
    z = np.load(path)
    n = z["erg"].size
    p = A.Params(**{k: z["params_" + k].item() for k in ("theta_m", "mass_a", "flat")})
    g = A.propagate_batch(p, z["x0"], z["k0"], z["erg"], z["dw"], z["ln_t0"], z["species"], max_crossings=-1)
    same = g["status"] == z["status"]
    if os.environ.get("ART_PARITY_REPORT"):
        rep = {"status_same": float(same.mean())}
        for key in ("x_end", "k_end"):
            rep[key] = np.percentile(_rel_end(g, z, n, key)[same], [50, 99]).tolist()
        for key in ("u7_end", "tau_end"):
            rep[key] = np.percentile(_rel1(g, z, key)[same], [50, 99]).tolist()
        cc = same & (z["status"] == 1) & (g["n_cross"] == z["n_cross"])
        rep.update({w: np.percentile(r_, [50, 99]).tolist() for w, r_ in _crossings(g, z, n, cc).items()})
        with open(os.environ["ART_PARITY_REPORT"], "a") as fh:
            fh.write(json.dumps({"test": "golden_fixture", **rep}) + "\n")
    assert same.mean() >= 0.995  # measured 1.0
    # the bulk is reproduced to rounding; the tail at the oracle's own 1-ulp sensitivity (module
    # doc). Measured (profiles/r03par2_parity.jsonl): medians <= 1e-12, 99th percentiles <= 1.9e-5
    # (k_end); the bounds are 1e-11 and 6e-5 (round 2: 1e-9 and 3e-4)
    for key in ("x_end", "k_end"):
        rel = _rel_end(g, z, n, key)[same]
        assert np.median(rel) <= 1e-11 and np.percentile(rel, 99) <= 6e-5, (key, np.percentile(rel, [50, 99]))
    for key in ("u7_end", "tau_end"):
        rel = _rel1(g, z, key)[same]
        assert np.median(rel) <= 1e-11 and np.percentile(rel, 99) <= 6e-5, (key, np.percentile(rel, [50, 99]))
    c = same & (z["status"] == 1) & (g["n_cross"] == z["n_cross"])
    assert c.sum() >= 20
    for what, rel in _crossings(g, z, n, c).items():
        assert np.median(rel) <= 1e-11 and np.percentile(rel, 99) <= 6e-5, (what, np.percentile(rel, [50, 99]))
    assert np.array_equal(g["n_cross"][same], z["n_cross"][same])


def test_invariants_full_size():
    """Size-independent properties at full size (1e6 rays, configs[1] geometry, θm = 0):
    with an aligned static dipole H does not depend on t or φ, so u7 (the energy) is
    conserved exactly and no step fails; every segment ends in a defined state."""
    import adiabatic_raytracer_amd as A
    from adiabatic_raytracer_amd import Engine
    import torch
    p = A.Params(theta_m=0.0, mass_a=1e-5, flat=True)
    eng = Engine(p)
    n = 1_000_000
    inp = eng.forward_roots(n, seed=1769)
    out = eng.propagate(inp)
    torch.cuda.synchronize()
    st = out["status"].cpu().numpy()
    assert np.all((st >= 0) & (st <= 2)), np.bincount(st)
    u7 = out["u7_end"].cpu().numpy()
    erg = inp["erg"].cpu().numpy()
    assert np.allclose(u7, -erg, rtol=1e-12, atol=0)  # du7 = ∂H/∂t ... = 0 for θm = 0
    tau = out["tau_end"].cpu().numpy()
    assert np.all(tau[st == 0] == p.to_c().ln_t_end)


def test_rt_propagate_mirror_make_tree(oracle_lib):
    """The host mirror raytracer.propagate called exactly as MainRunner.jl:179-182 calls
    RT.propagate (Mvars in the photon order, NumerP, func!, make_tree = true, splittings
    cutoff -1) returns the 14-tuple of the batched kernel; with make_tree = false (the
    reference's default) no callback is installed (RayTracer.jl:361-377): no crossing stops
    the segment, photons are not cut at 1.01 rNS, and the 4-tuple is returned. Both against
    the oracle run in the same mode."""
    import adiabatic_raytracer_amd as A
    from adiabatic_raytracer_amd.raytracer import ART_NO_CALLBACKS, func_photon
    kw = CONFIGS["flat"]
    po = oracle_lib.make_params(**kw)
    n = 128
    s = oracle_lib.sample(po, oracle_lib.find_conversion_surface(po), 1769, 0, n)
    x, k = s["x"].reshape(3, n).T, s["k_init"].reshape(3, n).T
    erg = s["erg"][0]
    p = A.Params(**kw)
    # MainRunner.jl:177-178 photon order: θm, ωPul, B0, rNS, gammaF, time0, Mass_NS, Mass_a, [erg], flat, isotropic,
    # melrose, bndry_lyr
    Mvars = [p.theta_m, p.omega_pul, p.B0, p.rNS, 1.0, 0.0, 1.0, p.mass_a, [erg], 1, 0, 1, -1.0]
    NumerP = [-30.0, float(np.log(1.0 / p.omega_pul)), 1e-6]
    t = A.raytracer.propagate(x, k, 3, Mvars, NumerP, func_photon, True, False, p.mass_a, -1, -1.0)
    assert len(t) == 18 and t.status.shape == (n,)
    o = oracle_lib.propagate(po, x, k, np.full(n, erg), -1.0, -30.0, 1, max_crossings=-1)
    assert np.mean(t.status == o["status"]) >= 0.97
    plain = A.raytracer.propagate(x, k, 3, Mvars, NumerP, func_photon, False, False, p.mass_a, -1, -1.0)
    assert len(plain) == 4 and plain.x.shape == (n, 3, 1)
    o2 = oracle_lib.propagate(po, x, k, np.full(n, erg), -1.0, -30.0, 1, max_crossings=ART_NO_CALLBACKS)
    assert np.all(o2["n_cross"] == 0) and np.all(o2["status"] != 1) and np.all(o2["status"] != 2)
    # without callbacks every photon escapes to ~3e5 km, where the end point carries the
    # solver's own ~1e-6 sensitivity: compared against the oracle's 1-ulp envelope
    xg = {"x_end": plain.x[:, :, 0].T.reshape(-1)}
    ref = []
    for sd in range(N_PERTURB):
        ulp = np.random.default_rng(1769 + sd).choice([-1.0, 1.0], x.shape) * 2.2e-16
        ref.append(_rel_end(oracle_lib.propagate(po, x * (1.0 + ulp), k, np.full(n, erg), -1.0, -30.0, 1,
                                                 max_crossings=ART_NO_CALLBACKS), o2, n))
    _within(_rel_end(xg, o2, n), np.max(ref, axis=0), "x_end (no callbacks)")
    # without callbacks every segment runs to ln t_end (none is terminated by a crossing)
    g = A.propagate_batch(p, s["x"], s["k_init"], np.full(n, erg), -np.ones(n), np.full(n, -30.0), np.ones(n, np.int8),
                          max_crossings=ART_NO_CALLBACKS)
    assert np.all(g["n_cross"] == 0) and np.all((g["status"] == 0) | (g["status"] >= 3))
    assert np.array_equal(g["x_end"], plain.x[:, :, 0].T.reshape(-1))
