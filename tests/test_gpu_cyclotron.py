"""Cyclotron-resonance optical depth on the GPU (art_propagate_cyclotron_*, art_eval_cyclotron_device;
propagate_kernel<..., CYC = true> in csrc/art_propagate.h).

Truth errors. The engine's crossings of ω_c = ω against tests/golden/cyclotron/*.npz (DOP853 at rtol
1e-13, the root by brentq on its dense output; make_cyclotron_fixture.py), measured on an MI355X over
the four cases (maximum relative error over the rays with a crossing; |pos| is the radius of the first
crossing):

    settings, case                                      τ          |pos|      ln t
    reference (abstol 1e-6,  reltol 1e-7)   flat         7.40e-5    2.61e-6    3.37e-5
                                            gr           7.64e-3    2.22e-5    6.11e-5
                                            gr_oblique   2.22e-5    1.61e-6    3.40e-5
    tight     (abstol 1e-10, reltol 1e-11)  flat         1.74e-8    6.0e-10    6.68e-8
                                            gr           4.73e-7    1.37e-9    1.29e-7
                                            gr_oblique   5.38e-8    8.3e-10    7.32e-8

(scan: no crossing in the truth or in the engine, 63 rays; every count equals the truth's, both
settings.) The largest τ error is a gr ray whose momentum runs nearly along the surface of constant
ω_c, where τ ∝ 1/|k̂·∇ω_c| magnifies the ray's own position error at the reference tolerances.

The bounds (TRUTH_BOUND) are 4x the measured maxima at the reference tolerances: the margin covers
compiler-version FMA differences and the h⁴ error of the root on the step's cubic Hermite interpolant
(steps of ~0.3 in ln t out there). The count of crossings must equal the truth's on every ray."""
import numpy as np
import pytest

import launch_path
from conftest import CONFIGS
from test_cyclotron import CASES, POINT_SETS, load, random_points

pytestmark = pytest.mark.gpu

NUMERICS = {"reference": dict(abstol=1e-6, reltol=1e-7), "tight": dict(abstol=1e-10, reltol=1e-11)}  # truth_compare's
# 4 x the measured maxima (docstring): relative errors of τ, |pos| and ln t
TRUTH_BOUND = {"tau": 4 * 7.64e-3, "pos": 4 * 2.22e-5, "ln_t": 4 * 6.11e-5}


@pytest.mark.parametrize("theta_m,B0", POINT_SETS)
def test_pointwise_matches_host_header(oracle_lib, theta_m, B0):
    """The device's ω_c and τ against the host compile of the same header (tools/corecheck): 1e-13
    relative, which allows for FMA contraction."""
    import torch
    import adiabatic_raytracer_amd as A
    from adiabatic_raytracer_amd import Engine
    from tools import corecheck
    kw = dict(theta_m=theta_m, B0=B0, mass_a=1e-5, flat=True)
    po = oracle_lib.make_params(**kw)
    pos, k, t = random_points(po, 100, seed=7)
    eng = Engine(A.Params(**kw))
    dev = lambda a: torch.as_tensor(np.ascontiguousarray(a).reshape(-1), device=eng.device)  # noqa: E731
    wc, tau = eng.eval_cyclotron(dev(pos), dev(k), dev(t))
    wc, tau = wc.cpu().numpy(), tau.cpu().numpy()
    e_wc = np.abs(wc - corecheck.cyclotron_wc(po, pos, t)) / wc
    e_tau = np.abs(tau - corecheck.cyclotron_tau(po, pos, k, t)) / tau
    print(f"theta_m {theta_m} B0 {B0:g}: max rel err wc {e_wc.max():.3g}, tau {e_tau.max():.3g}")
    assert e_wc.max() <= 1e-13 and e_tau.max() <= 1e-13


def _device_run(eng, inp, lanes, cyclotron):
    import torch
    eng.set_tail_donation(lanes)
    try:
        out = eng.propagate(inp, max_crossings=-1, cyclotron=cyclotron)
        torch.cuda.synchronize()
    finally:
        eng.set_tail_donation(-1)
    return {k: v.cpu().numpy() for k, v in out.items() if hasattr(v, "cpu")}


@pytest.mark.parametrize("cfg", ["flat", "gr", "gr_oblique"])
@pytest.mark.parametrize("n", [2000, 70])
def test_observation_is_passive(cfg, n):
    """Every array of art_segment_out and of the crossing buffer equals art_propagate_device's on the
    same input, for photons and for a mixed-species batch, without tail donation and with 16 lanes;
    axion lanes report τ = 0 and no crossing."""
    import torch
    import adiabatic_raytracer_amd as A
    from adiabatic_raytracer_amd import Engine
    eng = Engine(A.Params(**CONFIGS[cfg]))
    inp = eng.forward_roots(n, seed=1769)
    mixed = dict(inp)
    mixed["species"] = (torch.arange(n, device=eng.device) % 3 != 0).to(torch.int8)  # every third ray an axion
    for what, batch in (("photons", inp), ("mixed", mixed)):
        axion = batch["species"].cpu().numpy() == 0
        for lanes in (0, 16):
            plain = _device_run(eng, batch, lanes, False)
            cyc = _device_run(eng, batch, lanes, True)
            for k, v in plain.items():
                assert np.array_equal(v, cyc[k], equal_nan=True), (cfg, n, what, lanes, k)
            assert np.all(cyc["cyc_tau"][axion] == 0.0) and np.all(cyc["cyc_count"][axion] == 0), (cfg, n, what, lanes)
            none = cyc["cyc_count"] == 0
            assert np.all(cyc["cyc_tau"][none] == 0.0) and np.all(cyc["cyc_tau"][~none] > 0.0)
            assert np.all(np.isnan(cyc["cyc_ln_t"][none])) and np.all(np.isfinite(cyc["cyc_ln_t"][~none]))


def truth_errors(case, mode):
    """(count mismatches, max relative errors of τ, |pos|, ln t over the rays with a truth crossing)"""
    import adiabatic_raytracer_amd as A
    z = load(case)
    n = z["n"]
    p = A.Params(**NUMERICS[mode], **z["params"])
    g = A.propagate_batch(p, z["x0"], z["k0"], z["erg"], -np.ones(n), np.full(n, -30.0), np.ones(n, np.int8),
                          max_crossings=-1, cyclotron=True)
    geom = "FLAT" if p.flat else "GR"
    launch_path.persistent(launch_path.last(), (case, mode), build_is=("vern6", geom, False, 0, 2, True), cont=False, tail=False)
    bad = int(np.sum(g["cyc_count"] != z["count"]))
    one = (z["count"] == 1) & (g["cyc_count"] == 1)
    none = g["cyc_count"] == 0
    assert np.all(np.isnan(g["cyc_ln_t"][none])) and np.all(np.isnan(g["cyc_pos"][:, none]))  # the host contract
    assert np.all(g["cyc_tau"][none] == 0.0)
    if not one.any():
        return bad, 0.0, 0.0, 0.0
    rg, rz = np.linalg.norm(g["cyc_pos"][:, one], axis=0), np.linalg.norm(z["pos"].reshape(3, n)[:, one], axis=0)
    return (bad, float(np.max(np.abs(g["cyc_tau"][one] - z["tau"][one]) / z["tau"][one])),
            float(np.max(np.abs(rg - rz) / rz)), float(np.max(np.abs((g["cyc_ln_t"][one] - z["ln_t"][one]) / z["ln_t"][one]))))


@pytest.mark.parametrize("case", CASES)
def test_engine_against_truth(case):
    ref = truth_errors(case, "reference")
    tight = truth_errors(case, "tight")
    print(f"{case}: reference count mismatches {ref[0]}, tau {ref[1]:.3g}, |pos| {ref[2]:.3g}, ln_t {ref[3]:.3g}; "
          f"tight count mismatches {tight[0]}, tau {tight[1]:.3g}, |pos| {tight[2]:.3g}, ln_t {tight[3]:.3g}")
    assert ref[0] == 0 and tight[0] == 0
    assert ref[1] <= TRUTH_BOUND["tau"] and ref[2] <= TRUTH_BOUND["pos"] and ref[3] <= TRUTH_BOUND["ln_t"]
    assert tight[1] <= ref[1] and tight[2] <= ref[2] and tight[3] <= ref[3]


def test_refill_independence():
    """200 000 flat photons are ~1.5x the persistent grid's lanes, so about a third of the lanes take a
    second ray: τ and count of the last 4096 rays equal, bit for bit, those of the same rays run as
    their own batch. A start-of-step g inherited from the lane's previous ray would show here."""
    import torch
    import adiabatic_raytracer_amd as A
    from adiabatic_raytracer_amd import Engine
    n, m = 200000, 4096
    p = A.Params(**CONFIGS["flat"])
    s = A.sample_conversion_points(p, n, seed=1769)
    eng = Engine(p)

    def run(sel):
        k = sel.stop - sel.start
        dev = lambda a: torch.as_tensor(np.ascontiguousarray(a.reshape(3, n)[:, sel]).reshape(-1), device=eng.device)  # noqa: E731
        inp = {"x0": dev(s["x"]), "k0": dev(s["k_init"]), "erg": torch.as_tensor(s["erg"][sel].copy(), device=eng.device),
               "dw": torch.full((k,), -1.0, dtype=torch.float64, device=eng.device),
               "ln_t0": torch.full((k,), -30.0, dtype=torch.float64, device=eng.device),
               "species": torch.ones(k, dtype=torch.int8, device=eng.device)}
        out = eng.propagate(inp, max_crossings=-1, cyclotron=True)
        torch.cuda.synchronize()
        return out["cyc_tau"].cpu().numpy(), out["cyc_count"].cpu().numpy()

    tau_all, cnt_all = run(slice(0, n))
    eng.kernel_ms()
    grid = A.raytracer.last_stats()["grid"]
    assert grid * 256 < n  # (some lane does take a second ray)
    tau_own, cnt_own = run(slice(n - m, n))
    assert (cnt_own == 1).sum() > 100
    assert np.array_equal(cnt_all[n - m:], cnt_own)
    assert np.array_equal(tau_all[n - m:], tau_own)


def test_tree_rows_with_optical_depth():
    """main_runner_tree(cyclotron=True) against the same call without it: only columns 8 (the weight,
    times exp(-τ)) and 14 (τ) change, and run_info's photon flux is the attenuated one."""
    import adiabatic_raytracer_amd as A
    p = A.Params(**CONFIGS["flat"])
    plain = A.trees.main_runner_tree(p, 65, saveMode=1)
    info = {}
    rows = A.trees.main_runner_tree(p, 65, saveMode=1, cyclotron=True, run_info=info)
    assert rows.shape == plain.shape and rows.shape[1] == 29
    other = [c for c in range(29) if c not in (8, 14)]
    assert np.array_equal(rows[:, other], plain[:, other], equal_nan=True)
    assert np.all(plain[:, 14] == 0.0) and np.all(plain[:, 15] == 1.0)
    axion = rows[:, 1] == 0.0
    assert np.all(rows[:, 14] >= 0.0) and np.all(rows[axion, 14] == 0.0) and (rows[~axion, 14] > 0.0).any()
    assert np.array_equal(rows[:, 8], plain[:, 8] * np.exp(-rows[:, 14]))
    want = float(np.sum(rows[~axion, 8] * rows[~axion, 7]))
    assert abs(info["flux"][1].sum() - want) <= 1e-12 * want
