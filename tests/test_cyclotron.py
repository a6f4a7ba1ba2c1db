"""Cyclotron-resonance optical depth (cyclotron_wc / cyclotron_tau in csrc/art_core.h,
art_propagate_cyclotron_*): the CPU side. The header's math through tools/corecheck against an
independent numpy formula, the C interface, and the truth fixtures' own consistency
(tests/golden/cyclotron/*.npz, made by tests/golden/make_cyclotron_fixture.py)."""
import ctypes as C
import importlib.util
import math
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
CASES = ("flat", "gr", "gr_oblique", "scan")


def generator():
    """tests/golden/make_cyclotron_fixture.py as a module: its numpy dipole (Cartesian, written
    without the engine's header), Richardson-extrapolated central-difference gradient and τ."""
    spec = importlib.util.spec_from_file_location("make_cyclotron_fixture",
                                                  os.path.join(GOLDEN, "make_cyclotron_fixture.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def load(case):
    z = np.load(os.path.join(GOLDEN, "cyclotron", case + ".npz"))
    d = {k: z[k] for k in z.files}
    d["params"] = {k[len("params_"):]: z[k].item() for k in z.files if k.startswith("params_")}
    d["n"] = int(d["erg"].size)
    return d


def random_points(p, n, seed):
    """n Cartesian points with r in [1e3, 1e5] km, random directions of x and k, t in [0, 1/ωPul]"""
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(3, n))
    pos = d / np.linalg.norm(d, axis=0) * np.exp(rng.uniform(math.log(1e3), math.log(1e5), n))
    k = rng.normal(size=(3, n))
    k *= 1e-5 / np.linalg.norm(k, axis=0)
    return pos, k, rng.uniform(0.0, 1.0 / p.omega_pul, n)


POINT_SETS = [(0.0, 1e14), (0.0, -1e14), (0.2, 1e14), (0.2, -1e14)]  # 4 x 100 points


@pytest.mark.parametrize("theta_m,B0", POINT_SETS)
def test_header_math_matches_independent_formula(oracle_lib, theta_m, B0):
    from tools import corecheck
    G = generator()
    p = oracle_lib.make_params(theta_m=theta_m, B0=B0, mass_a=1e-5, flat=True)
    pos, k, t = random_points(p, 100, seed=int(1000 * theta_m) + (1 if B0 > 0 else 2))
    wc = corecheck.cyclotron_wc(p, pos, t)
    tau = corecheck.cyclotron_tau(p, pos, k, t)
    wc_np = np.array([G.omega_c(p, pos[:, i], t[i]) for i in range(t.size)])
    tau_np = np.array([G.tau_cyc(p, pos[:, i], k[:, i], t[i]) for i in range(t.size)])
    e_wc = np.abs(wc - wc_np) / wc_np
    e_tau = np.abs(tau - tau_np) / tau_np
    print(f"theta_m {theta_m} B0 {B0:g}: max rel err wc {e_wc.max():.3g}, tau {e_tau.max():.3g}")
    assert np.all(wc > 0.0) and np.all(np.isfinite(tau)) and np.all(tau > 0.0)
    assert e_wc.max() <= 1e-13
    assert e_tau.max() <= 1e-7  # the finite difference's accuracy


def test_interface():
    """The header declares the three entry points, the binding's table has them, and the ctypes
    mirror of art_cyclotron_out has the header's layout (four pointers)."""
    txt = open(os.path.join(ROOT, "include", "art.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    fns = set(re.findall(r"\b(art_[a-z0-9_]+)\s*\(", txt))
    from adiabatic_raytracer_amd import _lib
    for name in ("art_propagate_cyclotron_host", "art_propagate_cyclotron_device", "art_eval_cyclotron_device"):
        assert name in fns, name
        assert name in _lib.SIGNATURES, name
    assert re.search(r"typedef struct art_cyclotron_out \{[^}]*tau;[^}]*count;[^}]*pos;[^}]*ln_t;[^}]*\} art_cyclotron_out;",
                     txt, flags=re.S)
    assert C.sizeof(_lib.CyclotronOut) == 32
    assert [f[0] for f in _lib.CyclotronOut._fields_] == ["tau", "count", "pos", "ln_t"]
    assert re.search(r"#define\s+ART_ABI_VERSION\s+1\b", txt)


def test_invalid_requests_fail_before_any_device_call():
    """RK4 and a NULL art_cyclotron_out are refused with ART_E_INVALID"""
    import adiabatic_raytracer_amd as A
    from adiabatic_raytracer_amd._lib import CrossingBuf, CyclotronOut, SegmentOut
    lib = A.load_library()
    n = 4
    bufs = [np.zeros(3 * n) for _ in range(2)] + [np.zeros(n) for _ in range(4)]
    i32 = [np.zeros(n, np.int32) for _ in range(4)]
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    so = SegmentOut(ptr(bufs[0]), ptr(bufs[1]), ptr(bufs[2]), ptr(bufs[3]), ptr(i32[0]), ptr(i32[1]), ptr(i32[2]))
    pos = np.zeros(3 * n)
    cy = CyclotronOut(ptr(bufs[4]), ptr(i32[3]), ptr(pos), ptr(bufs[5]))
    arrs = [np.ones(3 * n), np.ones(3 * n), np.ones(n), np.ones(n), np.ones(n), np.ones(n, np.int8)]
    inp = [ptr(a) for a in arrs]
    rk4 = A.Params(integrator="rk4").to_c()
    assert lib.art_propagate_cyclotron_host(C.byref(rk4), n, *inp, -1, C.byref(so), None, C.byref(cy)) == -1
    assert b"Vern6" in lib.art_last_error()
    v6 = A.Params().to_c()
    assert lib.art_propagate_cyclotron_host(C.byref(v6), n, *inp, -1, C.byref(so), None, None) == -1
    assert lib.art_propagate_cyclotron_device(C.byref(v6), n, *inp, -1, C.byref(so), None, None, None) == -1
    with pytest.raises(ValueError):
        A.propagate_batch(A.Params(), np.ones(3), np.ones(3), np.ones(1), np.ones(1), np.ones(1), np.ones(1, np.int8),
                          ntimes=3, cyclotron=True)


@pytest.mark.parametrize("case", CASES)
def test_fixture_self_check(case):
    z = load(case)
    n = z["n"]
    assert int(z["dropped"]) <= 0.02 * int(z["drawn"]) and n == int(z["drawn"]) - int(z["dropped"])
    assert z["x0"].size == 3 * n and z["pos"].size == 3 * n
    cnt, tau = z["count"], z["tau"]
    assert np.all((cnt == 0) | (cnt == 1))
    if case in ("flat", "gr_oblique"):
        assert np.all(cnt[z["status"] == 0] == 1)  # every escaping photon passes ω_c = ω once
    if case == "scan":
        assert np.all(cnt == 0)  # the resonance lies beyond c/ωPul: never reached before ln_t_end
    one = cnt == 1
    assert np.all(np.isfinite(tau[one]) & (tau[one] > 0.0)) and np.all(tau[~one] == 0.0)
    assert np.all(np.isfinite(z["ln_t"][one])) and np.all(np.isfinite(z["pos"].reshape(3, n)[:, one]))


def test_fixture_points_lie_on_the_resonance(oracle_lib):
    """At each stored crossing the header's ω_c equals the ray's erg and its τ the stored one."""
    from tools import corecheck
    for case in ("flat", "gr", "gr_oblique"):
        z = load(case)
        one = z["count"] == 1
        p = oracle_lib.make_params(**z["params"])
        pos, t = z["pos"].reshape(3, -1)[:, one], np.exp(z["ln_t"][one])
        wc = corecheck.cyclotron_wc(p, pos, t)
        assert np.abs(wc / z["erg"][one] - 1.0).max() <= 1e-12, case
