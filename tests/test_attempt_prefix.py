"""The integrator attempt by attempt, with `maxiters` as the probe (CPU side: the oracle against
tools/cpu_same.cpp, the scalar port of the kernel's loop; tests/test_gpu_attempt_prefix.py runs
the same constructions on the device and imports them from here).

A full run of an adaptive solver is chaotic: a last-bit difference changes the accept/reject
sequence, so full runs are compared statistically (tests/test_gpu_propagate.py). Capping the
attempts makes two deterministic comparisons possible:

* the prefix invariant. With T_i = n_accept + n_reject of ray i in an unlimited run, a run with
  maxiters = M leaves every ray with T_i <= M bit-equal to the unlimited run and ends every other
  ray with status 3 after exactly M attempts, its counts and recorded crossings a prefix of the
  unlimited run's. One implementation against itself: no tolerance;
* the deterministic window. Up to 16 attempts the integers of a run (status, n_accept, n_reject,
  n_cross) survive 1-ulp perturbations of the start positions for all but a few rays, so two
  implementations must agree in them exactly on those rays, and in the states to the envelope of
  the perturbed runs. From 8 attempts on the window holds rejections, at 16 terminal crossings:
  the controller's reject branch, the Hermite scan, the re-step polish and affect!.

This module keeps the constructions honest (every precondition is asserted on the oracle) and is
the first test of the two CPU copies of the termination code: the attempt cap, the forced dtmin
step, the fixed-step RK4 under a cap, and non-finite inputs (status 4 before any attempt)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))

from conftest import CONFIGS  # noqa: E402
from test_gpu_propagate import _crossings, _rel1, _rel_end, _within  # noqa: E402

SEED = 1769
N_PERTURB = 8  # independent 1-ulp perturbations of the oracle's start positions
INTS = ("status", "n_accept", "n_reject", "n_cross")
STATE = ("x_end", "k_end", "u7_end", "tau_end")
SLOTS = ("xc_pos", "xc_k", "xc_t", "xc_dw", "xc_p")
WINDOW = (1, 2, 3, 5, 8, 16)
PREFIX_CASES = ("flat", "gr", "gr_oblique", "flat_backtrace")
POISON_AT = (0, 63, 64, 130, 255, 300)  # over several waves, at wave edges
POISONS = ("nan_x0", "inf_x0", "nan_k0", "inf_k0", "nan_erg", "zero_x0")
NT = min(os.cpu_count() or 1, 16)

_CASES = {}


def case(oracle_lib, name, n):
    """The start points of a construction, computed once and left unchanged: forward-tree photons of a
    reference configuration, or the flat axion backtrace (-k, -B0, every crossing, 8 slots)."""
    if (name, n) not in _CASES:
        cfg = name.replace("_backtrace", "")
        po = oracle_lib.make_params(**CONFIGS[cfg])
        s = oracle_lib.sample(po, oracle_lib.find_conversion_surface(po), SEED, 0, n)
        c = dict(name=name, cfg=cfg, n=n, x=s["x"], erg=s["erg"])
        if name.endswith("_backtrace"):
            c.update(kw=dict(CONFIGS[cfg], B0=-1e14), k0=-s["k_init"], species=0, mc=100000, cap=8)
        else:
            c.update(kw=dict(CONFIGS[cfg]), k0=s["k_init"], species=1, mc=-1, cap=1)
        for v in c.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _CASES[(name, n)] = c
    return _CASES[(name, n)]


def oracle_run(oracle_lib, c, x=None, k0=None, erg=None, ln_t0=-30.0, **numerics):
    po = oracle_lib.make_params(**c["kw"], **numerics)
    return oracle_lib.propagate(po, c["x"] if x is None else x, c["k0"] if k0 is None else k0,
                                c["erg"] if erg is None else erg, -1.0, ln_t0, c["species"], max_crossings=c["mc"],
                                cap=c["cap"], nthreads=NT)


def cpu_same_run(oracle_lib, c, x=None, k0=None, erg=None, ln_t0=-30.0, **numerics):
    """tools/cpu_same.cpp on the same rays (Vern6; it records the first crossing only: 1 slot)."""
    import cpu_same
    po = oracle_lib.make_params(**c["kw"], **numerics)
    return cpu_same.propagate(po, c["x"] if x is None else x, c["k0"] if k0 is None else k0,
                              c["erg"] if erg is None else erg, ln_t0=ln_t0, species=c["species"], max_crossings=c["mc"],
                              nthreads=NT)


def perturbed_runs(oracle_lib, c, **numerics):
    out = []
    for k in range(N_PERTURB):
        ulp = np.random.default_rng(SEED + k).choice([-1.0, 1.0], c["x"].shape) * 2.2e-16
        out.append(oracle_run(oracle_lib, c, x=c["x"] * (1.0 + ulp), **numerics))
    return out


def same_ints(a, b):
    return np.all([a[k] == b[k] for k in INTS], axis=0)


def stable_rays(o, o2):
    """Rays whose four integers no perturbed run changes."""
    return np.all([same_ints(q, o) for q in o2], axis=0)


def attempts(r):
    return r["n_accept"].astype(np.int64) + r["n_reject"]


def m_values(T):
    """The caps of the prefix invariant: 1, the most frequent T (rays ending exactly at the cap),
    the 10th and 90th percentile of T, the longest ray's T and one more."""
    vals, cnt = np.unique(T, return_counts=True)
    return {"one": 1, "mode": int(vals[cnt.argmax()]), "p10": int(np.percentile(T, 10)),
            "p90": int(np.percentile(T, 90)), "max": int(T.max()), "max+1": int(T.max()) + 1}


def check_m_values(T, ms):
    """The preconditions of the prefix invariant's caps."""
    n = T.size
    assert np.sum(T == ms["mode"]) >= 2, ("no rays end exactly at the cap", ms)
    for key in ("p10", "p90"):
        done = np.sum(T <= ms[key])
        assert done >= 0.05 * n and n - done >= 0.05 * n, (key, ms[key], done, n)
    assert np.all(T <= ms["max"]) and np.sum(T > ms["one"]) > 0


def _slot_view(r, key, n, cap):
    a = np.asarray(r[key])
    return a.reshape(-1, cap, n)  # [component][slot][ray]


def check_prefix(full, cut, M, n, cap, what):
    """The prefix invariant of one implementation: `cut` ran with maxiters = M, `full` without a cap."""
    T = attempts(full)
    done = T <= M
    for k in INTS + STATE:
        m = full[k].size // n
        a, b = np.asarray(full[k]).reshape(m, n)[:, done], np.asarray(cut[k]).reshape(m, n)[:, done]
        assert np.array_equal(a, b, equal_nan=True), (what, M, k, "rays within the cap differ", int(done.sum()))
    late = ~done
    assert np.all(cut["status"][late] == 3), (what, M, np.bincount(cut["status"][late], minlength=5))
    assert np.all(attempts(cut)[late] == M), (what, M, attempts(cut)[late])
    for k in ("n_accept", "n_reject", "n_cross"):
        assert np.all(cut[k][late] <= full[k][late]), (what, M, k)
    # the recorded crossings: every slot of a finished ray, the cut rays' slots as the first of the full run's
    slots = np.arange(cap)[:, None] < np.minimum(cut["n_cross"], cap)[None, :]
    assert slots[:, done].sum() == np.minimum(full["n_cross"], cap)[done].sum()
    for k in SLOTS:
        a, b = _slot_view(full, k, n, cap), _slot_view(cut, k, n, cap)
        assert np.array_equal(a[:, slots], b[:, slots], equal_nan=True), (what, M, k, int(slots.sum()))
    return done


def check_window(got, o, o2, n, what, max_unstable, excepted, printer=print, states=True):
    """`got` against the oracle `o` inside the deterministic window: the four integers equal on the
    rays stable under the perturbed runs `o2` (all but `excepted` rays, which are printed), the end
    states and, with 20 terminal crossings and more, the first crossing within the project's
    2x/4x/6x of the perturbed runs' envelope (_within; `states` = False: the integers alone). Returns
    (unstable, excepted) ray counts."""
    st = stable_rays(o, o2)
    unstable = int(n - st.sum())
    assert unstable <= max_unstable * n, (what, "unstable rays", unstable, n)
    differ = st & ~same_ints(got, o)
    for i in np.flatnonzero(differ):
        printer(what, "ray", int(i), "got", [int(got[k][i]) for k in INTS], "oracle", [int(o[k][i]) for k in INTS])
    assert differ.sum() <= excepted, (what, "integers differ on stable rays", np.flatnonzero(differ))
    if not states:
        return unstable, int(differ.sum())

    def env(f):
        return np.max([f(q) for q in o2], axis=0)
    for key in ("x_end", "k_end"):
        _within(_rel_end(got, o, n, key)[st], env(lambda q: _rel_end(q, o, n, key))[st], f"{what} {key}")
    for key in ("u7_end", "tau_end"):
        _within(_rel1(got, o, key)[st], env(lambda q: _rel1(q, o, key))[st], f"{what} {key}")
    c = st & ~differ & (o["status"] == 1)
    if c.sum() >= 20:
        gx = _crossings(got, o, n, c)
        ox = [_crossings(q, o, n, c) for q in o2]
        for key in gx:
            _within(gx[key], np.max([x[key] for x in ox], axis=0), f"{what} {key}")
    return unstable, int(differ.sum())


def poisoned(c):
    """The six non-finite inputs, one at each ray of POISON_AT: (x0, k0, erg) copies."""
    n = c["n"]
    x, k, e = c["x"].copy(), c["k0"].copy(), c["erg"].copy()
    for i, kind in zip(POISON_AT, POISONS):
        if kind == "nan_x0":
            x[i] = np.nan
        elif kind == "inf_x0":
            x[n + i] = np.inf
        elif kind == "nan_k0":
            k[2 * n + i] = np.nan
        elif kind == "inf_k0":
            k[i] = -np.inf
        elif kind == "nan_erg":
            e[i] = np.nan
        else:
            x[[i, n + i, 2 * n + i]] = 0.0
    return x, k, e


def check_poisoned(clean, got, n, cap, what):
    """Poisoned rays: status 4 before any attempt; every other ray bit-equal to the clean batch's."""
    bad = np.zeros(n, bool)
    bad[list(POISON_AT)] = True
    assert np.all(got["status"][bad] == 4), (what, got["status"][bad])
    for k in ("n_accept", "n_reject", "n_cross"):
        assert np.all(got[k][bad] == 0), (what, k, got[k][bad])
    for k in INTS + STATE:
        m = clean[k].size // n
        a, b = np.asarray(clean[k]).reshape(m, n)[:, ~bad], np.asarray(got[k]).reshape(m, n)[:, ~bad]
        assert np.array_equal(a, b, equal_nan=True), (what, k, "a poisoned ray reached its neighbours")
    slots = (np.arange(cap)[:, None] < np.minimum(clean["n_cross"], cap)[None, :]) & ~bad[None, :]
    for k in SLOTS:
        assert np.array_equal(_slot_view(clean, k, n, cap)[:, slots], _slot_view(got, k, n, cap)[:, slots], equal_nan=True), (what, k)


# ---------------------------------------------------------------------------------------------

_FULL = {}


def _full(oracle_lib, name, n, impl):
    if (name, n, impl) not in _FULL:
        c = case(oracle_lib, name, n)
        _FULL[(name, n, impl)] = (oracle_run if impl == "oracle" else cpu_same_run)(oracle_lib, c)
    return _FULL[(name, n, impl)]


@pytest.mark.parametrize("impl", ["oracle", "cpu_same"])
@pytest.mark.parametrize("name", PREFIX_CASES)
def test_prefix_invariant(name, impl, oracle_lib):
    n = 256 if name == "flat_backtrace" else 512
    c = case(oracle_lib, name, n)
    run, cap = (oracle_run, c["cap"]) if impl == "oracle" else (cpu_same_run, 1)
    full = _full(oracle_lib, name, n, impl)
    T = attempts(full)
    ms = m_values(T)
    check_m_values(T, ms)
    assert np.all(full["status"] != 3) and np.all(full["status"] != 4)
    if name == "flat_backtrace":
        assert (full["n_cross"] > 1).any()  # (several crossings a ray: prefixes of more than one slot)
    for key, M in ms.items():
        done = check_prefix(full, run(oracle_lib, c, maxiters=M), M, n, cap, (name, impl, key))
        assert done.all() == (key in ("max", "max+1"))


@pytest.mark.parametrize("m", WINDOW)
@pytest.mark.parametrize("cfg", sorted(CONFIGS))
def test_window_cpu_same_equals_oracle(cfg, m, oracle_lib):
    n = 512
    c = case(oracle_lib, cfg, n)
    o = oracle_run(oracle_lib, c, maxiters=m)
    o2 = perturbed_runs(oracle_lib, c, maxiters=m)
    # what the window holds: rejections from 8 attempts on, terminal crossings at 16
    if m == 8 and cfg == "flat":
        assert np.sum(o["n_reject"] > 0) >= n // 2
    if m == 16:
        assert np.sum(o["status"] == 1) >= 15
    if m < 8:
        assert np.all(o["n_reject"] == 0)
    got = cpu_same_run(oracle_lib, c, maxiters=m)
    unstable, _ = check_window(got, o, o2, n, f"cpu_same {cfg} m={m}", 0.02, 0)
    print(cfg, m, "unstable rays", unstable)


@pytest.mark.parametrize("cfg", ["flat", "gr"])
def test_forced_dtmin_cpu_same_equals_oracle(cfg, oracle_lib):
    """dtmin = 0.05 exceeds the controller's step for many rays within 16 attempts: the step is
    forced to dtmin. (Every such step here has an error estimate below 1; a forced step accepted
    over its error is test_forced_step_is_accepted_over_its_error's.)"""
    n = 256
    c = case(oracle_lib, cfg, n)
    num = dict(maxiters=16, dtmin=0.05)
    o = oracle_run(oracle_lib, c, **num)
    plain = oracle_run(oracle_lib, c, maxiters=16)
    forced = (o["n_accept"] != plain["n_accept"]) | (o["n_reject"] != plain["n_reject"])
    assert forced.sum() >= 0.2 * n, ("the forced branch is not taken", int(forced.sum()))
    got = cpu_same_run(oracle_lib, c, **num)
    unstable, _ = check_window(got, o, perturbed_runs(oracle_lib, c, **num), n, f"cpu_same {cfg} dtmin", 0.04, 0)
    print(cfg, "forced rays", int(forced.sum()), "unstable rays", unstable)


def first_step_error(oracle_lib, c, h, rays, ln_t0=-30.0):
    """EEst of a Vern6 step of size h from the start state of the rays given, in numpy from the
    oracle's RHS and tableau (the error norm of OrdinaryDiffEq: the embedded difference over
    abstol + max(|u|, |u_new|) reltol, root mean square)."""
    cc, A, b, bh = oracle_lib.vern6_tableau()
    po = oracle_lib.make_params(**c["kw"])
    n, out = c["n"], []
    for i in rays:
        erg = c["erg"][i]
        u = oracle_lib.initial_state(po, c["x"][[i, n + i, 2 * n + i]], c["k0"][[i, n + i, 2 * n + i]], erg, -1.0)
        assert u[0] > po.rNS  # (no clamp of the stage radius, RayTracer.jl:531, at these starts)
        k = np.zeros((9, 7))
        y = u
        for s in range(9):
            y = u + h * (A[s, :s] @ k[:s])
            k[s] = oracle_lib.rhs(po, c["species"], y, ln_t0 + cc[s] * h, erg)
        e = h * ((b - bh) @ k)
        out.append(np.sqrt(np.mean((e / (po.abstol + np.maximum(np.abs(u), np.abs(y)) * po.reltol)) ** 2)))
    return np.array(out)


# Forced steps whose error estimate is above 1: at ln t0 = -8 (the reference starts at -30, where
# the dynamics per unit ln t is ~1e-9 of what it is here) the first step of dtmin = 0.05 is far
# beyond the tolerance. With ln t0 = -30, dtmin = 0.05 and 16 attempts every forced step has an
# estimate below 1: a controller that rejected forced steps like any other passes there.
FORCED_OVER_ERROR = dict(maxiters=16, dtmin=0.05, ln_t0=-8.0)


def check_forced_over_error(oracle_lib, c):
    """The precondition of FORCED_OVER_ERROR, on the rays cut after two attempts without an event:
    one attempt rejected, then a step of exactly dtmin from the start state accepted, whose error
    estimate (recomputed in numpy) is above 1."""
    num = dict(FORCED_OVER_ERROR, maxiters=2)
    first = oracle_run(oracle_lib, c, **num)
    rays = np.arange(0, c["n"], 4)
    taken = (first["status"][rays] == 3) & (first["n_accept"][rays] == 1) & (first["n_reject"][rays] == 1)
    taken &= first["tau_end"][rays] == num["ln_t0"] + num["dtmin"]
    over = first_step_error(oracle_lib, c, num["dtmin"], rays, ln_t0=num["ln_t0"]) > 1.0
    assert np.sum(taken & over) >= 0.2 * rays.size, (int(taken.sum()), int(over.sum()))


def test_forced_step_is_accepted_over_its_error(oracle_lib):
    n = 512
    c = case(oracle_lib, "flat", n)
    check_forced_over_error(oracle_lib, c)
    o = oracle_run(oracle_lib, c, **FORCED_OVER_ERROR)
    got = cpu_same_run(oracle_lib, c, **FORCED_OVER_ERROR)
    check_window(got, o, perturbed_runs(oracle_lib, c, **FORCED_OVER_ERROR), n, "cpu_same flat forced over error", 0.02, 0)


@pytest.mark.parametrize("m", [1, 10, 100])
@pytest.mark.parametrize("cfg", ["flat", "gr"])
def test_rk4_cap_on_the_oracle(cfg, m, oracle_lib):
    """Fixed-step RK4 (2000 steps a span) under a cap: no step is rejected, so every ray that does
    not hit the star ends with status 3 after exactly m accepted steps, whatever the perturbation
    (tools/cpu_same.cpp has no RK4)."""
    n = 512
    c = case(oracle_lib, cfg, n)
    num = dict(maxiters=m, integrator=oracle_lib.ART_RK4, n_fixed=2000)
    o = oracle_run(oracle_lib, c, **num)
    check_rk4(o, m)
    assert stable_rays(o, perturbed_runs(oracle_lib, c, **num)).all()


def check_rk4(r, m):
    away = r["status"] != 2
    assert away.sum() >= 0.9 * away.size
    assert np.all(r["status"][away] == 3) and np.all(r["n_accept"][away] == m) and np.all(r["n_reject"] == 0)


@pytest.mark.parametrize("impl", ["oracle", "cpu_same"])
@pytest.mark.parametrize("cfg", ["flat", "gr"])
def test_nonfinite_inputs(cfg, impl, oracle_lib):
    n = 512
    c = case(oracle_lib, cfg, n)
    run = oracle_run if impl == "oracle" else cpu_same_run
    x, k, e = poisoned(c)
    check_poisoned(_full(oracle_lib, cfg, n, impl), run(oracle_lib, c, x=x, k0=k, erg=e), n, 1, (cfg, impl))
