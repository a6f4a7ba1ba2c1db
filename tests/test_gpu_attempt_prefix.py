"""The integrator attempt by attempt on the device, with `maxiters` as the probe: the constructions
of tests/test_attempt_prefix.py (whose CPU tests assert their preconditions on the oracle) run on
every copy of the kernel.

(a) the prefix invariant, the persistent integrator against itself: no tolerance;
(b) the same outputs from the tail kernel (small batches, graduation, early graduation) and from
    the streamed host pipeline, bit for bit;
(c) up to 16 attempts the four integers of every ray that is stable under eight 1-ulp perturbations
    of the oracle equal the oracle's (2 rays of 512 excepted, below the 0.6% outlier allowance of
    _within), and the states stay within the project's 2x/4x/6x of the perturbed runs' envelope;
(d) the same with forced dtmin steps, (e) with the fixed-step RK4 under a cap;
(f) non-finite inputs end with status 4 before any attempt and do not reach their neighbours.

Batches of 512 rays and fewer run on the tail kernel by default (one wave per ray): the reference
runs of this module switch that off (ART_SMALL_TAIL=0) to reach the persistent integrator, and the
default path is one of the copies held to it."""
import numpy as np
import pytest

import launch_path
from conftest import CONFIGS
from test_attempt_prefix import (FORCED_OVER_ERROR, INTS, POISON_AT, PREFIX_CASES, SLOTS, STATE, WINDOW, attempts, case,
                                 check_m_values, check_poisoned, check_prefix, check_rk4, check_window, m_values,
                                 oracle_run, perturbed_runs, poisoned, same_ints)
from test_edges import host_flux
from test_gpu_scan_cert import KEYS

pytestmark = pytest.mark.gpu

assert set(KEYS) == set(INTS + STATE + SLOTS)
NBINS = 50
COUNTERS = ("attempts", "accepted", "root_steps", "scan_evals", "rays", "cert_steps")
# the copies of the kernel beside the persistent integrator: the environment and the donation lanes
# (None: a host call; a number: a device call on a non-blocking stream, as tests/test_gpu_tail_donation.py)
COPIES = {
    "small_tail": ({}, None),  # every ray on a wave of its own from the start
    "graduate": ({"ART_SMALL_TAIL": "0", "ART_GRADUATE": "1", "ART_TAIL": "100000"}, 16),
    "hot": ({"ART_SMALL_TAIL": "0", "ART_HOT_AT": "16", "ART_HOT_DTAU": "1e9"}, 16),
}


def _params(c, **numerics):
    import adiabatic_raytracer_amd as A
    if numerics.get("integrator") == 1:
        numerics["integrator"] = "rk4"
    return A.Params(**c["kw"], **numerics)


def _inputs(c, x=None, k0=None, erg=None, ln_t0=-30.0):
    n = c["n"]
    return (c["x"] if x is None else x, c["k0"] if k0 is None else k0, c["erg"] if erg is None else erg, -np.ones(n),
            np.full(n, ln_t0), np.full(n, c["species"], np.int8))


def _host(c, flux=False, x=None, k0=None, erg=None, ln_t0=-30.0, **numerics):
    import adiabatic_raytracer_amd as A
    return A.propagate_batch(_params(c, **numerics), *_inputs(c, x, k0, erg, ln_t0), max_crossings=c["mc"],
                             capacity=c["cap"], flux_nbins=NBINS if flux else None)


def _device(c, lanes, x=None, k0=None, erg=None, ln_t0=-30.0, **numerics):
    import torch
    import adiabatic_raytracer_amd as A
    from adiabatic_raytracer_amd import Engine
    eng = Engine(_params(c, **numerics))
    names = ("x0", "k0", "erg", "dw", "ln_t0", "species")
    inp = {k: torch.tensor(v, device=eng.device) for k, v in zip(names, _inputs(c, x, k0, erg, ln_t0))}
    eng.set_tail_donation(lanes)
    torch.cuda.synchronize()
    try:
        with torch.cuda.stream(torch.cuda.Stream()):
            out = eng.propagate(inp, max_crossings=c["mc"], capacity=c["cap"])
            eng.kernel_ms()
            stats = dict(A.raytracer.last_stats())
    finally:
        eng.set_tail_donation(-1)
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in out.items() if hasattr(v, "cpu")}
    got["stats"] = stats
    return got


def _is_the_copy(copy, c, capped):
    """The last launch ran the copy of the kernel that COPIES names (raytracer.last_launch_path); without a cap
    on the attempts, rays went the copy's way."""
    rec = launch_path.last()
    if copy == "small_tail":
        launch_path.small_tail(rec, copy, c["n"])
    elif copy == "graduate":
        launch_path.persistent(rec, copy, don=1, cont=True, tail=True, graduate=1)
        assert capped or rec["grad_count"] > 0, rec
    else:
        launch_path.persistent(rec, copy, don=1, cont=True, tail=True, hot=True, hot_at=16)
        assert capped or rec["hot_count"] > 0, rec
        assert rec["hot_claimed"] == min(rec["hot_count"], rec["hot_cap"]), rec


def _copy(copy, c, monkeypatch, **kw):
    env, lanes = COPIES[copy]
    with monkeypatch.context() as mp:
        mp.delenv("ART_SMALL_TAIL", raising=False)
        for k, v in env.items():
            mp.setenv(k, v)
        got = _host(c, **kw) if lanes is None else _device(c, lanes, **kw)
        _is_the_copy(copy, c, "maxiters" in kw)
        return got


def _bulk(c, monkeypatch, **kw):
    """The persistent integrator: this module's reference launch."""
    with monkeypatch.context() as mp:
        mp.setenv("ART_SMALL_TAIL", "0")
        got = _host(c, **kw)
        launch_path.persistent(launch_path.last(), "the reference launch")
        return got


def _same(ref, got, n, cap, what):
    """Every per-ray output and every recorded crossing slot bit-equal, and the launch counters."""
    for k in INTS + STATE:
        assert np.array_equal(ref[k], got[k], equal_nan=True), (what, k)
    slots = np.arange(cap)[:, None] < np.minimum(ref["n_cross"], cap)[None, :]
    for k in SLOTS:
        a, b = np.asarray(ref[k]).reshape(-1, cap, n), np.asarray(got[k]).reshape(-1, cap, n)
        assert np.array_equal(a[:, slots], b[:, slots], equal_nan=True), (what, k)
    for k in COUNTERS:
        assert ref["stats"][k] == got["stats"][k], (what, k, ref["stats"][k], got["stats"][k])


_RUNS = {}  # (case, n) -> {"full": unlimited launch, "ms": its caps, M: the launch with maxiters = M}


def _prefix_runs(oracle_lib, name, monkeypatch):
    """(a)'s launches of the persistent integrator, shared with (b): computed once, left unchanged."""
    n = 256 if name == "flat_backtrace" else 512
    c = case(oracle_lib, name, n)
    if (name, n) not in _RUNS:
        full = _bulk(c, monkeypatch, flux=True)
        ms = m_values(attempts(full))
        runs = {"full": full, "ms": ms}
        for M in sorted(set(ms.values())):
            runs[M] = _bulk(c, monkeypatch, flux=True, maxiters=M)
        _RUNS[(name, n)] = runs
    return c, _RUNS[(name, n)]


@pytest.mark.parametrize("name", PREFIX_CASES)
def test_prefix_invariant_on_the_device(name, oracle_lib, monkeypatch):
    c, runs = _prefix_runs(oracle_lib, name, monkeypatch)
    n, full, ms = c["n"], runs["full"], runs["ms"]
    T = attempts(full)
    check_m_values(T, ms)
    assert np.all(full["status"] <= 2)
    if name == "flat_backtrace":
        assert (full["n_cross"] > 1).any()
    species = np.full(n, c["species"], np.int8)
    with_cut_flux = 0
    for key, M in ms.items():
        cut = runs[M]
        done = check_prefix(full, cut, M, n, c["cap"], (name, key))
        assert done.all() == (key in ("max", "max+1"))
        assert cut["stats"]["attempts"] == int(np.minimum(T, M).sum()), (name, key)
        assert cut["stats"]["rays"] == n
        # the flux of a run that holds status-3 rays (they count as escaping where they stand beyond 1.1 rNS)
        assert np.array_equal(cut["flux"], host_flux(_params(c), cut, species, NBINS)), (name, key)
        with_cut_flux += bool((cut["status"] == 3).any())
    assert with_cut_flux >= 4
    assert full["stats"]["attempts"] == int(T.sum())


@pytest.mark.parametrize("copy", sorted(COPIES))
@pytest.mark.parametrize("name", PREFIX_CASES)
def test_prefix_runs_in_every_copy_of_the_kernel(name, copy, oracle_lib, monkeypatch):
    c, runs = _prefix_runs(oracle_lib, name, monkeypatch)
    _same(runs["full"], _copy(copy, c, monkeypatch), c["n"], c["cap"], (name, copy, "unlimited"))
    for M in sorted(set(runs["ms"].values())):
        _same(runs[M], _copy(copy, c, monkeypatch, maxiters=M), c["n"], c["cap"], (name, copy, M))


@pytest.mark.parametrize("cfg", ["flat", "gr"])
def test_prefix_runs_in_the_streamed_host_path(cfg, oracle_lib, monkeypatch):
    import adiabatic_raytracer_amd as A
    n = 2048
    c = case(oracle_lib, cfg, n)
    species = np.full(n, 1, np.int8)
    monkeypatch.setenv("ART_HOST_CHUNK_MIN", "500")
    monkeypatch.setenv("ART_HOST_MODE", "single")
    full = _host(c, flux=True)
    T = attempts(full)
    ms = m_values(T)
    check_m_values(T, ms)
    for M in [None] + sorted(set(ms.values())):
        num = {} if M is None else {"maxiters": M}
        monkeypatch.setenv("ART_HOST_MODE", "single")
        ref = full if M is None else _host(c, flux=True, **num)
        if M is not None:
            check_prefix(full, ref, M, n, 1, (cfg, "single", M))
        monkeypatch.setenv("ART_HOST_MODE", "stream")
        A.raytracer.host_path_counters(reset=True)
        got = _host(c, flux=True, **num)
        assert A.raytracer.host_path_counters() == {"calls": 1, "streamed": 1, "stream_giveups": 0, "chunked": 0,
                                                    "single": 0}
        _same(ref, got, n, 1, (cfg, "stream", M))
        assert np.array_equal(ref["flux"], got["flux"])
        assert np.array_equal(got["flux"], host_flux(_params(c), got, species, NBINS)), (cfg, M)


def _window(c, oracle_lib, monkeypatch, what, max_unstable, copies, states=True, **num):
    """(c)'s comparison of the persistent integrator with the oracle, and the copies held to it."""
    n = c["n"]
    o = oracle_run(oracle_lib, c, **num)
    o2 = perturbed_runs(oracle_lib, c, **num)
    g = _bulk(c, monkeypatch, **num)
    unstable, excepted = check_window(g, o, o2, n, what, max_unstable, 2, states=states)
    print(what, "unstable rays", unstable, "excepted rays", excepted)
    for copy in copies:
        _same(g, _copy(copy, c, monkeypatch, **num), n, c["cap"], (what, copy))
    return g, o


@pytest.mark.parametrize("m", WINDOW)
@pytest.mark.parametrize("cfg", sorted(CONFIGS))
def test_window_against_the_oracle(cfg, m, oracle_lib, monkeypatch):
    n = 512
    c = case(oracle_lib, cfg, n)
    g, o = _window(c, oracle_lib, monkeypatch, f"{cfg} m={m}", 0.02, ["small_tail"], maxiters=m)
    if m == 8 and cfg == "flat":
        assert np.sum(o["n_reject"] > 0) >= n // 2 and np.sum(g["n_reject"] > 0) >= n // 2
    if m == 16:
        assert np.sum(o["status"] == 1) >= 15 and np.sum(g["status"] == 1) >= 15


@pytest.mark.parametrize("cfg", ["flat", "gr"])
def test_forced_dtmin_against_the_oracle(cfg, oracle_lib, monkeypatch):
    n = 256
    c = case(oracle_lib, cfg, n)
    num = dict(maxiters=16, dtmin=0.05)
    g, o = _window(c, oracle_lib, monkeypatch, f"{cfg} dtmin", 0.04, ["small_tail", "graduate"], **num)
    plain = oracle_run(oracle_lib, c, maxiters=16)
    forced = (o["n_accept"] != plain["n_accept"]) | (o["n_reject"] != plain["n_reject"])
    assert forced.sum() >= 0.2 * n, ("the forced branch is not taken", int(forced.sum()))


def test_forced_step_is_accepted_over_its_error(oracle_lib, monkeypatch):
    """Forced steps with an error estimate above 1 (the precondition is asserted on the oracle by
    tests/test_attempt_prefix.py): accepted all the same, or no integer below would agree.

    The integers alone. The kernel seeds the re-step polish of a crossing with the secant point of
    its bracket where the oracle and cpu_same seed it with the interpolant's root (open_bracket,
    art_propagate.h). The polish ends at |condition| <= 1e-12 from either seed
    while steps hold the tolerance, which the window's state comparisons show; over a step far beyond
    it the 9 re-steps can run out first, and the event time then depends on the seed. Measured
    here: x_end within the envelope at the median (3.8e-13 against 4.3e-13) and off at the 99th
    percentile (3.5e-2 against 1.5e-4) with every integer equal; cpu_same with the kernel's seed
    reproduces the device's event times to the last digits. So the states of this construction
    compare two seeds, not two roundings, and are not held to the envelope."""
    c = case(oracle_lib, "flat", 512)
    _window(c, oracle_lib, monkeypatch, "flat forced over error", 0.02, ["small_tail", "graduate"], states=False,
            **FORCED_OVER_ERROR)


@pytest.mark.parametrize("m", [1, 10, 100])
@pytest.mark.parametrize("cfg", ["flat", "gr"])
def test_rk4_under_a_cap(cfg, m, oracle_lib, monkeypatch):
    c = case(oracle_lib, cfg, 512)
    g, o = _window(c, oracle_lib, monkeypatch, f"{cfg} rk4 m={m}", 0.0, [], maxiters=m, integrator=1, n_fixed=2000)
    check_rk4(o, m)
    check_rk4(g, m)


@pytest.mark.parametrize("cfg", ["flat", "gr"])
def test_nonfinite_inputs(cfg, oracle_lib, monkeypatch):
    n = 512
    c = case(oracle_lib, cfg, n)
    x, k, e = poisoned(c)
    species = np.full(n, 1, np.int8)
    clean = _bulk(c, monkeypatch, flux=True)
    got = _bulk(c, monkeypatch, flux=True, x=x, k0=k, erg=e)
    check_poisoned(clean, got, n, 1, (cfg, "persistent"))
    o = oracle_run(oracle_lib, c, x=x, k0=k, erg=e)
    bad = list(POISON_AT)
    assert same_ints(got, o)[bad].all(), ([got[key][bad] for key in INTS], [o[key][bad] for key in INTS])
    assert np.array_equal(got["flux"], host_flux(_params(c), got, species, NBINS))
    assert got["stats"]["attempts"] == clean["stats"]["attempts"] - int(attempts(clean)[bad].sum()) + len(bad)
    for copy in ("small_tail", "graduate"):
        check_poisoned(clean, _copy(copy, c, monkeypatch, x=x, k0=k, erg=e), n, 1, (cfg, copy))
