"""Every build of the integrator and of the tail kernel, named by the launch that ran it.

One propagate launch picks among thirty propagate_kernel instantiations, two tail_kernels and four
hand-off mechanisms (art_launch_plan.h). raytracer.last_launch_path() reports what a launch picked and
how many rays each mechanism moved; this module is a table of launches (ROWS, SPECIAL) with the record
each must report, so no comparison below can hold because a policy silently stayed off:

  * the builds the table's rows ran are exactly the builds the plan can reach (tools/launchplancheck,
    the same sweep tests/test_launch_plan.py runs on the CPU);
  * Vern6 without saveat, in four geometries (flat, gr, gr_oblique, and a boundary layer for
    GEOM_ANY): every row is held to the oracle with test_gpu_propagate._compare (its 2x/4x/6x
    envelope of the oracle's own 1-ulp perturbations, unchanged), then bit for bit -- every output
    array and the six per-ray launch counters -- to the other rows of its geometry (one test for the rows
    that run propagate_kernel alone, one for the rows in which tail_kernel integrates rays). The share of
    rays _compare leaves out (status unstable under the oracle's own perturbations, or different on
    the GPU) is at most 5% in every row;
  * RK4, saveat (ntimes = 5) and the cyclotron observation are held to the oracle by
    test_gpu_propagate.test_rk4_fixed_step, test_gpu_saveat.py and test_gpu_cyclotron.py on their
    DON = 0 builds; here the DON = 1 build of each (16 lanes, and its continuation) equals the
    DON = 0 build bit for bit.

512 forward roots (seed 1769, as test_gpu_propagate._run) unless a row says otherwise; the oracle
runs once per geometry. Donating rows hand over 16 lanes, except in the boundary layer: half of its
rays stall there until maxiters, all to the same attempt, so no wave of its 512 rays ever falls to 16
live rays and a 16-lane row donated nothing (its DON = 1 build then ran as a DON = 0 one). Its rows
donate 63 lanes.

The general geometry has no tail kernel: tail_kernel<GEOM_ANY> did not reproduce propagate_kernel<GEOM_ANY>
bit for bit on this boundary layer (test_tail_kernel_rows_equal_the_persistent_ones), so the launch plan
keeps such a launch on the persistent integrator and its packed continuation. The boundary layer's rows
that ask for the small-batch path, second-level donation, graduation or the hot side launch assert that
the launch declined (ANY_ROWS) and are compared like the others."""
import contextlib
import os
import sys

import numpy as np
import pytest

from conftest import CONFIGS
from test_gpu_propagate import _compare, _run

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import launchplancheck  # noqa: E402

pytestmark = pytest.mark.gpu

N = 512
N_STREAM = 2048
SEED = 1769
INTS = ("status", "n_accept", "n_reject", "n_cross")
STATE = ("x_end", "k_end", "u7_end", "tau_end")
SLOTS = ("xc_pos", "xc_k", "xc_t", "xc_dw", "xc_p")
COUNTERS = ("attempts", "accepted", "root_steps", "scan_evals", "rays", "cert_steps")

# geometry -> (Params keywords, the configuration whose forward roots it starts from, the call's keywords, GEOM)
GEOMS = {
    "flat": (CONFIGS["flat"], CONFIGS["flat"], dict(max_crossings=-1, capacity=1), "FLAT"),
    "gr": (CONFIGS["gr"], CONFIGS["gr"], dict(max_crossings=-1, capacity=1), "GR"),
    "gr_oblique": (CONFIGS["gr_oblique"], CONFIGS["gr_oblique"], dict(max_crossings=-1, capacity=1), "GR"),
    # (the boundary layer of tests/test_gpu_stage_glue.py: half of its rays stall in the layer, hence maxiters)
    "layer": (dict(CONFIGS["flat"], bndry_lyr=3.0, maxiters=3000), CONFIGS["flat"], dict(max_crossings=4, capacity=4), "ANY"),
}
LANES = {"flat": 16, "gr": 16, "gr_oblique": 16, "layer": 63}  # a donating row's lanes (module docstring)

DONATING = "donating"
BULK = "ART_SMALL_TAIL"  # =0: past the small-batch tail path, to the persistent integrator


def _v6(geom, don, wps):
    return ("propagate", "vern6", geom, False, don, wps, False)


# row -> (environment, donation lanes (DONATING: the geometry's LANES), entry point, stream, rays, the record it must
# report given GEOM and the lanes)
# entry "host": propagate_batch (the library's own non-blocking stream); "device": Engine.propagate on
# torch's null stream ("null") or on a torch.cuda.Stream() ("side", a non-blocking one).
ROWS = {
    "tail": ({}, -1, "host", None, N, lambda G, L: dict(
        small_tail=True, bulk=False, cont=False, tail=True, tail_geom=G, tail_grid=N, hot=False, graduate=0,
        counts=lambda r: r["donated"] == N)),
    "w1_don0": ({BULK: "0"}, 0, "device", "null", N, lambda G, L: dict(
        small_tail=False, build=_v6(G, 0, 1), bulk_grid=2, cont=False, tail=False, hot=False, graduate=0,
        counts=lambda r: r["donated"] == 0 and r["grad_count"] == 0)),
    "w2_don0": ({BULK: "0", "ART_W1": "0"}, 0, "device", "null", N, lambda G, L: dict(
        small_tail=False, build=_v6(G, 0, 2), bulk_grid=2, cont=False, tail=False, hot=False, graduate=0,
        counts=lambda r: r["donated"] == 0 and r["grad_count"] == 0)),
    "don1_cont": ({BULK: "0", "ART_TAIL": "0"}, DONATING, "device", "null", N, lambda G, L: dict(
        small_tail=False, build=_v6(G, 1, 2), bulk_grid=2, donate=L, cont=True, cont_wps=1 if G == "GR" else 2,
        cont_donate=0, tail=False, hot=False, graduate=0,
        counts=lambda r: r["donated"] > 0 and r["donated2"] == 0 and r["grad_count"] == 0)),
    "don1_cont_tail": ({BULK: "0", "ART_TAIL": "100000"}, DONATING, "device", "null", N, lambda G, L: dict(
        small_tail=False, build=_v6(G, 1, 2), donate=L, cont=True, cont_wps=1 if G == "GR" else 2, cont_donate=4 if L == 16 else 63,
        tail=True, tail_geom=G, hot=False, graduate=2048,
        counts=lambda r: r["donated"] > 0 and r["donated2"] > 0 and r["grad_cap"] == N)),
    "graduate": ({BULK: "0", "ART_GRADUATE": "1"}, DONATING, "device", "null", N, lambda G, L: dict(
        small_tail=False, build=_v6(G, 1, 2), donate=L, cont=True, tail=True, tail_geom=G, hot=False, graduate=1,
        counts=lambda r: r["grad_count"] > 0 and r["grad_cap"] == N)),
    "hot": ({BULK: "0", "ART_HOT_AT": "16", "ART_HOT_DTAU": "1e9"}, DONATING, "device", "side", N, lambda G, L: dict(
        small_tail=False, build=_v6(G, 1, 2), donate=L, cont=True, tail=True, tail_geom=G, hot=True, sorted=True,
        graduate=2048, hot_at=16,
        counts=lambda r: r["hot_count"] > 0 and r["hot_cap"] == N and r["hot_claimed"] == min(r["hot_count"], r["hot_cap"]))),
    # (GR only: the continuation at 2 waves per SIMD)
    "cont_w2": ({BULK: "0", "ART_W1": "0"}, DONATING, "device", "null", N, lambda G, L: dict(
        small_tail=False, build=_v6(G, 1, 2), donate=L, cont=True, cont_wps=2, tail=True, hot=False,
        counts=lambda r: r["donated"] > 0)),
    "streamed": ({"ART_HOST_MODE": "stream", "ART_HOST_CHUNK_MIN": "500"}, -1, "host", None, N_STREAM, lambda G, L: dict(
        streamed=True, small_tail=False, build=_v6(G, 3, 2), cont=False, tail=False, hot=False, graduate=0,
        counts=lambda r: all(r[k] == 0 for k in _count_keys()))),
    # (the streamed row's batch as one launch: what its launch counters are compared with)
    "single_2048": ({"ART_HOST_MODE": "single"}, 0, "host", None, N_STREAM, lambda G, L: dict(streamed=False, small_tail=False)),
}


def _any_declines(L):
    """the general geometry, asked for the tail kernel's services with L donation lanes: the integrator and its packed
    continuation alone"""
    return dict(small_tail=False, build=_v6("ANY", 1 if L > 0 else 0, 2), bulk_grid=2, donate=max(L, 0), cont=L > 0,
                cont_wps=2 if L > 0 else 0, cont_donate=0, tail=False, hot=False, sorted=False, graduate=0, hot_at=0,
                counts=lambda r: (r["donated"] > 0) == (L > 0) and all(
                    r[k] == 0 for k in ("donated2", "grad_count", "grad_cap", "hot_count", "hot_cap", "hot_claimed")))


ANY_ROWS = ("tail", "don1_cont_tail", "graduate", "hot")  # the rows whose record in GEOM_ANY is _any_declines'
GEOM_ROWS = {g: [r for r in ROWS if not (r == "cont_w2" and GEOMS[g][3] != "GR") and not (r == "w1_don0" and GEOMS[g][3] == "ANY")]
             for g in GEOMS}


def _count_keys():
    from adiabatic_raytracer_amd._lib import LAUNCH_PATH_COUNTS
    return LAUNCH_PATH_COUNTS


@contextlib.contextmanager
def _env(env):
    keys = set(env) | {BULK, "ART_W1", "ART_TAIL", "ART_GRADUATE", "ART_HOT_AT", "ART_HOT_DTAU", "ART_HOST_MODE",
                       "ART_HOST_CHUNK_MIN", "ART_TAIL_DONATE"}
    old = {k: os.environ.get(k) for k in keys}
    for k in keys:
        os.environ.pop(k, None)
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _launch(kw, x0, k0, erg, env, lanes, entry, stream, call):
    """One launch: its outputs (host arrays), its launch counters and its launch-path record."""
    import torch
    import adiabatic_raytracer_amd as A
    from adiabatic_raytracer_amd import Engine
    n = erg.size
    p = A.Params(**kw)
    lib = A._lib.load()
    with _env(env):
        A._lib.check(lib.art_set_tail_donation(lanes))
        try:
            if entry == "host":
                out = A.propagate_batch(p, x0, k0, erg, -np.ones(n), np.full(n, -30.0), np.ones(n, np.int8), **call)
                res = {k: v for k, v in out.items() if isinstance(v, np.ndarray)}
                stats = dict(out["stats"])
            else:
                eng = Engine(p)
                dev = lambda a, dt=torch.float64: torch.as_tensor(a, dtype=dt, device=eng.device)  # noqa: E731
                din = {"x0": dev(x0), "k0": dev(k0), "erg": dev(erg), "dw": dev(-np.ones(n)), "ln_t0": dev(np.full(n, -30.0)),
                       "species": dev(np.ones(n, np.int8), torch.int8)}
                torch.cuda.synchronize()
                ctx = torch.cuda.stream(torch.cuda.Stream()) if stream == "side" else contextlib.nullcontext()
                with ctx:
                    out = eng.propagate(din, **{k: v for k, v in call.items() if k in ("max_crossings", "capacity", "cyclotron")})
                    eng.kernel_ms()
                    stats = dict(A.raytracer.last_stats())
                torch.cuda.synchronize()
                res = {k: v.cpu().numpy() for k, v in out.items() if hasattr(v, "cpu")}
            rec = A.raytracer.last_launch_path()
        finally:
            A._lib.check(lib.art_set_tail_donation(-1))
    return res, stats, rec


def _builds_of(rec):
    """the builds a record says its launch ran, as tools/launchplancheck names them"""
    b = set()
    bulk = launchplancheck.build_of_record(rec)
    if bulk:
        b.add(bulk)
    if rec["cont"]:
        b.add(("propagate", rec["integrator"], rec["geom"], rec["save"], 1, rec["cont_wps"], rec["cyc"]))
    if rec["tail"] or rec["hot"]:
        b.add(("tail", rec["tail_geom"]))
    return b


def _check_record(rec, want, what):
    want = dict(want)
    counts = want.pop("counts", None)
    build = want.pop("build", None)
    print(what, {k: rec[k] for k in rec if rec[k] not in (0, False)})
    if build is not None:
        assert rec["bulk"] and launchplancheck.build_of_record(rec) == build, (what, rec)
    for k, v in want.items():
        assert rec[k] == v, (what, k, rec[k], v, rec)
    assert rec["launches"] == 1, (what, rec)
    if counts is not None:
        assert counts(rec), (what, "counts", rec)


_GEOM = {}  # geometry -> {"oracle": (o, o2), "rows": {row: (outputs of the first N rays, counters, record)}}
_SEEN = set()  # the builds every record of this module reported


def _geometry(geom, oracle_lib):
    """The oracle's runs and every row's launch of one geometry: computed once, left unchanged."""
    if geom in _GEOM:
        return _GEOM[geom]
    kw, skw, call, G = GEOMS[geom]
    # the default environment's row is _run's own GPU launch; its oracle runs serve every row
    with _env({}):
        g, o, o2, s = _run(kw, N, max_crossings=call["max_crossings"], cap=call["capacity"], oracle_lib=oracle_lib, seed=SEED,
                           sample_kw=skw, with_sample=True)
        import adiabatic_raytracer_amd as A
        rec0 = A.raytracer.last_launch_path()
    po = oracle_lib.make_params(**skw)
    big = oracle_lib.sample(po, oracle_lib.find_conversion_surface(po), SEED, 0, N_STREAM)
    head = lambda a: np.asarray(a).reshape(-1, N_STREAM)[:, :N].reshape(-1)  # noqa: E731
    assert all(np.array_equal(head(big[k]), s[k]) for k in ("x", "k_init", "erg"))  # (the sampler is keyed by ray)
    rows = {}
    for row in GEOM_ROWS[geom]:
        env, lanes, entry, stream, n, want = ROWS[row]
        if lanes == DONATING:
            lanes = LANES[geom]
            env = dict(env, **({"ART_TAIL_DONATE": "63"} if lanes == 63 else {}))
        if row == "tail":
            res, stats, rec = {k: v for k, v in g.items() if isinstance(v, np.ndarray)}, dict(g["stats"]), rec0
        else:
            src = s if n == N else big
            res, stats, rec = _launch(kw, src["x"], src["k_init"], src["erg"], env, lanes, entry, stream, call)
        _check_record(rec, _any_declines(lanes) if (G == "ANY" and row in ANY_ROWS) else want(G, lanes), (geom, row))
        _SEEN.update(_builds_of(rec))
        cap = call["capacity"]
        first = {k: (np.asarray(res[k]).reshape(-1, n)[:, :N].reshape(-1)) for k in INTS + STATE + SLOTS}
        rows[row] = (first, stats, rec, cap)
    _GEOM[geom] = {"oracle": (o, o2), "rows": rows}
    return _GEOM[geom]


def _same(ref, got, cap, what):
    for k in INTS + STATE:
        assert np.array_equal(ref[k], got[k], equal_nan=True), (what, k, int(np.sum(ref[k] != got[k])))
    # (crossing slots without a crossing are never written)
    slots = np.arange(cap)[:, None] < np.minimum(ref["n_cross"], cap)[None, :]
    for k in SLOTS:
        a, b = ref[k].reshape(-1, cap, N), got[k].reshape(-1, cap, N)
        assert np.array_equal(a[:, slots], b[:, slots], equal_nan=True), (what, k)


REF_ROW = "w2_don0"
TAIL_ROWS = ("tail", "don1_cont_tail", "graduate", "hot", "cont_w2")  # rows in which tail_kernel integrates rays


@pytest.mark.parametrize("geom", list(GEOMS))
def test_vern6_rows_against_the_oracle(geom, oracle_lib):
    """Every row against the oracle (_compare's envelope), with at most 5% of the rays left out."""
    G = _geometry(geom, oracle_lib)
    o, o2 = G["oracle"]
    same2 = np.all([q["status"] == o["status"] for q in o2], axis=0)
    for row, (got, _, _, _) in G["rows"].items():
        left_out = 1.0 - np.mean((got["status"] == o["status"]) & same2)
        print(geom, row, "left out of the oracle comparison:", left_out, "(the oracle alone:", 1.0 - same2.mean(), ")")
        assert left_out <= 0.05, (geom, row, left_out)
        _compare(got, o, o2, N)


def _rows_equal(geom, G, names):
    ref, sref, _, cap = G["rows"][REF_ROW]
    for row in names:
        got, stats, _, _ = G["rows"][row]
        _same(ref, got, cap, (geom, row, "against", REF_ROW))
        if ROWS[row][4] == N:
            for k in COUNTERS:
                assert stats[k] == sref[k], (geom, row, k, stats[k], sref[k])


@pytest.mark.parametrize("geom", list(GEOMS))
def test_persistent_rows_are_bit_identical(geom, oracle_lib):
    """The rows that run propagate_kernel builds alone (DON = 0 at 1 and 2 waves/SIMD, DON = 1 with its packed
    continuation, the streamed DON = 3 build): every output array and the six launch counters."""
    G = _geometry(geom, oracle_lib)
    rows = G["rows"]
    _rows_equal(geom, G, [r for r in rows if r not in TAIL_ROWS])
    # the streamed call's counters: its own batch as one launch
    for k in COUNTERS:
        assert rows["streamed"][1][k] == rows["single_2048"][1][k], (geom, k)
    ref, sref = rows[REF_ROW][0], rows[REF_ROW][1]
    assert sref["rays"] == N and sref["attempts"] == int((ref["n_accept"] + ref["n_reject"]).sum())
    assert rows["streamed"][1]["rays"] == N_STREAM


@pytest.mark.parametrize("geom", list(GEOMS))
def test_tail_kernel_rows_equal_the_persistent_ones(geom, oracle_lib):
    """The rows in which tail_kernel integrates rays -- the small-batch path from the first attempt, second-level
    donation, graduation, early graduation -- against the persistent reference row, bit for bit.

    In the boundary layer (GEOM_ANY) this comparison failed while tail_kernel<GEOM_ANY> existed: measured on an
    MI355X, 512 rays, the small-batch launch against the 2-wave/SIMD DON = 0 one, 350 rays differed in n_accept
    (by -1263 ... +1260, median -2), 1 in status, 4 in n_cross, 1436 of 1536 x_end entries; 832183 against
    825905 attempts. Both kernels were deterministic and both held _compare's envelope of the oracle, so they
    differed by roundings that the layer's chaotic rays amplified. The launch plan now keeps the general geometry
    on propagate_kernel (no tail_kernel<GEOM_ANY> is built), so for the layer these rows are launches that
    declined the tail kernel, which their records assert, and the comparison holds."""
    G = _geometry(geom, oracle_lib)
    _rows_equal(geom, G, [r for r in G["rows"] if r in TAIL_ROWS])


# ---- RK4, saveat and the cyclotron observation: DON = 1 against DON = 0 ----

LAYER = GEOMS["layer"][0]
# case -> (Params keywords, roots, the call's keywords, the DON = 0 build)
SPECIAL = {
    "rk4_flat": (dict(CONFIGS["flat"], integrator="rk4"), CONFIGS["flat"], dict(max_crossings=-1, capacity=1),
                 ("propagate", "rk4", "FLAT", False, 0, 2, False)),
    "rk4_gr": (dict(CONFIGS["gr"], integrator="rk4"), CONFIGS["gr"], dict(max_crossings=-1, capacity=1),
               ("propagate", "rk4", "ANY", False, 0, 2, False)),
    "rk4_saveat": (dict(CONFIGS["flat"], integrator="rk4"), CONFIGS["flat"], dict(max_crossings=-1, capacity=1, ntimes=5),
                   ("propagate", "rk4", "ANY", True, 0, 2, False)),
    "saveat_flat": (CONFIGS["flat"], CONFIGS["flat"], dict(max_crossings=-1, capacity=1, ntimes=5),
                    ("propagate", "vern6", "FLAT", True, 0, 2, False)),
    "saveat_gr": (CONFIGS["gr"], CONFIGS["gr"], dict(max_crossings=-1, capacity=1, ntimes=5),
                  ("propagate", "vern6", "GR", True, 0, 2, False)),
    "saveat_layer": (LAYER, CONFIGS["flat"], dict(max_crossings=4, capacity=4, ntimes=5),
                     ("propagate", "vern6", "ANY", True, 0, 2, False)),
    "cyclotron_flat": (CONFIGS["flat"], CONFIGS["flat"], dict(max_crossings=-1, capacity=1, cyclotron=True),
                       ("propagate", "vern6", "FLAT", False, 0, 2, True)),
    "cyclotron_gr": (CONFIGS["gr"], CONFIGS["gr"], dict(max_crossings=-1, capacity=1, cyclotron=True),
                     ("propagate", "vern6", "GR", False, 0, 2, True)),
    "cyclotron_layer": (LAYER, CONFIGS["flat"], dict(max_crossings=4, capacity=4, cyclotron=True),
                        ("propagate", "vern6", "ANY", False, 0, 2, True)),
}


@pytest.mark.parametrize("case", list(SPECIAL))
def test_donating_build_equals_the_plain_one(case, oracle_lib):
    kw, skw, call, build = SPECIAL[case]
    po = oracle_lib.make_params(**skw)
    s = oracle_lib.sample(po, oracle_lib.find_conversion_surface(po), SEED, 0, N)
    runs = {}
    donating = 63 if kw is LAYER else 16  # (the boundary layer: module docstring)
    for lanes in (0, donating):
        res, stats, rec = _launch(kw, s["x"], s["k_init"], s["erg"], {}, lanes, "host", None, call)
        # no small-batch tail path, no tail kernel, graduation or hot side launch: the integrator and its continuation alone
        want = dict(small_tail=False, build=build[:4] + (1 if lanes else 0,) + build[5:], bulk_grid=2, donate=lanes,
                    cont=bool(lanes), cont_wps=2 if lanes else 0, cont_donate=0, tail=False, hot=False, sorted=False,
                    graduate=0, hot_at=0,
                    counts=(lambda r: r["donated"] > 0 and r["donated2"] == 0) if lanes else (lambda r: r["donated"] == 0))
        _check_record(rec, want, (case, lanes))
        _SEEN.update(_builds_of(rec))
        runs[lanes] = (res, stats)
    (ref, sref), (got, sgot) = runs[0], runs[donating]
    assert sorted(ref) == sorted(got)
    cap = call["capacity"]
    slots = np.arange(cap)[:, None] < np.minimum(ref["n_cross"], cap)[None, :]
    for k in sorted(ref):
        a, b = ref[k], got[k]
        if k in SLOTS:
            a, b = a.reshape(-1, cap, N)[:, slots], b.reshape(-1, cap, N)[:, slots]
        if k in ("traj", "traj_t"):  # only a ray's first traj_n saved points are written (include/art.h)
            saved = np.arange(call["ntimes"])[:, None] < ref["traj_n"][None, :]
            a, b = a[..., saved], b[..., saved]
        assert np.array_equal(a, b, equal_nan=True), (case, k)
    for k in COUNTERS:
        assert sref[k] == sgot[k], (case, k, sref[k], sgot[k])
    assert sref["rays"] == N and ref["n_accept"].min() > 0
    if "ntimes" in call:
        assert ref["traj_n"].max() == call["ntimes"]
    if "cyclotron" in call and kw is not LAYER:  # (no ray of the layer batch meets the cyclotron resonance)
        assert ref["cyc_count"].max() > 0


def test_the_rows_ran_every_build_the_plan_can_reach(oracle_lib):
    """(Last in the module: the rows above have run, or run here.) The builds the table's launches
    reported are the builds tools/launchplancheck's sweep of the plan reaches -- which
    tests/test_launch_plan.py holds equal to the instantiation lists -- no more and no fewer."""
    for geom in GEOMS:
        _geometry(geom, oracle_lib)
    if not any(b[1:] == ("rk4", "FLAT", False, 1, 2, False) for b in _SEEN):  # (this test alone was selected)
        for case in SPECIAL:
            test_donating_build_equals_the_plain_one(case, oracle_lib)
    ok, reached, unreached, text = launchplancheck.sweep()
    assert ok, text
    assert _SEEN == set(reached), (sorted(set(reached) - _SEEN), sorted(_SEEN - set(reached)))
