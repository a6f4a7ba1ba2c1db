"""Where the integrator keeps its wave-uniform arguments -- in registers across the stage slots, or re-read
from the kernel-argument segment inside the cold block that needs them (cold_args, art_ray_io.h), each hot
scalar in a register pair of its own (own_pair) -- must not change one bit of any output or launch counter.
tests/test_gpu_stage_glue.py pins the plain device launches; these are the instantiations and argument
values it does not reach, each pinned to what the build of a recorded parent commit gave
(tests/golden/scalar_args/<case>.npz, written by tests/golden/make_scalar_args_fixture.py on that build):

  streamed     the streamed host call (flat DON = 3: chunk flags, piece counts, the wave counters), forced the
               way tests/test_gpu_host_pieces.py forces it
  donate16     a donating launch and its packed continuation (flat DON = 1 at 2 waves/SIMD twice, 16 lanes,
               ART_TAIL=0)
  gr_graduate  a GR launch with graduation after 64 attempts (GR DON = 1 at 2 waves/SIMD, its continuation at 1,
               the graduation records, tail_kernel<GR> after them and, on this non-blocking stream, beside them
               for the hot records)
  cyclotron    the cyclotron build (flat CYC, DON = 0)
  no_callbacks max_crossings = ART_NO_CALLBACKS   } flat DON = 0 at 1 wave/SIMD, as every plain flat batch of at
  cap8         crossing capacity 8: axion backtraces that record every crossing   } most 65 536 rays
  mixed        every third segment an axion       }
(BUILDS below; each case asserts the build its launch reports, raytracer.last_launch_path.)

2,048 rays per case (the stage-glue fixtures' forward roots): 32 chunks over 8 blocks' worth of lanes, so
every wave refills and claims several chunks; one wave per block slot would exercise neither."""
import contextlib
import os
from dataclasses import replace

import numpy as np
import pytest

import launch_path
from conftest import CONFIGS
from test_gpu_stage_glue import N, load_inputs

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "scalar_args")
COUNTERS = ("attempts", "accepted", "root_steps", "scan_evals", "rays", "cert_steps")  # (per ray: no wave's make-up in them)

# case -> (configuration, environment of the call, what run_case does with it)
CASES = {
    "streamed": ("flat", {"ART_HOST_MODE": "stream", "ART_HOST_CHUNK_MIN": "500"}, dict(host=True)),
    "donate16": ("flat", {"ART_TAIL": "0"}, dict(lanes=16)),
    "gr_graduate": ("gr", {"ART_GRADUATE": "64"}, dict(lanes=16)),
    "cyclotron": ("flat", {}, dict(call=dict(cyclotron=True))),
    "no_callbacks": ("flat", {}, dict(call=dict(max_crossings=-(2 ** 31)))),
    "cap8": ("flat", {}, dict(backtrace=True, call=dict(max_crossings=100000, capacity=8))),
    "mixed": ("flat", {}, dict(mixed=True)),
}

# case -> the bulk integrator's build (integrator, geometry, saveat, DON, waves per SIMD, cyclotron) and what else the launch reports
BUILDS = {
    "streamed": (("vern6", "FLAT", False, 3, 2, False), dict(streamed=True, cont=False, tail=False)),
    "donate16": (("vern6", "FLAT", False, 1, 2, False), dict(donate=16, cont=True, cont_wps=2, tail=False, graduate=0)),
    "gr_graduate": (("vern6", "GR", False, 1, 2, False), dict(donate=16, cont=True, cont_wps=1, tail=True, tail_geom="GR",
                                                              graduate=64, hot=True, sorted=True)),
    "cyclotron": (("vern6", "FLAT", False, 0, 2, True), dict(cont=False, tail=False)),
    "no_callbacks": (("vern6", "FLAT", False, 0, 1, False), dict(cont=False, tail=False)),
    "cap8": (("vern6", "FLAT", False, 0, 1, False), dict(cont=False, tail=False)),
    "mixed": (("vern6", "FLAT", False, 0, 1, False), dict(cont=False, tail=False)),
}
PATHS = {}  # case -> the record of run_case's launch


@contextlib.contextmanager
def _env(env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def run_case(case):
    """Every output array of one case and its launch counters (as counter_<name>), from the stored inputs."""
    import torch
    import adiabatic_raytracer_amd as A
    from adiabatic_raytracer_amd import Engine
    from adiabatic_raytracer_amd.raytracer import ART_NO_CALLBACKS
    cfg, env, how = CASES[case]
    assert ART_NO_CALLBACKS == -(2 ** 31)
    inp = load_inputs(cfg)
    p = A.Params(**CONFIGS[cfg])
    k0, species = inp["k0"], np.ones(N, np.int8)
    if how.get("backtrace"):  # an axion traced back through the magnetosphere: B0 negated, k reversed
        p, k0, species = replace(p, B0=-p.B0), -inp["k0"], np.zeros(N, np.int8)
    if how.get("mixed"):
        species = (np.arange(N) % 3 != 0).astype(np.int8)
    call = how.get("call", dict(max_crossings=-1))
    with _env(env):
        if how.get("host"):
            A.raytracer.host_path_counters(reset=True)
            out = A.propagate_batch(p, inp["x0"], k0, inp["erg"], -np.ones(N), np.full(N, -30.0), species,
                                    max_crossings=-1, capacity=1, flux_nbins=50)
            assert A.raytracer.host_path_counters()["streamed"] == 1, A.raytracer.host_path_counters()
            res = {k: v for k, v in out.items() if isinstance(v, np.ndarray)}
            stats = dict(out["stats"])
        else:
            eng = Engine(p)
            dev = lambda a, dt=torch.float64: torch.as_tensor(a, dtype=dt, device=eng.device)  # noqa: E731
            din = {"x0": dev(inp["x0"]), "k0": dev(k0), "erg": dev(inp["erg"]), "dw": dev(-np.ones(N)),
                   "ln_t0": dev(np.full(N, -30.0)), "species": dev(species, torch.int8)}
            eng.set_tail_donation(how.get("lanes", 0))
            torch.cuda.synchronize()
            try:
                with torch.cuda.stream(torch.cuda.Stream()):  # (a non-blocking stream, as the donation tests use)
                    out = eng.propagate(din, **call)
                    eng.kernel_ms()
                    stats = dict(A.raytracer.last_stats())
            finally:
                eng.set_tail_donation(-1)
            torch.cuda.synchronize()
            res = {k: v.cpu().numpy() for k, v in out.items() if hasattr(v, "cpu")}
    for k in COUNTERS + (("init_rhs",) if how.get("host") else ()):
        res["counter_" + k] = np.array(stats[k], np.int64)
    PATHS[case] = launch_path.last()
    return res


@pytest.mark.parametrize("case", list(CASES))
def test_scalar_arguments_are_bit_exact(case):
    with np.load(os.path.join(GOLDEN, f"{case}.npz")) as z:
        ref = {k: z[k] for k in z.files}
    assert len(str(ref.pop("parent_sha"))) == 40
    got = run_case(case)
    path = launch_path.expect(PATHS[case], case, build_is=BUILDS[case][0], small_tail=False, **BUILDS[case][1])
    if case == "donate16":
        assert path["donated"] > 0, path
    if case == "gr_graduate":
        assert path["grad_count"] > 0 and path["donated"] > 0, path
    assert sorted(got) == sorted(ref), (case, sorted(got), sorted(ref))
    for k in sorted(ref):
        assert got[k].dtype == ref[k].dtype and got[k].shape == ref[k].shape, (case, k)
        assert np.array_equal(got[k], ref[k], equal_nan=True), (case, k, int(np.sum(got[k] != ref[k])))
    # the batch does what the docstring says of it
    assert ref["counter_rays"] == N and ref["n_accept"].min() > 0 and ref["n_reject"].max() > 0, case
    if case == "no_callbacks":
        assert ref["n_cross"].max() == 0 and ref["counter_scan_evals"] == 0
    else:
        assert ref["n_cross"].max() > 0, case
    if case == "cap8":
        assert ref["n_cross"].max() > 1 and ref["xc_t"].size == 8 * N
    if case == "cyclotron":
        assert ref["cyc_count"].max() > 0
