"""The integrator's stage glue (the head of every stage slot: y = u + h (cf f + cA kA + Σ_q cL[q] L_q),
and the error norm's sum over the parked stages) may be rescheduled -- coefficient loads hoisted, LDS
reads batched -- but never re-associated: every component keeps cf*f (or fma(cf, f, cA*kA)), then
+= cL[q]*L_q for ascending q. So every output of the instantiations below is pinned bit for bit to what
the build of a recorded parent commit gave (tests/golden/stage_glue/<case>.npz, written by
tests/golden/make_stage_glue_fixture.py on that build from the inputs stored beside them).

2,048 rays per case take every slot row of both tables, the q = 1 start of Vern6's last row, both
RK4 masks, refills (32 chunks over 8 waves' worth of lanes) and crossings. The cases: flat Vern6,
GR, oblique GR, a boundary layer (GEOM_ANY; up to 4 crossings kept), RK4, and flat saved points
(ntimes = 5: the SAVE build, whose only entry is the host call propagate_batch).

The builds these launches run (BUILDS; each case asserts what its launch reports, raytracer.last_launch_path):
flat: the 1-wave/SIMD DON = 0 build (2,048 rays are below the 65,536 of one ray per lane); gr and gr_oblique:
GR DON = 1 at 2 waves/SIMD (16 lanes by default), its packed continuation at 1 wave/SIMD and tail_kernel<GR>;
layer: ANY DON = 0; rk4: flat RK4 DON = 0; saveat5: flat SAVE DON = 0. The other builds, the flat 2-wave/SIMD
DON = 0 one that the benchmark's device-resident launch runs among them, are held to the oracle and to these
by tests/test_gpu_launch_paths.py."""
import os

import numpy as np
import pytest

import launch_path
from conftest import CONFIGS

pytestmark = pytest.mark.gpu

N = 2048
SEED = 1769
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "stage_glue")

# case -> (Params keywords, the configuration whose forward roots it starts from, the call's keywords)
CASES = {
    "flat": (CONFIGS["flat"], "flat", dict(max_crossings=-1, capacity=1)),
    "gr": (CONFIGS["gr"], "gr", dict(max_crossings=-1, capacity=1)),
    "gr_oblique": (CONFIGS["gr_oblique"], "gr_oblique", dict(max_crossings=-1, capacity=1)),
    # (maxiters: half of these rays stall in the layer, and the default 100000 attempts each take seconds)
    "layer": (dict(CONFIGS["flat"], bndry_lyr=3.0, maxiters=3000), "flat", dict(max_crossings=4, capacity=4)),
    "rk4": (dict(CONFIGS["flat"], integrator="rk4"), "flat", dict(max_crossings=-1, capacity=1)),
    "saveat5": (CONFIGS["flat"], "flat", dict(max_crossings=-1, capacity=1, ntimes=5)),
}
INPUT_KEYS = ("x0", "k0", "erg")
# case -> the bulk integrator's build (integrator, geometry, saveat, DON, waves per SIMD, cyclotron) and what else the launch reports
_GR = (("vern6", "GR", False, 1, 2, False), dict(donate=16, cont=True, cont_wps=1, tail=True, tail_geom="GR", graduate=2048, hot=False))
BUILDS = {
    "flat": (("vern6", "FLAT", False, 0, 1, False), dict(cont=False, tail=False)),
    "gr": _GR,
    "gr_oblique": _GR,
    "layer": (("vern6", "ANY", False, 0, 2, False), dict(cont=False, tail=False)),
    "rk4": (("rk4", "FLAT", False, 0, 2, False), dict(cont=False, tail=False)),
    "saveat5": (("vern6", "FLAT", True, 0, 2, False), dict(cont=False, tail=False)),
}
PATHS = {}  # case -> the record of run_case's launch


def make_inputs(cfg):
    """The forward roots a case starts from, as host arrays (the fixture script stores them)."""
    import adiabatic_raytracer_amd as A
    from adiabatic_raytracer_amd import Engine
    inp = Engine(A.Params(**CONFIGS[cfg])).forward_roots(N, seed=SEED)
    return {k: inp[k].cpu().numpy() for k in INPUT_KEYS}


def load_inputs(cfg):
    with np.load(os.path.join(GOLDEN, f"in_{cfg}.npz")) as z:
        return {k: z[k] for k in INPUT_KEYS}


def run_case(case, inp):
    """Every output array of one case, from the stored inputs."""
    import torch
    import adiabatic_raytracer_amd as A
    from adiabatic_raytracer_amd import Engine
    kw, _, call = CASES[case]
    p = A.Params(**kw)
    if "ntimes" in call:
        out = A.propagate_batch(p, inp["x0"], inp["k0"], inp["erg"], -np.ones(N), np.full(N, -30.0),
                                np.ones(N, np.int8), **call)
        PATHS[case] = launch_path.last()
        return {k: v for k, v in out.items() if isinstance(v, np.ndarray)}
    eng = Engine(p)
    dev = lambda a, dt=torch.float64: torch.as_tensor(a, dtype=dt, device=eng.device)  # noqa: E731
    din = {"x0": dev(inp["x0"]), "k0": dev(inp["k0"]), "erg": dev(inp["erg"]), "dw": dev(-np.ones(N)),
           "ln_t0": dev(np.full(N, -30.0)), "species": dev(np.ones(N, np.int8), torch.int8)}
    out = eng.propagate(din, **call)
    eng.kernel_ms()  # (latches the launch's record)
    PATHS[case] = launch_path.last()
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items() if hasattr(v, "cpu")}


@pytest.mark.parametrize("case", list(CASES))
def test_stage_glue_is_bit_exact(case):
    with np.load(os.path.join(GOLDEN, f"{case}.npz")) as z:
        ref = {k: z[k] for k in z.files}
    assert len(str(ref.pop("parent_sha"))) == 40
    got = run_case(case, load_inputs(CASES[case][1]))
    path = launch_path.expect(PATHS[case], case, build_is=BUILDS[case][0], small_tail=False, streamed=False, **BUILDS[case][1])
    assert case not in ("gr", "gr_oblique") or path["donated"] > 0, path
    assert sorted(got) == sorted(ref), (case, sorted(got), sorted(ref))
    if "traj" in ref:  # only a ray's first traj_n saved points are written (include/art.h): the rest is not compared
        for d in (ref, got):
            unsaved = np.arange(d["traj_t"].shape[0])[:, None] >= d["traj_n"][None, :]
            d["traj"], d["traj_t"] = np.where(unsaved[None], 0.0, d["traj"]), np.where(unsaved, 0.0, d["traj_t"])
        assert ref["traj_n"].min() < ref["traj_t"].shape[0] and ref["traj_n"].max() == ref["traj_t"].shape[0]
    for k in sorted(ref):
        assert got[k].dtype == ref[k].dtype and got[k].shape == ref[k].shape, (case, k)
        assert np.array_equal(got[k], ref[k], equal_nan=True), (case, k, int(np.sum(got[k] != ref[k])))
    # the batch does what the docstring says of it: accepted and rejected attempts, crossings recorded
    assert ref["n_accept"].min() > 0 and ref["n_cross"].max() > 0, case
    if case != "rk4":
        assert ref["n_reject"].max() > 0, case
