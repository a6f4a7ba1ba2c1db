"""TEST TOOL ONLY: builds and loads tools/build/libeventgrid.so, a host compile of the coupling x halo grid's
per-record and per-event functions (art_event_grid.h, tools/eventgrid.cpp), so CPU tests can hold them against
trees.grid_tables without a GPU. The product never loads this."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "eventgrid.cpp")
LIB = os.path.join(HERE, "build", "libeventgrid.so")
CSRC = os.path.join(HERE, "..", "adiabatic_raytracer_amd", "csrc")
DEPS = [SRC] + [os.path.join(CSRC, h) for h in ("art_event_grid.h", "art_event_reweight.h", "art_event_replicates.h",
                                                "art_event_moments.h", "art_core.h")] + \
       [os.path.join(HERE, "..", "include", "art.h")]
_lib = None


def build():
    if os.path.exists(LIB) and all(os.path.getmtime(LIB) >= os.path.getmtime(d) for d in DEPS):
        return LIB
    os.makedirs(os.path.dirname(LIB), exist_ok=True)
    subprocess.run(["/opt/rocm/bin/hipcc", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=on", SRC, "-o",
                    LIB + ".tmp"], check=True)
    os.replace(LIB + ".tmp", LIB)
    return LIB


def lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(build())
        _lib.eg_forest.restype = C.c_int
        _lib.eg_limits.restype = C.c_int
    return _lib


def limits():
    """(GRID_MAX_COUPLINGS, GRID_MAX_MODELS, GRID_TOT_COUNT, GRID_EVENTS_PER_WAVE) of the header"""
    return tuple(lib().eg_limits(C.c_int(q)) for q in range(4))


def forest(start, tree, fin, species, fb, tau, sln, a, W, B, R, nbins, n_groups=0, moments=True, event_offset=0,
           cyclotron=False, into=None):
    """The grid's tables of a forest (eventgrid.cpp): start (n_trees + 1); per record tree, fin, species, fb (the flux
    bin, -1 for none) and tau; per tree sln and a = attempts - 1; W (K_g, n_nodes), B (K_g, n_trees), R (K_h,
    n_trees). Returns a dict of CELL-MINOR tables as art_event_grid_out lays them out: flux (2 nbins, C), totals
    (3, C), with n_groups flux_rep (n_groups, 2 nbins, C), totals_rep (n_groups, 2, C) and groups (n_groups, 3), with
    moments moment_totals (8, C). into: such a dict, added to."""
    start, tree, a = (np.ascontiguousarray(v, np.int64) for v in (start, tree, a))
    fin, species, fb = (np.ascontiguousarray(v, np.int32) for v in (fin, species, fb))
    tau, sln, W, B, R = (np.ascontiguousarray(v, np.float64) for v in (tau, sln, W, B, R))
    Kg, Kh = B.shape[0], R.shape[0]
    Cn, G = Kg * Kh, int(n_groups)
    out = into or {"flux": np.zeros((2 * nbins, Cn)), "totals": np.zeros((3, Cn)),
                   "flux_rep": np.zeros((G, 2 * nbins, Cn)) if G else None, "totals_rep": np.zeros((G, 2, Cn)) if G else None,
                   "groups": np.zeros((G, 3)) if G else None, "moment_totals": np.zeros((8, Cn)) if moments else None}
    ptr = lambda v: None if v is None else v.ctypes.data_as(C.c_void_p)  # noqa: E731
    rc = lib().eg_forest(C.c_int64(len(start) - 1), C.c_int64(event_offset), ptr(start), ptr(tree), ptr(fin), ptr(species),
                         ptr(fb), ptr(tau), ptr(sln), ptr(a), C.c_int32(bool(cyclotron)), C.c_int32(Kg), C.c_int32(Kh),
                         C.c_int32(nbins), C.c_int32(G), ptr(W), ptr(B), ptr(R),
                         *[ptr(out[k]) for k in ("flux", "totals", "flux_rep", "totals_rep", "groups", "moment_totals")])
    if rc:
        raise RuntimeError(f"eg_forest failed: {rc}")
    return out
