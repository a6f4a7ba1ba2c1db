"""TEST TOOL ONLY: builds and loads tools/build/libeventorigin.so, a host compile of the product's origin
binning (art_event_origin.h, tools/eventorigin.cpp), so CPU tests can hold origin_bin_of against
trees.origin_bins without a GPU. The product never loads this."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "eventorigin.cpp")
LIB = os.path.join(HERE, "build", "libeventorigin.so")
CSRC = os.path.join(HERE, "..", "adiabatic_raytracer_amd", "csrc")
DEPS = [SRC, os.path.join(HERE, "..", "include", "art.h")] + [
    os.path.join(CSRC, h) for h in ("art_event_origin.h", "art_event_rows.h", "art_ray_io.h", "art_internal.h", "art_core.h")]
_lib = None


def build():
    if os.path.exists(LIB) and all(os.path.getmtime(LIB) >= os.path.getmtime(d) for d in DEPS):
        return LIB
    os.makedirs(os.path.dirname(LIB), exist_ok=True)
    # (the product's contraction rule; the header itself switches contraction off where numpy rounds. The header's
    # includes hold device code, of which a host build wants none: --offload-host-only)
    subprocess.run(["/opt/rocm/bin/hipcc", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=on", "--offload-host-only",
                    SRC, "-o", LIB], check=True)
    return LIB


def lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(build())
        _lib.eo_bins.restype = None
    return _lib


def bins(x, y, z, spec):
    """origin_bin_of of the points (x, y, z) for a trees.origin_spec dict: the flat origin labels, int32"""
    xyz = np.ascontiguousarray(np.stack([np.asarray(v, np.float64) for v in (x, y, z)]))
    n = xyz.shape[1]
    out = np.full(n, -2, np.int32)
    lo, hi = spec["r_range"] or (0.0, 0.0)
    lib().eo_bins(C.c_int64(n), xyz.ctypes.data_as(C.c_void_p), C.c_int32(spec["n_r"]), C.c_int32(spec["n_theta"]),
                  C.c_int32(spec["n_phi"]), C.c_int32(1 if spec["theta_axis"] == "cos" else 0),
                  C.c_int32(1 if spec["r_range"] is None else 0), C.c_double(lo), C.c_double(hi), C.c_double(spec["cm"]),
                  C.c_double(spec["sm"]), out.ctypes.data_as(C.c_void_p))
    return out
