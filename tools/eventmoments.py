"""TEST TOOL ONLY: builds and loads tools/build/libeventmoments.so, a host compile of the product's
per-tree group-by (art_event_moments.h, tools/eventmoments.cpp), so CPU tests can hold the second
moments against trees.event_moments without a GPU. The product never loads this."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "eventmoments.cpp")
LIB = os.path.join(HERE, "build", "libeventmoments.so")
CSRC = os.path.join(HERE, "..", "adiabatic_raytracer_amd", "csrc")
DEPS = [SRC, os.path.join(CSRC, "art_event_moments.h"), os.path.join(CSRC, "art_core.h"),
        os.path.join(HERE, "..", "include", "art.h")]
NONE, AXION, PHOTON = -1, -2, -3  # MomentEntry::flux of a record that is not final, of an unbinned axion, photon
_lib = None


def build():
    if os.path.exists(LIB) and all(os.path.getmtime(LIB) >= os.path.getmtime(d) for d in DEPS):
        return LIB
    os.makedirs(os.path.dirname(LIB), exist_ok=True)
    subprocess.run(["/opt/rocm/bin/hipcc", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=on", SRC, "-o", LIB],
                   check=True)
    return LIB


def lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(build())
        _lib.em_forest.restype = C.c_int
        _lib.em_entry_bytes.restype = C.c_int
    return _lib


def forest(start, flux, sky, power, a, nbins, sky_size):
    """The tables of a forest (eventmoments.cpp): start (n_trees + 1), per record flux (the encoded
    flux field), sky and power, per tree a = attempts - 1. Returns a dict: flux_sq, flux_xa (2 nbins),
    sky_sq, sky_xa (sky_size), totals (8)."""
    start, a = np.ascontiguousarray(start, np.int64), np.ascontiguousarray(a, np.int64)
    flux, sky = np.ascontiguousarray(flux, np.int32), np.ascontiguousarray(sky, np.int32)
    power = np.ascontiguousarray(power, np.float64)
    out = {"flux_sq": np.zeros(2 * nbins), "flux_xa": np.zeros(2 * nbins), "sky_sq": np.zeros(sky_size),
           "sky_xa": np.zeros(sky_size), "totals": np.zeros(8)}
    ptr = lambda v: v.ctypes.data_as(C.c_void_p)  # noqa: E731
    rc = lib().em_forest(C.c_int64(len(start) - 1), ptr(start), ptr(flux), ptr(sky), ptr(power), ptr(a), C.c_int32(nbins),
                         C.c_int64(sky_size), *[ptr(out[k]) for k in ("flux_sq", "flux_xa", "sky_sq", "sky_xa", "totals")])
    if rc:
        raise RuntimeError(f"em_forest failed: {rc}")
    return out
