"""TEST TOOL ONLY: builds and loads tools/build/libeventspectrum.so, a host compile of the product's event power
spectrum functions (art_event_spectrum.h, tools/eventspectrum.cpp), so CPU tests can hold the bin rule, the merge of
the top lists and the per-tree X against numpy without a GPU. The product never loads this."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "eventspectrum.cpp")
LIB = os.path.join(HERE, "build", "libeventspectrum.so")
CSRC = os.path.join(HERE, "..", "adiabatic_raytracer_amd", "csrc")
DEPS = [SRC] + [os.path.join(CSRC, h) for h in ("art_event_spectrum.h", "art_event_moments.h", "art_event_replicates.h",
                                                "art_event_reweight.h", "art_core.h")] + [
    os.path.join(HERE, "..", "include", "art.h")]
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
        _lib.es_bins.restype = None
        _lib.es_merge.restype = None
        _lib.es_forest.restype = C.c_int64
    return _lib


_ptr = lambda v: v.ctypes.data_as(C.c_void_p)  # noqa: E731


def bins(x, m):
    """spectrum_bin of every x with m sub-octave bits"""
    x = np.ascontiguousarray(x, np.float64)
    out = np.zeros(len(x), np.int32)
    lib().es_bins(C.c_int64(len(x)), _ptr(x), C.c_int32(m), _ptr(out))
    return out


def merge(ap, ai, bp, bi, T):
    """spectrum_merge of two sorted lists (power, id) into the best T, padded with (0.0, -1)"""
    ap, bp = np.ascontiguousarray(ap, np.float64), np.ascontiguousarray(bp, np.float64)
    ai, bi = np.ascontiguousarray(ai, np.int64), np.ascontiguousarray(bi, np.int64)
    op, oi = np.zeros(T), np.zeros(T, np.int64)
    lib().es_merge(C.c_int32(len(ap)), _ptr(ap), _ptr(ai), C.c_int32(len(bp)), _ptr(bp), _ptr(bi), C.c_int32(T), _ptr(op),
                   _ptr(oi))
    return op, oi


def forest(start, species, power, check=True):
    """X (2, n_trees) of a forest (eventspectrum.cpp): start (n_trees + 1), per record species (-1 not final, 0 axion,
    1 photon) and power. Returns (X, the number of X that differ from moment_group's)."""
    start = np.ascontiguousarray(start, np.int64)
    species, power = np.ascontiguousarray(species, np.int32), np.ascontiguousarray(power, np.float64)
    n = len(start) - 1
    X = np.zeros((2, n))
    differ = lib().es_forest(C.c_int64(n), _ptr(start), _ptr(species), _ptr(power), _ptr(X), C.c_int32(1 if check else 0))
    return X, int(differ)
