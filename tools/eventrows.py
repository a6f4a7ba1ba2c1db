"""TEST TOOL ONLY: builds and loads tools/build/libeventrows.so, a host compile of the product's row
math (art_event_rows.h, tools/eventrows.cpp), so CPU tests can hold the columns of main_runner_tree's
rows against numpy without a GPU. The product never loads this."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "eventrows.cpp")
LIB = os.path.join(HERE, "build", "libeventrows.so")
CSRC = os.path.join(HERE, "..", "adiabatic_raytracer_amd", "csrc")
DEPS = [SRC, os.path.join(CSRC, "art_event_rows.h"), os.path.join(CSRC, "art_core.h"),
        os.path.join(HERE, "..", "include", "art.h")]
_lib = None


def build():
    if os.path.exists(LIB) and all(os.path.getmtime(LIB) >= os.path.getmtime(d) for d in DEPS):
        return LIB
    os.makedirs(os.path.dirname(LIB), exist_ok=True)
    # (the product's contraction rule; the header itself switches contraction off where numpy rounds)
    subprocess.run(["/opt/rocm/bin/hipcc", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=on", SRC, "-o", LIB],
                   check=True)
    return LIB


def lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(build())
        _lib.er_rows.restype = C.c_int
        _lib.er_same.restype = None
    return _lib


def rows(nodes, ev, *, event_offset=0, mass_a=1e-5, tau=None, ncols=29):
    """The rows of the final nodes `nodes` (a trees.NODE_DTYPE record array) of the events ev
    (n_events, 14; eventrows.cpp). Returns (rows (n, ncols), kz / |k| (n,))."""
    nodes = np.ascontiguousarray(nodes)
    ev = np.ascontiguousarray(ev, np.float64)
    n = len(nodes)
    out, ct = np.full((n, ncols), np.nan), np.full(n, np.nan)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None  # noqa: E731
    tau = None if tau is None else np.ascontiguousarray(tau, np.float64)
    rc = lib().er_rows(C.c_int64(n), ptr(nodes), C.c_int64(len(ev)), ptr(ev), C.c_int64(event_offset), C.c_double(mass_a),
                       ptr(tau), C.c_int32(ncols), ptr(out), ptr(ct))
    if rc:
        raise RuntimeError(f"er_rows failed: {rc}")
    return out, ct


def same(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    out = np.zeros(a.size, np.int32)
    lib().er_same(C.c_int64(a.size), a.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p),
                  out.ctypes.data_as(C.c_void_p))
    return out.astype(bool)
