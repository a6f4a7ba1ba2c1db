"""TEST TOOL ONLY: builds and loads tools/build/libtreestep.so, a host compile of the product's
per-tree step (art_tree_step.h) with its own driver loop over canned segment outcomes
(tools/treestep.cpp), so CPU tests can hold the device forest's bookkeeping against
oracle/tree.py without a GPU. The product never loads this."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "treestep.cpp")
LIB = os.path.join(HERE, "build", "libtreestep.so")
CSRC = os.path.join(HERE, "..", "adiabatic_raytracer_amd", "csrc")
DEPS = [SRC, os.path.join(CSRC, "art_tree_step.h"), os.path.join(CSRC, "art_core.h"),
        os.path.join(HERE, "..", "include", "art.h")]
_lib = None


def build():
    if os.path.exists(LIB) and all(os.path.getmtime(LIB) >= os.path.getmtime(d) for d in DEPS):
        return LIB
    os.makedirs(os.path.dirname(LIB), exist_ok=True)
    # (the product's contraction rule: a multiply and an add fuse inside one expression only)
    subprocess.run(["/opt/rocm/bin/hipcc", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=on", SRC, "-o", LIB],
                   check=True)
    return LIB


def lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(build())
        _lib.ts_stack_capacity.restype = C.c_int64
        _lib.ts_stack_capacity.argtypes = [C.c_int32, C.c_int32, C.c_int32]
        _lib.ts_run.restype = C.c_int
    return _lib


def stack_capacity(mc_nodes, max_nodes, split_all=False):
    return int(lib().ts_stack_capacity(int(mc_nodes), int(max_nodes), int(bool(split_all))))


def run(opts, node_dtype, root_pn, ncross, xc, r_end, rNS=10.0, stack_cap=0):
    """Grow len(root_pn) trees from the tables (treestep.cpp: ncross (n, steps), xc (n, steps, xcap, 9),
    r_end (n, steps)). opts: the binding's TreeOpts. Returns (nodes, counts, infos, max_depth, overflow)."""
    root_pn = np.ascontiguousarray(root_pn, np.float64)
    ncross = np.ascontiguousarray(ncross, np.int32)
    xc = np.ascontiguousarray(xc, np.float64)
    r_end = np.ascontiguousarray(r_end, np.float64)
    n, steps = ncross.shape
    xcap = xc.shape[2]
    assert xc.shape == (n, steps, xcap, 9) and r_end.shape == (n, steps) and root_pn.shape == (n,)
    cap = n * steps
    nodes = np.zeros(cap, node_dtype)
    counts, infos = np.zeros(n, np.int32), np.zeros(n, np.int32)
    nn, depth, over = C.c_int64(0), C.c_int32(0), C.c_int32(0)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    rc = lib().ts_run(C.c_int64(n), C.byref(opts), C.c_double(rNS), C.c_int32(stack_cap), C.c_int32(steps),
                      C.c_int32(xcap), ptr(root_pn), ptr(ncross), ptr(xc), ptr(r_end), C.c_int64(cap), ptr(nodes),
                      C.byref(nn), ptr(counts), ptr(infos), C.byref(depth), C.byref(over))
    if rc:
        raise RuntimeError(f"ts_run failed: {rc}")
    return nodes[:nn.value], counts, infos, depth.value, over.value
