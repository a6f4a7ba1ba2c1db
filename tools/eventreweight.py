"""TEST TOOL ONLY: builds and loads tools/build/libeventreweight.so, a host compile of the product's
coupling-scan reweight (art_event_reweight.h, tools/eventreweight.cpp) with each crossing's exponent
taken from a table, so CPU tests can hold it against trees.reweight_nodes without a GPU. The product
never loads this."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "eventreweight.cpp")
LIB = os.path.join(HERE, "build", "libeventreweight.so")
CSRC = os.path.join(HERE, "..", "adiabatic_raytracer_amd", "csrc")
DEPS = [SRC, os.path.join(CSRC, "art_event_reweight.h"), os.path.join(CSRC, "art_event_moments.h"),
        os.path.join(CSRC, "art_core.h"), os.path.join(HERE, "..", "include", "art.h")]
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
        _lib.rw_forest.restype = C.c_int
        _lib.rw_tables.restype = C.c_int
        _lib.rw_node_bytes.restype = C.c_int
        _lib.rw_back.restype = None
        _lib.rw_power.restype = C.c_double
        _lib.rw_power.argtypes = [C.c_double, C.c_double, C.c_int32, C.c_double, C.c_double]
    return _lib


def _ptr(v):
    return v.ctypes.data_as(C.c_void_p)


def forest(nodes, start, x_nonad, scales, mc_nodes):
    """reweight_tree over a forest (eventreweight.cpp): nodes (trees.NODE_DTYPE records), start
    (n_trees + 1), x_nonad per record, scales (K). Returns (W (K, n_nodes), coverage (K, n_trees), unlinked,
    recomputed_differs, grouped_lost)."""
    nodes = np.ascontiguousarray(nodes)
    assert nodes.dtype.itemsize == lib().rw_node_bytes()
    start, x = np.ascontiguousarray(start, np.int64), np.ascontiguousarray(x_nonad, np.float64)
    s = np.ascontiguousarray(scales, np.float64)
    n, nt, K = len(nodes), len(start) - 1, len(s)
    assert start[-1] == n and len(x) == n
    W, cov, cnt = np.zeros((K, n)), np.zeros((K, nt)), np.zeros(3)
    rc = lib().rw_forest(C.c_int64(nt), _ptr(start), _ptr(nodes), _ptr(x), C.c_int32(mc_nodes), C.c_int32(K), _ptr(s), _ptr(W),
                         _ptr(cov), _ptr(cnt))
    if rc:
        raise RuntimeError(f"rw_forest failed: {rc}")
    return W, cov, int(cnt[0]), int(cnt[1]), int(cnt[2])


def back(x_root, bweight, scales, x_single=None):
    """B (K, n): the backtrace factors of n events at every scale. x_single (n): the exponent of the
    backtrace's crossing where it has exactly one, NaN elsewhere (None: nowhere)"""
    x, w = np.ascontiguousarray(x_root, np.float64), np.ascontiguousarray(bweight, np.float64)
    s = np.ascontiguousarray(scales, np.float64)
    xs = np.full(len(x), np.nan) if x_single is None else np.ascontiguousarray(x_single, np.float64)
    B = np.zeros((len(s), len(x)))
    lib().rw_back(C.c_int64(len(x)), _ptr(x), _ptr(w), _ptr(xs), C.c_int32(len(s)), _ptr(s), _ptr(B))
    return B


def power(W, B, cyclotron, tau, sln):
    return lib().rw_power(W, B, int(cyclotron), tau, sln)


def tables(start, flux, sky, pw, a, nbins, sky_size):
    """The second moments per coupling (eventreweight.cpp rw_tables): tools/eventmoments.forest's
    arguments with pw (K, n_nodes), the records' powers at every coupling, in the place of power. Returns
    a dict: flux_sq, flux_xa (K, 2 nbins), sky_sq, sky_xa (K, sky_size), totals (K, 8)."""
    start, a = np.ascontiguousarray(start, np.int64), np.ascontiguousarray(a, np.int64)
    flux, sky = np.ascontiguousarray(flux, np.int32), np.ascontiguousarray(sky, np.int32)
    pw = np.ascontiguousarray(pw, np.float64)
    K = pw.shape[0]
    out = {"flux_sq": np.zeros((K, 2 * nbins)), "flux_xa": np.zeros((K, 2 * nbins)), "sky_sq": np.zeros((K, sky_size)),
           "sky_xa": np.zeros((K, sky_size)), "totals": np.zeros((K, 8))}
    rc = lib().rw_tables(C.c_int64(len(start) - 1), _ptr(start), _ptr(flux), _ptr(sky), _ptr(pw), _ptr(a), C.c_int32(nbins),
                         C.c_int64(sky_size), C.c_int32(K), *[_ptr(out[k]) for k in ("flux_sq", "flux_xa", "sky_sq", "sky_xa",
                                                                                       "totals")])
    if rc:
        raise RuntimeError(f"rw_tables failed: {rc}")
    return out
