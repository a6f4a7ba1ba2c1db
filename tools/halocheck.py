"""TEST TOOL ONLY: builds and runs tools/build/halocheck, a host compile of the halo velocity model's
plain-C++ header (art_halo.h: the proposal speed, the Kepler orbit's incoming asymptote and the
importance ratio), so a CPU test can hold the three formulas to numpy without a GPU. The product
never runs this."""
import os
import shutil
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "halocheck.cpp")
EXE = os.path.join(HERE, "build", "halocheck")
DEPS = [SRC, os.path.join(HERE, "..", "adiabatic_raytracer_amd", "csrc", "art_halo.h")]


def _cxx():
    for c in (os.environ.get("CXX"), shutil.which("c++"), shutil.which("g++"), shutil.which("clang++"),
              "/opt/rocm/llvm/bin/clang++"):
        if c and (os.path.isabs(c) and os.path.exists(c) or shutil.which(c)):
            return c
    raise RuntimeError("no host C++ compiler found")


def build():
    if os.path.exists(EXE) and all(os.path.getmtime(EXE) >= os.path.getmtime(d) for d in DEPS):
        return EXE
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    # -ffp-contract=off: the header's expressions as written, rounded once per operation
    subprocess.run([_cxx(), "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", SRC, "-o",
                    EXE + ".tmp"], check=True)
    os.replace(EXE + ".tmp", EXE)
    return EXE


def _run(mode, cases, nin, nout):
    a = np.ascontiguousarray(cases, np.float64).reshape(-1, nin)
    r = subprocess.run([build(), mode], input=a.tobytes(), capture_output=True, check=True)
    return np.frombuffer(r.stdout, np.float64).reshape(a.shape[0], nout).copy()


def speed(U, vp):
    """halo_speed(U, vp), elementwise"""
    U, vp = np.broadcast_arrays(np.asarray(U, np.float64), np.asarray(vp, np.float64))
    return _run("speed", np.stack([U.ravel(), vp.ravel()], axis=1), 2, 1)[:, 0]


def asymptote(x, d, s, GM):
    """halo_asymptote: x, d (n, 3), s (n) or a number, GM a number -> u (n, 3)"""
    x, d = np.asarray(x, np.float64).reshape(-1, 3), np.asarray(d, np.float64).reshape(-1, 3)
    n = x.shape[0]
    col = lambda v: np.broadcast_to(np.asarray(v, np.float64), (n,)).reshape(n, 1)  # noqa: E731
    return _run("asymptote", np.hstack([x, d, col(s), col(GM)]), 8, 3)


def factor(u, s, v0, v_ns, vp):
    """halo_factor: u (n, 3), s (n), v0, v_ns (3), vp numbers -> F (n)"""
    u = np.asarray(u, np.float64).reshape(-1, 3)
    n = u.shape[0]
    col = lambda v: np.broadcast_to(np.asarray(v, np.float64), (n,)).reshape(n, 1)  # noqa: E731
    vn = np.broadcast_to(np.asarray(v_ns, np.float64), (n, 3))
    return _run("factor", np.hstack([u, col(s), col(v0), vn, col(vp)]), 9, 1)[:, 0]
