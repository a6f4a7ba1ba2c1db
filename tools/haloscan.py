"""TEST TOOL ONLY: builds and runs tools/build/haloscan, a host compile of the halo scan's formula
(art_halo.h: halo_ratio, the ratio of two models' importance factors), so a CPU test can hold it to
numpy without a GPU. The product never runs this."""
import os
import shutil
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "haloscan.cpp")
EXE = os.path.join(HERE, "build", "haloscan")
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


def ratio(u, base, target):
    """halo_ratio: u (n, 3) [km/s]; base and target (v0, (vx, vy, vz)) -> R (n)"""
    u = np.asarray(u, np.float64).reshape(-1, 3)
    n = u.shape[0]
    par = np.array([base[0], *base[1], target[0], *target[1]], np.float64)
    a = np.ascontiguousarray(np.hstack([u, np.broadcast_to(par, (n, 8))]))
    r = subprocess.run([build(), "ratio"], input=a.tobytes(), capture_output=True, check=True)
    return np.frombuffer(r.stdout, np.float64).copy()
