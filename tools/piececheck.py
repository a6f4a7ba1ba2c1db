"""TEST TOOL ONLY: builds and runs tools/build/piececheck, a host compile of the streamed host
pipeline's partition header (art_pieces.h: which output piece a ray belongs to, the pieces' bounds
and their blobs' offsets -- shared by the host, the helpers and the integrator), so a CPU test can
check the partition without a GPU. The product never runs this."""
import os
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "piececheck.cpp")
EXE = os.path.join(HERE, "build", "piececheck")
DEPS = [SRC, os.path.join(HERE, "..", "adiabatic_raytracer_amd", "csrc", "art_pieces.h")]


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
    subprocess.run([_cxx(), "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", SRC, "-o", EXE + ".tmp"], check=True)
    os.replace(EXE + ".tmp", EXE)
    return EXE


def check(n, shift, fine_shift, region):
    """(ok, text): text is 'ok count ncoarse shift fine_shift split' or the first failed check"""
    r = subprocess.run([build(), str(n), str(shift), str(fine_shift), str(region)], capture_output=True, text=True)
    return r.returncode == 0, r.stdout.strip()
