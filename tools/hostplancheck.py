"""TEST TOOL ONLY: builds and runs tools/build/hostplancheck, a host compile of the host paths' plain-C++
plan header (art_host_plan.h: the streamed call's upload units and block counts, and the row segments
that scatter an output blob into the caller's arrays and gather the caller's inputs), so a CPU test
can check them without a GPU. The product never runs this."""
import os
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "hostplancheck.cpp")
EXE = os.path.join(HERE, "build", "hostplancheck")
CSRC = os.path.join(HERE, "..", "adiabatic_raytracer_amd", "csrc")
DEPS = [SRC, os.path.join(CSRC, "art_host_plan.h"), os.path.join(CSRC, "art_pieces.h"),
        os.path.join(HERE, "..", "include", "art.h")]


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


def _run(*args):
    r = subprocess.run([build(), *[str(a) for a in args]], capture_output=True, text=True)
    return r.returncode == 0, r.stdout.strip()


def units(n, first, step, ramp, lanes):
    """(ok, bounds): the upload units' bounds, checked to tile [0, n) and to increase strictly"""
    ok, text = _run("units", n, first, step, int(bool(ramp)), lanes)
    return ok, ([int(v) for v in text.split()] if ok else text)


def blocks(slots, hw, helpers, serial):
    """(helpers, iblocks)"""
    ok, text = _run("blocks", slots, hw, helpers, int(bool(serial)))
    assert ok, text
    h, i = text.split()
    return int(h), int(i)


def scatter(n, lo, m, cap):
    """(ok, text): text is 'ok segments bytes' (of the scatter) or the first failed check"""
    return _run("scatter", n, lo, m, cap)
