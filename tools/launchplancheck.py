"""TEST TOOL ONLY: builds and runs tools/build/launchplancheck, a host compile of the launch plan's plain-C++
header (art_launch_plan.h: which kernels one propagate launch runs, and the lists of the builds that
exist), so a CPU test can check the plan without a GPU and a GPU test can compare the builds its rows
ran with the builds the plan can reach. The product never runs this."""
import os
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "launchplancheck.cpp")
EXE = os.path.join(HERE, "build", "launchplancheck")
CSRC = os.path.join(HERE, "..", "adiabatic_raytracer_amd", "csrc")
DEPS = [SRC, os.path.join(CSRC, "art_launch_plan.h"), os.path.join(HERE, "..", "include", "art.h")]

INT_KEYS = ("launches", "save", "don", "wps", "cyc", "bulk_grid", "donate", "cont_wps", "cont_donate", "tail_grid",
            "graduate", "hot_at", "ncont", "nhot", "cont_grid", "cont_don")
BOOL_KEYS = ("streamed", "small_tail", "bulk", "save", "cyc", "cont", "tail", "hot", "sorted", "grad_records", "hot_records",
             "bulk_exists", "cont_exists", "tail_exists")


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
    return r.returncode, r.stdout.strip()


def _parse(text):
    d = dict(line.split("=", 1) for line in text.splitlines())
    for k in INT_KEYS:
        d[k] = int(d[k])
    for k in BOOL_KEYS:
        d[k] = bool(int(d[k]))
    return d


def plan(**inputs):
    """One plan: the record's decisions as last_launch_path() names them (the counts left out), and
    beside them ncont, nhot, grad_records, hot_records, the continuation's grid / geometry / DON and
    whether the named builds exist. Inputs: LaunchPlanIn's fields (geom "FLAT" / "GR" / "ANY", integrator
    "vern6" / "rk4", small_tail=k for ART_SMALL_TAIL=k); booleans as 0 / 1."""
    rc, text = _run("plan", *[f"{k}={int(v) if isinstance(v, bool) else v}" for k, v in inputs.items()])
    assert rc == 0, text
    return _parse(text)


def streamed(n, geom, blocks):
    rc, text = _run("streamed", n, geom, blocks)
    assert rc == 0, text
    return _parse(text)


def _build_of(words):
    if words[0] == "tail":
        return ("tail", words[1])
    integ, geom, save, don, wps, cyc = words[1:]
    return ("propagate", integ, geom, bool(int(save)), int(don), int(wps), bool(int(cyc)))


def builds():
    """the instantiation lists: ("propagate", integrator, geom, save, don, wps, cyc) and ("tail", geom)"""
    rc, text = _run("builds")
    assert rc == 0, text
    return [_build_of(line.split()) for line in text.splitlines()]


def sweep():
    """(ok, reached, unreached, text): the full input grid; ok is False when some plan names a build
    that is not in the lists (text says which); reached / unreached partition the lists"""
    rc, text = _run("sweep")
    if rc != 0:
        return False, [], [], text
    reached, unreached = [], []
    for line in text.splitlines():
        w = line.split()
        if w[0] == "reached":
            reached.append(_build_of(w[1:]))
        elif w[0] == "unreached":
            unreached.append(_build_of(w[1:]))
    return True, reached, unreached, text


def build_of_record(rec):
    """the bulk build of a last_launch_path() record (or of plan()), as builds() names it; None without a bulk pass"""
    if not rec["bulk"]:
        return None
    return ("propagate", rec["integrator"], rec["geom"], bool(rec["save"]), int(rec["don"]), int(rec["wps"]), bool(rec["cyc"]))
