"""Rehearsal of the driver's N-GPU bench on the one card of a GPU box: bench.py launched by
torch.distributed.run exactly as the SCALE run launches it, here with 8
ranks, every rank on device 0 and gloo for the all-reduce (ART_BENCH_DEVICE /
ART_BENCH_BACKEND). Checks the contract's one JSON line, totals equal to the sum over the
shards (= the single-process run's) and a reduced flux equal to the single-process run's,
bin for bin (Gen_Samples.jl:195-239 merges per-process runs; here one all-reduce). This
makes no scaling claim: the 8 ranks share one GPU."""
import json
import os
import socket
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = ["--rays", "1250000", "--steps", "2", "--warmup", "1", "--no-device", "--no-cpu-baseline"]


def _json_lines(out):
    return [json.loads(ln) for ln in out.splitlines() if ln.startswith("{")]


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_plain_run_is_lean_and_dumps_its_outputs(tmp_path):
    """A plain run prints the headline without the side figures that --full adds, and
    --dump-outputs writes the last timed call's outputs (a seeded sample of a batch larger than
    bench.DUMP_RAYS) as float64 arrays that agree with the result line."""
    import numpy as np
    rays, kept = 200000, 131072
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--rays", str(rays), "--steps", "2", "--warmup", "1",
                        "--dump-outputs", str(tmp_path)], cwd=ROOT, env=dict(os.environ), capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    lines = _json_lines(r.stdout)
    assert len(lines) == 1, r.stdout[-4000:]
    line = lines[0]
    assert line["steps"] == 2 and line["ms_per_step"] > 0 and line["value"] > 0
    assert not {"device_resident", "device_resident_in_flight", "cpu_baseline"} & set(line)
    d = {f[:-4]: np.load(os.path.join(tmp_path, f)) for f in os.listdir(tmp_path)}
    assert {"x_end", "k_end", "u7_end", "tau_end", "status", "n_accept", "n_reject", "n_cross", "xc_pos", "xc_k", "xc_t",
            "xc_dw", "xc_p", "ray_index", "flux_hist"} == set(d)
    assert all(a.dtype == np.float64 for a in d.values()) and sum(a.nbytes for a in d.values()) <= 64e6
    assert all(np.isfinite(a).all() for a in d.values())
    idx = d["ray_index"]
    assert idx.shape == (kept,) and np.all(np.diff(idx) > 0) and idx[0] >= 0 and idx[-1] < rays
    assert d["x_end"].shape == (3, kept) and d["xc_pos"].shape == (3, kept) and d["status"].shape == (kept,)
    assert d["flux_hist"].tolist() == line["flux_hist"]
    assert set(np.unique(d["status"])) <= set(range(5)) and d["n_accept"].min() >= 0
    assert (d["n_cross"] > 0).any() and np.all(d["xc_p"][d["n_cross"] == 0] == 0)


def test_bench_eight_gloo_ranks_on_one_card():
    env = dict(os.environ, ART_BENCH_DEVICE="0", ART_BENCH_BACKEND="gloo")
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "8", "--master-addr",
           "127.0.0.1", "--master-port", str(_free_port()), "bench.py", "--gpus", "8", *ARGS]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=420)
    assert r.returncode == 0, r.stderr[-4000:]
    lines = _json_lines(r.stdout)
    assert len(lines) == 1, r.stdout[-4000:]  # rank 0 only
    multi = lines[0]
    one = _json_lines(subprocess.run([sys.executable, "bench.py", *ARGS], cwd=ROOT, env=dict(os.environ),
                                     capture_output=True, text=True, timeout=300, check=True).stdout)
    assert len(one) == 1
    one = one[0]
    assert multi["n_gpus"] == 8 and one["n_gpus"] == 1
    assert multi["totals"] == one["totals"] and multi["totals"]["rays"] == 1250000
    assert multi["flux_hist"] == one["flux_hist"] and sum(one["flux_hist"]) > 0
    assert multi["value"] > 0 and multi["steps"] == 2 and multi["warmup"] == 1
