"""Bit-exact fixtures of the integrator's outputs for tests/test_gpu_stage_glue.py (TEST INFRASTRUCTURE ONLY).

Run ON THE BUILD OF THE PARENT of a commit that reschedules the stage glue (needs the GPU), with that
parent's sha, which every file records:

    python tests/golden/make_stage_glue_fixture.py PARENT_SHA [OUT_DIR]

Writes in_<cfg>.npz (the 2,048 forward roots a case starts from: x0, k0, erg) and <case>.npz (every
output array of the case, and parent_sha) into OUT_DIR (default: tests/golden/stage_glue). The cases
and how they are run are the test's own (CASES, run_case)."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))                   # tests/: conftest, the test module
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))  # the package

import test_gpu_stage_glue as T  # noqa: E402

if __name__ == "__main__":
    sha = sys.argv[1]
    assert len(sha) == 40 and all(c in "0123456789abcdef" for c in sha), "give the parent commit's full sha"
    out_dir = sys.argv[2] if len(sys.argv) > 2 else T.GOLDEN
    os.makedirs(out_dir, exist_ok=True)
    inputs = {}
    for cfg in sorted({c[1] for c in T.CASES.values()}):
        inputs[cfg] = T.make_inputs(cfg)
        np.savez_compressed(os.path.join(out_dir, f"in_{cfg}.npz"), **inputs[cfg])
    for case, (_, cfg, _) in T.CASES.items():
        out = T.run_case(case, inputs[cfg])
        np.savez_compressed(os.path.join(out_dir, f"{case}.npz"), parent_sha=np.array(sha), **out)
        print(case, {k: (v.dtype.str, v.shape) for k, v in out.items()},
              "attempts", int(out["n_accept"].sum() + out["n_reject"].sum()), "crossings", int(out["n_cross"].sum()),
              "status", np.bincount(out["status"].astype(np.int64) - out["status"].min()).tolist(), flush=True)
