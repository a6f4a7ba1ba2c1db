"""Bit-exact fixtures of the integrator's outputs for tests/test_gpu_scalar_args.py (TEST INFRASTRUCTURE ONLY).

Run ON THE BUILD OF THE PARENT of a commit that moves the integrator's arguments between registers and the
kernel-argument segment (needs the GPU), with that parent's sha, which every file records:

    python tests/golden/make_scalar_args_fixture.py PARENT_SHA [OUT_DIR]

Writes <case>.npz (every output array of the case, its launch counters and parent_sha) into OUT_DIR
(default: tests/golden/scalar_args). The cases and how they are run are the test's own (CASES, run_case);
the inputs are the stage-glue fixtures' forward roots (tests/golden/stage_glue/in_<cfg>.npz)."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))                   # tests/: conftest, the test modules
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))  # the package

import test_gpu_scalar_args as T  # noqa: E402

if __name__ == "__main__":
    sha = sys.argv[1]
    assert len(sha) == 40 and all(c in "0123456789abcdef" for c in sha), "give the parent commit's full sha"
    out_dir = sys.argv[2] if len(sys.argv) > 2 else T.GOLDEN
    os.makedirs(out_dir, exist_ok=True)
    for case in T.CASES:
        out = T.run_case(case)
        np.savez_compressed(os.path.join(out_dir, f"{case}.npz"), parent_sha=np.array(sha), **out)
        print(case, {k: int(v) for k, v in out.items() if k.startswith("counter_")}, "crossings", int(out["n_cross"].sum()),
              "max", int(out["n_cross"].max()), "status", np.bincount(out["status"].astype(np.int64) - out["status"].min()).tolist(),
              flush=True)
