"""main_runner_tree(sky_map=...) sharded by global event id: two processes on the one card of the
test box (gloo for the collective, as tests/test_gpu_distributed.py does) bin their own rows and
sum the maps in the run's single all-reduce. Every rank then holds the single-process map: the
same terms w_i / f_inx added in another order, so each bin is within 2 (count + 1) 2^-53 Σ|w| of it
(two recursive sums of count terms), and the bins that are empty are the same."""
import os
import socket

import numpy as np
import pytest

from conftest import CONFIGS

pytestmark = pytest.mark.gpu

N_TRAJS = 41  # 40 events
SHAPE = dict(n_theta=6, n_phi=10, n_dw=4)


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, kw, outdir, dw_range):
    import torch
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import adiabatic_raytracer_amd as A
        info = {}
        A.trees.main_runner_tree(A.Params(**kw), N_TRAJS, saveMode=1, dir_tag=outdir, file_tag="s", rank=rank,
                                 world=world, run_info=info, sky_map=dict(SHAPE, dw_range=dw_range))
        np.savez(os.path.join(outdir, f"sky{rank}.npz"), sky=info["sky_map"], f_inx=info["f_inx"])
    finally:
        dist.destroy_process_group()


def test_sky_map_shards_sum_to_the_single_process_map(tmp_path):
    import torch.multiprocessing as mp
    import adiabatic_raytracer_amd as A
    kw = CONFIGS["flat"]
    p = A.Params(**kw)
    info = {}
    rows = A.trees.main_runner_tree(p, N_TRAJS, saveMode=1, run_info=info, sky_map=SHAPE)
    dw_range = tuple(float(v) for v in info["sky_map_edges"][2][[0, -1]])  # the rows' (min, max), now fixed
    mp.start_processes(_worker, args=(2, _free_port(), kw, str(tmp_path), dw_range), nprocs=2, join=True,
                       start_method="spawn")
    sky = info["sky_map"]
    pts = np.stack([np.cos(rows[:, 2]), rows[:, 3], rows[:, 12]], axis=1)
    w = rows[:, 8] * rows[:, 7]
    shape = (SHAPE["n_theta"], SHAPE["n_phi"], SHAPE["n_dw"])
    ranges = ((-1.0, 1.0), (-np.pi, np.pi), dw_range)
    for r in range(2):
        z = np.load(tmp_path / f"sky{r}.npz")
        assert int(z["f_inx"]) == info["f_inx"] and z["sky"].shape == sky.shape
        for s in (0, 1):
            m = rows[:, 1] == s
            count, _ = np.histogramdd(pts[m], bins=shape, range=ranges)
            tot, _ = np.histogramdd(pts[m], bins=shape, range=ranges, weights=np.abs(w[m]))
            assert count.sum() == m.sum()  # every row lies in the map
            assert np.all(np.abs(z["sky"][s] - sky[s]) <= 2 * (count + 1) * 2.0 ** -53 * tot), (r, s)
            assert np.array_equal(z["sky"][s] == 0, count == 0)
    assert sky[1].sum() > 0
    # each rank saves the reduced map beside its own rows
    names = sorted(f.name for f in (tmp_path / "npy").glob("skymap_*.npz"))
    assert len(names) == 2 and names[0].endswith("_s0.npz") and names[1].endswith("_s1.npz")
    with np.load(tmp_path / "npy" / names[1]) as f:
        assert np.array_equal(f["sky_map"], np.load(tmp_path / "sky1.npz")["sky"])
