"""The streamed host pipeline with two levels of output pieces (coarse pieces over the bulk of the
batch, fine ones over its last rays: ART_HOST_PIECE_SHIFT, ART_HOST_FINE_SHIFT, ART_HOST_FINE_RAYS)
and with ramped upload units (ART_HOST_FIRST_UNIT, ART_HOST_UNIT): every output array, crossing
slot, statistic and the flux equal the single launch's bit for bit, every call streams, none gives
up. The partition itself is checked on the CPU (test_pieces.py)."""
from dataclasses import replace

import numpy as np
import pytest

from conftest import CONFIGS
from test_edges import host_flux

_REF = {}  # (cfg, species, cap, n) -> (params, args, max_crossings, the single launch's outputs): computed once


def _case(cfg, species, cap, n, monkeypatch):
    import adiabatic_raytracer_amd as A
    key = (cfg, species, cap, n)
    if key not in _REF:
        p = A.Params(**CONFIGS[cfg])
        s = A.sample_conversion_points(p, n, seed=1769)
        q, k, mc = (p, s["k_init"], -1) if species == 1 else (replace(p, B0=-p.B0), -s["k_init"], 100000)
        args = (s["x"], k, s["erg"], -np.ones(n), np.full(n, -30.0), np.full(n, species, np.int8))
        monkeypatch.setenv("ART_HOST_MODE", "single")
        ref = A.propagate_batch(q, *args, max_crossings=mc, capacity=cap, flux_nbins=50)
        for v in ref.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _REF[key] = (q, args, mc, ref)
    return _REF[key]


def _streamed_equals_single(cfg, species, cap, n, env, monkeypatch):
    import adiabatic_raytracer_amd as A
    q, args, mc, ref = _case(cfg, species, cap, n, monkeypatch)
    monkeypatch.setenv("ART_HOST_MODE", "stream")
    monkeypatch.setenv("ART_HOST_CHUNK_MIN", "500")
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))
    A.raytracer.host_path_counters(reset=True)
    for _ in range(2):  # the second call reuses the streams, signals and staging
        got = A.propagate_batch(q, *args, max_crossings=mc, capacity=cap, flux_nbins=50)
        for key, v in ref.items():
            if isinstance(v, np.ndarray):
                assert np.array_equal(v, got[key], equal_nan=True), (cfg, env, key)
        for key in ("attempts", "accepted", "root_steps", "scan_evals", "rays", "init_rhs", "cert_steps"):
            assert ref["stats"][key] == got["stats"][key], (cfg, env, key)
        assert np.array_equal(ref["flux"], got["flux"])
    assert A.raytracer.host_path_counters() == {"calls": 2, "streamed": 2, "stream_giveups": 0, "chunked": 0,
                                                "single": 0}
    assert np.array_equal(got["flux"], host_flux(q, got, np.full(n, species, np.int8), 50))


# coarse 2^12, fine 2^10 over the last 7723 of 20011 rays: 3 coarse pieces, 7 full fine pieces and a partial eighth
TWO_LEVEL = {"ART_HOST_PIECE_SHIFT": 12, "ART_HOST_FINE_SHIFT": 10, "ART_HOST_FINE_RAYS": 7723}


@pytest.mark.gpu
@pytest.mark.parametrize("cfg,species,cap,direct", [("flat", 1, 1, 0), ("flat", 0, 3, 0), ("gr", 1, 2, 0), ("flat", 0, 3, 1)])
def test_two_level_pieces_are_bit_exact(cfg, species, cap, direct, monkeypatch):
    """Flat photons, flat all-crossings axion backtraces and GR photons through coarse and fine
    pieces; once with the blobs in pinned host memory (ART_HOST_DIRECT=1)."""
    _streamed_equals_single(cfg, species, cap, 20011, dict(TWO_LEVEL, ART_HOST_DIRECT=direct), monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("n,region", [(20011, 0), (20011, 1 << 30), (4096, 100)])
def test_degenerate_partitions_are_bit_exact(n, region, monkeypatch):
    """No fine region (one level), a fine region beyond the batch (every piece fine), and a batch
    of exactly one coarse piece whose split falls at n (no fine piece)."""
    _streamed_equals_single("flat", 1, 1, n, dict(TWO_LEVEL, ART_HOST_FINE_RAYS=region), monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("n,blocks", [(20011, 0), (20011, 48), (777, 0)])
def test_ramped_upload_units_are_bit_exact(n, blocks, monkeypatch):
    """First upload units of 1024 rays and a steady unit of 4096: with every block slot of the GPU
    the launch has more lanes than the batch has rays, so every unit stays small; with 48 slots
    (16 helpers, 32 integrator blocks: 8192 lanes) the units double to 4096 after the first eight;
    and a batch smaller than the first unit is one unit."""
    env = dict(TWO_LEVEL, ART_HOST_FIRST_UNIT=1024, ART_HOST_UNIT=4096)
    if blocks:
        env["ART_HOST_BLOCKS"] = blocks
    _streamed_equals_single("flat", 1, 1, n, env, monkeypatch)
