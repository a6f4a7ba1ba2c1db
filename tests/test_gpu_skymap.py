"""Sky maps on the GPU: the generic 3-D histogram (art_histogram3_device) against np.histogramdd,
the fused end-state kernel (art_sky_map_segments_device, Engine.sky_map) against its own per-ray
labels, the 1-D flux kernel and numpy, and main_runner_tree(sky_map=...) against the run's flux.

Counts (unit weights) must be exact in every accumulation mode. A weighted bin is a sum of the same
terms in another order than numpy's: two recursive sums of `count` terms differ by at most
2 (count - 1) u Σ|w| (1 + O(u)) with u = 2^-53 (Higham, Accuracy and Stability, §4.2), which the bound
2 (count + 1) u Σ|w| used below covers."""
import ctypes as C

import numpy as np
import pytest

from conftest import CONFIGS

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
N = 20037  # no multiple of 64 or 256, and four grid-stride passes (the launcher gives a thread >= 4 items)
RANGES = ((0.0, np.pi), (-np.pi, np.pi), (-2e-6, 3e-6))
LDS_SHAPES = [(1, 50, 1), (3, 5, 2), (16, 32, 4)]
BIG_SHAPE = (20, 37, 7)  # 10360 doubles: above the 8192 of the LDS budget


def _torch():
    import torch
    return torch


def _dev(a, dtype=None):
    torch = _torch()
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).cuda()


def _h3(coords, species, w, shape, ranges=RANGES, mode=0, hist=None):
    """art_histogram3_device on device tensors, on the current stream; returns the (2, *shape) tensor"""
    import adiabatic_raytracer_amd as A
    torch = _torch()
    lib = A.load_library()
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
    if hist is None:
        hist = torch.zeros(2, *shape, dtype=torch.float64, device="cuda")
    A._lib.check(lib.art_histogram3_device(
        coords[0].numel(), p(coords[0]), p(coords[1]), p(coords[2]), p(species), p(w), (C.c_int32 * 3)(*shape),
        (C.c_double * 3)(*[r[0] for r in ranges]), (C.c_double * 3)(*[r[1] for r in ranges]), mode, p(hist),
        C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    return hist


def _items(shape, ranges=RANGES):
    """N items uniform over slightly more than the ranges, then on each axis every edge of `shape`, its
    two neighbours, ±inf, NaN and -0.0 (the other two coordinates stay where the draw put them)"""
    rng = np.random.default_rng(20037)
    cols = []
    for (lo, hi) in ranges:
        cols.append(rng.uniform(lo - 0.02 * (hi - lo), hi + 0.02 * (hi - lo), N))
    at = 0
    for d, (lo, hi) in enumerate(ranges):
        e = np.linspace(lo, hi, shape[d] + 1)
        sp = np.concatenate([e, np.nextafter(e, -np.inf), np.nextafter(e, np.inf), [np.inf, -np.inf, np.nan, -0.0]])
        cols[d][at:at + sp.size] = sp
        at += sp.size
    assert at < N
    species = rng.integers(0, 2, N).astype(np.int8)
    return cols, species


@pytest.fixture(scope="module")
def weights():
    w = np.random.default_rng(7).lognormal(0.0, 4.6, N)  # ±3σ spans 12 decades
    assert w.min() > 0 and np.log10(w.max() / w.min()) > 11
    return w


def _numpy_map(cols, species, shape, ranges=RANGES, w=None):
    pts = np.stack(cols, axis=1)
    out = np.zeros((2, *shape))
    for s in (0, 1):
        m = species == s
        out[s], _ = np.histogramdd(pts[m], bins=shape, range=ranges, weights=None if w is None else w[m])
    return out


def _modes(shape):
    return (0, 1, 2) if 2 * int(np.prod(shape)) <= 8192 else (0, 2)


@pytest.mark.parametrize("shape", LDS_SHAPES + [BIG_SHAPE])
def test_counts_equal_histogramdd_in_every_mode(shape):
    cols, species = _items(shape)
    ref = _numpy_map(cols, species, shape)
    assert ref.sum() > 0.8 * N and ref.sum() < N  # some items lie outside
    d, sp = [_dev(c) for c in cols], _dev(species)
    for mode in _modes(shape):
        got = _h3(d, sp, None, shape, mode=mode).cpu().numpy()
        assert np.array_equal(got, ref), (shape, mode, np.abs(got - ref).sum())


def test_mode_1_refuses_a_table_over_the_lds_budget():
    from adiabatic_raytracer_amd._lib import ArtError
    cols, species = _items(BIG_SHAPE)
    with pytest.raises(ArtError, match="LDS budget"):
        _h3([_dev(c) for c in cols], _dev(species), None, BIG_SHAPE, mode=1)


def test_azimuth_histogram_equals_radiated_flux():
    from adiabatic_raytracer_amd.trees import radiated_flux
    cols, species = _items((1, 50, 1))
    phi = cols[1]
    one = np.full(N, 0.5)
    ref = radiated_flux(phi, species, np.ones(N), 50)
    rngs = ((0.0, 1.0), (-np.pi, np.pi), (0.0, 1.0))
    for mode in (0, 1, 2):
        got = _h3([_dev(one), _dev(phi), _dev(one)], _dev(species), None, (1, 50, 1), rngs, mode).cpu().numpy()
        assert np.array_equal(got.reshape(-1), ref), mode


@pytest.mark.parametrize("shape", [(3, 5, 2), (16, 32, 4), BIG_SHAPE])
def test_weighted_bins_within_the_summation_bound(shape, weights):
    cols, species = _items(shape)
    ref = _numpy_map(cols, species, shape, w=weights)
    count = _numpy_map(cols, species, shape)
    bound = 2 * (count + 1) * U * ref  # the weights are positive: Σ|w| of a bin is its sum
    d, sp, w = [_dev(c) for c in cols], _dev(species), _dev(weights)
    for mode in _modes(shape):
        got = _h3(d, sp, w, shape, mode=mode).cpu().numpy()
        err = np.abs(got - ref)
        print(f"shape {shape} mode {mode}: max err / bound = {np.max(err[ref > 0] / bound[ref > 0]):.3g}")
        assert np.all(err <= bound), (shape, mode, np.max(err[ref > 0] / bound[ref > 0]))
        assert np.array_equal(got == 0, ref == 0)


@pytest.mark.parametrize("mode", [1, 2])
def test_accumulates_keeps_species_apart_and_leaves_hist_alone_for_no_items(mode):
    torch = _torch()
    shape = (3, 5, 2)
    cols, species = _items(shape)
    d, sp = [_dev(c) for c in cols], _dev(species)
    once = _h3(d, sp, None, shape, mode=mode)
    twice = _h3(d, sp, None, shape, mode=mode, hist=once.clone())
    assert torch.equal(twice, 2 * once)
    # all items as axions: the photon table stays empty, the axion table holds both
    ax = _h3(d, torch.zeros_like(sp), None, shape, mode=mode)
    assert torch.count_nonzero(ax[1]) == 0 and torch.equal(ax[0], once[0] + once[1])
    ph = _h3(d, None, None, shape, mode=mode)  # no species array: photons
    assert torch.count_nonzero(ph[0]) == 0 and torch.equal(ph[1], once[0] + once[1])
    # n = 0: the table is not touched
    h = torch.full((2, *shape), 3.5, dtype=torch.float64, device="cuda")
    empty = torch.empty(0, dtype=torch.float64, device="cuda")
    _h3([empty] * 3, None, None, shape, mode=mode, hist=h)
    torch.cuda.synchronize()
    assert torch.all(h == 3.5)


def test_runs_on_the_callers_stream():
    torch = _torch()
    shape = (16, 32, 4)
    cols, species = _items(shape)
    ref = _numpy_map(cols, species, shape)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        d, sp = [_dev(c) for c in cols], _dev(species)
        got = [_h3(d, sp, None, shape, mode=m) for m in (1, 2)]
    side.synchronize()
    for g in got:
        assert np.array_equal(g.cpu().numpy(), ref)


def test_rows_sky_map_takes_numpys_cosine():
    from adiabatic_raytracer_amd.trees import sky_map
    rng = np.random.default_rng(3)
    n = 5000
    theta, phi, dw = np.arccos(rng.uniform(-1, 1, n)), rng.uniform(-np.pi, np.pi, n), rng.normal(0, 1e-6, n)
    theta[:3], dw[3:6] = (0.0, np.pi, np.pi / 2), (np.nan, np.inf, -1e-6)
    ident = rng.integers(0, 2, n).astype(float)
    for axis, a, rng_a in (("cos", np.cos(theta), (-1.0, 1.0)), ("theta", theta, (0.0, np.pi))):
        pts = np.stack([a, phi, dw], axis=1)
        for kw, rng_c in ((dict(n_dw=5, dw_range=(-1e-6, 2e-6)), (-1e-6, 2e-6)), (dict(), None)):
            got = sky_map(theta, phi, dw, ident, None, n_theta=6, n_phi=9, theta_axis=axis, **kw)
            for s in (0, 1):
                m = (ident == s) & (np.isfinite(dw) if rng_c is None else True)
                ref, _ = np.histogramdd(pts[m][:, :2] if rng_c is None else pts[m], bins=(6, 9) if rng_c is None else (6, 9, 5),
                                        range=(rng_a, (-np.pi, np.pi)) + (() if rng_c is None else (rng_c,)))
                assert np.array_equal(got[s], ref.reshape(got[s].shape)), (axis, kw, s)


# ---- the fused kernel on propagated batches

@pytest.fixture(scope="module", params=[("flat", 4096), ("gr", 2048)], ids=["flat", "gr"])
def batch(request):
    """A propagated batch (default max_crossings: some rays end in a crossing or on the star), its end
    state on the host, labels and weights"""
    import adiabatic_raytracer_amd as A
    torch = _torch()
    cfg, n = request.param
    p = A.Params(**CONFIGS[cfg])
    eng = A.Engine(p, device=0)
    inp = eng.forward_roots(n, seed=1769)
    out = eng.propagate(inp)
    torch.cuda.synchronize()
    rng = np.random.default_rng(11)
    host = {k: out[k].cpu().numpy() for k in ("x_end", "k_end", "u7_end", "status")}
    return dict(eng=eng, p=p, n=n, out=out, host=host, species=_dev(rng.integers(0, 2, n).astype(np.int8)),
                w=_dev(rng.lognormal(0.0, 4.6, n)), off=_dev(rng.normal(0.0, 2e-7, n)))


def _host_coords(b, theta_axis, off):
    h, p = b["host"], b["p"]
    n = b["n"]
    x, k = h["x_end"].reshape(3, n).T, h["k_end"].reshape(3, n).T
    final = (h["status"] != 1) & (np.linalg.norm(x, axis=-1) > 1.1 * p.rNS)
    with np.errstate(invalid="ignore", divide="ignore"):
        ct = k[:, 2] / np.linalg.norm(k, axis=-1)
        a = ct if theta_axis == "cos" else np.arccos(ct)
        dw = h["u7_end"] / p.mass_a + (0.0 if off is None else off)
        return final, a, np.arctan2(k[:, 1], k[:, 0]), dw


def _dw_range(b):
    _, _, _, dw = _host_coords(b, "cos", b["off"].cpu().numpy())
    lo, hi = np.nanquantile(dw, [0.02, 0.98])  # some rays fall outside
    return float(lo), float(hi)


@pytest.mark.parametrize("theta_axis", ["cos", "theta"])
@pytest.mark.parametrize("mode", [1, 2])
def test_fused_map_is_the_bincount_of_its_labels(batch, theta_axis, mode):
    b, eng = batch, batch["eng"]
    kw = dict(n_theta=6, n_phi=11, n_dw=5, theta_axis=theta_axis, dw_range=_dw_range(b), dw_offset=b["off"], mode=mode)
    size = 2 * 6 * 11 * 5
    hist, bins = eng.sky_map(b["out"], b["species"], None, return_bins=True, **kw)
    bins = bins.cpu().numpy()
    # (most forward photons end in a crossing; the labels must still cover some rays)
    assert bins.min() == -1 and bins.max() < size and (bins >= 0).sum() >= 50
    ref = np.bincount(bins[bins >= 0], minlength=size).astype(float)
    assert np.array_equal(hist.cpu().numpy().reshape(-1), ref)
    # weighted: the same labels, numpy's sum of each bin
    w = b["w"].cpu().numpy()
    hw, bw = eng.sky_map(b["out"], b["species"], b["w"], return_bins=True, **kw)
    assert np.array_equal(bw.cpu().numpy(), bins)
    refw = np.bincount(bins[bins >= 0], weights=w[bins >= 0], minlength=size)
    err, bound = np.abs(hw.cpu().numpy().reshape(-1) - refw), 2 * (ref + 1) * U * refw
    print(f"{theta_axis} mode {mode}: max err / bound = {np.max(err[ref > 0] / bound[ref > 0]):.3g}")
    assert np.all(err <= bound)


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_fused_azimuth_map_equals_the_flux_kernel(batch, mode):
    b, eng = batch, batch["eng"]
    flux = eng.flux_histogram(b["out"], b["species"], None, 50)
    sky = eng.sky_map(b["out"], b["species"], None, n_theta=1, n_phi=50, n_dw=1, theta_axis="theta", mode=mode)
    assert sky.shape == (2, 1, 50, 1) and flux.sum() > 0
    assert _torch().equal(sky.reshape(-1), flux)
    st = b["host"]["status"]
    assert flux.sum().item() < b["n"] and (st == 1).sum() > 0  # the filter had rays to refuse


@pytest.mark.parametrize("theta_axis", ["cos", "theta"])
def test_fused_labels_are_numpys_bins(batch, theta_axis):
    b, eng = batch, batch["eng"]
    shape, rng_dw = (6, 11, 5), _dw_range(b)
    off = b["off"].cpu().numpy()
    _, bins = eng.sky_map(b["out"], b["species"], None, n_theta=6, n_phi=11, n_dw=5, theta_axis=theta_axis,
                          dw_range=rng_dw, dw_offset=b["off"], return_bins=True)
    bins = bins.cpu().numpy()
    final, a, phi, dw = _host_coords(b, theta_axis, off)
    ranges = ((-1.0, 1.0) if theta_axis == "cos" else (0.0, np.pi), (-np.pi, np.pi), rng_dw)
    _, edges = np.histogramdd(np.zeros((1, 3)), bins=shape, range=ranges)
    idx, near = [], np.zeros(b["n"], bool)
    for v, e in zip((a, phi, dw), edges):
        i = np.searchsorted(e, v, side="right") - 1
        i[v == e[-1]] -= 1
        idx.append(np.where((i >= 0) & (i < e.size - 1) & np.isfinite(v), i, -1))
        gap = np.abs(v[:, None] - e[None, :])
        near |= np.any(gap <= 4 * np.spacing(np.maximum(np.abs(v[:, None]), np.abs(e[None, :]))), axis=1)
    sp = b["species"].cpu().numpy().astype(int)
    ok = final & (idx[0] >= 0) & (idx[1] >= 0) & (idx[2] >= 0)
    ref = np.where(ok, ((sp * shape[0] + idx[0]) * shape[1] + idx[1]) * shape[2] + idx[2], -1)
    print(f"{theta_axis}: {near.sum()} of {b['n']} rays within 4 ulp of an edge, {(ref >= 0).sum()} counted")
    assert near.sum() <= 1e-3 * b["n"]
    assert np.array_equal(bins[~near], ref[~near]), np.flatnonzero((bins != ref) & ~near)[:10]


def test_fused_no_offset_is_an_offset_of_zeros(batch):
    b, eng = batch, batch["eng"]
    torch = _torch()
    _, _, _, dw = _host_coords(b, "cos", None)
    kw = dict(n_theta=6, n_phi=11, n_dw=5, dw_range=tuple(float(v) for v in np.nanquantile(dw, [0.02, 0.98])),
              return_bins=True)
    h0, b0 = eng.sky_map(b["out"], b["species"], b["w"], dw_offset=None, mode=1, **kw)
    h1, b1 = eng.sky_map(b["out"], b["species"], b["w"], dw_offset=torch.zeros(b["n"], dtype=torch.float64, device="cuda"),
                         mode=1, **kw)
    assert torch.equal(b0, b1)
    # the same labels and weights: equal up to the order of the adds
    cnt = np.bincount(b0.cpu().numpy()[b0.cpu().numpy() >= 0], minlength=h0.numel())
    h0, h1 = h0.cpu().numpy().reshape(-1), h1.cpu().numpy().reshape(-1)
    assert np.all(np.abs(h0 - h1) <= 2 * (cnt + 1) * U * h0)
    # unit weights: identical tables
    u0 = eng.sky_map(b["out"], b["species"], None, dw_offset=None, **{**kw, "return_bins": False})
    u1 = eng.sky_map(b["out"], b["species"], None, dw_offset=torch.zeros(b["n"], dtype=torch.float64, device="cuda"),
                     **{**kw, "return_bins": False})
    assert torch.equal(u0, u1)


# ---- main_runner_tree(sky_map=...)

N_EV = 48  # tests/test_gpu_trees.py's smallest run


def test_main_runner_tree_sky_map(tmp_path):
    import adiabatic_raytracer_amd as A
    from adiabatic_raytracer_amd.trees import pulse_profile
    p = A.Params(**CONFIGS["flat"])
    info0, info = {}, {}
    rows0 = A.trees.main_runner_tree(p, N_EV + 1, saveMode=1, run_info=info0)
    spec = dict(n_theta=8, n_phi=50, n_dw=3)
    rows = A.trees.main_runner_tree(p, N_EV + 1, saveMode=1, run_info=info, sky_map=spec, dir_tag=str(tmp_path),
                                    file_tag="s")
    assert rows.tobytes() == rows0.tobytes() and len(rows) > N_EV // 2
    assert "sky_map" not in info0 and set(info) - set(info0) == {"sky_map", "sky_map_edges"}
    for k in set(info0) - {"flux"}:
        assert np.array_equal(info[k], info0[k]), k
    sky = info["sky_map"]
    assert sky.shape == (2, 8, 50, 3)
    # the same terms w_i / f_inx summed in other orders: each of the two sums is within
    # (terms - 1) u Σ|w| of the exact one; terms <= rows for the flux and the totals, plus the
    # n_theta n_dw = 24 bins numpy adds up here, plus one rounding of each division by f_inx
    terms = len(rows) + 24 + 2
    w = rows[:, 8] * rows[:, 7]  # after the division of column 7: weight * sln_prob / f_inx
    for s in (0, 1):
        tot_abs = np.abs(w[rows[:, 1] == s]).sum()
        bound = 2 * terms * U * tot_abs
        # (the flux itself is a weighted device histogram: two runs agree to the order of its adds)
        assert np.all(np.abs(info["flux"][s] - info0["flux"][s]) <= bound), s
        assert np.all(np.abs(sky[s].sum(axis=(0, 2)) - info["flux"][s]) <= bound), s
        assert abs(sky[s].sum() - info["sum_weight_sln_prob"][s]) <= bound, s
    assert sky[1].sum() > 0
    # the Δω range was the rows' (min, max): numpy's edges
    te, pe, de = info["sky_map_edges"]
    assert np.array_equal(de, np.linspace(rows[:, 12].min(), rows[:, 12].max(), 4))
    # the file beside the npy
    npy = list((tmp_path / "npy").glob("tree_*.npy"))
    z = list((tmp_path / "npy").glob("skymap_*.npz"))
    assert len(npy) == 1 and len(z) == 1 and z[0].name == "skymap_" + npy[0].stem + ".npz"
    with np.load(z[0]) as f:
        assert np.array_equal(f["sky_map"], sky) and str(f["theta_axis"]) == "cos" and int(f["f_inx"]) == info["f_inx"]
        for k, e in zip(("theta_edges", "phi_edges", "dw_edges"), (te, pe, de)):
            assert np.array_equal(f[k], e)
    # pulse profiles: finite, and the rows weighted by their solid angle give back the photon total
    omega = (2.0 / 8) * (2 * np.pi / 50)
    total = 0.0
    for c in 0.5 * (te[:-1] + te[1:]):
        prof, phi = pulse_profile(sky, np.arccos(c), "cos")
        assert prof.shape == (50,) and np.all(np.isfinite(prof)) and phi.shape == (50,)
        total += prof.sum() * omega
    assert total == pytest.approx(sky[1].sum(), rel=1e-13)
