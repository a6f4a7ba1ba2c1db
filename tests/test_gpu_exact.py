"""Exact tables on the GPU (art_exact_histogram_device, art_exact_finish_device, art_event_exact_device,
Engine.event_exact, run_events(exact=True), main_runner_tree(exact=True); DESIGN.md §3, "Exact tables") against the
oracle float(sum(map(Fraction, values))) and trees.rows_exact on the rows that Engine.event_rows and run_events return.

An exact table has no tolerance: every comparison of exact tables and of limbs is bit for bit -- across the two
accumulation paths, permutations, chunk sizes, event_offset splits and ranks. The float tables are compared with the
exact ones by the bound the other weighted-table tests use between two float sums, |a - b| <= 2 (cnt + 1) u S with
u = 2^-53 and S the bin's sum of non-negative powers (Higham §4.2); the exact sum is one more ordering's limit, so the
bound holds against it with room.

The sky maps here bin θ itself (theta_axis="theta"): the device then bins column 2 of the row it writes, and
trees.rows_exact bins the same number, so the labels are equal by construction (with the cos θ axis the host takes
np.cos of column 2, which may differ from the device's kz / |k| in the last bit at a bin edge).

ART_PARITY_REPORT=path collects the JSON lines the tests print."""
import json
import math
import os
import socket
from fractions import Fraction

import numpy as np
import pytest

from conftest import CONFIGS
from test_gpu_event_moments import _synthetic_forest
from test_gpu_event_rows import SEED, _engine, _run

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
NBINS = 50
LIMBS = 66


def _report(what, **vals):
    line = json.dumps({"test": "exact", "what": what, **vals})
    print(line)
    if os.environ.get("ART_PARITY_REPORT"):
        with open(os.environ["ART_PARITY_REPORT"], "a") as fh:
            fh.write(line + "\n")


def oracle(values):
    s = sum(map(Fraction, values))
    try:
        return float(s)
    except OverflowError:
        return math.inf if s > 0 else -math.inf


def _same(a, b):
    return np.asarray(a, np.float64).tobytes() == np.asarray(b, np.float64).tobytes()


def _within(what, flt, exact, cnt):
    """a float table against the exact one: the module docstring's bound per entry; the largest measured / bound"""
    flt, exact, cnt = (np.asarray(v, np.float64).reshape(-1) for v in (flt, exact, cnt))
    assert flt.shape == exact.shape == cnt.shape and np.all(exact >= 0), what
    err, bound = np.abs(flt - exact), 2 * (cnt + 1) * U * np.maximum(flt, exact)
    f = (cnt > 0) & (bound > 0)
    ratio = float(np.max(err[f] / bound[f])) if f.any() else 0.0
    _report(what, bound_ratio_max=ratio, filled=int((cnt > 0).sum()), differ=int((flt != exact).sum()))
    assert np.all(err <= bound), (what, ratio)
    assert np.all(flt[cnt == 0] == 0) and np.all(exact[cnt == 0] == 0), what
    return ratio


def _counts(rows, sky):
    """the rows per bin of every table: rows_exact of the same rows with unit powers"""
    from adiabatic_raytracer_amd import trees as T
    unit = np.array(rows, np.float64)
    unit[:, 7] = unit[:, 8] = 1.0
    return T.rows_exact(unit, NBINS, sky)


# ---- 1. art_exact_histogram_device on the adversarial sets

def _adversarial():
    """(values, bins) of 4096 items: three bins of sets whose float sums depend on the order, padded with skipped items"""
    rng = np.random.default_rng(1769)
    bulk = 10.0 ** rng.uniform(-300, 300, 600) * rng.choice([-1.0, 1.0], 600)
    big = float.fromhex("0x1.fffffffffffffp+1023")
    sets = [[1e308, 1.0, -1e308, 2.0 ** 53, 1.0, 1.0] + bulk[:300].tolist(),
            [2.0 ** 53, 3.0, 5e-324, 5e-324, 5e-324, math.ldexp(1.0, -1022) - 5e-324, 5e-324, 1.5, -1.5] + bulk[300:].tolist(),
            [1.7e308, 1.7e308, -1.7e308, -big, big] + [float.fromhex("0x1.fffffffffffffp+0")] * 700]
    values = np.concatenate([np.asarray(s) for s in sets])
    bins = np.concatenate([np.full(len(s), b, np.int32) for b, s in enumerate(sets)])
    pad = 4096 - len(values)
    assert pad > 1000
    values = np.concatenate([values, 10.0 ** rng.uniform(-300, 300, pad)])
    bins = np.concatenate([bins, np.where(rng.random(pad) < 0.5, -1, 3).astype(np.int32)])  # skipped: -1 and out of range
    return values, bins, [oracle(s) for s in sets]


def test_histogram_adversarial_sets_both_modes_two_permutations():
    import torch
    from adiabatic_raytracer_amd import trees as T
    eng = _engine()
    values, bins, want = _adversarial()
    rng = np.random.default_rng(5)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(eng.device)  # noqa: E731
    runs = []
    for perm in (np.arange(4096), rng.permutation(4096)):
        for mode in ("lds", "global"):
            acc, bad = eng.exact_histogram(up(bins[perm]), up(values[perm]), 3, mode=mode)
            out = eng.exact_round(acc)
            assert bad.item() == 0
            runs.append((acc.cpu().numpy(), out.cpu().numpy()))
    for acc, out in runs:
        assert np.array_equal(acc, runs[0][0]) and _same(out, want), (out, want)
        assert np.all((acc[:, :-1] >= 0) & (acc[:, :-1] < 2 ** 32))  # normalised
    # the host twins give the same limbs and the same doubles
    host, _ = T.exact_add(values, bins, 3)
    assert np.array_equal(host, runs[0][0]) and _same(T.exact_round(host), want)
    keep = (bins >= 0) & (bins < 3)
    assert not _same(np.bincount(bins[keep], weights=values[keep], minlength=3), want)  # (a float sum does not)
    # accumulated into, and finishing does not consume: the same items again double every sum
    acc, bad = eng.exact_histogram(up(bins), up(values), 3, mode="auto")
    again, _ = eng.exact_histogram(up(bins), up(values), 3, acc=acc.clone(), nonfinite=bad, mode="global")
    assert _same(eng.exact_round(again).cpu().numpy(), [oracle([w, w]) if math.isfinite(w) else w for w in want])
    # NaN and ±inf are counted and leave the bins untouched; in a skipped bin they are not even looked at
    bad_v = np.array([math.nan, math.inf, -math.inf, math.nan, 1.0, math.inf])
    bad_b = np.array([0, 1, 2, 1, 2, -1], np.int32)
    for mode in ("lds", "global"):
        acc2, cnt = eng.exact_histogram(up(bad_b), up(bad_v), 3, acc=acc.clone(), mode=mode)
        ref, _ = T.exact_add([1.0], [2], 3, acc=acc.cpu().numpy().copy())
        assert cnt.item() == 4 and np.array_equal(acc2.cpu().numpy(), ref)
    # more than the 124 bins the LDS path holds, more than one block per path, an odd size
    n, nb = 70001, 1000
    v = 10.0 ** rng.uniform(-30, 30, n) * rng.choice([-1.0, 1.0], n)
    b = rng.integers(-1, nb + 1, n).astype(np.int32)
    acc, _ = eng.exact_histogram(up(b), up(v), nb)
    assert np.array_equal(acc.cpu().numpy(), T.exact_add(v, b, nb)[0])
    b124 = (b % 124).astype(np.int32)
    accs = [eng.exact_histogram(up(b124), up(v), 124, mode=m)[0].cpu().numpy() for m in ("auto", "lds", "global")]
    assert np.array_equal(accs[0], accs[1]) and np.array_equal(accs[0], accs[2]) and np.array_equal(accs[0], T.exact_add(v, b124, 124)[0])
    with pytest.raises(Exception, match="124"):
        eng.exact_histogram(up(b), up(v), 125, mode="lds")


# ---- 2. the synthetic forest with non-integer powers: event_exact against rows_exact of event_rows' rows

SKY = dict(n_theta=6, n_phi=11, n_dw=4, theta_axis="theta", dw_range=(-2e-6, 2e-6))


def _fractional_forest():
    """test_gpu_event_moments' synthetic forest with powers that are not integers"""
    parts, nd, recs = _synthetic_forest()
    s, w5, back, fwd = parts
    rng = np.random.default_rng(42)
    nd = nd.copy()
    nd["weight"] = nd["weight"] * 10.0 ** rng.uniform(-9, 3, len(nd))
    w5 = w5.clone()
    w5[2] *= 0.1
    return (s, w5, back, dict(fwd, nodes=recs(nd))), nd


def test_synthetic_forest_equals_rows_exact_in_both_modes():
    from adiabatic_raytracer_amd import trees as T
    eng = _engine()
    parts, nd = _fractional_forest()
    lo = 1003
    er = eng.event_rows(*parts, event_offset=lo, nbins=NBINS, sky=SKY)
    rows = er["rows"].cpu().numpy()
    pps = rows[:, 8] * rows[:, 7]
    assert len(rows) == (nd["is_final"] != 0).sum() > 100 and not np.array_equal(pps, np.rint(pps))
    ref = T.rows_exact(rows, NBINS, SKY)
    cnt = _counts(rows, SKY)
    assert (cnt["flux_raw"] > 1).any() and (cnt["sky_raw"] > 1).any() and cnt["totals_raw"].sum() == len(rows)
    assert cnt["sky_raw"].sum() < len(rows)  # rows no sky bin counts (NaN directions)
    accs = {}
    for mode in ("lds", "global", "auto"):
        acc = eng.event_exact(*parts, event_offset=lo, nbins=NBINS, sky=SKY, mode=mode)
        got = {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in eng.exact_finish(acc).items() if k != "acc"}
        accs[mode] = T.exact_raw(acc)
        for name in ("flux_raw", "sky_raw", "totals_raw"):
            assert got[name].shape == ref[name].shape and np.array_equal(got[name], ref[name]), (mode, name)
        assert got["nonfinite"] == 0 and accs[mode]["misplaced"][0] == 0
        assert _same(T.exact_finish(acc)["flux_raw"], got["flux_raw"])  # the host twin of the finish
    for k in ("flux", "sky", "totals"):
        assert np.array_equal(accs["lds"][k], accs["global"][k]) and np.array_equal(accs["lds"][k], accs["auto"][k]), k
    # the float tables of the same call count the same rows in the same bins: within the float bound of the exact ones
    _within("synthetic_flux", er["flux"].cpu().numpy(), ref["flux_raw"], cnt["flux_raw"])
    _within("synthetic_sky", er["sky_hist"].cpu().numpy(), ref["sky_raw"], cnt["sky_raw"])
    _within("synthetic_totals", er["totals"].cpu().numpy()[2:4], ref["totals_raw"], cnt["totals_raw"])
    # accumulated into: a second call doubles every exact sum, exactly
    twice = eng.event_exact(*parts, event_offset=lo, nbins=NBINS, sky=SKY, acc=eng.event_exact(*parts, event_offset=lo, nbins=NBINS, sky=SKY))
    assert np.array_equal(T.exact_finish(twice)["sky_raw"], 2.0 * ref["sky_raw"])
    # a non-finite power is counted and added nowhere; more than 56 flux bins leave the flux table in HBM
    s, w5, back, fwd = parts
    w5b = w5.clone()
    w5b[2, 7] = math.inf  # sln_prob of the tree of 300 records
    acc = eng.event_exact(s, w5b, back, fwd, event_offset=lo, nbins=64, sky=SKY)
    keep = rows[:, 0] != lo + 8
    assert acc["nonfinite"].item() == (~keep).sum() > 50
    ref64 = T.rows_exact(rows[keep], 64, SKY)
    fin = T.exact_finish(acc)
    for name in ("flux_raw", "sky_raw", "totals_raw"):
        assert np.array_equal(fin[name], ref64[name]), name
    with pytest.raises(Exception, match="56"):
        eng.event_exact(*parts, nbins=64, mode="lds")


# ---- 3. run_events(exact=True): chunk sizes

N = 256
RUN_SKY = dict(n_theta=6, n_phi=11, n_dw=1, theta_axis="theta")


def _exact_run(**kw):
    return _run("flat", N, sky_map=RUN_SKY, exact=True, **kw)


def _tables_equal(a, b, keys=("flux_raw", "sky_raw", "totals_raw", "flux", "sky_map", "sum_weight_sln_prob")):
    import torch
    for k in keys:
        assert torch.equal(a[k], b[k]), k
    for k in ("flux", "sky", "totals"):
        assert torch.equal(a["acc"][k], b["acc"][k]), k


def test_run_events_exact_does_not_depend_on_the_chunk():
    from adiabatic_raytracer_amd import trees as T
    one = _exact_run()
    assert one["n_photon_rows"] > 100
    ref = T.rows_exact(one["rows_raw"], NBINS, RUN_SKY, f_inx=one["f_inx"])
    for chunk in (None, 64, 100):
        r = one if chunk is None else _exact_run(chunk=chunk)
        ex = r["exact"]
        _tables_equal(ex, one["exact"])
        for name in ("flux_raw", "sky_raw", "totals_raw", "flux", "sky_map", "sum_weight_sln_prob"):
            got = ex[name].cpu().numpy()
            assert got.shape == ref[name].shape and np.array_equal(got, ref[name]), (chunk, name)
        assert ex["nonfinite"].item() == 0 and ex["acc"]["misplaced"].item() == 0
        acc = T.exact_raw(ex["acc"])
        assert all(np.all((acc[k][..., :-1] >= 0) & (acc[k][..., :-1] < 2 ** 32)) for k in ("flux", "sky", "totals"))
    # the float tables are what they are without the keyword's work being asked of them, and lie within their bound
    cnt = _counts(one["rows_raw"], RUN_SKY)
    _within("run_flux", one["flux_raw"], ref["flux_raw"], cnt["flux_raw"])
    _within("run_sky", one["sky_raw"], ref["sky_raw"], cnt["sky_raw"])
    _within("run_totals", one["totals"][2:4], ref["totals_raw"], cnt["totals_raw"])


# ---- 4. splitting by event_offset and merging

def test_event_offset_halves_merge_to_the_single_run():
    from adiabatic_raytracer_amd import trees as T
    eng = _engine()
    one = _exact_run()["exact"]
    halves = [eng.run_events(128, seed=SEED, event_offset=lo, sky_map=RUN_SKY, exact=True, rows=False)["exact"]["acc"]
              for lo in (0, 128)]
    want = T.exact_raw(one["acc"])
    for order in (halves, halves[::-1]):
        m = T.exact_merge(order)
        for k in ("flux", "sky", "totals"):
            assert np.array_equal(m[k], want[k]), k
        fin = T.exact_finish(m)
        for name in ("flux_raw", "sky_raw", "totals_raw"):
            assert _same(fin[name], one[name].cpu().numpy()), name


# ---- 5. the scans

def test_scans_exact_do_not_depend_on_the_chunk():
    import torch
    import adiabatic_raytracer_amd as A
    eng = _engine()
    g0 = eng.params.g_agg
    base = A.Halo(220.0, (0.0, 0.0, 0.0), v_prop=300.0)
    models = [base, A.Halo(180.0, (30.0, -20.0, 10.0))]
    kw = dict(seed=SEED, halo=base, halos=models, couplings=[0.5 * g0, g0, 3.0 * g0], sky_map=RUN_SKY, exact=True)
    one = eng.run_events(N, **kw)
    ch = eng.run_events(N, chunk=64, rows=False, **kw)
    for key, K in (("coupling_scan", 3), ("halo_scan", 2)):
        a, b = one[key]["exact"], ch[key]["exact"]
        assert tuple(a["flux_raw"].shape) == (K, 2, NBINS) and tuple(a["sky_raw"].shape) == (K, 2, 6, 11, 1)
        assert tuple(a["totals_raw"].shape) == (K, 2) and tuple(a["acc"]["flux"].shape) == (K, 2 * NBINS, LIMBS)
        _tables_equal(a, b)
        assert a["nonfinite"].sum().item() == 0 and a["totals_raw"][:, 1].min().item() > 0
    _tables_equal(one["exact"], ch["exact"])
    assert not torch.equal(one["coupling_scan"]["exact"]["flux_raw"][0], one["coupling_scan"]["exact"]["flux_raw"][2])
    # the base coupling's and the base model's powers are the run's own but for their roundings: within the float bound
    # of the run's exact flux, with the run's photon rows per bin for the count
    cnt = _counts(one["rows_raw"].cpu().numpy(), RUN_SKY)["flux_raw"].reshape(-1)
    run = one["exact"]["flux_raw"].cpu().numpy()
    for what, got in (("coupling_base", one["coupling_scan"]["exact"]["flux_raw"][1]), ("halo_base", one["halo_scan"]["exact"]["flux_raw"][0])):
        got = got.cpu().numpy().reshape(-1)
        err, bound = np.abs(got - run.reshape(-1)), 2 * (cnt + 1) * U * np.maximum(got, run.reshape(-1))
        _report(what, bound_ratio_max=float(np.max(err[bound > 0] / bound[bound > 0])))
        assert np.all(err <= bound) and run.sum() > 0, what
    # and within the float bound of the scan's own float table
    flt = one["coupling_scan"]["raw"]["flux"][1].reshape(-1)
    got = one["coupling_scan"]["exact"]["flux_raw"][1].cpu().numpy().reshape(-1)
    assert np.all(np.abs(flt - got) <= 2 * (cnt + 1) * U * np.maximum(flt, got))


# ---- 6. the defaults and the cap

def test_exact_false_is_the_call_without_the_keyword():
    import adiabatic_raytracer_amd as A
    eng = _engine()
    base = A.Halo(220.0, (0.0, 0.0, 0.0), v_prop=300.0)
    kw = dict(seed=SEED, halo=base, halos=[base], couplings=[eng.params.g_agg], sky_map=RUN_SKY)
    plain, off, on = eng.run_events(24, **kw), eng.run_events(24, exact=False, **kw), eng.run_events(24, exact=True, **kw)
    assert set(plain) == set(off) and set(on) - set(plain) == {"exact"}
    for key in ("coupling_scan", "halo_scan"):
        assert set(plain[key]) == set(off[key]) and set(on[key]) - set(plain[key]) == {"exact"}
        assert set(plain[key]["raw"]) == set(off[key]["raw"]) == set(on[key]["raw"])
    assert plain["rows"].cpu().numpy().tobytes() == on["rows"].cpu().numpy().tobytes()
    # over the cap: a ValueError before any kernel runs (nothing of the engine is touched)
    big = dict(n_theta=64, n_phi=128, n_dw=16, dw_range=(-1e-6, 1e-6))
    from adiabatic_raytracer_amd.engine import Engine
    with pytest.raises(ValueError, match="exact: the accumulators of the coupling scan"):
        Engine.run_events(eng, 10, couplings=[eng.params.g_agg] * 32, sky_map=big, exact=True)
    with pytest.raises(ValueError, match="exact: the accumulators of the halo scan"):
        Engine.run_events(eng, 10, halo=base, halos=[base] * 32, sky_map=big, exact=True)


# ---- 7. two ranks

N_TRAJS = 41  # 40 events


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, kw, outdir):
    import torch
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import adiabatic_raytracer_amd as A
        info = {}
        A.trees.main_runner_tree(A.Params(**kw), N_TRAJS, device_events=True, exact=True, sky_map=RUN_SKY, rank=rank,
                                 world=world, run_info=info)
        ex = info["exact"]
        np.savez(os.path.join(outdir, f"exact{rank}.npz"), f_inx=info["f_inx"], flux_float=info["flux"],
                 **{k: ex[k] for k in ("flux_raw", "sky_raw", "totals_raw", "flux", "sky_map", "sum_weight_sln_prob")},
                 **{"acc_" + k: ex["acc"][k] for k in ("flux", "sky", "totals")})
    finally:
        dist.destroy_process_group()


def test_two_ranks_equal_one(tmp_path):
    import torch.multiprocessing as mp
    import adiabatic_raytracer_amd as A
    kw = CONFIGS["flat"]
    mp.start_processes(_worker, args=(2, _free_port(), kw, str(tmp_path)), nprocs=2, join=True, start_method="spawn")
    info, plain = {}, {}
    rows = A.trees.main_runner_tree(A.Params(**kw), N_TRAJS, device_events=True, exact=True, sky_map=RUN_SKY, run_info=info)
    A.trees.main_runner_tree(A.Params(**kw), N_TRAJS, device_events=True, sky_map=RUN_SKY, run_info=plain)
    assert set(info) - set(plain) == {"exact"} and info["rows"] == len(rows) > 20
    ex = info["exact"]
    for r in range(2):
        z = np.load(tmp_path / f"exact{r}.npz")
        assert int(z["f_inx"]) == info["f_inx"]
        for k in ("flux_raw", "sky_raw", "totals_raw", "flux", "sky_map", "sum_weight_sln_prob"):
            assert np.array_equal(z[k], ex[k]), k
        for k in ("flux", "sky", "totals"):
            assert np.array_equal(z["acc_" + k], ex["acc"][k]), k
    # and they are run_events' own, of the same events in one chunk on one rank
    one = _engine().run_events(N_TRAJS - 1, seed=SEED, sky_map=RUN_SKY, exact=True)
    assert one["f_inx"] == info["f_inx"]
    for k in ("flux_raw", "sky_raw", "totals_raw", "flux", "sky_map", "sum_weight_sln_prob"):
        assert np.array_equal(one["exact"][k].cpu().numpy(), ex[k]), k
    assert ex["flux_raw"][1].sum() > 0 and ex["nonfinite"] == 0
