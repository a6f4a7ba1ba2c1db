"""The device-resident tree driver (art_grow_trees_device, Engine.grow_trees) against the host
forest (art_grow_trees) in the same process, on the same Philox-sampled roots.

The two forests run the same integrator and probability kernels; they differ in the exp and log of
the bookkeeping only (the device's against glibc's, each within 1 ulp of the true value). So the
first round starts from bit-equal inputs and must give bit-equal segments, with
prob = 1 - exp(-x) within two ulp of a value near 1 (4.5e-16 absolute: 1 - exp(-x) carries exp's
rounding absolutely, so a relative bound would be wrong for small P). Later rounds start from
log(t) a possible ulp apart, and a grazing segment may then flip (test_gpu_trees.py): at least 95%
of the trees must agree in node sequence, count and info, and on those the weights and end points
agree to that file's bound (median <= 1e-8 relative).

Measured on an MI355X (profiles/device_forest_parity.jsonl; ART_PARITY_REPORT=path collects the
lines the tests print): root round bit-equal, prob within 1.2e-16; full and Monte-Carlo trees 48 of 48,
relative differences <= 1e-15; every stop-rule set 48 of 48; the GR backtrace equal in every field;
main_runner_tree rows 48 of 48 events equal."""
import ctypes as C
import json
import os
from dataclasses import replace

import numpy as np
import pytest

from conftest import CONFIGS

pytestmark = pytest.mark.gpu

AXION, PHOTON = 0, 1
N = 48
TWO_ULP_NEAR_ONE = 4.5e-16
EXACT = ("tree", "species", "is_final", "n_cross", "status", "x0", "k0", "t0", "dw0", "x_end", "k_end", "u7_end",
         "tau_end", "xc", "kc", "tc", "dwc")

_cache = {}


def _roots(cfg, n, **over):
    """(params, sample) of n roots, seed 1769 (the sampler is the product's; test_gpu_sampler.py holds it
    to the oracle)."""
    import adiabatic_raytracer_amd as A
    key = ("roots", cfg, n, tuple(sorted(over.items())))
    if key not in _cache:
        p = A.Params(**{**CONFIGS[cfg], **over})
        _cache[key] = (p, A.sample_conversion_points(p, n, seed=1769))
    return _cache[key]


def _host(cfg, n, over=(), **kw):
    """The host forest of the roots, computed once per option set and left unchanged."""
    import adiabatic_raytracer_amd as A
    key = ("host", cfg, n, tuple(over), tuple(sorted(kw.items())))
    if key not in _cache:
        p, s = _roots(cfg, n, **dict(over))
        nodes, counts, infos = A.trees.grow_trees(p, s["x"], s["k_init"], s["erg"], PHOTON, **kw)
        for a in (nodes, counts, infos):
            a.setflags(write=False)
        _cache[key] = (nodes, counts, infos)
    return _cache[key]


def _device(p, x, k, erg, species, lo=0, hi=None, **kw):
    """Engine.grow_trees on roots [lo, hi) of SoA arrays; numpy results."""
    import torch
    from adiabatic_raytracer_amd.engine import Engine, nodes_to_numpy
    n = erg.size
    hi = n if hi is None else hi
    eng = Engine(p)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(eng.device)  # noqa: E731
    sl = lambda a: np.asarray(a).reshape(3, n)[:, lo:hi].reshape(-1)  # noqa: E731
    sp = np.full(hi - lo, species, np.int8)
    r = eng.grow_trees(up(sl(x)), up(sl(k)), up(erg[lo:hi]), up(sp), **kw)
    return (nodes_to_numpy(r["nodes"]), r["counts"].cpu().numpy(), r["infos"].cpu().numpy(),
            r["node_start"].cpu().numpy(), r["n_nodes"])


def _report(what, **vals):
    line = json.dumps({"test": "device_forest", "what": what, **vals})
    print(line)
    if os.environ.get("ART_PARITY_REPORT"):
        with open(os.environ["ART_PARITY_REPORT"], "a") as fh:
            fh.write(line + "\n")


def _agreement(what, gn, gc, gi, gs, hn, hc, hi, n):
    """Trees with the host forest's node sequence, count and info, and on those the relative
    differences of weights and end points."""
    assert np.array_equal(gs, np.concatenate([[0], np.cumsum(gc.astype(np.int64))])) and gs[-1] == len(gn)
    h_start = np.concatenate([[0], np.cumsum(hc.astype(np.int64))])
    same, rel = 0, []
    for i in range(n):
        g, h = gn[gs[i]:gs[i + 1]], hn[h_start[i]:h_start[i + 1]]
        assert np.all(g["tree"] == i) and np.all(g["pad"] == 0)
        sig = lambda a: list(zip(a["species"].tolist(), a["is_final"].tolist(), a["n_cross"].tolist()))  # noqa: E731
        if sig(g) == sig(h) and gc[i] == hc[i] and gi[i] == hi[i]:
            same += 1
            rel.extend(np.abs(g["weight"] - h["weight"]) / np.abs(h["weight"]))
            rel.extend(np.abs(g["x_end"] - h["x_end"]).max(1) / np.linalg.norm(h["x_end"], axis=1))
    _report(what, same_trees=same, n=n, rel_p50_p90_max=np.percentile(rel, [50, 90, 100]).tolist(),
            rounds=int(gc.max()), batch_sum=int(len(gn)))
    return same, np.asarray(rel)


def test_root_round_is_bit_equal_flat_65():
    n = 65  # one more than a wave
    p, s = _roots("flat", n)
    hn, hc, _ = _host("flat", n)
    gn, gc, gi, gs, total = _device(p, s["x"], s["k_init"], s["erg"], PHOTON)
    assert total == len(gn) == gs[-1]
    g0, h0 = gn[gs[:-1]], hn[np.concatenate([[0], np.cumsum(hc.astype(np.int64))])[:-1]]
    for f in EXACT:
        assert np.array_equal(g0[f], h0[f], equal_nan=True), f
    d_prob, d_pc = np.abs(g0["prob"] - h0["prob"]).max(), np.abs(g0["pc"] - h0["pc"]).max()
    _report("root_round", n=n, prob_abs=float(d_prob), pc_abs=float(d_pc))
    assert d_prob <= TWO_ULP_NEAR_ONE and d_pc <= TWO_ULP_NEAR_ONE
    assert np.array_equal(g0["weight"], h0["weight"]) and (g0["n_cross"] > 0).any() and (g0["n_cross"] == 0).any()


@pytest.mark.parametrize("mode", ["full", "mc"])
def test_forward_trees_match_host_forest(mode):
    over = () if mode == "full" else (("g_agg", 1e-11),)
    kw = dict(num_cutoff=5, mc_nodes=1000 if mode == "full" else 2, max_nodes=50, prob_cutoff=1e-10, seed=1769)
    p, s = _roots("flat", N, **dict(over))
    hn, hc, hi = _host("flat", N, over, **kw)
    gn, gc, gi, gs, _ = _device(p, s["x"], s["k_init"], s["erg"], PHOTON, **kw)
    same, rel = _agreement(f"forward_{mode}", gn, gc, gi, gs, hn, hc, hi, N)
    assert same >= 0.95 * N, (same, N)
    assert np.median(rel) <= 1e-8, np.percentile(rel, [50, 90, 100])
    if mode == "mc":
        assert (hi < 0).sum() >= 10  # the Monte-Carlo branch is what these trees exercise


def test_bushy_trees_grow_the_node_log():
    """Full splitting at P ~ 0.03-0.95 for up to 21 rounds: far more than the three nodes per tree the
    driver's node log starts with (it doubles, keeping what earlier rounds wrote), stacks 22 deep."""
    over = (("g_agg", 1e-11),)
    kw = dict(num_cutoff=50, mc_nodes=1000, max_nodes=20)
    p, s = _roots("flat", N, **dict(over))
    hn, hc, hi = _host("flat", N, over, **kw)
    assert len(hn) > 3 * N, len(hn)  # (the log starts at 3 records per tree)
    gn, gc, gi, gs, _ = _device(p, s["x"], s["k_init"], s["erg"], PHOTON, **kw)
    same, rel = _agreement("bushy", gn, gc, gi, gs, hn, hc, hi, N)
    assert same >= 0.95 * N, (same, N)
    assert np.median(rel) <= 1e-8, np.percentile(rel, [50, 90, 100])


def test_rounds_beyond_the_small_batch_path():
    """1100 roots: the first rounds hold more segments than the one-wave-per-ray path takes (one per
    SIMD, 1024), so they run on the persistent integrator, later ones on the small-batch path."""
    n = 1100
    p, s = _roots("flat", n)
    hn, hc, hi = _host("flat", n)
    gn, gc, gi, gs, _ = _device(p, s["x"], s["k_init"], s["erg"], PHOTON)
    same, rel = _agreement("n1100", gn, gc, gi, gs, hn, hc, hi, n)
    assert same >= 0.95 * n, (same, n)
    assert np.median(rel) <= 1e-8, np.percentile(rel, [50, 90, 100])


@pytest.mark.parametrize("name,kw,code", [
    ("num_cutoff", dict(num_cutoff=1), 3),
    ("max_nodes", dict(max_nodes=3, num_cutoff=50, mc_nodes=1000), 4),
    ("prob_cutoff", dict(prob_cutoff=0.5), 2),
])
def test_stop_rules(name, kw, code):
    p, s = _roots("flat", N)
    hn, hc, hi = _host("flat", N, (), **kw)
    assert code in np.abs(hi), (code, sorted(set(hi.tolist())))
    gn, gc, gi, gs, _ = _device(p, s["x"], s["k_init"], s["erg"], PHOTON, **kw)
    ok = int(np.sum((gc == hc) & (gi == hi)))
    _report(f"stop_{name}", same_trees=ok, n=N, infos=sorted(set(gi.tolist())))
    assert ok >= 0.95 * N, (ok, N)


def test_split_invariance():
    """One call on 48 roots equals two calls on roots 0..23 and 24..47 with tree_offset 0 and 24."""
    kw = dict(mc_nodes=2, seed=1769)
    p, s = _roots("flat", N, g_agg=1e-11)
    whole = _device(p, s["x"], s["k_init"], s["erg"], PHOTON, **kw)
    a = _device(p, s["x"], s["k_init"], s["erg"], PHOTON, 0, 24, tree_offset=0, **kw)
    b = _device(p, s["x"], s["k_init"], s["erg"], PHOTON, 24, 48, tree_offset=24, **kw)
    assert np.array_equal(whole[1], np.concatenate([a[1], b[1]])) and np.array_equal(whole[2], np.concatenate([a[2], b[2]]))
    bn = b[0].copy()
    bn["tree"] += 24
    parts = np.concatenate([a[0], bn])
    assert whole[0].tobytes() == parts.tobytes()
    assert (whole[2] < 0).any()


def test_backtrace_form_gr():
    """main_runner_tree's backtrace: axion, -k, -B0, every crossing up to the cap, the root only."""
    import adiabatic_raytracer_amd as A
    p, s = _roots("gr", N)
    pb = replace(p, B0=-p.B0)
    kw = dict(num_cutoff=0, splittings_cutoff=100000, crossing_cap=256)
    x, k = s["x"], -s["k_init"]
    hn, hc, hi = A.trees.grow_trees(pb, x, k, s["erg"], AXION, **kw)
    gn, gc, gi, gs, total = _device(pb, x, k, s["erg"], AXION, **kw)
    assert total == N == len(hn) and np.all(gc == 1) and np.array_equal(gc, hc) and np.array_equal(gi, hi)
    for f in ("n_cross", "status", "x_end", "xc", "species", "is_final", "k_end", "u7_end", "tau_end", "kc", "tc", "dwc"):
        assert np.array_equal(gn[f], hn[f], equal_nan=True), f
    rel_w = np.abs(gn["weight"] - hn["weight"]) / np.abs(hn["weight"])
    d_prob = np.abs(gn["prob"] - hn["prob"]).max()
    _report("backtrace", n=N, n_cross_max=int(gn["n_cross"].max()), grouped=int((gn["n_cross"] >= 2).sum()),
            weight_rel_max=float(rel_w.max()), prob_abs=float(d_prob))
    assert rel_w.max() <= 1e-12  # at most 256 factors, each off by at most two ulp
    assert d_prob <= TWO_ULP_NEAR_ONE
    assert (gn["n_cross"] >= 2).any()


def test_edges():
    import torch
    from adiabatic_raytracer_amd import _lib
    from adiabatic_raytracer_amd.engine import Engine, nodes_to_numpy
    from adiabatic_raytracer_amd.trees import NODE_DTYPE
    p, s = _roots("flat", N)
    eng = Engine(p)
    # no roots: no nodes, ART_OK
    e = eng.empty(0)
    r0 = eng.grow_trees(e, e, e, eng.empty(0, dtype=torch.int8))
    assert r0["n_nodes"] == 0 and r0["nodes"].numel() == 0 and r0["node_start"].tolist() == [0]
    # one root
    one = _device(p, s["x"], s["k_init"], s["erg"], PHOTON, 0, 1)
    hn, hc, hi = _host("flat", N)
    assert one[4] == len(one[0]) == one[1][0] and one[3].tolist() == [0, one[4]]
    assert one[1][0] == hc[0] and one[2][0] == hi[0]
    # a capacity one short: ART_E_NOMEM with the exact count and nothing written; the retry succeeds
    full = _device(p, s["x"], s["k_init"], s["erg"], PHOTON)
    total = full[4]
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt)).to(eng.device)  # noqa: E731
    x, k, erg = up(s["x"], np.float64), up(s["k_init"], np.float64), up(s["erg"], np.float64)
    sp = torch.ones(N, dtype=torch.int8, device=eng.device)
    nodes = torch.zeros(total - 1, NODE_DTYPE.itemsize, dtype=torch.uint8, device=eng.device)
    opts = _lib.TreeOpts(5, 5, 50, -1, 64, 0, 1e-10, 1769)
    nn = C.c_int64(0)
    ptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    torch.cuda.synchronize()
    rc = eng.lib.art_grow_trees_device(C.byref(eng.cp), N, ptr(x), ptr(k), ptr(erg), ptr(sp), C.byref(opts), total - 1,
                                       ptr(nodes), None, None, None, C.byref(nn), None)
    assert rc == -3 and nn.value == total and not nodes.any()
    short = eng.grow_trees(x, k, erg, sp, node_capacity=total - 1)
    assert short["n_nodes"] == total and nodes_to_numpy(short["nodes"]).tobytes() == full[0].tobytes()
    # a stream of the caller's
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        r = eng.grow_trees(x, k, erg, sp)
    side.synchronize()
    assert nodes_to_numpy(r["nodes"]).tobytes() == full[0].tobytes()
    assert np.array_equal(r["counts"].cpu().numpy(), full[1]) and np.array_equal(r["node_start"].cpu().numpy(), full[3])


def test_main_runner_tree_device_trees():
    import adiabatic_raytracer_amd as A
    p = A.Params(**CONFIGS["flat"])
    info_d, info_h = {}, {}
    ref = A.trees.main_runner_tree(p, N + 1, saveMode=1, run_info=info_h)
    rows = A.trees.main_runner_tree(p, N + 1, saveMode=1, run_info=info_d, device_trees=True)
    assert set(info_d) == set(info_h)
    ev_g, ev_o = rows[:, 0], ref[:, 0]
    same, rel = 0, []
    cols = (2, 3, 4, 5, 6, 8, 9, 10, 11, 12, 16, 17, 18, 19, 21, 22, 23, 24, 25)  # independent of f_inx
    for e in range(1, N + 1):
        g, o = rows[ev_g == e], ref[ev_o == e]
        if g.shape == o.shape and np.array_equal(g[:, 1], o[:, 1]):
            same += 1
            d = np.abs(g[:, cols] - o[:, cols]) / np.maximum(np.abs(o[:, cols]), 1e-12)
            rel.extend(d.reshape(-1))
    rel = np.asarray(rel)
    _report("main_runner_rows", same_events=same, n=N, rel_p50_p90_max=np.percentile(rel, [50, 90, 100]).tolist())
    assert same >= 0.9 * N, same
    assert np.median(rel) <= 1e-8 and np.mean(rel <= 1e-6) >= 0.9, np.percentile(rel, [50, 90, 99, 100])
