"""The coupling scan on the GPU (art_event_reweight_device, Engine.event_reweight, run_events(couplings=),
main_runner_tree(device_events=True, couplings=)): forests grown on the flat configuration at g0 = 1e-11,
where pc spans 0.04 to nearly 1 and some default trees go Monte-Carlo (one case at 2e-11, where some pc are
exactly 1.0), reweighted and held against the stored weights (s = 1), against trees.reweight_nodes in numpy
with x from Engine.get_prob_nonad, and against direct runs at the target couplings.

Bounds, u = 2^-53:
  δ     the largest relative difference between 1 - fexp(-x0), x0 recomputed from the stored crossing by
        Engine.get_prob_nonad and fexp by Engine.eval_math, and the stored pc (the parent commit's in-kernel
        value). Measured on an MI355X (profiles/coupling_scan_parity.jsonl): DELTA_MEASURED below; the tests
        use D = max(4 δ, 2u) and re-measure it.
  chain Σ over a record's ancestors' crossings of (2 + s x_i) (D + 2u): each factor 1 - exp(-s x) carries
        the relative error of its exponent damped by x e^-x / (1 - e^-x) <= 1, each factor exp(-s x)
        carries s x times it, plus the roundings. The direct run forms the unconverted factor as 1 - P,
        whose ABSOLUTE error is u/2 whatever its size, while the reweight takes exp(-s x) itself: so tree
        weights are compared on the scale of the root's weight 1, |ΔW| <= chain. Columns 25 and 28 are
        probabilities on the same unit scale and take their chain's sum as it is written, absolute: the
        root's crossing for column 28, and for column 25 also the backtrace's n_cross crossings, whose
        exponents sum to |ln bweight|
        (1 - exp(-y) of two exponents a few ulp apart may differ by an ulp of exp(-y), which is
        u / (e^y - 1) relative to it); column 8 = W back: |Δ| <= chain column 25 + column 25's bound.
  pow   bweight^s through exp(s log w): (1 + s |ln w|) 4u relative (column 25, and through it column 8).
  adds  a table bin is a sum of the same terms in another order: 2 (terms + 1) u Σ|w|
        (tests/test_gpu_event_rows.py); to it the terms' own bounds are added where the terms differ.
  numpy W against trees.reweight_nodes: the CPU test's (depth + 2) 4u (1 + s x_max) relative.
ART_PARITY_REPORT=path collects the JSON lines the tests print. Measured on an MI355X
(profiles/coupling_scan_parity.jsonl; DESIGN.md §3, "Coupling scan"): δ = 0, every one of 1547 (1e-11) and
1514 (2e-11) crossings, 1100 roots and 903 single backtrace crossings bit-equal, pc from 0.010 to exactly 1.0
(5 and 10 crossings), 162 Monte-Carlo trees with 404 drawn children; W at s = 1 bit-equal to the stored weight
on 96 % of 3763 records, the rest at most 0.05 of the bound; W against numpy at most 0.04 of the bound, tables
0.19; against direct runs 41-42 of 42 and 211-216 of 217 events compared, column 28 bit-equal, columns 8 and
25 at most 0.02 of their bound from 1e-11 and 0.2 from 2e-11; chunks 0.0007; σ per coupling at most 0.17 of
the bound on V; the photon total at 2e-11 from 1e-11 0.03 combined σ from the direct run's."""
import json
import os
from dataclasses import replace

import numpy as np
import pytest

from test_gpu_event_moments import _bound as _moment_bound
from test_gpu_event_moments import _groups
from test_gpu_event_rows import SEED, U, _np, _params

pytestmark = pytest.mark.gpu

AXION, PHOTON = 0, 1
N, NBINS = 1100, 50
G0 = 1e-11
SKY = dict(n_theta=6, n_phi=11, n_dw=1)
FULL = dict(num_cutoff=1000, MC_nodes=1000, max_nodes=60)  # no Monte-Carlo branches
DELTA_MEASURED = 0.0  # MI355X, profiles/coupling_scan_parity.jsonl ("delta")
D = max(4.0 * DELTA_MEASURED, 2.0 * U)

_cache = {}


def _report(what, **vals):
    line = json.dumps({"test": "event_reweight", "what": what, **vals})
    print(line)
    if os.environ.get("ART_PARITY_REPORT"):
        with open(os.environ["ART_PARITY_REPORT"], "a") as fh:
            fh.write(line + "\n")


def _eng(g=G0):
    from adiabatic_raytracer_amd.engine import Engine
    if ("eng", g) not in _cache:
        p = replace(_params("flat"), g_agg=g)
        _cache[("eng", g)] = (Engine(p), Engine(replace(p, B0=-p.B0)))
    return _cache[("eng", g)]


def _pipe(g, lo, c, **tree):
    """run_events' steps for events [lo, lo + c) at base coupling g: (sample, weight5, back, forward), mc_nodes"""
    key = ("pipe", g, lo, c, tuple(sorted(tree.items())))
    if key not in _cache:
        eng, beng = _eng(g)
        s = eng.sample(c, seed=SEED, ray_offset=lo)
        w5 = eng.event_weight(s)
        back = beng.grow_trees(s["x"], -s["k_init"], s["erg"], AXION, num_cutoff=0, splittings_cutoff=100000,
                               crossing_cap=256, seed=SEED, tree_offset=lo)
        kw = dict(num_cutoff=tree.get("num_cutoff", 5), mc_nodes=tree.get("MC_nodes", 5), max_nodes=tree.get("max_nodes", 50))
        fwd = eng.grow_trees(s["x"], s["k_init"], s["erg"], PHOTON, seed=SEED, tree_offset=lo, **kw)
        _cache[key] = ((s, w5, back, fwd), kw["mc_nodes"])
    return _cache[key]


def _pulled(g, lo, c, **tree):
    """the forest on the host: nodes, node_start, x (P_nonAD at g of every stored crossing, by get_prob_nonad),
    x_root, the back nodes, erg, parents and depths"""
    import torch
    from adiabatic_raytracer_amd.engine import nodes_to_numpy
    key = ("pulled", g, lo, c, tuple(sorted(tree.items())))
    if key in _cache:
        return _cache[key]
    (s, w5, back, fwd), mc = _pipe(g, lo, c, **tree)
    eng, beng = _eng(g)
    nodes, start = nodes_to_numpy(fwd["nodes"]), fwd["node_start"].cpu().numpy()
    erg = s["erg"].cpu().numpy()
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(eng.device)  # noqa: E731
    x = np.zeros(len(nodes))
    cr = np.flatnonzero(nodes["n_cross"] > 0)
    if len(cr):
        eff = erg[nodes["tree"][cr]] * np.abs(nodes["dwc"][cr])
        x[cr] = eng.get_prob_nonad(up(nodes["xc"][cr].T.reshape(-1)), up(nodes["kc"][cr].T.reshape(-1)), up(eff)).cpu().numpy()
    x_root = beng.get_prob_nonad(s["x"], -s["k_init"], s["erg"]).cpu().numpy()
    bk = nodes_to_numpy(back["nodes"])
    x_single = np.full(c, np.nan)  # the exponent of a backtrace's crossing where it has exactly one
    one = np.flatnonzero((bk["n_cross"] == 1) & (bk["weight"] != 0.0) & (bk["weight"] != 1.0))
    if len(one):
        x_single[one] = beng.get_prob_nonad(up(bk["xc"][one].T.reshape(-1)), up(bk["kc"][one].T.reshape(-1)),
                                            up(erg[one] * np.abs(bk["dwc"][one]))).cpu().numpy()
    # parents and depths, by the rule of trees.reweight_nodes
    bits = lambda v: np.ascontiguousarray(v).view(np.uint64)  # noqa: E731
    own = np.c_[bits(nodes["t0"]), bits(nodes["x0"]).reshape(-1, 3)]
    cross = np.c_[bits(nodes["tc"]), bits(nodes["xc"]).reshape(-1, 3)]
    parent, depth = np.full(len(nodes), -1), np.zeros(len(nodes), np.int64)
    for t in range(len(start) - 1):
        a = int(start[t])
        for j in range(a + 1, int(start[t + 1])):
            cand = a + np.flatnonzero((nodes["n_cross"][a:j] > 0) & np.all(cross[a:j] == own[j], axis=1))
            assert len(cand) == 1
            parent[j], depth[j] = cand[0], depth[cand[0]] + 1
    out = dict(nodes=nodes, start=start, x=x, x_root=x_root, x_single=x_single, back=bk, erg=erg, parent=parent,
               depth=depth, mc=mc, sln=w5[2].cpu().numpy(), up=up)
    _cache[key] = out
    return out


def _chain(P, s):
    """Σ over each record's ancestors' crossings of (2 + s x_i) (D + 2u)"""
    ch = np.zeros(len(P["nodes"]))
    for j in range(len(ch)):  # (a parent precedes its children)
        p = P["parent"][j]
        if p >= 0:
            ch[j] = ch[p] + (2.0 + s * P["x"][p]) * (D + 2 * U)
    return ch


def _back_bound(P, s, prob_only=False):
    """per event: (the backtrace's chain, absolute on the unit scale; bweight^s, relative). The chain of
    column 28 is the root's crossing alone; column 25's also holds the backtrace's n_cross crossings, whose
    factors 1 - P_q made the stored bweight and whose exponents sum to |ln bweight|."""
    if prob_only:
        return (2.0 + s * P["x_root"]) * (D + 2 * U)
    lw = np.abs(np.log(np.where(P["back"]["weight"] > 0, P["back"]["weight"], 1.0)))
    chain = 2.0 * (1 + P["back"]["n_cross"]) + s * (P["x_root"] + lw)
    return chain * (D + 2 * U), (0.0 if s == 1.0 else 1.0) * (1.0 + s * lw) * 4 * U


def _d_back(P, s, back):
    """|Δ(bprob bweight^s)| <= Δbprob bweight^s + bprob Δ(bweight^s) <= abs + rel back"""
    ab, rl = _back_bound(P, s)
    return ab + rl * back


def _scan(g, lo, c, couplings, tree=None, **kw):
    (parts, mc) = _pipe(g, lo, c, **(tree or {}))
    return _eng(g)[0].event_reweight(*parts, couplings, mc_nodes=mc, event_offset=lo, nbins=NBINS, **kw)


def _host(scan):
    import torch
    return {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in scan.items()}


# ---- 0. δ: the recomputed 1 - fexp(-x0) against the stored pc, and the kernel's own count

def test_delta_of_the_recomputed_probability():
    for g in (G0, 2e-11):
        P = _pulled(g, 0, N)
        eng = _eng(g)[0]
        cr = np.flatnonzero(P["nodes"]["n_cross"] > 0)
        e = eng.eval_math("EXP", P["up"](-P["x"][cr])).cpu().numpy()
        pc, mine = P["nodes"]["pc"][cr], 1.0 - e
        rel = np.abs(mine - pc) / np.abs(pc)
        er = eng.eval_math("EXP", P["up"](-P["x_root"])).cpu().numpy()
        bp = P["back"]["prob"]
        relb = np.abs((1.0 - er) - bp)[bp > 0] / bp[bp > 0]
        delta = float(max(rel.max(), relb.max() if relb.size else 0.0))
        sc = _host(_scan(g, 0, N, [g]))
        differs = int(sc["totals"][0, 5])
        _report("delta", g0=g, delta=delta, crossings=int(len(cr)), bit_equal_share=float(np.mean(mine == pc)),
                root_bit_equal_share=float(np.mean((1.0 - er) == bp)), kernel_recomputed_differs=differs,
                single_crossing_backtraces=int((~np.isnan(P["x_single"])).sum()),
                pc_min=float(pc.min()), pc_max=float(pc.max()), pc_exactly_1=int((pc == 1.0).sum()),
                monte_carlo_trees=int((_pipe(g, 0, N)[0][3]["infos"].cpu().numpy() < 0).sum()))
        assert delta <= D / 4, delta  # the docstring's δ holds here
        # the kernel counts exactly the values this test finds not bit-equal
        one = ~np.isnan(P["x_single"])
        es = eng.eval_math("EXP", P["up"](-P["x_single"][one])).cpu().numpy()
        assert differs == int((mine != pc).sum() + ((1.0 - er) != bp).sum() + ((1.0 - es) != P["back"]["pc"][one]).sum())


# ---- 1. identity: couplings = [g0]

def test_identity_at_the_base_coupling():
    (parts, mc) = _pipe(G0, 0, N)
    eng = _eng(G0)[0]
    P = _pulled(G0, 0, N)
    er = eng.event_rows(*parts, nbins=NBINS, sky=SKY, return_bins=True)
    sc = _host(_scan(G0, 0, N, [G0], sky=SKY, return_weights=True))
    nodes = P["nodes"]
    assert sc["totals"][0, 4] == 0  # unlinked
    W, ch = sc["weights"][0], _chain(P, 1.0)
    err = np.abs(W - nodes["weight"])
    assert np.all(err <= ch), float((err[ch > 0] / ch[ch > 0]).max())
    assert np.array_equal(W[P["parent"] < 0], np.ones(N))
    _report("identity_W", nodes=int(len(nodes)), bit_equal_share=float(np.mean(W == nodes["weight"])),
            worst_over_bound=float((err[ch > 0] / ch[ch > 0]).max()))
    # the tables: the same bins; each term within its weight bound, then the order of the adds
    rows, bins = er["rows"].cpu().numpy(), er["bins"].cpu().numpy().astype(np.int64)
    fin = np.flatnonzero(nodes["is_final"] != 0)
    ev = nodes["tree"][fin]
    p = rows[:, 8] * rows[:, 7]
    back_e = P["back"]["prob"] * P["back"]["weight"]
    back = back_e[ev]
    dp = (ch[fin] * back + nodes["weight"][fin] * _d_back(P, 1.0, back_e)[ev]) * rows[:, 7]  # |Δ power| per row
    sp = rows[:, 1].astype(np.int64)
    from adiabatic_raytracer_amd import trees as T
    fb = T.hist_bins(rows[:, 3], NBINS)
    worst = 0.0
    for name, lab, size, got, ref in (("flux", np.where(fb >= 0, sp * NBINS + fb, -1), 2 * NBINS, sc["flux"][0],
                                       er["flux"].cpu().numpy()),
                                      ("sky", bins, 2 * 6 * 11, sc["sky"][0].reshape(-1), er["sky_hist"].cpu().numpy().reshape(-1)),
                                      ("totals", sp, 2, sc["totals"][0, :2], er["totals"].cpu().numpy()[2:4])):
        k = lab >= 0
        cnt = np.bincount(lab[k], minlength=size)
        S = np.bincount(lab[k], weights=p[k], minlength=size)
        tol = 2 * (cnt + 1) * U * S + np.bincount(lab[k], weights=dp[k], minlength=size)
        e = np.abs(got - ref)
        assert np.all(e <= tol), (name, float((e[tol > 0] / tol[tol > 0]).max()))
        assert np.all(got[cnt == 0] == 0) and S.sum() > 0
        worst = max(worst, float((e[tol > 0] / tol[tol > 0]).max()))
    _report("identity_tables", worst_over_bound=worst)
    # coverage: every tree of the g0 run closed its probability to prob_cutoff or stopped by a rule
    cov = sc["totals"][0, 2] / N
    assert 0.5 < cov <= 1.0 + 1e-12
    _report("identity_coverage", mean=float(cov))


# ---- 2. against numpy, default tree options (Monte-Carlo trees among them)

def test_weights_and_tables_against_numpy():
    from adiabatic_raytracer_amd import trees as T
    g = [G0 / 2, G0, 3 * G0]
    s = (np.array(g) / G0) ** 2
    (parts, mc) = _pipe(G0, 0, N)
    eng = _eng(G0)[0]
    P = _pulled(G0, 0, N)
    nodes = P["nodes"]
    infos = parts[3]["infos"].cpu().numpy()
    assert (infos < 0).sum() > 0 and mc == 5  # some trees went Monte-Carlo
    er = eng.event_rows(*parts, nbins=NBINS, sky=SKY, return_bins=True)
    sc = _host(_scan(G0, 0, N, g, sky=SKY, return_weights=True))
    Wn, covn, unl = T.reweight_nodes(nodes, P["start"], P["x"], s, mc)
    assert unl == 0 and sc["totals"][0, 4] == 0
    W = sc["weights"]
    bound = (P["depth"][None, :] + 2.0) * 4 * U * (1.0 + s[:, None] * P["x"].max())
    m = np.maximum(np.abs(W), np.abs(Wn))
    rel = np.where(m > 0, np.abs(W - Wn) / np.where(m > 0, m, 1.0), 0.0)
    pj = P["parent"][P["parent"] >= 0]
    _report("numpy_W", worst_over_bound=float((rel / bound).max()), bit_equal_share=float(np.mean(W == Wn)),
            x_max=float(P["x"].max()), depth_max=int(P["depth"].max()),
            mc_children=int((pj - P["start"][nodes["tree"][pj]] + 1 > mc).sum()))
    assert np.all(rel <= bound), float((rel / bound).max())
    # the back factors
    Bn = T.reweight_back(P["x_root"], P["back"]["weight"], s, P["x_single"])
    # (two exps, each within 1 ulp of libm, differ by at most 4u e^-y: relative to 1 - e^-y that is 4u / (e^y - 1);
    # then the subtraction, the power and the product)
    for k in range(3):
        with np.errstate(over="ignore", divide="ignore"):
            bb = 4 * U / np.expm1(s[k] * P["x_root"]) + 4 * U + _back_bound(P, s[k])[1]
        e = np.abs(sc["back"][k] - Bn[k])
        assert np.all(e <= bb * np.maximum(Bn[k], sc["back"][k])), (k, float((e / (bb * np.maximum(Bn[k], sc["back"][k]))).max()))
    # the tables against numpy binning of the device's own W and B: the order of the adds only
    rows, bins = er["rows"].cpu().numpy(), er["bins"].cpu().numpy().astype(np.int64)
    fin = np.flatnonzero(nodes["is_final"] != 0)
    ev, sp = nodes["tree"][fin], rows[:, 1].astype(np.int64)
    fb = T.hist_bins(rows[:, 3], NBINS)
    worst = 0.0
    for k in range(3):
        p = (W[k][fin] * sc["back"][k][ev]) * rows[:, 7]
        for name, lab, size, got in (("flux", np.where(fb >= 0, sp * NBINS + fb, -1), 2 * NBINS, sc["flux"][k]),
                                     ("sky", bins, 2 * 6 * 11, sc["sky"][k].reshape(-1)), ("totals", sp, 2, sc["totals"][k, :2])):
            kk = lab >= 0
            cnt = np.bincount(lab[kk], minlength=size)
            S = np.bincount(lab[kk], weights=p[kk], minlength=size)
            tol = 2 * (cnt + 1) * U * S
            e = np.abs(got - S)
            assert np.all(e <= tol), (name, k)
            worst = max(worst, float((e[tol > 0] / tol[tol > 0]).max()))
        # coverage: Σ W over the records without a crossing, the trees' sums added in another order
        c = sc["totals"][k, 2]
        assert abs(c - covn[k].sum()) <= 2 * (len(nodes) + 1) * U * covn[k].sum() + (bound[k] * np.abs(Wn[k])).sum()
    _report("numpy_tables", worst_over_bound=worst, coverage=[float(v) / N for v in sc["totals"][:, 2]])


# ---- 3. against direct runs at the target couplings

def _direct(g, n):
    key = ("direct", g, n)
    if key not in _cache:
        _cache[key] = _np(_eng(g)[0].run_events(n, seed=SEED, saveMode=1, **FULL))
    return _cache[key]


def _compare_with_direct(g0, n, targets):
    eng = _eng(g0)[0]
    (parts, mc) = _pipe(g0, 0, n, **FULL)
    P = _pulled(g0, 0, n, **FULL)
    nodes = P["nodes"]
    base = eng.event_rows(*parts, saveMode=1, nbins=NBINS)["rows"].cpu().numpy()
    sc = _host(_scan(g0, 0, n, targets, tree=FULL, return_weights=True))
    fin = np.flatnonzero(nodes["is_final"] != 0)
    assert len(base) == len(fin)
    ev = nodes["tree"][fin]
    key = lambda r: [(int(a), float(b).hex(), float(c).hex()) for a, b, c in zip(r[:, 1], r[:, 2], r[:, 3])]  # noqa: E731
    kb = key(base)
    out = {}
    for k, g in enumerate(targets):
        s = (g / g0) ** 2
        d = _direct(g, n)["rows_raw"]
        kd, evd = key(d), d[:, 0].astype(np.int64) - 1
        ch, (b_abs, b_rel), b28 = _chain(P, s), _back_bound(P, s), _back_bound(P, s, prob_only=True)
        compared, worst, misses = 0, {8: 0.0, 25: 0.0, 28: 0.0}, []
        for e in range(n):
            ib, idd = np.flatnonzero(ev == e), np.flatnonzero(evd == e)
            mb, md = {kb[i]: i for i in ib}, {kd[i]: i for i in idd}
            if set(mb) != set(md) or len(mb) != len(ib) or len(md) != len(idd) or not mb:
                continue
            compared += 1
            for kk, i in mb.items():
                r = d[md[kk]]
                c25, c28 = sc["back"][k][e], sc["back_prob"][k][e]
                c8 = sc["weights"][k][fin[i]] * c25
                d25 = b_abs[e] + b_rel[e] * max(r[25], c25)
                for col, mine, tol in ((28, c28, b28[e]), (25, c25, d25), (8, c8, ch[fin[i]] * max(r[25], c25) + d25)):
                    err = abs(mine - r[col])
                    if tol > 0:
                        worst[col] = max(worst[col], err / tol)
                    if not err <= tol:
                        misses.append(dict(event=e, col=col, mine=float(mine), direct=float(r[col]), err=float(err),
                                           tol=float(tol), bweight_g0=float(P["back"]["weight"][e]),
                                           back_crossings=int(P["back"]["n_cross"][e]), W=float(sc["weights"][k][fin[i]]),
                                           W_direct=float(r[8] / r[25]) if r[25] else None))
        with_rows = len(set(ev.tolist()) | set(evd.tolist()))
        _report("direct", g0=g0, g=g, events=n, events_with_rows=with_rows, compared=compared,
                worst_over_bound={str(c): v for c, v in worst.items()},
                saturated=int(sc["totals"][k, 3]), coverage=float(sc["totals"][k, 2] / n), n_misses=len(misses),
                miss_events_by_back_crossings={str(c): len({m["event"] for m in misses if m["back_crossings"] == c})
                                               for c in sorted({m["back_crossings"] for m in misses})},
                misses=misses[:3])
        assert not misses, (len(misses), misses[:3])
        assert compared >= 0.9 * with_rows, (compared, with_rows)
        out[g] = sc["totals"][k]
    return sc, out


@pytest.mark.parametrize("n", [48, 256])
def test_against_direct_runs_from_1e_11(n):
    _compare_with_direct(G0, n, [2e-11, 5e-12])


def test_against_a_direct_run_down_from_2e_11():
    """saturated pc (exactly 1.0 at the base coupling). A small stored bweight is 1 - P with an absolute error of
    u/2 (5.7e-10 for one event here), which exp(s log w) would carry into column 25; a single backtrace
    crossing's exponent is recomputed instead, and the bound holds. No backtrace weight of these 256 events
    underflowed to 0, so `saturated` is 0 on both sides here: a nonzero count is asserted on the synthetic forest."""
    P = _pulled(2e-11, 0, 256, **FULL)
    sc, _ = _compare_with_direct(2e-11, 256, [1e-11])
    assert (P["nodes"]["pc"] == 1.0).sum() > 0
    assert sc["totals"][0, 3] == (P["back"]["weight"] == 0.0).sum()


def test_report_photon_total_against_the_direct_run():
    """Report only: the photon total at 2e-11 reweighted from 1e-11 against the direct run's, in σ"""
    eng = _eng(G0)[0]
    r = _np(eng.run_events(256, seed=SEED, rows=False, errors=True, couplings=[2e-11], **FULL))
    d = _np(_eng(2e-11)[0].run_events(256, seed=SEED, rows=False, errors=True, **FULL))
    a, sa = r["coupling_scan"]["sum_weight_sln_prob"][0, 1], r["coupling_scan"]["sum_weight_sln_prob_sigma"][0, 1]
    b, sb = d["sum_weight_sln_prob"][1], d["sum_weight_sln_prob_sigma"][1]
    _report("photon_total_2e-11", reweighted=float(a), direct=float(b), sigma_reweighted=float(sa), sigma_direct=float(sb),
            difference_in_combined_sigma=float((a - b) / np.hypot(sa, sb)), coverage=float(r["coupling_scan"]["coverage"][0]))


# ---- 4. chunk invariance

def test_chunks_400_400_300_against_one_chunk():
    g = [G0 / 2, G0, 3 * G0]
    whole = _host(_scan(G0, 0, N, g, sky=SKY, return_weights=True))
    acc, Ws = None, []
    for lo, c in ((0, 400), (400, 400), (800, 300)):
        (parts, mc) = _pipe(G0, lo, c)
        acc = _eng(G0)[0].event_reweight(*parts, g, mc_nodes=mc, event_offset=lo, nbins=NBINS, sky=SKY, scan=acc,
                                         return_weights=True)
        Ws.append(acc["weights"].cpu().numpy())
    assert np.array_equal(np.concatenate(Ws, axis=1), whole["weights"])  # bit-identical
    a = _host(acc)
    assert a["n_events"] == N
    P = _pulled(G0, 0, N)
    fin = P["nodes"]["is_final"] != 0
    rows = int(fin.sum())
    worst = 0.0
    for name in ("flux", "sky"):
        x, y = a[name].reshape(3, -1), whole[name].reshape(3, -1)
        tol = 2 * 2 * (rows + 1) * U * np.maximum(x, y)  # (at most every row in one bin: twice the add-order bound)
        assert np.all(np.abs(x - y) <= tol), name
        worst = max(worst, float((np.abs(x - y)[tol > 0] / tol[tol > 0]).max()))
    x, y = a["totals"], whole["totals"]
    assert np.all(np.abs(x - y)[:, :3] <= 2 * 2 * (len(P["nodes"]) + 1) * U * np.maximum(x, y)[:, :3])
    assert np.array_equal(x[:, 3:], y[:, 3:])
    _report("chunks", worst_over_bound=worst)


# ---- 5. errors

def test_errors_per_coupling_against_numpy():
    from adiabatic_raytracer_amd import trees as T
    from test_gpu_event_moments import _var_check
    g = [G0 / 2, G0, 3 * G0]
    eng = _eng(G0)[0]
    r = _np(eng.run_events(N, seed=SEED, sky_map=SKY, errors=True, couplings=g))

    def var_check_terms(what, sig_a, sig_b, S, Q, Cc, grp, dS, a_max):
        """test_gpu_event_moments._var_check between two device results (sides = 2) whose powers differ by at
        most dp per row, dS = Σ dp per bin: |ΔQ| <= 2 max_e X_e dS <= 2 sqrt(Q) dS, |ΔC| <= a_max dS"""
        sig_a, sig_b = (np.asarray(v, np.float64).reshape(-1) for v in (sig_a, sig_b))
        E, m, cnt = grp
        F = S / f
        bQ, bC, bS = _moment_bound(Q, Q, grp) + 2 * np.sqrt(Q) * dS, _moment_bound(Cc, Cc, grp) + a_max * dS, 2 * (cnt + 1) * U * S + dS
        dV = 2 * (bQ + 2 * F * bC + (2 * Cc + 2 * F * A2) * bS / f + 8 * U * (Q + 2 * F * Cc + F * F * A2))
        Va, Vb = ((v * f) ** 2 * (N - 1) / N for v in (sig_a, sig_b))
        err = np.abs(Va - Vb)
        ratio = float(np.max(err[dV > 0] / dV[dV > 0])) if (dV > 0).any() else 0.0
        _report(what, bound_ratio_max=ratio)
        assert np.all(np.isfinite(sig_a)) and np.all(np.isfinite(sig_b)) and np.all(err <= dV), (what, ratio)

    cs = r["coupling_scan"]
    assert cs["flux_sigma"].shape == (3, 2, NBINS) and cs["sky_map_sigma"].shape == (3, 2, 6, 11, 1)
    assert cs["sum_weight_sln_prob_sigma"].shape == (3, 2) and cs["unlinked"] == 0
    (parts, mc) = _pipe(G0, 0, N)
    P = _pulled(G0, 0, N)
    nodes = P["nodes"]
    sc = _host(_scan(G0, 0, N, g, sky=SKY, return_weights=True))
    rows = r["rows_raw"]
    fin = np.flatnonzero(nodes["is_final"] != 0)
    ev, sp = nodes["tree"][fin], rows[:, 1].astype(np.int64)
    att = parts[0]["attempts"].cpu().numpy()
    a = att.astype(np.int64) - 1 + np.bincount(ev[sp == 1], minlength=N)
    f, A2 = float(r["f_inx"]), float((a * a).sum())
    fb = T.hist_bins(rows[:, 3], NBINS)
    labels = {"flux": (np.where(fb >= 0, sp * NBINS + fb, -1), 2 * NBINS),
              "sky": (T.sky_bins(rows[:, 2], rows[:, 3], rows[:, 12], rows[:, 1], **SKY), 2 * 6 * 11), "tot": (sp, 2)}
    for k in range(3):
        p = (sc["weights"][k][fin] * sc["back"][k][ev]) * rows[:, 7]
        for name, key in (("flux", "flux_sigma"), ("sky", "sky_map_sigma"), ("tot", "sum_weight_sln_prob_sigma")):
            lab, size = labels[name]
            S, Q, Cc = T.event_moments(ev, lab, p, size, a)
            want = T.moments_sigma(S, Q, Cc, f, A2, N)
            _var_check(f"scan_sigma_{name}_{k}", cs[key][k], want, S, Q, Cc, _groups(ev, lab, size), f, A2, N)
    # at the base coupling the scan's σ are run_events' own: the same groups, powers within their weight bound
    k1 = 1
    back_e = P["back"]["prob"] * P["back"]["weight"]
    dp = (_chain(P, 1.0)[fin] * back_e[ev] + nodes["weight"][fin] * _d_back(P, 1.0, back_e)[ev]) * rows[:, 7]  # (the identity test's)
    for name, key in (("flux", "flux_sigma"), ("sky", "sky_map_sigma"), ("tot", "sum_weight_sln_prob_sigma")):
        lab, size = labels[name]
        p = rows[:, 8] * rows[:, 7]
        S, Q, Cc = T.event_moments(ev, lab, p, size, a)
        dS = np.bincount(lab[lab >= 0], weights=dp[lab >= 0], minlength=size)
        var_check_terms(f"scan_sigma_{name}_base", cs[key][k1], np.asarray(r[key], np.float64), S, Q, Cc,
                        _groups(ev, lab, size), dS, float(a.max()))


# ---- 6. off: couplings=None is the parent's result, key for key and byte for byte

def test_off_by_default_and_main_runner_tree():
    import adiabatic_raytracer_amd as A
    import torch
    eng = _eng(G0)[0]
    a = eng.run_events(200, seed=SEED, sky_map=SKY)
    b = eng.run_events(200, seed=SEED, sky_map=SKY, couplings=[G0 / 2, 3 * G0])
    assert set(b) - set(a) == {"coupling_scan"}
    assert set(a) == {"rows", "flux", "f_inx", "sum_weight_sln_prob", "n_rows", "n_photon_rows", "totals", "flux_raw",
                      "rows_raw", "sky_map", "sky_raw", "sky_map_edges"}
    for k in ("rows", "rows_raw"):
        assert torch.equal(a[k], b[k])  # the scan does not touch the run's own rows
    assert a["f_inx"] == b["f_inx"] and a["n_rows"] == b["n_rows"]
    # the run's own tables: the same adds in whatever order the hardware took them (exact counts; a weighted sum
    # within the add-order bound, as between any two runs of the parent)
    ta, tb = a["totals"].cpu().numpy(), b["totals"].cpu().numpy()
    assert np.array_equal(ta[[0, 1, 4, 5]], tb[[0, 1, 4, 5]])
    for k in ("flux_raw", "sky_raw", "totals"):
        x, y = a[k].cpu().numpy().reshape(-1), b[k].cpu().numpy().reshape(-1)
        assert np.array_equal(x == 0, y == 0) and np.all(np.abs(x - y) <= 2 * (a["n_rows"] + 1) * U * np.maximum(x, y)), k
    # a bad list is refused before any work is done
    for bad in ([], [G0, -1.0], [G0, float("nan")], [G0] * 33):
        with pytest.raises(ValueError, match="couplings"):
            eng.run_events(0, couplings=bad)
    p = replace(_params("flat"), g_agg=G0)
    i0, i1 = {}, {}
    r0 = A.trees.main_runner_tree(p, 201, seed=SEED, device_events=True, run_info=i0, sky_map=SKY)
    r1 = A.trees.main_runner_tree(p, 201, seed=SEED, device_events=True, run_info=i1, sky_map=SKY, couplings=[G0 / 2, 3 * G0])
    assert set(i1) - set(i0) == {"coupling_scan"} and np.array_equal(r0, r1, equal_nan=True)
    assert set(i0) == {"f_inx", "flux", "sum_weight_sln_prob", "rows", "events", "n_events", "sky_map", "sky_map_edges"}
    cs, ms = _np(b)["coupling_scan"], i1["coupling_scan"]
    for k in ("g", "scale", "flux", "sky_map", "sum_weight_sln_prob", "coverage"):
        x, y = np.asarray(cs[k]), np.asarray(ms[k])
        assert x.shape == y.shape and np.all(np.abs(x - y) <= 2 * 2 * (a["n_rows"] + 201) * U * np.maximum(np.abs(x), np.abs(y))), k
    assert (cs["saturated"], cs["unlinked"]) == (ms["saturated"], ms["unlinked"])
    for kw in ({}, {"device_trees": True}):
        with pytest.raises(ValueError, match="device_events"):
            A.trees.main_runner_tree(p, 5, couplings=[G0], **kw)
    g, power, sigma = A.trees.coupling_curve(cs)
    assert len(g) == 2 and power[1] > power[0] > 0 and sigma is None


# ---- 7. a synthetic forest in HBM: the CPU test's hand-built records

def test_synthetic_forest_counters_and_coverage():
    import torch
    from adiabatic_raytracer_amd.trees import NODE_DTYPE
    from adiabatic_raytracer_amd import trees as T
    from test_event_reweight import SCALES, _grouped_forest, _hand_built, _unlinked_forest
    eng = _eng(G0)[0]
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(eng.device)  # noqa: E731
    recs = lambda a: up(a.view(np.uint8).reshape(len(a), NODE_DTYPE.itemsize))  # noqa: E731
    # (forest, unlinked records, grouped records whose pc is 1.0)
    for F, want_unlinked, lost in ((_hand_built()[0], 0, 0), (_unlinked_forest()[0], 2, 0), (_grouped_forest()[0], 0, 1)):
        nodes, start, x = F.arrays()
        n, nn = len(start) - 1, len(nodes)
        # real crossings cannot be dialled to an exponent: put the records where P_nonAD is whatever the
        # physics gives there (a point of the real sample), and compare with numpy on the device's own x
        P = _pulled(G0, 0, 48, **FULL)
        real = P["nodes"][P["nodes"]["n_cross"] > 0]
        bits = lambda t, v: (float(t).hex(),) + tuple(float(c).hex() for c in v)  # noqa: E731
        moved = {}
        for i in np.flatnonzero(nodes["n_cross"] > 0):  # each distinct hand-built crossing becomes a real one
            moved.setdefault(bits(nodes["tc"][i], nodes["xc"][i]), real[len(moved)])
        for i in range(nn):
            to = moved.get(bits(nodes["t0"][i], nodes["x0"][i]))
            if to is not None:
                nodes["t0"][i], nodes["x0"][i] = to["tc"], to["xc"]
        for i in np.flatnonzero(nodes["n_cross"] > 0):
            to = moved[bits(nodes["tc"][i], nodes["xc"][i])]
            for f in ("tc", "xc", "kc", "dwc"):
                nodes[f][i] = to[f]
        bk = np.zeros(n, NODE_DTYPE)
        bk["tree"], bk["prob"] = np.arange(n), 0.5
        bk["weight"] = np.where(np.arange(n) % 3 == 0, 0.0, np.where(np.arange(n) % 3 == 1, 1.0, 0.25))
        w5 = np.ones((5, n))
        rs = _pipe(G0, 0, 48, **FULL)[0][0]  # the first n events of the real sample
        sample = {"x": rs["x"].view(3, 48)[:, :n].contiguous().view(-1), "k_init": rs["k_init"].view(3, 48)[:, :n].contiguous().view(-1),
                  "erg": rs["erg"][:n].contiguous(), "attempts": up(np.ones(n, np.int32))}
        ones = up(np.ones(n, np.int32))
        back = {"nodes": recs(bk), "counts": ones, "n_nodes": n}
        fwd = {"nodes": recs(nodes), "node_start": up(start), "counts": up(np.diff(start).astype(np.int32)),
               "infos": up(np.zeros(n, np.int32)), "n_nodes": nn}
        g = [G0 * float(np.sqrt(s)) for s in SCALES[:3]]
        sc = _host(eng.event_reweight(sample, up(w5), back, fwd, g, mc_nodes=F.mc_nodes, nbins=NBINS, return_weights=True))
        assert np.all(np.isfinite(sc["weights"]))
        tot = sc["totals"]
        assert np.all(tot[:, 4] == want_unlinked) and np.all(tot[:, 3] == (bk["weight"] == 0.0).sum() + lost)
        # every linked tree is closed: its coverage is 1 at every coupling, whatever the exponents are
        W = sc["weights"]
        closed = np.diff(start) > 0
        cov = np.array([[W[k, start[t]:start[t + 1]][nodes["n_cross"][start[t]:start[t + 1]] == 0].sum() for t in range(n)]
                        for k in range(3)])
        if lost:
            # records with n_cross = 2, whose pc is not what their stored crossing gives: the exponent comes
            # from pc, s = 1 returns the stored weights, every scale agrees with numpy (x is not looked at)
            assert np.all(nodes["n_cross"][nodes["n_cross"] > 0] == 2) and np.all(tot[:, 5] == n)  # (only the roots' prob 0.5 differs)
            assert np.all(np.abs(W[1] - nodes["weight"]) <= 4 * U)
            Wn = T.reweight_nodes(nodes, start, np.full(nn, 0.9), SCALES[:3], F.mc_nodes)[0]
            d = np.array(F.depth, np.float64)
            tol = (d[None, :] + 2.0) * 4 * U * (1.0 + SCALES[:3, None] * 1.0) + (d[None, :] + 1.0) * 4 * U / np.expm1(SCALES[:3] * 0.35)[:, None]
            assert np.all(np.abs(W - Wn) <= tol * np.maximum(np.abs(W), np.abs(Wn))), float(np.abs(W - Wn).max())
            assert abs(cov[1, 0] - 1.0) <= 64 * U
        elif want_unlinked == 0:
            assert np.all(np.abs(cov[:, closed] - 1.0) <= 64 * U) and np.all(cov[:, ~closed] == 0)
            assert np.all(np.abs(tot[:, 2] - closed.sum()) <= 64 * nn * U)
        else:
            assert np.all(tot[:, 2] < closed.sum())
        assert np.all(np.abs(tot[:, 2] - cov.sum(axis=1)) <= 4 * nn * U * cov.sum(axis=1))
        # the back factors: bweight 0 stays 0, 1 stays 1
        B, Bp = sc["back"], sc["back_prob"]
        assert np.all(B[:, bk["weight"] == 0.0] == 0.0) and np.array_equal(B[:, bk["weight"] == 1.0], Bp[:, bk["weight"] == 1.0])
        assert np.all(Bp > 0) and np.all(Bp <= 1)
