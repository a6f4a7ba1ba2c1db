"""The coupling scan without a GPU: the argument checks of art_event_reweight_device, which come before
any device is touched; the Python surface (Engine.event_reweight, run_events(couplings=),
main_runner_tree(couplings=), trees.reweight_nodes, scan_result, coupling_curve); and the per-tree reweight
of art_event_reweight.h in a host build (tools/eventreweight.py, each crossing's exponent from a table)
against trees.reweight_nodes on hand-built forests.

The hand-built forests form their stored weights by tree_step's products with libm's exp (math.exp), the
function the host build of fexp is: at s = 1 the compiled header reproduces them exactly. numpy's exp is
another implementation; it and the compiled header agree bit for bit except for their exp / log calls,
each within 1 ulp of libm, so W differs by at most (depth + 2) 4u (1 + s x_max) relative, u = 2^-53.
Powers of two make the second-moment tables exact."""
import ctypes as C
import inspect
import math

import numpy as np
import pytest

INVALID = -1  # ART_E_INVALID
U = 2.0 ** -53
AXION, PHOTON = 0, 1
SCALES = np.array([0.25, 1.0, 9.0, 1e-4, 30.0])
XS = (0.0, 1e-12, 1.0, 800.0)


# ---------------------------------------------------------------------------------------------------
# hand-built forests
class _Forest:
    """Records appended in the order their tree processed them; add() returns the record's index."""

    def __init__(self, mc_nodes):
        self.mc_nodes, self.recs, self.x, self.start, self.depth = mc_nodes, [], [], [0], []
        self.gpc = {}  # record -> the pc of a grouped crossing (n_cross = 2)
        self._tick = 0

    def end_tree(self):
        self.start.append(len(self.recs))

    def add(self, parent=None, converted=False, x=None, final=None, rare=False, weight=None, t0x0=None, cross=None,
            grouped_pc=None):
        """x: the exponent of the record's own first crossing (None: no crossing). parent: index of the
        record it was pushed by (None: a root). weight: stored weight, else by tree_step's products.
        t0x0 / cross: (t, x[3]) to use instead of the parent's crossing / a fresh crossing. grouped_pc: the
        record has n_cross = 2 and this pc, which x (what its stored first crossing alone would give) is not."""
        from adiabatic_raytracer_amd.trees import NODE_DTYPE
        nd = np.zeros((), NODE_DTYPE)
        first = self.start[-1]
        j = len(self.recs) - first
        nd["tree"], nd["pad"] = len(self.start) - 1, j
        d = 0
        if parent is None:
            nd["species"], w = PHOTON, 1.0
            nd["t0"], nd["x0"] = 0.0, (3.0 + j, 4.0, 5.0)
        else:
            p = self.recs[parent]
            xp = self.x[parent]
            nd["species"] = (1 - p["species"]) if converted else p["species"]
            e = math.exp(-(1.0 * xp))
            f = 1.0 - e if converted else e
            if parent in self.gpc:  # tree_step's products with the group's P1
                f = self.gpc[parent] if converted else 1.0 - self.gpc[parent]
            mc = (parent - first) + 1 > self.mc_nodes
            w = float(p["weight"]) if mc else f * float(p["weight"])
            nd["t0"], nd["x0"] = p["tc"], p["xc"]
            d = self.depth[parent] + 1
        if t0x0 is not None:
            nd["t0"], nd["x0"] = t0x0
        nd["weight"] = w if weight is None else weight
        if x is not None and not rare:
            self._tick += 1
            nd["n_cross"] = 1
            nd["tc"], nd["xc"] = (0.125 * self._tick, (10.0 + self._tick, 0.5 * self._tick, -1.0)) if cross is None else cross
            nd["kc"], nd["dwc"] = (0.1, 0.2, 0.3), -1.0
            nd["pc"] = 1.0 - math.exp(-(1.0 * x))
            if grouped_pc is not None:
                nd["n_cross"], nd["pc"] = 2, grouped_pc
                self.gpc[len(self.recs)] = grouped_pc
        nd["is_final"] = int(x is None and not rare) if final is None else int(final)
        self.recs.append(nd)
        self.x.append(0.0 if (x is None or rare) else x)
        self.depth.append(d)
        return len(self.recs) - 1

    def arrays(self):
        from adiabatic_raytracer_amd.trees import NODE_DTYPE
        nodes = np.array(self.recs, NODE_DTYPE) if self.recs else np.zeros(0, NODE_DTYPE)
        return nodes, np.array(self.start, np.int64), np.array(self.x, np.float64)


def _hand_built(mc_nodes=1000):
    """The forests of the module: (forest, expectations). Every tree is closed with end_tree()."""
    F = _Forest(mc_nodes)
    info = {}
    # 0: a one-record tree
    F.add()
    F.end_tree()
    # 1-4: a root with two children, at each exponent
    for x in XS:
        r = F.add(x=x)
        F.add(r, True)
        F.add(r, False)
        F.end_tree()
    # 5: a depth-4 chain through every exponent, each crossing with both children
    r = F.add(x=1e-12)
    a = F.add(r, True, x=1.0)
    F.add(r, False)
    c = F.add(a, True, x=800.0)
    F.add(a, False)
    e = F.add(c, True, x=0.0)
    F.add(c, False)
    F.add(e, True)
    F.add(e, False)
    F.end_tree()
    # 6: a rare-fail record (crossings on its segment, recorded without: n_cross = 0, not final, no children)
    r = F.add(x=0.5)
    info["rare"] = F.add(r, True, x=0.25, rare=True)
    F.add(r, False)
    F.end_tree()
    # 7: an empty tree
    F.end_tree()
    info["empty"] = len(F.start) - 2
    return F, info


def _unlinked_forest():
    """An orphan and a record with two candidate parents beside a healthy child"""
    F = _Forest(1000)
    r = F.add(x=0.5)
    a = F.add(r, True, x=0.75)
    b = F.add(r, False, x=0.75, cross=(F.recs[a]["tc"].copy(), F.recs[a]["xc"].copy()))  # the same crossing twice
    two = F.add(a, True)  # matches a and b
    orphan = F.add(r, False, t0x0=(77.0, (1.0, 2.0, 3.0)))
    ok = F.add(r, True, x=None, t0x0=None)  # (a third child of the root: linked, the converted factor)
    F.end_tree()
    return F, two, orphan, ok


def _mc_forest():
    """mc_nodes = 2: the root and the second pop split fully, the third pop draws one Monte-Carlo child"""
    F = _Forest(2)
    r = F.add(x=0.7)
    a = F.add(r, True, x=0.3)
    b = F.add(r, False, x=1.1)  # pop 3 > mc_nodes: its child is a draw
    F.add(a, True)
    F.add(a, False)
    mc = F.add(b, True, x=0.2)  # the converted branch was drawn; it crosses again
    mc2 = F.add(mc, False)  # and its own draw is the unconverted branch
    F.end_tree()
    return F, b, mc, mc2


def _grouped_forest():
    """Records with n_cross = 2: their pc came from the group of their segment's crossings and is NOT
    1 - exp(-x) of the stored first crossing (x = 0.9 below); one of them has pc == 1.0"""
    F = _Forest(2)
    r = F.add(x=0.9, grouped_pc=0.3)
    a = F.add(r, True, x=0.9, grouped_pc=1.0)
    b = F.add(r, False, x=0.9, grouped_pc=0.625)  # pop 3 > mc_nodes: its child is a draw
    F.add(a, True)
    F.add(a, False)
    F.add(b, True)
    F.end_tree()
    return F, r, a, b


def _both(F, scales=SCALES):
    from adiabatic_raytracer_amd import trees
    from tools import eventreweight
    nodes, start, x = F.arrays()
    Wc, cc, uc, dc, _ = eventreweight.forest(nodes, start, x, scales, F.mc_nodes)
    Wn, cn, un = trees.reweight_nodes(nodes, start, x, scales, F.mc_nodes)
    return nodes, start, x, (Wc, cc, uc, dc), (Wn, cn, un)


def _bound(F, scales):
    """(depth + 2) 4u (1 + s x_max) per (scale, record)"""
    x_max = max(F.x) if F.x else 0.0
    d = np.array(F.depth, np.float64)
    return (d[None, :] + 2.0) * 4.0 * U * (1.0 + np.asarray(scales)[:, None] * x_max)


def _rel(a, b):
    with np.errstate(invalid="ignore", divide="ignore"):
        m = np.maximum(np.abs(a), np.abs(b))
        return np.where(m > 0, np.abs(a - b) / m, 0.0)


# ---------------------------------------------------------------------------------------------------
def test_identity_at_s_1_is_exact():
    for F in (_hand_built()[0], _mc_forest()[0]):
        nodes, start, x, (Wc, cc, uc, dc), (Wn, cn, un) = _both(F)
        k1 = int(np.flatnonzero(SCALES == 1.0)[0])
        assert uc == 0 and un == 0 and dc == 0
        assert np.array_equal(Wc[k1], nodes["weight"])  # the same products with the same exp: exact
        # numpy's exp is another one: within the module's bound of the stored weights
        assert np.all(_rel(Wn[k1], nodes["weight"]) <= _bound(F, SCALES)[k1])
        # every tree was explored to its end: its coverage is 1 up to the rounding of its factors
        n_trees = len(start) - 1
        full = np.diff(start) > 0
        assert np.all(np.abs(cc[k1][full] - 1.0) <= 64 * U) and np.all(cc[:, ~full] == 0.0)
        assert cc.shape == (len(SCALES), n_trees)


def test_header_and_numpy_agree_across_scales():
    worst = 0.0
    for F in (_hand_built()[0], _mc_forest()[0], _unlinked_forest()[0]):
        nodes, start, x, (Wc, cc, uc, dc), (Wn, cn, un) = _both(F)
        assert uc == un
        r, b = _rel(Wc, Wn), _bound(F, SCALES)
        worst = max(worst, float((r / b).max()) if r.size else 0.0)
        assert np.all(r <= b), float((r / b).max())
        assert np.all(np.isfinite(Wc)) and np.all(Wc >= 0.0)
        # the two exps agree on most arguments: the bulk is bit-equal
        assert np.mean(Wc == Wn) > 0.5
        assert np.all(_rel(cc, cn) <= (len(nodes) + 2) * b.max())
    print({"test": "event_reweight", "what": "header_vs_numpy", "worst_over_bound": worst})


def test_weights_follow_the_rules():
    F, info = _hand_built()
    nodes, start, x, (Wc, cc, uc, dc), _ = _both(F)
    # a root with two children at exponent X: 1 - exp(-s X) and exp(-s X), and they close the tree
    for t, X in enumerate(XS, start=1):
        a = start[t]
        for k, s in enumerate(SCALES):
            e = math.exp(-(s * X))
            assert Wc[k, a] == 1.0 and Wc[k, a + 1] == 1.0 - e and Wc[k, a + 2] == e
            assert abs(cc[k, t] - 1.0) <= 2 * U
    # x0 = 0 never converts at any scale; x0 = 800 always does wherever exp(-800 s) underflows
    assert np.all(Wc[:, start[1] + 1] == 0.0) and np.all(Wc[:, start[1] + 2] == 1.0)
    big = SCALES * 800.0 > 750.0
    assert big.sum() >= 3 and np.all(Wc[big, start[4] + 1] == 1.0) and np.all(Wc[big, start[4] + 2] == 0.0)
    # the rare-fail record keeps its weight in the coverage although it is not final
    t = int(nodes["tree"][info["rare"]])
    assert nodes["is_final"][info["rare"]] == 0 and np.all(np.abs(cc[:, t] - 1.0) <= 4 * U)
    assert np.all(cc[:, info["empty"]] == 0.0)


def test_monte_carlo_children_take_the_likelihood_ratio():
    F, b, mc, mc2 = _mc_forest()
    nodes, start, x, (Wc, cc, uc, dc), (Wn, cn, un) = _both(F)
    k1 = int(np.flatnonzero(SCALES == 1.0)[0])
    for W in (Wc, Wn):
        assert W[k1, mc] == W[k1, b] and W[k1, mc2] == W[k1, b]  # the ratio is exactly 1 at s = 1
    for k, s in enumerate(SCALES):
        f, f0 = 1.0 - math.exp(-(s * 1.1)), 1.0 - math.exp(-1.1)
        assert Wc[k, mc] == Wc[k, b] * (f / f0)
        assert Wc[k, mc2] == Wc[k, mc] * (math.exp(-(s * 0.2)) / math.exp(-0.2))
    # a full-split child of the same forest takes the product
    assert Wc[0, 1] == (1.0 - math.exp(-(SCALES[0] * 0.7))) * 1.0


def test_grouped_crossings_take_their_exponent_from_pc():
    from tools import eventreweight
    F, r, a, b = _grouped_forest()
    nodes, start, x, (Wc, cc, uc, dc), (Wn, cn, un) = _both(F)
    k1 = int(np.flatnonzero(SCALES == 1.0)[0])
    assert uc == un == 0 and dc == 0  # nothing is recomputed for a grouped record, so nothing can differ
    assert eventreweight.forest(nodes, start, x, SCALES, F.mc_nodes)[4] == 1  # the record with pc == 1.0
    # s = 1 returns the stored weights (1 - exp(log(1 - pc)) against pc: two roundings), not those of x = 0.9
    assert np.all(np.abs(Wc[k1] - nodes["weight"]) <= 4 * U) and np.all(np.abs(Wn[k1] - nodes["weight"]) <= 4 * U)
    assert abs(Wc[k1, a] - (1.0 - math.exp(-0.9))) > 0.1
    for k, s in enumerate(SCALES):
        xr, xb = -math.log(1.0 - 0.3), -math.log(1.0 - 0.625)
        assert Wc[k, a] == 1.0 - math.exp(-(s * xr)) and Wc[k, b] == math.exp(-(s * xr))
        # pc == 1.0: the exponent is lost, the crossing converts at every coupling
        assert Wc[k, a + 2] == Wc[k, a] and Wc[k, a + 3] == 0.0
        # the Monte-Carlo child of a grouped record: the likelihood ratio from its pc
        assert Wc[k, b + 3] == Wc[k, b] * ((1.0 - math.exp(-(s * xb))) / (1.0 - math.exp(-(1.0 * xb))))
    # (two exps within an ulp of libm differ by 4u e^-y: 4u / (e^y - 1) relative to 1 - e^-y, per factor of the chain)
    d = np.array(F.depth, np.float64)
    assert np.all(_rel(Wc, Wn) <= _bound(F, SCALES) + (d[None, :] + 1.0) * 4 * U / np.expm1(SCALES * min(xr, xb))[:, None])


def test_orphan_and_two_candidates_are_unlinked():
    F, two, orphan, ok = _unlinked_forest()
    nodes, start, x, (Wc, cc, uc, dc), (Wn, cn, un) = _both(F)
    assert uc == 2 and un == 2
    for W in (Wc, Wn):
        assert np.all(W[:, two] == 0.0) and np.all(W[:, orphan] == 0.0)
        assert np.all(W[:, ok] > 0.0)


def test_recomputed_differs_counts_stale_pc():
    F, _ = _hand_built()
    nodes, start, x = F.arrays()
    from tools import eventreweight
    nodes = nodes.copy()
    cross = np.flatnonzero(nodes["n_cross"] > 0)
    nodes["pc"][cross[:3]] = np.nextafter(nodes["pc"][cross[:3]], 2.0)
    assert eventreweight.forest(nodes, start, x, SCALES, 1000)[3] == 3


def test_back_factors():
    from adiabatic_raytracer_amd import trees
    from tools import eventreweight
    xr = np.array([0.0, 1e-12, 1.0, 800.0, 0.3, 0.3, 0.3, 2.0])
    bw = np.array([0.5, 0.5, 0.5, 0.5, 0.0, 1.0, 1e-300, 0.9])
    Bc, Bn = eventreweight.back(xr, bw, SCALES), trees.reweight_back(xr, bw, SCALES)
    k1 = int(np.flatnonzero(SCALES == 1.0)[0])
    for B in (Bc, Bn):
        assert np.all(B[:, 4] == 0.0)  # bweight 0 stays 0
        assert np.all(B[:, 0] == 0.0)  # no conversion at the root
    assert np.array_equal(Bc[:, 5], 1.0 - np.array([math.exp(-(s * 0.3)) for s in SCALES]))  # bweight 1 stays 1
    assert np.array_equal(Bc[k1], np.array([(1.0 - math.exp(-(1.0 * a))) * b for a, b in zip(xr, bw)]))  # s = 1: stored
    # bweight^s through exp(s log w): (1 + s |ln w|) 4u, and 2u for the root's probability
    lw = np.abs(np.log(np.where(bw > 0, bw, 1.0)))
    bound = (1.0 + SCALES[:, None] * lw[None, :]) * 4 * U + 4 * U * (1.0 + SCALES[:, None] * xr[None, :])
    assert np.all(_rel(Bc, Bn) <= bound)
    # a backtrace with one crossing: bweight^s from its recomputed exponent, where bweight is not 0 or 1 and s != 1
    xs = np.array([np.nan, 0.7, np.nan, 0.7, 0.7, 0.7, 690.0, np.nan])
    Bc1, Bn1 = eventreweight.back(xr, bw, SCALES, xs), trees.reweight_back(xr, bw, SCALES, xs)
    one = ~np.isnan(xs)
    assert np.array_equal(Bc1[:, ~one], Bc[:, ~one]) and np.array_equal(Bc1[k1], Bc[k1])
    assert np.array_equal(Bc1[:, [4, 5]], Bc[:, [4, 5]])  # bweight 0 and 1 stay
    for k, sv in enumerate(SCALES):
        if sv != 1.0:
            assert Bc1[k, 1] == (1.0 - math.exp(-(sv * xr[1]))) * math.exp(-(sv * 0.7))
            assert Bc1[k, 6] == (1.0 - math.exp(-(sv * xr[6]))) * math.exp(-(sv * 690.0))
    assert np.all(_rel(Bc1, Bn1) <= 8 * U * (1.0 + SCALES[:, None] * xr[None, :]))
    assert eventreweight.power(0.5, 0.25, 0, 7.0, 3.0) == 0.5 * 0.25 * 3.0
    assert eventreweight.power(0.5, 0.25, 1, 0.5, 3.0) == ((0.5 * 0.25) * math.exp(-0.5)) * 3.0


def test_unit_power_tables_are_integers_times_w():
    """Every final row's power is W_k = 2^-k: the tables are exact, Σ_e (m_eb 2^-k)² and Σ_e m_eb 2^-k a_e"""
    from adiabatic_raytracer_amd import trees
    from tools import eventmoments, eventreweight
    rng = np.random.default_rng(5)
    nbins, sky_size, n_trees = 6, 10, 40
    counts = rng.integers(0, 7, n_trees)
    start = np.concatenate([[0], np.cumsum(counts)])
    n = int(start[-1])
    sp = rng.integers(0, 2, n)
    fb = rng.integers(-1, nbins, n)
    final = rng.random(n) < 0.8
    flux = np.where(final, np.where(fb >= 0, sp * nbins + fb, np.where(sp == 1, eventmoments.PHOTON, eventmoments.AXION)),
                    eventmoments.NONE).astype(np.int32)
    sky = np.where(final, rng.integers(-1, sky_size, n), -1).astype(np.int32)
    a = rng.integers(0, 5, n_trees)
    K = 4
    pw = np.where(final[None, :], (2.0 ** -np.arange(K))[:, None] * np.ones(n)[None, :], 0.0)
    got = eventreweight.tables(start, flux, sky, pw, a, nbins, sky_size)
    one = eventmoments.forest(start, flux, sky, np.where(final, 1.0, 0.0), a, nbins, sky_size)
    for k in range(K):
        w = 2.0 ** -k
        for key in ("flux_sq", "sky_sq"):
            assert np.array_equal(got[key][k], one[key] * (w * w)), (key, k)
        for key in ("flux_xa", "sky_xa"):
            assert np.array_equal(got[key][k], one[key] * w), (key, k)
        assert np.array_equal(got["totals"][k, :3], one["totals"][:3])
        assert np.array_equal(got["totals"][k, 3:5], one["totals"][3:5] * (w * w))
        assert np.array_equal(got["totals"][k, 5:7], one["totals"][5:7] * w)
    # and against numpy's statement of the moments on the powers of coupling 2
    ev = np.repeat(np.arange(n_trees), counts)
    ae = a + np.bincount(ev[final & (sp == 1)], minlength=n_trees)
    _, Q, Cx = trees.event_moments(ev, np.where(flux >= 0, flux, -1), pw[2], 2 * nbins, ae)
    assert np.array_equal(got["flux_sq"][2], Q) and np.array_equal(got["flux_xa"][2], Cx)


# ---------------------------------------------------------------------------------------------------
# the C boundary and the Python surface
def _structs():
    from adiabatic_raytracer_amd._lib import EventReweightOut, EventRowsIn, TreeOpts
    d = (C.c_double * 64)()
    a = C.addressof(d)
    ein = EventRowsIn(4, 0, a, a, a, a, a, a, a, 4, a, a, None, 0, None, None)
    ro = EventReweightOut(a, 50, 0, a, None, None, a, None, None, None, None, None, None, None, None)
    opts = TreeOpts(5, 5, 50, -1, 64, 0, 1e-10, 1769)
    return d, ein, ro, opts


def _call(lib, cp, ein, start, opts, g, ro, n=None):
    arr = (C.c_double * max(len(g), 1))(*g) if g is not None else None
    ref = lambda v: C.byref(v) if v is not None else None  # noqa: E731
    return lib.art_event_reweight_device(ref(cp), ref(ein), start, ref(opts), len(g) if n is None else n, arr, ref(ro), None)


def test_event_reweight_argument_checks_need_no_device():
    import adiabatic_raytracer_amd as A
    from adiabatic_raytracer_amd._lib import SkySpec
    lib = A.load_library()
    cp = A.Params(g_agg=1e-11).to_c()
    d, ein, ro, opts = _structs()
    start = C.c_void_p(C.addressof(d))
    g = [1e-11, 2e-11]
    assert _call(lib, None, ein, start, opts, g, ro) == INVALID and b"params" in lib.art_last_error()
    assert _call(lib, cp, None, start, opts, g, ro) == INVALID and b"NULL in, out or opts" in lib.art_last_error()
    assert _call(lib, cp, ein, start, opts, g, None) == INVALID and b"NULL in, out or opts" in lib.art_last_error()
    assert _call(lib, cp, ein, start, None, g, ro) == INVALID and b"NULL in, out or opts" in lib.art_last_error()
    assert _call(lib, cp, ein, start, opts, None, ro, n=2) == INVALID and b"couplings is NULL" in lib.art_last_error()
    assert _call(lib, cp, ein, start, opts, g, ro, n=0) == INVALID and b"n_couplings" in lib.art_last_error()
    assert _call(lib, cp, ein, start, opts, [1e-11] * 33, ro) == INVALID and b"n_couplings" in lib.art_last_error()
    for v in (0.0, -1e-11, float("nan"), float("inf")):
        assert _call(lib, cp, ein, start, opts, [1e-11, v], ro) == INVALID and b"every coupling" in lib.art_last_error()
        bad_g0 = A.Params(g_agg=v).to_c()
        assert _call(lib, bad_g0, ein, start, opts, g, ro) == INVALID and b"base coupling" in lib.art_last_error()

    def bad(msg, start=start, **kw):
        _, i, o, _ = _structs()
        for k, v in kw.items():
            setattr(i if hasattr(i, k) else o, k, v)
        assert _call(lib, cp, i, start, opts, g, o) == INVALID, msg
        assert msg.encode() in lib.art_last_error(), (msg, lib.art_last_error())

    bad("n_events must be", n_events=-1)
    bad("n_nodes must be", n_nodes=-1)
    bad("n_nodes must be", n_nodes=2 ** 31)
    bad("nbins must be", nbins=4097)
    bad("reserved must be 0", reserved=1)
    bad("node_start is NULL", start=None)
    bad("totals is NULL", totals=None)
    bad("erg is NULL", erg=None)
    bad("flux is NULL", flux=None)
    bad("NULL input buffer", weight5=None)
    bad("flux_sq or flux_xa", moment_totals=C.addressof(d))
    good = dict(n_theta=4, n_phi=8, n_dw=3, theta_axis=1, mode=0, dw_lo=-1e-6, dw_hi=1e-6)
    for msg, kw in {"bin counts": dict(good, n_theta=0), "theta_axis": dict(good, theta_axis=2), "sky_hist is NULL": good}.items():
        spec = SkySpec(**kw)
        bad(msg, sky=C.pointer(spec))
    # no events: ART_OK after the checks, nothing touched
    _, i, o, _ = _structs()
    i.n_events = i.n_nodes = 0
    o.flux = o.totals = o.erg = None
    assert _call(lib, cp, i, None, opts, g, o) == 0


def test_symbol_struct_and_python_surface():
    import adiabatic_raytracer_amd as A
    from adiabatic_raytracer_amd import _lib, trees
    from adiabatic_raytracer_amd.engine import Engine
    lib = A.load_library()
    assert "art_event_reweight_device" in _lib.SIGNATURES and hasattr(lib, "art_event_reweight_device")
    assert C.sizeof(_lib.EventReweightOut) == 2 * 4 + 13 * 8
    assert len(_lib.REWEIGHT_TOTALS) == 6 and lib.art_abi_version() == 1
    run = inspect.signature(Engine.run_events).parameters
    assert run["couplings"].kind is inspect.Parameter.KEYWORD_ONLY and run["couplings"].default is None
    assert inspect.signature(trees.main_runner_tree).parameters["couplings"].default is None
    er = inspect.signature(Engine.event_reweight).parameters
    assert list(er)[:6] == ["self", "sample", "weight5", "back", "forward", "couplings"]
    assert er["mc_nodes"].kind is inspect.Parameter.KEYWORD_ONLY and er["mc_nodes"].default is inspect.Parameter.empty
    for k, v in dict(event_offset=0, nbins=50, sky=None, errors=False, cyclotron_rerun=None, scan=None).items():
        assert er[k].kind is inspect.Parameter.KEYWORD_ONLY and er[k].default == v, k
    # a bad list is refused before any work: run_events checks it first (no engine is needed to see that)
    src = inspect.getsource(Engine.run_events)
    assert src.index("self._couplings(couplings)") < src.index("self.sample(")
    # the host paths have no forests in HBM to reweight
    for kw in ({}, {"device_trees": True}):
        with pytest.raises(ValueError, match="device_events"):
            trees.main_runner_tree(A.Params(), 3, couplings=[1e-12], **kw)


def test_scan_result_and_curve():
    from adiabatic_raytracer_amd import trees
    K, nbins = 3, 4
    rng = np.random.default_rng(2)
    raw = {"g": [5e-12, 1e-11, 3e-11], "n_events": 10, "flux": rng.random((K, 2 * nbins)), "sky": None,
           "totals": np.array([[1.0, 2.0, 9.5, 1, 0, 0], [2.0, 4.0, 10.0, 1, 0, 0], [3.0, 8.0, 7.0, 1, 0, 0]])}
    res = trees.scan_result(raw, 1e-11, 20)
    assert np.array_equal(res["scale"], (np.array(raw["g"]) / 1e-11) ** 2) and res["scale"][1] == 1.0
    assert np.array_equal(res["flux"], (raw["flux"] / 20.0).reshape(K, 2, nbins))
    assert np.array_equal(res["coverage"], [0.95, 1.0, 0.7]) and res["saturated"] == 1 and res["unlinked"] == 0
    g, p, s = trees.coupling_curve(res)
    assert np.array_equal(g, raw["g"]) and np.array_equal(p, [0.1, 0.2, 0.4]) and s is None
    assert np.array_equal(trees.coupling_curve(res, species=AXION)[1], [0.05, 0.1, 0.15])
    # with moments: σ per coupling by moments_sigma, and the vector for the all-reduce round-trips
    mt = np.tile(np.array([10.0, 20.0, 50.0, 0.3, 0.9, 0.5, 1.5, 0.0]), (K, 1))
    raw.update(flux_sq=rng.random((K, 2 * nbins)), flux_xa=rng.random((K, 2 * nbins)), sky_sq=None, sky_xa=None,
               moment_totals=mt)
    res = trees.scan_result(raw, 1e-11, 20)
    for k in range(K):
        ref = trees.moments_sigma(raw["flux"][k], raw["flux_sq"][k], raw["flux_xa"][k], 20, 50.0, 10.0)
        assert np.array_equal(res["flux_sigma"][k].reshape(-1), ref, equal_nan=True)
    assert trees.coupling_curve(res)[2].shape == (K,)
    back = trees.scan_unpack(2.0 * trees.scan_pack(raw), raw)
    assert back["n_events"] == 20 and np.array_equal(back["flux"], 2.0 * raw["flux"]) and back["sky"] is None
    assert np.array_equal(back["moment_totals"], 2.0 * mt)
