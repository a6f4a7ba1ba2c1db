"""The device-resident tree driver without a GPU: art_grow_trees_device is exported, bound and
checks its arguments before it touches a device; and the per-tree step it runs one lane per tree
(csrc/art_tree_step.h), compiled for the host with a driver loop of its own (tools/treestep.cpp),
grows the trees oracle/tree.py's get_tree grows from the same canned segment outcomes.

The step test replaces the oracle module that get_tree calls by a stub: propagate and
get_prob_nonad answer from a table indexed by (tree, count) -- crossing or not, its position, k, t,
Δω and P_nonAD, the end radius, a |kc| > 1 flag -- and philox4x32_10 is the oracle's own. A group's
probabilities are the fixed function of the table that treestep.cpp computes. Both sides take exp
from the host's libm, so weights and probabilities must agree bit for bit."""
import ctypes as C
import math
import os
import sys
import types

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import treestep as ts  # noqa: E402

AXION, PHOTON = 0, 1


# ---------------------------------------------------------------- export, binding, argument checks
def _call(lib, p, n, x0, k0, erg, sp, opts, nn):
    return lib.art_grow_trees_device(p, n, x0, k0, erg, sp, opts, 0, None, None, None, None, nn, None)


def test_export_binding_and_argument_checks():
    import adiabatic_raytracer_amd as A
    from adiabatic_raytracer_amd import _lib
    lib = A.load_library()
    assert hasattr(lib, "art_grow_trees_device") and "art_grow_trees_device" in _lib.SIGNATURES
    cp = A.Params().to_c()
    p = C.byref(cp)
    good = lambda **kw: _lib.TreeOpts(**{**dict(num_cutoff=5, mc_nodes=5, max_nodes=50, splittings_cutoff=-1,  # noqa: E731
                                                crossing_cap=64, tree_offset=0, prob_cutoff=1e-10, seed=1769), **kw})
    o = C.byref(good())
    nn = C.c_int64(7)
    pnn = C.byref(nn)
    buf = np.zeros(8)
    d = buf.ctypes.data_as(C.c_void_p)
    cases = [
        ((None, 1, d, d, d, d, o, pnn), b"params"),
        ((p, 1, d, d, d, d, None, pnn), b"opts"),
        ((p, 1, d, d, d, d, o, None), b"n_nodes"),
        ((p, -1, d, d, d, d, o, pnn), b"n must be"),
        ((p, 1, None, d, d, d, o, pnn), b"input buffers"),
        ((p, 1, d, None, d, d, o, pnn), b"input buffers"),
        ((p, 1, d, d, None, d, o, pnn), b"input buffers"),
        ((p, 1, d, d, d, None, o, pnn), b"input buffers"),
        ((p, 1, d, d, d, d, C.byref(good(max_nodes=-1)), pnn), b"max_nodes"),
        ((p, 1, d, d, d, d, C.byref(good(crossing_cap=-1)), pnn), b"crossing_cap"),
        ((p, 1, d, d, d, d, C.byref(good(splittings_cutoff=100000, num_cutoff=5)), pnn), b"no device form"),
    ]
    for args, word in cases:
        assert _call(lib, *args) == -1, word  # ART_E_INVALID, before any device is touched
        assert word in lib.art_last_error(), (word, lib.art_last_error())
    # no roots and nothing to write: ART_OK without a device, as the host forest
    assert _call(lib, p, 0, None, None, None, None, o, pnn) == 0 and nn.value == 0


def test_python_surface():
    """Engine.grow_trees and nodes_to_numpy exist, grow_trees and main_runner_tree take the switch,
    and main_runner_tree refuses tree dumps with it before any work."""
    import inspect
    import adiabatic_raytracer_amd as A
    from adiabatic_raytracer_amd import engine, trees
    assert "node_capacity" in inspect.signature(engine.Engine.grow_trees).parameters
    assert inspect.signature(trees.grow_trees).parameters["device"].default is False
    assert inspect.signature(trees.main_runner_tree).parameters["device_trees"].default is False
    with pytest.raises(ValueError, match="tree dumps"):
        trees.main_runner_tree(A.Params(theta_m=0.2, flat=True), 3, saveMode=3, dir_tag="unused", device_trees=True)
    rec = np.zeros(3, trees.NODE_DTYPE)
    rec["tree"] = [0, 0, 1]
    import torch
    back = engine.nodes_to_numpy(torch.from_numpy(rec.view(np.uint8).reshape(3, -1)))
    assert back.dtype == trees.NODE_DTYPE and np.array_equal(back["tree"], [0, 0, 1])


# ---------------------------------------------------------------- the step against get_tree
def _group_pn(x, row, mk):
    """treestep.cpp's GroupProbTable::eval, operation by operation."""
    s = 0.05 + 0.1 * row
    s = s + 0.01 * mk
    return s + 1e-3 * abs(x)


class _Stub:
    """Stands in for oracle.oracle inside oracle.tree: segments and probabilities from the table."""

    def __init__(self, oracle_lib, tab):
        self.philox4x32_10 = oracle_lib.philox4x32_10
        self.tab = tab
        self.tree, self.calls = 0, 0

    def start(self, tree):
        self.tree, self.calls = tree, 0

    def get_prob_nonad(self, p, pos, kpos, erg_eff, group_start=None):
        if group_start is None:  # the root (:134)
            return np.array([self.tab["root_pn"][self.tree]])
        mk = len(erg_eff)
        x = np.asarray(pos, np.float64).reshape(3, mk)[0]
        return np.array([_group_pn(x[r], r, mk) for r in range(mk)])

    def propagate(self, p, x, k, erg, dw, ln_t0, species, max_crossings=-1, cap=1, nthreads=None):
        t, step = self.tab, self.calls
        self.calls += 1
        i = self.tree
        nc = int(t["ncross"][i, step])
        out = {"x_end": np.array([t["r_end"][i, step], 0.0, 0.0]), "k_end": np.array([0.0, 0.0, 1e-5]),
               "u7_end": np.array([-1e-5]), "status": np.array([1 if nc else 0], np.int32),
               "n_cross": np.array([nc], np.int32), "xc_pos": np.full(3 * cap, np.nan), "xc_k": np.full(3 * cap, np.nan),
               "xc_t": np.full(cap, np.nan), "xc_dw": np.full(cap, np.nan), "xc_p": np.full(cap, np.nan)}
        for q in range(min(nc, cap)):
            c = t["xc"][i, step, q]
            out["xc_pos"].reshape(3, cap)[:, q] = c[0:3]
            out["xc_k"].reshape(3, cap)[:, q] = c[3:6]
            out["xc_t"][q], out["xc_dw"][q], out["xc_p"][q] = c[6], c[7], c[8]
        return out


def _table(n, steps, xcap=1, seed=0, p_cross=0.6, pn_log10=(-3.0, 0.5)):
    """Random outcomes: a segment crosses with probability p_cross (P_nonAD log-uniform), else ends
    either far out (final) or at the star."""
    rng = np.random.default_rng(seed)
    tab = {"root_pn": rng.uniform(0.01, 2.0, n), "ncross": (rng.random((n, steps)) < p_cross).astype(np.int32),
           "xc": np.zeros((n, steps, xcap, 9)), "r_end": np.where(rng.random((n, steps)) < 0.7, 50.0, 10.5)}
    for i in range(n):
        for s in range(steps):
            for q in range(xcap):
                tab["xc"][i, s, q] = [15.0 + i + 0.01 * s + 0.5 * q, 1.0 + 0.25 * q, 2.0, 1e-5, -2e-6, 3e-6,
                                      1e-4 * (s + 1) * (q + 1), -1.0 - 0.01 * s - 0.001 * q,
                                      10.0 ** rng.uniform(*pn_log10)]
    return tab


def _compare(oracle_lib, monkeypatch, tab, *, num_cutoff=5, mc_nodes=5, max_nodes=50, splittings_cutoff=-1,
             crossing_cap=64, prob_cutoff=1e-10, seed=1769, tree_offset=0):
    from adiabatic_raytracer_amd import _lib
    from adiabatic_raytracer_amd.trees import NODE_DTYPE
    from oracle import tree as T
    n = len(tab["root_pn"])
    opts = _lib.TreeOpts(num_cutoff, mc_nodes, max_nodes, splittings_cutoff, crossing_cap, tree_offset, prob_cutoff, seed)
    nodes, counts, infos, depth, over = ts.run(opts, NODE_DTYPE, tab["root_pn"], tab["ncross"], tab["xc"], tab["r_end"])
    assert over == 0
    stub = _Stub(oracle_lib, tab)
    monkeypatch.setattr(T, "O", stub)
    p = types.SimpleNamespace(rNS=10.0)
    ref = []
    for i in range(n):
        stub.start(i)
        root = T.Node(np.array([20.0 + i, 0.0, 0.0]), np.array([1e-5, 0.0, 0.0]), 0.0, -1.0, PHOTON, 1.0, 1.0, -1.0,
                      -1.0, -1.0)
        ref.append(T.get_tree(p, root, 1e-5, tree_offset + i, num_cutoff=num_cutoff, prob_cutoff=prob_cutoff,
                              splittings_cutoff=splittings_cutoff, MC_nodes=mc_nodes, max_nodes=max_nodes,
                              cap=max(1, crossing_cap), seed=seed))
    assert len(nodes) == sum(len(t[0]) for t in ref)
    o = 0
    for i, (tree, count, info) in enumerate(ref):
        g = nodes[o:o + len(tree)]
        o += len(tree)
        assert np.all(g["tree"] == i) and counts[i] == count and infos[i] == info, (i, counts[i], count, infos[i], info)
        sig_g = [(int(a), int(b), int(c)) for a, b, c in zip(g["species"], g["is_final"], g["n_cross"])]
        sig_o = [(e.species, int(e.is_final), len(e.xc)) for e in tree]
        assert sig_g == sig_o, (i, sig_g, sig_o)
        for q, e in enumerate(tree):  # bit for bit: both sides use the host's exp
            assert g["weight"][q] == e.weight and g["prob"][q] == e.prob, (i, q)
            assert g["parent_weight"][q] == e.parent_weight and g["prob_conv"][q] == e.prob_conv
            assert g["prob_conv0"][q] == e.prob_conv0 and g["t0"][q] == e.t and g["dw0"][q] == e.dw
            assert np.array_equal(g["x0"][q], e.x) and g["status"][q] == e.status
            if e.xc:
                assert np.array_equal(g["xc"][q], e.xc[0][0]) and g["pc"][q] == e.xc[0][4]
    return nodes, counts, infos, depth, ref


def test_every_segment_crosses_reaches_the_stack_bound_and_info_4(oracle_lib, monkeypatch):
    n, max_nodes = 5, 6
    tab = _table(n, max_nodes + 2, seed=1, p_cross=1.0, pn_log10=(-1.0, 0.3))
    _, counts, infos, depth, _ = _compare(oracle_lib, monkeypatch, tab, num_cutoff=50, mc_nodes=1000, max_nodes=max_nodes)
    assert np.all(infos == 4) and np.all(counts == max_nodes + 1)
    # the derived bound min(max(mc_nodes, 0), max_nodes + 1) + 1 is reached, and is what the stack is sized to
    assert depth == max_nodes + 2 == ts.stack_capacity(1000, max_nodes)
    assert ts.stack_capacity(2, 50) == 3 and ts.stack_capacity(0, 50) == 1 and ts.stack_capacity(-4, 50) == 1
    assert ts.stack_capacity(5, 2) == 4 and ts.stack_capacity(5, 50, split_all=True) == 1


def test_stack_overflow_is_reported_not_dropped():
    from adiabatic_raytracer_amd import _lib
    from adiabatic_raytracer_amd.trees import NODE_DTYPE
    tab = _table(2, 8, seed=1, p_cross=1.0)
    opts = _lib.TreeOpts(50, 1000, 6, -1, 64, 0, 1e-10, 1769)
    *_, over = ts.run(opts, NODE_DTYPE, tab["root_pn"], tab["ncross"], tab["xc"], tab["r_end"], stack_cap=3)
    assert over == 1


def test_equal_weights_keep_push_order(oracle_lib, monkeypatch):
    # P = 1/2 exactly: both children of every split weigh the same, so only the stable order decides
    pn = next(v for v in (math.log(2.0), np.nextafter(math.log(2.0), 0), np.nextafter(math.log(2.0), 1))
              if 1.0 - math.exp(-v) == 0.5)
    n, steps = 4, 40
    tab = _table(n, steps, seed=2, p_cross=0.0)
    tab["r_end"][:] = 50.0
    for i in range(n):
        tab["ncross"][i, :3 + i] = 1
    tab["xc"][..., 8] = pn
    nodes, counts, _, _, ref = _compare(oracle_lib, monkeypatch, tab, num_cutoff=50, mc_nodes=1000, max_nodes=30)
    w = nodes["weight"][nodes["tree"] == n - 1]
    assert len(set(w.tolist())) < len(w)  # ties did occur
    # the order shows in the species sequence, which _compare held equal
    assert any(len({e.species for e in t[0]}) == 2 for t in ref)


def test_rare_fail_node_mid_tree(oracle_lib, monkeypatch):
    tab = _table(6, 60, seed=3)
    tab["ncross"][:, :3] = 1
    tab["xc"][:, 1, 0, 3] = 2.0  # |kc| > 1 on every tree's second segment
    tab["xc"][2, 0, 0, 4] = -1.5  # and on one root
    nodes, _, _, _, ref = _compare(oracle_lib, monkeypatch, tab, mc_nodes=1000, max_nodes=50)
    for i in range(len(ref)):
        g = nodes[nodes["tree"] == i]
        q = 0 if i == 2 else 1  # the rare node: recorded without crossings though its segment ended on one
        assert len(g) > q and g["n_cross"][q] == 0 and g["status"][q] == 1
        assert len(g) == 1 if i == 2 else len(g) > 2  # a root's rare fail ends its tree; later ones go on


def test_prob_cutoff_gives_info_2(oracle_lib, monkeypatch):
    tab = _table(4, 60, seed=4)
    tab["ncross"][0, 0] = 0  # a root that escapes at once: tot_prob = 1
    tab["r_end"][0, 0] = 50.0
    _, _, infos, _, _ = _compare(oracle_lib, monkeypatch, tab, mc_nodes=1000, prob_cutoff=0.5)
    assert infos[0] == 2 and np.all(np.abs(infos) >= 1)


def test_num_cutoff_gives_info_3(oracle_lib, monkeypatch):
    tab = _table(4, 60, seed=5, p_cross=0.3, pn_log10=(-3.0, -2.0))
    tab["ncross"][:, 0] = 1  # P ~ 1e-3: the unconverted branch ends first and leaves tot_prob < 1 - 1e-10
    tab["ncross"][:, 1] = 0
    _, _, infos, _, _ = _compare(oracle_lib, monkeypatch, tab, num_cutoff=1, mc_nodes=1000)
    assert np.all(infos == 3)


@pytest.mark.parametrize("mc_nodes", [0, 2])
def test_monte_carlo(oracle_lib, monkeypatch, mc_nodes):
    tab = _table(24, 60, seed=6 + mc_nodes, p_cross=0.7, pn_log10=(-1.5, 0.5))
    _, counts, infos, depth, ref = _compare(oracle_lib, monkeypatch, tab, mc_nodes=mc_nodes, tree_offset=1000)
    assert depth <= ts.stack_capacity(mc_nodes, 50)
    assert np.any(infos < 0) and np.any(counts > mc_nodes + 1)
    # both branches of the draw were taken somewhere
    kinds = {(a.species == b.species) for t in ref for a, b in zip(t[0], t[0][1:])}
    assert kinds == {True, False}


def test_split_all_root(oracle_lib, monkeypatch):
    """The backtrace form: only the root, every crossing merged and grouped, weight = prod(1 - P_j)."""
    cap = 6
    ncs = [0, 1, 2, 5, 5, 9]  # none; one; two; five; five with a close pair (and the last pair); over the cap
    n = len(ncs)
    tab = _table(n, 2, xcap=cap, seed=9)
    tab["ncross"][:, 0] = ncs
    tab["xc"][4, 0, 2, 0:3] = tab["xc"][4, 0, 1, 0:3] + [3e-6, 0.0, -4e-6]  # 5e-6 km apart: one crossing
    tab["xc"][4, 0, 4, 0:3] = tab["xc"][4, 0, 3, 0:3] + [0.0, 9e-6, 0.0]
    tab["xc"][2, 0, 1, 0:3] = tab["xc"][2, 0, 0, 0:3] + [0.0, 2e-5, 0.0]  # 2e-5 km apart: stays two
    nodes, counts, infos, depth, ref = _compare(oracle_lib, monkeypatch, tab, num_cutoff=0, splittings_cutoff=100000,
                                                crossing_cap=cap)
    assert len(nodes) == n and np.all(counts == 1) and depth <= 1
    assert nodes["n_cross"].tolist() == [0, 1, 2, 5, 3, cap]
    for i in (2, 3, 4, 5):  # grouped: the fixed function of the table, and the product of (1 - P)
        P = [1.0 - math.exp(-_group_pn(c[0][0], r, len(ref[i][0][0].xc))) for r, c in enumerate(ref[i][0][0].xc)]
        w = 1.0
        for v in P:
            w = w * (1.0 - v)
        assert nodes["weight"][i] == w and nodes["pc"][i] == P[0]
    assert nodes["pc"][1] == 1.0 - math.exp(-tab["xc"][1, 0, 0, 8])  # Nc = 1: the crossing buffer's value
