"""Trees and events on the GPU engine: the host side of main_runner_tree (MainRunner.jl:354-763).

grow_trees()        get_tree (MainRunner.jl:126-352) for many trees at once, through the
                    native batched driver art_grow_trees (csrc/art_forest.cpp), or with
                    device=True through art_grow_trees_device, every tree's state in HBM.
main_runner_tree()  the event loop: sample conversion points, weight them (sln_prob),
                    backtrace each one (axion, -k, -B0, every crossing), grow its forward
                    photon tree, and write the reference's npy rows, with the same columns
                    and the same file name (MainRunner.jl:715-761), so Combine_Files.py and
                    plot/*.py read them unchanged.
"""
from __future__ import annotations

import ctypes as C
import math
import os
from dataclasses import replace

import numpy as np

from . import _lib
from ._lib import TreeOpts, TreeTraj, check
from .raytracer import Params, event_weight, propagate_batch, sample_conversion_points

AXION, PHOTON = 0, 1


# include/art.h art_tree_node, as a numpy record (checked against the C layout in tests)
NODE_DTYPE = np.dtype([
    ("tree", np.int32), ("species", np.int32), ("is_final", np.int32), ("n_cross", np.int32),
    ("status", np.int32), ("pad", np.int32),
    ("weight", np.float64), ("prob", np.float64), ("parent_weight", np.float64), ("prob_conv", np.float64),
    ("prob_conv0", np.float64),
    ("x0", np.float64, 3), ("k0", np.float64, 3), ("t0", np.float64), ("dw0", np.float64),
    ("x_end", np.float64, 3), ("k_end", np.float64, 3), ("u7_end", np.float64), ("tau_end", np.float64),
    ("xc", np.float64, 3), ("kc", np.float64, 3), ("tc", np.float64), ("dwc", np.float64), ("pc", np.float64),
], align=True)


def grow_trees(params: Params, x0, k0, erg, species, *, num_cutoff=5, mc_nodes=5, max_nodes=50,
               splittings_cutoff=-1, crossing_cap=64, prob_cutoff=1e-10, seed=1769, ntimes=None, tree_offset=0,
               device=False):
    """get_tree for n roots RT.node(x0, k0, 0, -1, species, 1, 1, -1, -1, -1) (MainRunner.jl:578-590,
    :653-667). x0, k0: (n, 3) or SoA 3n; erg: erg_inf_ini per root. Returns (nodes, counts,
    infos): nodes is a NODE_DTYPE record array grouped by tree in get_tree's push order.
    With ntimes (>= 2, saveMode 3) a fourth item holds every node's saveNode data
    (art_grow_trees_traj): traj (nodes, ntimes, 3) Cartesian saved points, times (nodes,
    ntimes) their ln t, count (nodes,), xc (nodes, cap, 4) the kept crossings (x, y, z, tc).
    tree_offset: global id of root 0 (the Monte-Carlo draws are keyed by the global tree id).
    device: grow the forest with every tree's state in HBM (art_grow_trees_device through
    Engine.grow_trees: one batched launch per round and no per-round copies) instead of the host
    forest; the same arguments and the same three results. It has no trajectory form (ntimes) and
    takes the forward and the backtrace form only (not splittings_cutoff > 0 with num_cutoff > 0)."""
    x0, k0 = np.asarray(x0, np.float64), np.asarray(k0, np.float64)
    erg = np.ascontiguousarray(erg, np.float64).reshape(-1)
    n = erg.size
    if x0.ndim == 2:
        x0, k0 = x0.T, k0.T
    x0, k0 = np.ascontiguousarray(x0).reshape(-1), np.ascontiguousarray(k0).reshape(-1)
    sp = np.ascontiguousarray(np.broadcast_to(np.asarray(species, np.int8), (n,)))
    if device:
        if ntimes:
            raise ValueError("grow_trees: device=True has no trajectory form (ntimes)")
        import torch
        from .engine import Engine, nodes_to_numpy
        eng = Engine(params)
        up = lambda a: torch.from_numpy(a).to(eng.device)  # noqa: E731
        r = eng.grow_trees(up(x0), up(k0), up(erg), up(sp), num_cutoff=num_cutoff, mc_nodes=mc_nodes, max_nodes=max_nodes,
                           splittings_cutoff=splittings_cutoff, crossing_cap=crossing_cap, prob_cutoff=prob_cutoff,
                           seed=seed, tree_offset=tree_offset)
        return nodes_to_numpy(r["nodes"]), r["counts"].cpu().numpy(), r["infos"].cpu().numpy()
    opts = TreeOpts(num_cutoff, mc_nodes, max_nodes, splittings_cutoff, crossing_cap, int(tree_offset), prob_cutoff,
                    seed)
    per_tree = 1 if (splittings_cutoff > 0 and num_cutoff <= 0) else max_nodes + 2
    cap = max(1, n * per_tree)
    lib = _lib.load()
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    xcap = max(1, crossing_cap) if splittings_cutoff > 0 else 1
    while True:
        nodes = np.zeros(cap, NODE_DTYPE)
        nn = C.c_int64(0)
        counts, infos = np.zeros(n, np.int32), np.zeros(n, np.int32)
        if ntimes:
            tr = {"traj": np.zeros((cap, ntimes, 3)), "times": np.zeros((cap, ntimes)),
                  "count": np.zeros(cap, np.int32), "xc": np.zeros((cap, xcap, 4))}
            tt = TreeTraj(int(ntimes), xcap, *[ptr(tr[k]) for k in ("traj", "times", "count", "xc")])
            rc = lib.art_grow_trees_traj(C.byref(params.to_c()), n, ptr(x0), ptr(k0), ptr(erg), ptr(sp),
                                         C.byref(opts), cap, ptr(nodes), C.byref(nn), ptr(counts), ptr(infos),
                                         C.byref(tt))
        else:
            rc = lib.art_grow_trees(C.byref(params.to_c()), n, ptr(x0), ptr(k0), ptr(erg), ptr(sp), C.byref(opts),
                                    cap, ptr(nodes), C.byref(nn), ptr(counts), ptr(infos))
        if rc == -3 and nn.value > cap:  # ART_E_NOMEM: grow and redo (pathological trees only)
            cap = nn.value
            continue
        check(rc)
        if ntimes:
            return nodes[:nn.value], counts, infos, {k: v[:nn.value] for k, v in tr.items()}
        return nodes[:nn.value], counts, infos


def _angles(v):
    a = np.linalg.norm(v, axis=-1)
    return np.arccos(v[..., 2] / a), np.arctan2(v[..., 1], v[..., 0]), a


def jl(x) -> str:
    """Julia's string(::Float64): shortest round-trip digits, scientific notation (1.0e14,
    2.0e-5) outside [1e-4, 1e6)."""
    x = float(x)
    if x == 0.0:
        return "-0.0" if math.copysign(1.0, x) < 0 else "0.0"
    if not math.isfinite(x):
        return "NaN" if math.isnan(x) else ("Inf" if x > 0 else "-Inf")
    if 1e-4 <= abs(x) < 1e6:
        r = repr(x)
        return r if ("." in r or "e" in r) else r + ".0"
    m, e = np.format_float_scientific(x, unique=True, trim="-").split("e")
    return f"{m if '.' in m else m + '.0'}e{int(e)}"


def tree_file_name(dir_tag, Mass_a, Ax_g, θm, ωPul, B0, Ntajs, ntimes, num_cutoff, MC_nodes, max_nodes, file_tag):
    """The npy name of MainRunner.jl:750-760, with Julia's number formatting."""
    name = (f"tree_MassAx_{jl(Mass_a)}_AxionG_{jl(Ax_g)}_ThetaM_{jl(θm)}_rotPulsar_{jl(ωPul)}_B0_{jl(B0)}"
            f"_Ax_trajs_{int(Ntajs)}_N_Times_{int(ntimes)}_num_cutoff_{int(num_cutoff)}_MC_nodes_{int(MC_nodes)}"
            f"_max_nodes_{int(max_nodes)}_{file_tag}.npy")
    return os.path.join(dir_tag, "npy", name)


def _write_event_text(dir_tag, file_tag, n_ev, s, w, x, k, tree, fin, ev, wgt, ident, counts, elapsed=None,
                      ev_offset=0):
    """event_<file_tag> and final_<file_tag> of saveMode > 1 (MainRunner.jl:438-444, 592-609,
    690-702, 735-741), Julia number formatting. The reference's per-event wall time
    time() - time0 has no per-event meaning in a batched run; the mean per event is written."""
    d = os.path.join(dir_tag, "event")
    os.makedirs(d, exist_ok=True)
    v = s["vifty"].reshape(3, n_ev).T
    t_ev = 0.0 if elapsed is None else elapsed / max(1, n_ev)
    with open(os.path.join(d, "event_" + file_tag), "w") as fe:
        for i in range(n_ev):
            vals = [*v[i], w["sln_prob"][i], *x[i], *(-k[i]), *x[i], *k[i]]
            fe.write(f"{ev_offset + i + 1} " + " ".join(jl(a) for a in vals) + f" {jl(t_ev)} {int(counts[i])}\n")
    θf, ϕf, absf = _angles(fin["k_end"])
    θfX, ϕfX, absfX = _angles(fin["x_end"])
    # node.t: the root's is the integer literal 0 of RT.node(..., 0, ...) (MainRunner.jl:661)
    first = np.zeros(len(tree), bool)
    first[np.r_[0, np.flatnonzero(np.diff(tree["tree"])) + 1]] = True
    is_root = first[tree["is_final"] != 0]
    with open(os.path.join(d, "final_" + file_tag), "w") as ff:
        for q in range(len(fin)):
            t = "0" if is_root[q] else jl(fin["t0"][q])
            vals = [θf[q], ϕf[q], absf[q], θfX[q], ϕfX[q], absfX[q]]
            ff.write(f"{ev_offset + int(ev[q]) + 1} {jl(wgt[q])} {int(ident[q])} " + " ".join(jl(a) for a in vals) + f" {t}\n")


SPECIES_NAME = {AXION: "axion", PHOTON: "photon"}


def save_node(fh, node, tr, q):
    """saveNode(f, n) (MainRunner.jl:17-65) for node q of a grow_trees(..., ntimes) result:
    species, weight, prob, parent_weight; the crossing x, y, z and tc lines (or "-" x 3);
    the saved trajectory's x, y, z and ln t lines. Julia number formatting."""
    fh.write(f"{SPECIES_NAME[int(node['species'])]} {jl(node['weight'])} {jl(node['prob'])} "
             f"{jl(node['parent_weight'])}\n")
    m = min(int(node["n_cross"]), tr["xc"].shape[1])
    if m > 0:
        for c in range(3):
            fh.write("".join("  " + jl(tr["xc"][q, j, c]) for j in range(m)) + "\n")
        fh.write("".join("  " + jl(tr["xc"][q, j, 3]) for j in range(m)))
    else:
        fh.write("-\n-\n-")
    fh.write("\n")
    cnt = int(tr["count"][q])
    for c in range(3):
        fh.write("".join("  " + jl(tr["traj"][q, k, c]) for k in range(cnt)) + "\n")
    fh.write("".join("  " + jl(tr["times"][q, k]) for k in range(cnt)) + "\n")


def _sky_keywords(sky_map, device_events, world):
    """main_runner_tree's sky_map keywords completed and checked (None: no map). Without a dw_range n_dw > 1 bins
    over the rows' own (min, max), which device_events cannot do, nor more than one process."""
    if sky_map is None:
        return None
    sky_kw = {"n_theta": 32, "n_phi": 64, "n_dw": 1, "theta_axis": "cos", "dw_range": None}
    if set(sky_map) - set(sky_kw):
        raise ValueError(f"sky_map: unknown keys {sorted(set(sky_map) - set(sky_kw))}")
    sky_kw.update(sky_map)
    _theta_range(sky_kw["theta_axis"])
    if sky_kw["n_dw"] > 1 and sky_kw["dw_range"] is None:
        if device_events:
            raise ValueError("sky_map: device_events bins on the device as it goes: n_dw > 1 needs a dw_range")
        if world > 1:
            raise ValueError("sky_map: n_dw > 1 needs a dw_range when world > 1 (the ranks' rows span different Δω)")
    return sky_kw


def main_runner_tree(params: Params, Ntajs: int, *, seed=1769, ntimes=1000, rho_DM=0.45, n_maxSample=6,
                     num_cutoff=5, MC_nodes=5, max_nodes=50, prob_cutoff=1e-10, saveMode=0, dir_tag=None,
                     file_tag="", backtrace_cap=256, rank=0, world=1, nbins=50, run_info=None, cyclotron=False,
                     sky_map=None, device_trees=False, device_events=False, halo=None, errors=False,
                     couplings=None, halos=None, replicates=None, grid=False, spectrum=None, exact=False, origin_map=None):
    """main_runner_tree (MainRunner.jl:354-763) for Ntajs - 1 events (the reference's
    `while photon_trajs < desired_trajs` loop), all events batched on the GPU. Returns the
    row matrix (13 columns, 29 with saveMode > 0) after the final division of column 8 by
    f_inx, and writes it to the reference's npy path when dir_tag is given; saveMode > 1
    also writes the event_/final_ text files and saveMode > 2 one tree_<file_tag><event>
    file per event with saveNode of the backtrace node and of every forward-tree node
    (MainRunner.jl:573-577, :612, :671), each segment saved at ntimes points.

    Sharding, world > 1 with torch.distributed initialised (one process per
    GPU): the Ntajs - 1 events of ONE logical run are split by global event id
    (shard.shard_range). Rank r samples its block (Philox keyed by the global event id),
    backtraces it and grows its trees (Monte-Carlo draws keyed by the global tree id), and
    numbers its rows by global event id, so the ranks' rows in rank order are the
    single-process rows. f_inx (MainRunner.jl:469,477,711-713) is all-reduced and column 8
    is divided by the GLOBAL f_inx (:747): the normalisation of one large run, not the
    per-file /Nruns of Gen_Samples.jl:220. Rank r writes file_tag + str(r) (:750-761).

    run_info (a dict, optional) receives the run's reduced totals: f_inx (global), the
    binned radiated flux of plot/flux.py:38-48 -- np.histogram(φf, nbins, range=(-π, π),
    weights = weight * sln_prob) of the rows, axions in flux[0], photons in flux[1], after
    the f_inx division, binned on the GPU and summed over ranks in the same all-reduce --
    Σ weight * sln_prob per species and the global row count.

    cyclotron (beyond the reference, which writes opticalDepth = 0, MainRunner.jl:703-708): the
    escaping photons' cyclotron-resonance optical depth τ (cyclotron_optical_depth) goes into
    column 14 (saveMode > 0) and column 8, the weight (weight_tmp, :707-708), is multiplied by
    exp(-τ), so the flux of run_info is the absorbed one; columns 13 (the tree weight) and 15
    (weightC) stay. With the default False every row, file and histogram is unchanged.

    sky_map (beyond the reference; a dict of sky_map()'s keywords n_theta, n_phi, n_dw, theta_axis,
    dw_range, or {} for its defaults): the rows' flux binned over (θf or cos θf, φf, Δω) per species
    with the weights of run_info["flux"], summed over the ranks in the same all-reduce and divided
    by the global f_inx: run_info["sky_map"] (2, n_theta, n_phi, n_dw) and run_info["sky_map_edges"];
    with dir_tag also saved beside the npy as skymap_<its stem>.npz (sky_map, theta_edges, phi_edges,
    dw_edges, theta_axis, f_inx). n_dw > 1 without a dw_range bins Δω over (min, max) of the rows
    (numpy's rule, flux_range), which only one process can do: with world > 1 it is an error. With
    the default None every row, file, run_info key and the reduced vector are unchanged.

    device_trees: grow the backtrace and the forward forest with every tree's state in HBM
    (grow_trees(..., device=True), art_grow_trees_device) instead of the host forest. Tree dumps
    (saveMode > 2 with a dir_tag) need trajectories, which that driver does not save: ValueError.
    With the default False every row, file and run_info key is unchanged.

    device_events: the rank's block of events runs through Engine.run_events: sampler, weights, both
    forests, the rows, the flux and the sky map stay in HBM (art_event_rows_device), the rows come to the
    host once, for the npy file and the return value, and the raw flux, sky map and totals feed the same
    all-reduce. The event_/final_ text files of saveMode > 1 need per-node data on the host: with a
    dir_tag that is a ValueError. A sky map with n_dw > 1 needs a dw_range. With the default False every
    row, file and run_info key is unchanged.

    halo (a raytracer.Halo, beyond the reference): the events' speeds at infinity are drawn from the halo
    velocity model and their weights carry its importance ratio (sample_conversion_points, event_weight),
    on all three paths; column 12 is then u7_end/m_a + |vifty|²/2 event by event ("Halo
    velocity model"). With the default None every row, file and run_info key is unchanged.

    errors (beyond the reference): the Monte-Carlo standard errors of the reduced estimates, on all three
    paths: run_info["flux_sigma"] (2, nbins), ["sky_map_sigma"] (with a sky map, also saved into the
    skymap npz) and ["sum_weight_sln_prob_sigma"] (2), by moments_sigma from per-event second moments
    (event_moments; the event, not the row, is the independent unit) that follow the sky map in the same
    all-reduce: σ comes from the global tables, the global f_inx and the global number of events. The
    host paths bin the rows' own columns with numpy's rule; device_events takes the tables from
    art_event_moments_device. With the default False every row, file, run_info key and the reduced vector
    are unchanged.

    couplings (beyond the reference, which sweeps --Axg with one process per value; device_events only,
    ValueError on the other two paths): a list of 1 to 32 values of g_agg to which the run's forests, grown
    at params.g_agg, are reweighted in HBM (Engine.run_events(couplings=); DESIGN.md §3, "Coupling scan").
    run_info["coupling_scan"] is scan_result's dict from the tables summed over the ranks, which follow
    everything else in the same all-reduce; the rows and files are those of params.g_agg. With the default
    None every row, file, run_info key and the reduced vector are unchanged.

    halos (beyond the reference; device_events only, ValueError on the other two paths; needs halo=, the base): a
    list of 1 to 32 raytracer.Halo to which the run, sampled and weighted under `halo`, is reweighted in HBM
    (Engine.run_events(halos=); DESIGN.md §3, "Halo scan"). run_info["halo_scan"] is halo_scan_result's dict from
    the tables summed over the ranks, which follow everything else in the same all-reduce; the rows and files
    are those of `halo`. With the default None every row, file, run_info key and the reduced vector are
    unchanged.

    replicates (beyond the reference; a group count R, 2 to 64; DESIGN.md §3, "Jackknife replicates"): the run's
    first-moment tables per group of events, g = global event id mod R, on all three paths: run_info["replicates"] is
    replicates_result's dict from the tables summed over the ranks, which end the vector of the same all-reduce, and
    jackknife(run_info["replicates"], fn) gives the value and error of any function of the flux, the sky map and the
    totals. The host paths take the tables from the rows (rows_replicates with the sampler's attempts); device_events
    takes them from art_event_replicates_device, and there the scans' dicts get "replicates" too. With the default
    None every row, file, run_info key and the reduced vector are unchanged.

    grid (beyond the reference; device_events only, ValueError on the other two paths; needs couplings=, halos= and
    halo=; DESIGN.md §3, "Coupling x halo grid"): the run's first-moment tables at every (coupling, halo model) cell
    (Engine.run_events(grid=True)), with the per-group tables under replicates= and the moment totals under errors=.
    run_info["grid"] is grid_result's dict from the tables summed over the ranks, the last part of the vector of the
    same all-reduce; limit_band(run_info["grid"], power) reads the limit on g per halo model off it. With the default
    False every row, file, run_info key and the reduced vector are unchanged.

    spectrum (beyond the reference; {} or a dict of sub_bits, 0 to 4, and top, 0 to 256; DESIGN.md §3, "Event power
    spectrum"): the distribution of the per-event power, on all three paths: run_info["spectrum"] is spectrum_result's
    dict -- the histogram over range-free bins, n_eff, the top events with their global ids and the share of the
    power they carry, and the Hill tail index α -- from the tables summed over the ranks and the ranks' lists merged,
    the last parts of the vector of the same all-reduce. The host paths take the tables from the rank's rows
    (rows_spectrum); device_events takes them from art_event_spectrum_device, and there the scans' dicts get
    "spectrum" too. With the default None every row, file, run_info key and the reduced vector are unchanged.

    exact (beyond the reference; needs device_events=True; DESIGN.md §3, "Exact tables"): the flux table, the sky map
    and the totals also as the correctly rounded exact sums of the same row powers (Engine.run_events(exact=True)),
    which do not depend on the order of the adds, the chunks or the number of ranks. The ranks' normalised limbs are
    integers below 2^32, which float64 holds exactly, and their sums over the ranks too: they ride as the LAST part of
    the vector of the same all-reduce and are converted back and rounded after it. run_info["exact"] is exact_result's
    dict of host arrays, and the scans' dicts get "exact" too. On the other two paths the tables are built on the host
    and exact=True is a ValueError: rows_exact gives the same tables from their rows. With the default False every
    row, file, run_info key and the reduced vector are unchanged.

    origin_map (beyond the reference; {} or a dict of origin_spec's origin keys plus an optional observer=dict(n_theta,
    n_phi, theta_axis); DESIGN.md §3, "Emission maps"): the power per species over where its event converted (columns 9
    to 11, in the magnetic or the rotation frame) and, with observer, jointly over the direction it left in, on all
    three paths: device_events takes Engine.run_events' table (art_event_origin_device), the other two bin their rows
    with rows_origin. The rank's raw table rides as the LAST part of the vector of the same all-reduce, after `exact`,
    and run_info["origin"] is origin_result's dict of the reduced table: map (divided by the global f_inx), raw, edges,
    spec, misplaced. The scans, the grid, errors and the spectrum get no origin table. With the default None every
    row, file, run_info key and the reduced vector are unchanged."""
    ospec = None
    if origin_map is not None:  # (before any work is done)
        ospec = origin_spec({k: v for k, v in origin_map.items() if k != "observer"}, origin_map.get("observer"), params)
    if exact and not device_events:
        raise ValueError("exact: the exact tables are accumulated from forests held in HBM and need device_events=True "
                         "(trees.rows_exact gives the same tables from the rows of the other paths)")
    if spectrum is not None:
        spectrum_keywords(spectrum)  # (before any work is done)
    if grid and not device_events:
        raise ValueError("grid: the coupling x halo grid is formed from forests held in HBM and needs device_events=True")
    if grid and (couplings is None or halos is None or halo is None):
        raise ValueError("grid: the coupling x halo grid needs couplings=, halos= and halo= (the base)")
    if replicates is not None and not _lib.REPLICATES_MIN_GROUPS <= int(replicates) <= _lib.REPLICATES_MAX_GROUPS:
        raise ValueError(f"replicates: {_lib.REPLICATES_MIN_GROUPS} to {_lib.REPLICATES_MAX_GROUPS} groups, not {replicates!r}")
    if couplings is not None and not device_events:
        raise ValueError("couplings: the coupling scan reweights forests held in HBM and needs device_events=True")
    if halos is not None:
        if not device_events:
            raise ValueError("halos: the halo scan reweights a run held in HBM and needs device_events=True")
        halos = halo_scan_models(halo, halos)
    if device_events:
        if saveMode > 1 and dir_tag is not None:
            raise ValueError("device_events: the text files and tree dumps of saveMode > 1 with a dir_tag need the "
                             "nodes on the host")
        return _main_runner_tree_device(params, Ntajs, seed=seed, rho_DM=rho_DM, n_maxSample=n_maxSample,
                                        num_cutoff=num_cutoff, MC_nodes=MC_nodes, max_nodes=max_nodes,
                                        prob_cutoff=prob_cutoff, saveMode=saveMode, dir_tag=dir_tag, file_tag=file_tag,
                                        backtrace_cap=backtrace_cap, rank=rank, world=world, nbins=nbins, run_info=run_info,
                                        cyclotron=cyclotron, sky_map=sky_map, halo=halo, errors=errors,
                                        couplings=couplings, halos=halos, replicates=replicates,
                                        **({"grid": True} if grid else {}),
                                        **({} if spectrum is None else {"spectrum": spectrum}),
                                        **({"exact": True} if exact else {}),
                                        **({} if origin_map is None else {"origin_map": origin_map}))
    if device_trees and saveMode > 2 and dir_tag is not None:
        raise ValueError("device_trees: tree dumps (saveMode > 2 with dir_tag) need the host forest's trajectories")
    if saveMode < 3:
        ntimes = 3  # "Times to store in ODE" (MainRunner.jl:379-381): also names the npy file
    sky_kw = _sky_keywords(sky_map, False, world)
    import time
    from .shard import shard_range
    t_start = time.perf_counter()
    n_glob = max(0, int(Ntajs) - 1)
    lo, hi = shard_range(n_glob, rank, world)
    n_ev = hi - lo
    tag = f"{file_tag}{rank}" if world > 1 else file_tag
    max_r = params.max_r()
    if max_r < params.rNS:
        raise ValueError("maxR < rNS: this neutron star has no conversion surface (MainRunner.jl:387-396)")
    s = sample_conversion_points(params, n_ev, seed=seed, ray_offset=lo, max_r=max_r, halo=halo)
    w = event_weight(params, s["x"], s["k_init"], s["vifty"], max_r=max_r, rho_DM=rho_DM, n_maxSample=n_maxSample,
                     halo=halo)
    x = s["x"].reshape(3, n_ev).T
    k = s["k_init"].reshape(3, n_ev).T
    erg = s["erg"]
    # f_inx: find_samples_new calls minus accepted samples (MainRunner.jl:463-481)
    f_inx = int(np.sum(s["attempts"].astype(np.int64) - 1))
    # backtrace: axion, -k, -B0, every crossing, only the root is processed (:578-590)
    dumps = saveMode > 2 and dir_tag is not None
    got = grow_trees(replace(params, B0=-params.B0), x, -k, erg, AXION, num_cutoff=0, splittings_cutoff=100000,
                     crossing_cap=backtrace_cap, prob_cutoff=prob_cutoff, seed=seed, ntimes=ntimes if dumps else None,
                     tree_offset=lo, device=device_trees)
    nb, c_bck = got[0], got[1]
    samp_back_weight = nb["prob"] * nb["weight"]  # (:635)
    prob0 = nb["prob"]
    # forward photon tree from the sample (:653-667)
    fwd = grow_trees(params, x, k, erg, PHOTON, num_cutoff=num_cutoff, mc_nodes=MC_nodes, max_nodes=max_nodes,
                     prob_cutoff=prob_cutoff, seed=seed, ntimes=ntimes if dumps else None, tree_offset=lo,
                     device=device_trees)
    tree, counts, infos = fwd[:3]
    if dumps:  # saveMode > 2: one file per event, the backtrace node then the forward tree
        d = os.path.join(dir_tag, "tree")
        os.makedirs(d, exist_ok=True)
        for e in range(n_ev):
            with open(os.path.join(d, f"tree_{file_tag}{lo + e + 1}"), "w") as fh:
                save_node(fh, nb[e], got[3], e)
                for q in np.flatnonzero(tree["tree"] == e):
                    save_node(fh, tree[q], fwd[3], q)
    fin = tree[tree["is_final"] != 0]
    ev = fin["tree"]
    θf, ϕf, _ = _angles(fin["k_end"])
    θfX, ϕfX, absfX = _angles(fin["x_end"])
    wgt = fin["weight"] * samp_back_weight[ev]  # tree[ii].weight *= samp_back_weight (:690)
    wgt_tree = wgt  # column 13
    ident = np.where(fin["species"] == AXION, 0.0, 1.0)
    tau_c = np.zeros_like(wgt)
    if cyclotron:
        tau_c = cyclotron_optical_depth(params, fin, erg[ev])
        wgt = wgt * np.exp(-tau_c)
    f_inx += int(np.sum(ident == 1.0))
    dω = fin["u7_end"] / params.mass_a + w["vel_eng"][ev]  # (:713)
    photon_trajs = lo + ev + 1.0  # global event number
    cols = [photon_trajs, ident, θf, ϕf, θfX, ϕfX, absfX, w["sln_prob"][ev], wgt, x[ev, 0], x[ev, 1], x[ev, 2], dω]
    if saveMode > 0:
        zero = np.zeros_like(wgt)
        cols += [wgt_tree, zero + tau_c, zero + 1.0, k[ev, 0], k[ev, 1], k[ev, 2], w["cos_w"][ev], counts[ev].astype(float),
                 infos[ev].astype(float), fin["prob"], fin["prob_conv"], fin["prob_conv0"], samp_back_weight[ev],
                 absfX, c_bck[ev].astype(float), prob0[ev]]
    rows = np.stack(cols, axis=1) if len(fin) else np.zeros((0, len(cols)))
    if saveMode > 1 and dir_tag is not None:
        _write_event_text(dir_tag, tag, n_ev, s, w, x, k, tree, fin, ev, wgt, ident, counts,
                          elapsed=time.perf_counter() - t_start, ev_offset=lo)
    # the run's totals: [flux (2 nbins, weight * sln_prob before the f_inx division) | f_inx |
    # Σ weight * sln_prob (axions, photons) | rows], ONE sum over the ranks
    # the binned flux (a GPU histogram) only when someone reads it: the reduced run_info, or the
    # other ranks' sum (every rank must contribute its part); f_inx alone normalises column 8
    want_flux = len(rows) and (world > 1 or run_info is not None)
    flux = radiated_flux(rows[:, 3], rows[:, 1], rows[:, 8] * rows[:, 7], nbins) if want_flux else np.zeros(2 * nbins)
    pps = rows[:, 8] * rows[:, 7] if len(rows) else np.zeros(0)
    sky = None
    if sky_kw is not None:  # the rows' sky map, the flux's weights (every rank adds its part)
        if sky_kw["n_dw"] > 1 and sky_kw["dw_range"] is None:
            sky_kw["dw_range"] = flux_range(rows[:, 12])
        sky = np.zeros((2, sky_kw["n_theta"], sky_kw["n_phi"], sky_kw["n_dw"]))
        if len(rows):
            sky = _sky_map_rows(rows[:, 2], rows[:, 3], rows[:, 12], rows[:, 1], pps, **sky_kw)
    mom = rows_moments(rows, lo, s["attempts"], nbins, sky_kw) if errors else None
    tot = pack_totals(flux, f_inx, pps[rows[:, 1] == 0].sum() if len(rows) else 0.0,
                      pps[rows[:, 1] == 1].sum() if len(rows) else 0.0, len(rows), sky, mom)
    path = None if dir_tag is None else tree_file_name(dir_tag, params.mass_a, params.g_agg, params.theta_m, params.omega_pul,
                                                       params.B0, Ntajs, ntimes, num_cutoff, MC_nodes, max_nodes, tag)
    rep = None if replicates is None else {"run": rows_replicates(rows, replicates, nbins, sky_kw, s["attempts"], lo)}
    spec = None if spectrum is None else {"run": rows_spectrum(rows, *spectrum_keywords(spectrum), event_lo=lo, n_events=n_ev)}
    return _finish_run(rows, tot, nbins=nbins, sky_kw=sky_kw, errors=errors, world=world, run_info=run_info,
                       events=(lo, hi), n_events=n_glob, g0=params.g_agg, path=path, **({} if rep is None else {"replicates": rep}),
                       **({} if spec is None else {"spectrum": spec, "rank": rank}),
                       **({} if ospec is None else {"origin": (rows_origin(rows, ospec), ospec)}))


def _main_runner_tree_device(params, Ntajs, *, seed, rho_DM, n_maxSample, num_cutoff, MC_nodes, max_nodes, prob_cutoff,
                             saveMode, dir_tag, file_tag, backtrace_cap, rank, world, nbins, run_info, cyclotron, sky_map,
                             halo=None, errors=False, couplings=None, halos=None, replicates=None, grid=False,
                             spectrum=None, exact=False, origin_map=None):
    """main_runner_tree(device_events=True): the rank's events through Engine.run_events, then the same
    totals vector, all-reduce, division, run_info and files as the host assembly."""
    from .engine import Engine
    from .shard import shard_range
    sky_kw = _sky_keywords(sky_map, True, world)
    ntimes = 3 if saveMode < 3 else 1000  # names the npy file only (main_runner_tree's default beyond saveMode 2)
    n_glob = max(0, int(Ntajs) - 1)
    lo, hi = shard_range(n_glob, rank, world)
    tag = f"{file_tag}{rank}" if world > 1 else file_tag
    r = Engine(params).run_events(hi - lo, seed=seed, event_offset=lo, saveMode=saveMode, num_cutoff=num_cutoff,
                                  MC_nodes=MC_nodes, max_nodes=max_nodes, prob_cutoff=prob_cutoff,
                                  backtrace_cap=backtrace_cap, rho_DM=rho_DM, n_maxSample=n_maxSample, nbins=nbins,
                                  sky_map=sky_kw, cyclotron=cyclotron, rows=True, halo=halo, errors=errors,
                                  **({} if couplings is None else {"couplings": couplings}),
                                  **({} if halos is None else {"halos": halos}),
                                  **({} if replicates is None else {"replicates": replicates}),
                                  **({"grid": True} if grid else {}),
                                  **({} if spectrum is None else {"spectrum": spectrum}),
                                  **({"exact": True} if exact else {}),
                                  **({} if origin_map is None else {"origin_map": origin_map}))
    xa = None
    if exact:
        xa = {"run": exact_raw(r["exact"]["acc"])}
        xa.update({k: exact_raw(r[k + "_scan"]["exact"]["acc"]) for k in ("coupling", "halo") if k + "_scan" in r})
    spec = None
    if spectrum is not None:
        spec = {"run": r["spectrum"]["raw"]}
        spec.update({k: r[k + "_scan"]["spectrum"]["raw"] for k in ("coupling", "halo") if k + "_scan" in r})
    rep = None
    if replicates is not None:
        rep = {"run": r["replicates"]["raw"]}
        rep.update({k: r[k + "_scan"]["replicates"]["raw"] for k in ("coupling", "halo") if k + "_scan" in r})
    rows = r["rows_raw"].cpu().numpy()
    t6 = r["totals"].cpu().numpy()
    tot = pack_totals(r["flux_raw"].cpu().numpy(), t6[4] + t6[1], t6[2], t6[3], t6[0],
                      None if sky_kw is None else r["sky_raw"].cpu().numpy(),
                      {k: (None if v is None else v.cpu().numpy()) for k, v in r["moments"].items()} if errors else None)
    path = None if dir_tag is None else tree_file_name(dir_tag, params.mass_a, params.g_agg, params.theta_m, params.omega_pul,
                                                       params.B0, Ntajs, ntimes, num_cutoff, MC_nodes, max_nodes, tag)
    return _finish_run(rows, tot, None if couplings is None else r["coupling_scan"]["raw"],
                       None if halos is None else r["halo_scan"]["raw"], nbins=nbins, sky_kw=sky_kw, errors=errors,
                       world=world, run_info=run_info, events=(lo, hi), n_events=n_glob, g0=params.g_agg, path=path,
                       **({} if rep is None else {"replicates": rep}), **({"grid": r["grid"]["raw"]} if grid else {}),
                       **({} if spec is None else {"spectrum": spec, "rank": rank}), **({} if xa is None else {"exact": xa}),
                       **({} if origin_map is None else {"origin": (r["origin"]["raw"], r["origin"]["spec"])}))


def cyclotron_optical_depth(params: Params, fin, erg) -> np.ndarray:
    """τ of the cyclotron resonance along the last segment of each final node (0 for axions): the
    photon nodes' segments (x0, k0, t0, dw0) run again in one batch through
    art_propagate_cyclotron_host, as get_tree ran them (art_forest.cpp: ln t0 = log(max(t0, e^-30)),
    max_crossings = -1). The observation is passive, so each re-run must end where its node did,
    bit for bit; that is asserted."""
    tau = np.zeros(len(fin))
    ph = np.flatnonzero(fin["species"] == PHOTON)
    if ph.size == 0:
        return tau
    f = fin[ph]
    dt0 = math.exp(-30.0)
    lnt = np.array([math.log(max(float(t), dt0)) for t in f["t0"]])
    res = propagate_batch(params, f["x0"].T, f["k0"].T, np.asarray(erg, np.float64)[ph], f["dw0"], lnt,
                          np.full(ph.size, PHOTON, np.int8), max_crossings=-1, cyclotron=True)
    same = (np.array_equal(res["x_end"].reshape(3, -1).T, f["x_end"], equal_nan=True)
            and np.array_equal(res["k_end"].reshape(3, -1).T, f["k_end"], equal_nan=True)
            and np.array_equal(res["u7_end"], f["u7_end"], equal_nan=True)
            and np.array_equal(res["tau_end"], f["tau_end"], equal_nan=True)
            and np.array_equal(res["status"], f["status"]))
    if not same:
        raise AssertionError("the cyclotron re-run of the final photon segments does not reproduce their end states")
    tau[ph] = res["cyc_tau"]
    return tau


def radiated_flux(phif, ident, weights, nbins=50, range=(-np.pi, np.pi)) -> np.ndarray:
    """The binned flux of plot/flux.py:38-48 on the GPU: np.histogram(phif, nbins,
    range=range, weights=weights) for axion rows (ident 0) and photon rows (ident 1), as a
    (2 * nbins,) array [axions | photons]. The reference's radiated flux is the photon half with
    weights = weight * sln_prob (npy columns 9 and 8). range=None bins like flux.py:43-47 itself,
    np.histogram(phif, bins=nbins) without a range: over [min φf, max φf] of ALL the rows
    (numpy's rule, ±0.5 when they are equal); `flux_edges` gives those edges."""
    import torch
    lib = _lib.load()
    n = len(phif)
    lo, hi = flux_range(phif) if range is None else (float(range[0]), float(range[1]))
    dev = torch.device("cuda", torch.cuda.current_device())
    f = lambda a, dt=torch.float64: torch.as_tensor(np.ascontiguousarray(a), dtype=dt).to(dev)  # noqa: E731
    ph, sp, ww = f(phif), f(np.asarray(ident) != 0, torch.int8), f(weights)
    hist = torch.zeros(2 * nbins, dtype=torch.float64, device=dev)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    check(lib.art_flux_histogram_phi_range_device(n, C.c_void_p(ph.data_ptr()), C.c_void_p(sp.data_ptr()),
                                                  C.c_void_p(ww.data_ptr()), int(nbins), lo, hi,
                                                  C.c_void_p(hist.data_ptr()), stream))
    return hist.cpu().numpy()


def flux_range(phif):
    """np.histogram's range when none is given: (min, max) of the data, widened by 0.5 on each
    side when they are equal, (0, 1) for no data."""
    a = np.asarray(phif, np.float64)
    if a.size == 0:
        return 0.0, 1.0
    lo, hi = float(a.min()), float(a.max())
    return (lo - 0.5, hi + 0.5) if lo == hi else (lo, hi)


def flux_edges(lo, hi, nbins=50):
    """The bin edges np.histogram uses for `nbins` equal bins of [lo, hi] (np.linspace)."""
    return np.linspace(lo, hi, nbins + 1)


def _theta_range(theta_axis):
    if theta_axis not in _lib.THETA_AXIS:
        raise ValueError(f"theta_axis must be 'cos' or 'theta', not {theta_axis!r}")
    return (-1.0, 1.0) if theta_axis == "cos" else (0.0, np.pi)


def sky_map_edges(n_theta=32, n_phi=64, n_dw=1, theta_axis="cos", dw_range=None):
    """The bin edges of sky_map's three axes, as np.histogramdd returns them (np.linspace):
    cos θf over [-1, 1] or θf over [0, π], φf over [-π, π], Δω over dw_range. With n_dw = 1 and no
    dw_range the Δω axis is one bin for every finite value: edges (-inf, inf)."""
    lo, hi = _theta_range(theta_axis)
    if dw_range is None:
        if n_dw != 1:
            raise ValueError("sky_map: n_dw > 1 needs dw_range")
        dw_edges = np.array([-np.inf, np.inf])
    else:
        dw_edges = np.linspace(float(dw_range[0]), float(dw_range[1]), n_dw + 1)
    return np.linspace(lo, hi, n_theta + 1), np.linspace(-np.pi, np.pi, n_phi + 1), dw_edges


def sky_map(theta_f, phi_f, dw, ident, weights=None, *, n_theta=32, n_phi=64, n_dw=1, theta_axis="cos", dw_range=None,
            mode=0) -> np.ndarray:
    """The sky map of npy rows on the GPU (art_histogram3_device): np.histogramdd of (θf or cos θf,
    φf, Δω) -- columns 2, 3 and 12 -- with `weights` (the radiated power: column 8 * column 7; None
    counts rows), for axion rows (ident 0, column 1) in [0] and photon rows in [1]: a
    (2, n_theta, n_phi, n_dw) array over sky_map_edges(...). theta_axis "cos" takes np.cos(theta_f) on
    the host, so the device bins numpy's values. A row outside a range, or NaN, on any axis is dropped;
    with n_dw = 1 and no dw_range every row with a finite Δω counts. mode: the accumulation path
    (0 by the table's size, 1 LDS, 2 HBM; include/art.h)."""
    import torch
    lib = _lib.load()
    th = np.asarray(theta_f, np.float64)
    a = np.cos(th) if theta_axis == "cos" else th
    c = np.asarray(dw, np.float64)
    lo, hi = _theta_range(theta_axis)
    if dw_range is None:
        if n_dw != 1:
            raise ValueError("sky_map: n_dw > 1 needs dw_range")
        c, dw_range = np.where(np.isfinite(c), 0.0, np.nan), (-1.0, 1.0)
    n = a.size
    dev = torch.device("cuda", torch.cuda.current_device())
    f = lambda v, dt=torch.float64: torch.as_tensor(np.ascontiguousarray(v), dtype=dt).to(dev)  # noqa: E731
    da, db, dc, sp = f(a), f(np.asarray(phi_f, np.float64)), f(c), f(np.asarray(ident) != 0, torch.int8)
    ww = None if weights is None else f(weights)
    hist = torch.zeros(2, n_theta, n_phi, n_dw, dtype=torch.float64, device=dev)
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
    check(lib.art_histogram3_device(n, ptr(da), ptr(db), ptr(dc), ptr(sp), ptr(ww), (C.c_int32 * 3)(n_theta, n_phi, n_dw),
                                    (C.c_double * 3)(lo, -np.pi, float(dw_range[0])),
                                    (C.c_double * 3)(hi, np.pi, float(dw_range[1])), int(mode), ptr(hist),
                                    C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    return hist.cpu().numpy()


_sky_map_rows = sky_map  # (main_runner_tree's keyword of the same name hides the function there)


def pulse_profile(sky, theta_obs, theta_axis="cos", species=PHOTON):
    """The pulse profile an observer at inclination theta_obs [rad] sees: the φf row of the θ bin
    that holds theta_obs (numpy's bin rule: an edge belongs to the bin on its right, π to the last),
    summed over Δω. The magnetosphere is stationary in the corotating frame and every sample starts at
    the same rotational phase, so φf at fixed θf is the rotational phase. With theta_axis "cos" the
    row is divided by the bin's solid angle (2 / n_theta)(2π / n_phi): power per steradian. Returns
    (profile, the φ bin centres). sky: (2, n_theta, n_phi, n_dw), as sky_map and run_info give it."""
    sky = np.asarray(sky)
    _, n_theta, n_phi, _ = sky.shape
    lo, hi = _theta_range(theta_axis)
    x = math.cos(theta_obs) if theta_axis == "cos" else float(theta_obs)
    if not lo <= x <= hi:
        raise ValueError(f"theta_obs = {theta_obs} lies outside the map")
    edges = np.linspace(lo, hi, n_theta + 1)
    row = min(int(np.searchsorted(edges, x, side="right")) - 1, n_theta - 1)
    prof = sky[species, row].sum(axis=-1)
    if theta_axis == "cos":
        prof = prof / ((2.0 / n_theta) * (2.0 * np.pi / n_phi))
    phi_edges = np.linspace(-np.pi, np.pi, n_phi + 1)
    return prof, 0.5 * (phi_edges[:-1] + phi_edges[1:])


def line_profile(sky, theta_obs, dw_range, theta_axis="cos", species=PHOTON, phase_resolved=False):
    """The line profile an observer at inclination theta_obs [rad] sees, pulse_profile's companion: the
    Δω rows of the θ bin that holds theta_obs (the same bin rule: an edge belongs to the bin on its
    right, the upper end to the last), as power per steradian per unit Δω -- divided by the solid angle
    of what is summed and by the Δω bin width (dw_range[1] - dw_range[0]) / n_dw. By default the φ
    bins are summed, the average over the rotation: shape (n_dw,), the solid angle the θ bin's whole
    ring. phase_resolved: one profile per φ bin, shape (n_phi, n_dw). With theta_axis "theta" the ring
    [θ_lo, θ_hi] spans 2π (cos θ_lo - cos θ_hi). Returns (profile, the Δω bin centres).
    sky: (2, n_theta, n_phi, n_dw), as sky_map and run_info give it, binned over dw_range."""
    sky = np.asarray(sky)
    _, n_theta, n_phi, n_dw = sky.shape
    lo, hi = _theta_range(theta_axis)
    x = math.cos(theta_obs) if theta_axis == "cos" else float(theta_obs)
    if not lo <= x <= hi:
        raise ValueError(f"theta_obs = {theta_obs} lies outside the map")
    d_lo, d_hi = float(dw_range[0]), float(dw_range[1])
    if not (np.isfinite(d_lo) and np.isfinite(d_hi) and d_lo < d_hi):
        raise ValueError("line_profile: dw_range needs finite lo < hi")
    edges = np.linspace(lo, hi, n_theta + 1)
    row = min(int(np.searchsorted(edges, x, side="right")) - 1, n_theta - 1)
    ring = 2.0 * np.pi * ((edges[row + 1] - edges[row]) if theta_axis == "cos"
                          else (math.cos(edges[row]) - math.cos(edges[row + 1])))
    width = (d_hi - d_lo) / n_dw
    if phase_resolved:
        prof = sky[species, row] / ((ring / n_phi) * width)
    else:
        prof = sky[species, row].sum(axis=0) / (ring * width)
    dw_edges = np.linspace(d_lo, d_hi, n_dw + 1)
    return prof, 0.5 * (dw_edges[:-1] + dw_edges[1:])


def event_moments(event, bins, power, size, trials=None):
    """The first and second moments of binned event power, the numpy statement of
    art_event_moments_device: event (per row, the integer id of the row's event), bins (per row, the
    flat label in a table of `size` bins; a negative label drops the row), power (per row, column 8 *
    column 7). The rows of one event are correlated, so per event e and bin b the content
    X = Σ power of e's rows in b is formed first (in row order). Returns (S, Q, C), each (size,):
    S = Σ_e X, Q = Σ_e X², C = Σ_e X a_e with a_e = trials[e], the event's part of f_inx
    (attempts - 1 + its photon rows), indexed by the ids in `event`. trials=None, for row files, which
    do not store the attempts: a_e is taken constant and C is None (moments_sigma's constant form)."""
    event, bins = np.asarray(event, np.int64).reshape(-1), np.asarray(bins, np.int64).reshape(-1)
    power = np.asarray(power, np.float64).reshape(-1)
    size = int(size)
    keep = bins >= 0
    event, bins, power = event[keep], bins[keep], power[keep]
    if bins.size and bins.max() >= size:
        raise ValueError("event_moments: a label lies outside the table")
    groups, inv = np.unique(event * size + bins, return_inverse=True)
    X = np.bincount(inv.reshape(-1), weights=power, minlength=groups.size)  # (adds in row order)
    gb, ge = groups % size, groups // size
    S = np.bincount(gb, weights=X, minlength=size)
    Q = np.bincount(gb, weights=X * X, minlength=size)
    if trials is None:
        return S, Q, None
    a = np.asarray(trials, np.float64).reshape(-1)
    return S, Q, np.bincount(gb, weights=X * a[ge], minlength=size)


def moments_sigma(S, Q, C, f_inx, A2, n_events):
    """The Monte-Carlo standard error of F = S / f_inx per bin, from event_moments' tables (or the
    device's): F is a ratio of two sums over n_events independent events, Σ_e X_e / Σ_e a_e, and its
    linearised (delta-method) error is
        σ = sqrt(max(Q - 2 F C + F² A2, 0) n / (n - 1)) / f_inx,        A2 = Σ_e a_e²,
    which is n / (n - 1) Σ_e (X_e - F a_e)² / f_inx² expanded; an event without a row in the bin adds
    (F a_e)², carried by A2. C = None (and A2 ignored): a_e constant, the textbook
    n / (n - 1) (Q - S² / n) / f_inx². NaN for n_events < 2 or f_inx <= 0. Under heavy-tailed weights a
    variance estimate is biased low (the largest weights are rarely drawn): read σ as a lower scale of
    the scatter. The bins of one event are correlated, so the σ of a sum of bins is not the quadrature
    sum of the bins' σ."""
    S, Q = np.asarray(S, np.float64), np.asarray(Q, np.float64)
    n, f = float(n_events), float(f_inx)
    if not (n >= 2 and f > 0):
        return np.full(S.shape, np.nan)
    if C is None:
        var = Q - S * S / n
    else:
        F = S / f
        var = Q - 2.0 * F * np.asarray(C, np.float64) + F * F * float(A2)
    return np.sqrt(np.maximum(var, 0.0) * (n / (n - 1.0))) / f


def reweight_nodes(nodes, node_start, x_nonad, scales, mc_nodes):
    """The numpy statement of art_event_reweight_device's per-tree reweight (csrc/art_event_reweight.h;
    DESIGN.md §3, "Coupling scan") over NODE_DTYPE records: tree e owns node_start[e] .. node_start[e + 1],
    in the order it processed them. x_nonad: per record, P_nonAD at the base coupling of the record's
    stored first crossing (xc, kc, erg |dwc|, e.g. by Engine.get_prob_nonad; read where n_cross > 0), so
    forests saved earlier can be reweighted too. scales: (g_k / g0)². The parent of a record is the one
    earlier record of its tree with n_cross > 0 whose (tc, xc) equal its (t0, x0) bit for bit; a child of
    the other species takes f = 1 - exp(-s x), one of the same species exp(-s x); W(root) = 1,
    W = f W(parent) where the parent was pop number <= mc_nodes, else W = W(parent) (f / f at s = 1).
    A record with n_cross > 1 took its pc from the group of its segment's crossings, which one stored
    crossing cannot give back: its exponent is -log(1 - pc) whatever x_nonad says (the grouped exponent is
    ∝ g² too), and with pc == 1 its children keep the probabilities 1 and 0 at every scale. The device and
    host drivers store one crossing per forward segment, so their records have n_cross <= 1.
    Returns (W (K, n_nodes), coverage (K, trees): Σ W over each tree's records with n_cross == 0, unlinked:
    the records without exactly one parent, whose W is 0)."""
    nodes = np.asarray(nodes)
    start = np.asarray(node_start, np.int64).reshape(-1)
    s = np.asarray(scales, np.float64).reshape(-1)
    x_nonad = np.array(x_nonad, np.float64).reshape(-1)
    grouped = nodes["n_cross"] > 1
    with np.errstate(divide="ignore"):
        x_nonad[grouped] = -np.log(1.0 - nodes["pc"][grouped])  # (inf for pc == 1: exp(-s inf) = 0)
    n, n_trees = len(nodes), len(start) - 1
    W, cov, unlinked = np.zeros((len(s), n)), np.zeros((len(s), n_trees)), 0
    bits = lambda v: np.ascontiguousarray(v, np.float64).view(np.uint64)  # noqa: E731
    own = np.concatenate([bits(nodes["t0"])[:, None], bits(nodes["x0"]).reshape(n, 3)], axis=1)
    cross = np.concatenate([bits(nodes["tc"])[:, None], bits(nodes["xc"]).reshape(n, 3)], axis=1)
    has, species = nodes["n_cross"] > 0, nodes["species"]

    def factor(converted, sv, x):
        e = np.exp(-(sv * x))
        return 1.0 - e if converted else e

    for t in range(n_trees):
        a, b = int(start[t]), int(start[t + 1])
        for j in range(a, b):
            if j == a:
                W[:, j] = 1.0
                continue
            cand = a + np.flatnonzero(has[a:j] & np.all(cross[a:j] == own[j], axis=1))
            if len(cand) != 1:
                unlinked += 1
                continue
            p = int(cand[0])
            converted = species[j] != species[p]
            f = factor(converted, s, x_nonad[p])
            if p - a + 1 > mc_nodes:
                f0 = factor(converted, 1.0, x_nonad[p])
                W[:, j] = W[:, p] * (f / f0 if f0 > 0.0 else 0.0)
            else:
                W[:, j] = f * W[:, p]
        cov[:, t] = W[:, a:b][:, ~has[a:b]].sum(axis=1)
    return W, cov, unlinked


def reweight_back(x_root, bweight, scales, x_single=None):
    """The backtrace factor of art_event_reweight_device per event and scale, (K, n): (1 - exp(-s x_root))
    bweight^s, with x_root the backtrace root's P_nonAD at the base coupling and bweight the backtrace node's
    stored weight (0 stays 0, 1 stays 1, and s = 1 takes the stored value). x_single (n, optional): the
    exponent of the backtrace's crossing where it has exactly one (its node stores it), NaN elsewhere:
    there bweight^s is exp(-s x_single), free of the rounding of the stored 1 - P."""
    s = np.asarray(scales, np.float64).reshape(-1, 1)
    x, w = np.asarray(x_root, np.float64).reshape(1, -1), np.asarray(bweight, np.float64).reshape(1, -1)
    with np.errstate(divide="ignore", invalid="ignore"):
        p = np.exp(s * np.log(w))
    if x_single is not None:
        xs = np.asarray(x_single, np.float64).reshape(1, -1)
        p = np.where(np.isnan(xs), p, np.exp(-(s * np.where(np.isnan(xs), 0.0, xs))))
    keep = (w == 0.0) | (w == 1.0) | (s == 1.0)
    return (1.0 - np.exp(-(s * x))) * np.where(keep, w + 0.0 * s, p)


SCAN_KEYS = ("flux", "sky", "totals", "flux_sq", "flux_xa", "sky_sq", "sky_xa", "moment_totals")


def _scan_raw(scan, **ident) -> dict:
    """A scan's dict (Engine.event_reweight's or event_halo_scan's) with its tables on the host (numpy): what adds
    over chunks and ranks, then `ident`, what the scan was made for, and the number of events"""
    out = {k: (None if scan[k] is None else (scan[k].cpu().numpy() if hasattr(scan[k], "cpu") else np.asarray(scan[k])))
           for k in SCAN_KEYS if k in scan}
    out.update(**ident, n_events=int(scan["n_events"]))
    return out


def scan_raw(scan) -> dict:
    """Engine.event_reweight's dict with its tables on the host (numpy): what adds over chunks and ranks"""
    return _scan_raw(scan, g=[float(v) for v in scan["g"]])


def scan_pack(raw) -> np.ndarray:
    """A rank's scan tables (scan_raw, halo_scan_raw) as one vector for the run's all-reduce: the tables there
    are, in SCAN_KEYS' order, then the number of events."""
    parts = [np.asarray(raw[k], np.float64).reshape(-1) for k in SCAN_KEYS if raw.get(k) is not None]
    return np.concatenate(parts + [np.array([float(raw["n_events"])])])


def _scan_unpack(vec, like) -> dict:
    """scan_pack's vector back into tables shaped like those of `like` (the rank's own raw dict), and n_events"""
    out, at = {}, 0
    for k in SCAN_KEYS:
        if k not in like:
            continue
        if like[k] is None:
            out[k] = None
            continue
        out[k] = np.asarray(vec[at:at + like[k].size]).reshape(like[k].shape)
        at += like[k].size
    out["n_events"] = int(round(vec[at]))
    return out


def scan_unpack(vec, like) -> dict:
    """scan_pack's vector back into a dict shaped like `like` (the rank's own scan_raw)"""
    return {"g": list(like["g"]), **_scan_unpack(vec, like)}


def _scan_result(raw, K, f_inx, first, own) -> dict:
    """What scan_result and halo_scan_result share, from raw tables over K sets: flux (K, 2, nbins) and sky_map,
    divided by f_inx, sum_weight_sln_prob (K, 2), f_inx, raw, and with moment tables the three σ per set
    (moments_sigma; the bins, a_e and f_inx are the run's own for every set). first: the scan's keys before these;
    own(tot): its keys from its totals (K, their width). Returns (the dict, tot, the moment totals or None)."""
    f = float(f_inx) if f_inx > 0 else 1.0
    tot = np.asarray(raw["totals"], np.float64).reshape(K, -1)
    nbins = raw["flux"].shape[1] // 2
    res = {**first, "flux": (raw["flux"] / f).reshape(K, 2, nbins), "sum_weight_sln_prob": tot[:, 0:2] / f, **own(tot),
           "f_inx": int(f_inx), "raw": raw}
    if raw.get("sky") is not None:
        res["sky_map"] = raw["sky"] / f
    if raw.get("moment_totals") is None:
        return res, tot, None
    mt = np.asarray(raw["moment_totals"], np.float64).reshape(K, -1)
    sig = lambda S, Q, Cx, k: moments_sigma(S, Q, Cx, f_inx, mt[k, 2], mt[k, 0])  # noqa: E731
    res["flux_sigma"] = np.stack([sig(raw["flux"][k], raw["flux_sq"][k], raw["flux_xa"][k], k)
                                  for k in range(K)]).reshape(K, 2, nbins)
    res["sum_weight_sln_prob_sigma"] = np.stack([sig(tot[k, 0:2], mt[k, 3:5], mt[k, 5:7], k) for k in range(K)])
    if raw.get("sky") is not None:
        res["sky_map_sigma"] = np.stack([sig(raw["sky"][k], raw["sky_sq"][k], raw["sky_xa"][k], k) for k in range(K)])
    return res, tot, mt


def scan_result(raw, g0, f_inx) -> dict:
    """The coupling scan of a run from its raw tables (scan_raw, summed over the ranks) and the run's
    f_inx: g, scale = (g / g0)² (K), flux (K, 2, nbins) and sky_map (K, the map's shape; with a map), both
    divided by f_inx, sum_weight_sln_prob (K, 2), coverage (K: the mean over the events of Σ W_k over the
    records that closed their tree's probability; 1 where the g0 run's stop rules cut nothing that
    matters at g_k), saturated (events whose backtrace weight underflowed to 0 at g0), unlinked,
    recomputed_differs, raw, and with moment tables flux_sigma, sky_map_sigma, sum_weight_sln_prob_sigma
    per coupling (moments_sigma; the bins, a_e and f_inx are those of the g0 run for every coupling)."""
    g = np.array(raw["g"], np.float64)
    q = g / float(g0)
    return _scan_result(raw, len(g), f_inx, {"g": g, "scale": q * q}, lambda tot: {
        "coverage": tot[:, 2] / max(int(raw["n_events"]), 1), "saturated": int(round(tot[0, 3])),
        "unlinked": int(round(tot[0, 4])), "recomputed_differs": int(round(tot[0, 5]))})[0]


def coupling_curve(scan, species=PHOTON):
    """(g, power, sigma or None) of a coupling scan (run_events' or run_info's "coupling_scan") for
    plotting: the radiated power Σ weight sln_prob / f_inx of `species` at every coupling, and its
    Monte-Carlo standard error when the scan was made with errors."""
    sp = 0 if species == AXION else 1
    sigma = scan.get("sum_weight_sln_prob_sigma")
    return scan["g"], scan["sum_weight_sln_prob"][:, sp], None if sigma is None else sigma[:, sp]


C_KM = 2.99792e5  # art_core.h's: vifty is u / c


def _halo_of(h):
    """(v0, (vx, vy, vz)) of a raytracer.Halo or of such a pair"""
    v0, v = (h.v0, h.v_ns) if hasattr(h, "v0") else h
    v = tuple(float(c) for c in v)
    if len(v) != 3:
        raise ValueError("halos: v_ns has three components")
    return float(v0), v


def halo_scan_models(base, halos) -> list:
    """The model list of a halo scan as [(v0, (vx, vy, vz)), ...], checked as art_event_halo_scan_device
    checks it (ValueError "halos: ..."): base, the raytracer.Halo the run is sampled and weighted with (None:
    there is nothing to reweight), 1 to 32 models, each v0 finite and positive and not above the base's
    proposal scale base.vp() -- beyond it a model's weights are unbounded in the drawn speed -- and each
    v_ns finite. A model's own v_prop plays no part."""
    if base is None:
        raise ValueError("halos: a halo scan reweights a run made with a halo model and needs halo=")
    models = [_halo_of(h) for h in halos]
    if not 1 <= len(models) <= _lib.HALO_SCAN_MAX_MODELS:
        raise ValueError(f"halos: 1 to {_lib.HALO_SCAN_MAX_MODELS} models, not {len(models)}")
    vp = base.vp()
    for v0, v in models:
        if not (math.isfinite(v0) and v0 > 0.0 and all(math.isfinite(c) for c in v)):
            raise ValueError("halos: every model needs a finite v0 > 0 and a finite v_ns")
        if v0 > vp:
            raise ValueError(f"halos: a model's v0 = {v0} exceeds the base's proposal scale {vp} (its weights are "
                             "unbounded under that proposal: give the base a larger v_prop)")
    return models


def halo_ratio(vifty, base, halos) -> np.ndarray:
    """The numpy statement of art_halo.h's halo_ratio, in its order of operations: R (K, n) of the n events
    whose sampler output vifty (3n, SoA: u / c) was drawn and weighted under `base`, for each model of
    `halos` (raytracer.Halo objects or (v0, v_ns) pairs):
        R = ((r r) r) exp(q_b - q_h),  r = v0_b / v0_h,  q = ((w0² + w1²) + w2²) / (v0 v0),  w = u + v_ns,
    with u = vifty C_KM. The proposal scale cancels. A model equal to the base gives exactly 1.0."""
    u = np.asarray(vifty, np.float64).reshape(3, -1) * C_KM

    def q(h):
        v0, v = h
        w0, w1, w2 = u[0] + v[0], u[1] + v[1], u[2] + v[2]
        return ((w0 * w0 + w1 * w1) + w2 * w2) / (v0 * v0)

    b = _halo_of(base)
    qb = q(b)
    out = np.empty((len(halos), u.shape[1]))
    for k, h in enumerate(halos):
        h = _halo_of(h)
        r = b[0] / h[0]
        out[k] = ((r * r) * r) * np.exp(qb - q(h))
    return out


def halo_scan_tables(rows_raw, ratio, nbins, sky_kw=None, event_lo=0) -> dict:
    """art_event_halo_scan_device's first-moment tables in numpy from the run's own rows (column 7 raw) and
    the ratios R (K, n_events) of the events event_lo .. event_lo + n_events: the power of a row under model
    k is column 8 * column 7 times R[k, its event], binned as the run's own tables are (hist_bins of column
    3, sky_bins). Returns flux (K, 2 nbins), sky (K, 2 n_theta n_phi n_dw; None without sky_kw) and totals
    (K, 2: Σ power of the axion and of the photon rows)."""
    rows, R = np.asarray(rows_raw, np.float64), np.atleast_2d(np.asarray(ratio, np.float64))
    K, nbins = R.shape[0], int(nbins)
    ev = np.rint(rows[:, 0]).astype(np.int64) - 1 - int(event_lo)
    sp = (rows[:, 1] != 0).astype(np.int64)
    p = rows[:, 8] * rows[:, 7]
    fb = hist_bins(rows[:, 3], nbins) if nbins > 0 else np.full(len(rows), -1)
    labels = [("flux", np.where(fb >= 0, sp * nbins + fb, -1), 2 * nbins), ("totals", sp, 2)]
    out = {"sky": None}
    if sky_kw is not None:
        kw = {k: sky_kw[k] for k in ("n_theta", "n_phi", "n_dw", "theta_axis", "dw_range") if k in sky_kw}
        size = 2 * kw.get("n_theta", 32) * kw.get("n_phi", 64) * kw.get("n_dw", 1)
        labels.append(("sky", sky_bins(rows[:, 2], rows[:, 3], rows[:, 12], rows[:, 1], **kw), size))
    for name, lab, size in labels:
        keep = lab >= 0
        out[name] = np.stack([np.bincount(lab[keep], weights=(p * R[k, ev])[keep], minlength=size) for k in range(K)])
    return out


def halo_scan_raw(scan) -> dict:
    """Engine.event_halo_scan's dict with its tables on the host (numpy): what adds over chunks and ranks"""
    return _scan_raw(scan, models=[_halo_of(h) for h in scan["models"]])


def halo_scan_pack(raw) -> np.ndarray:
    """A rank's halo-scan tables (halo_scan_raw) as one vector for the run's all-reduce: scan_pack's layout"""
    return scan_pack(raw)


def halo_scan_unpack(vec, like) -> dict:
    """halo_scan_pack's vector back into a dict shaped like `like` (the rank's own halo_scan_raw)"""
    return {**_scan_unpack(vec, like), "models": list(like["models"])}


def halo_scan_result(raw, f_inx) -> dict:
    """The halo scan of a run from its raw tables (halo_scan_raw, summed over the ranks) and the run's f_inx:
    models, flux (K, 2, nbins) and sky_map (K, the map's shape; with a map; pulse_profile and line_profile
    take sky_map[k]), both divided by f_inx, sum_weight_sln_prob (K, 2), ratio_sum and ratio_sq (K: Σ_e R and
    Σ_e R² over the events), misplaced (records outside their tree's range, which must be 0), f_inx, raw, and
    with moment tables flux_sigma, sky_map_sigma and sum_weight_sln_prob_sigma per model (moments_sigma; the
    bins, a_e and f_inx are the run's own for every model) and n_eff (K) = S_photon² / Q_photon, the Kish
    effective number of events behind the photon total: a small n_eff says the model lies far from the base."""
    models = list(raw["models"])
    res, tot, mt = _scan_result(raw, len(models), f_inx, {"models": models}, lambda tot: {
        "ratio_sum": tot[:, 2].copy(), "ratio_sq": tot[:, 3].copy(), "misplaced": int(round(tot[0, 4]))})
    if mt is not None:
        with np.errstate(divide="ignore", invalid="ignore"):
            res["n_eff"] = tot[:, 1] * tot[:, 1] / mt[:, 4]
    return res


def hist_bins(x, nbins, lo=-np.pi, hi=np.pi) -> np.ndarray:
    """np.histogram's bin of each x for nbins equal bins over [lo, hi]: an edge belongs to the bin on
    its right, hi to the last; -1 outside the range and for NaN."""
    x = np.asarray(x, np.float64)
    edges = np.linspace(lo, hi, int(nbins) + 1)
    i = np.searchsorted(edges, x, side="right") - 1
    i[x == edges[-1]] = int(nbins) - 1
    with np.errstate(invalid="ignore"):
        return np.where((x >= lo) & (x <= hi), i, -1)


def sky_bins(theta_f, phi_f, dw, ident, *, n_theta=32, n_phi=64, n_dw=1, theta_axis="cos", dw_range=None) -> np.ndarray:
    """The flat sky-map label of each npy row (columns 2, 3, 12 and 1), np.histogramdd's bins of what
    sky_map() hands the device: np.cos(θf) or θf, φf, Δω; -1 for a row the map does not count."""
    th = np.asarray(theta_f, np.float64)
    lo, hi = _theta_range(theta_axis)
    ia = hist_bins(np.cos(th) if theta_axis == "cos" else th, n_theta, lo, hi)
    ib = hist_bins(phi_f, n_phi)
    c = np.asarray(dw, np.float64)
    if dw_range is None:
        if n_dw != 1:
            raise ValueError("sky_map: n_dw > 1 needs dw_range")
        ic = np.where(np.isfinite(c), 0, -1)
    else:
        ic = hist_bins(c, n_dw, float(dw_range[0]), float(dw_range[1]))
    sp = (np.asarray(ident) != 0).astype(np.int64)
    flat = ((sp * n_theta + ia) * n_phi + ib) * n_dw + ic
    return np.where((ia >= 0) & (ib >= 0) & (ic >= 0), flat, -1)


def rows_moments(rows, event_lo, attempts, nbins, sky_kw=None) -> dict:
    """art_event_moments_device's tables in numpy from the npy rows of the events event_lo ..
    event_lo + len(attempts) (column 7 raw or divided alike: pass the powers' own rows): flux_sq,
    flux_xa, sky_sq, sky_xa (None without sky_kw) and totals (8), for pack_totals(moments=)."""
    n = len(attempts)
    ev = np.rint(rows[:, 0]).astype(np.int64) - 1 - int(event_lo)
    sp = (rows[:, 1] != 0).astype(np.int64)
    pps = rows[:, 8] * rows[:, 7]
    a = np.asarray(attempts, np.int64) - 1 + np.bincount(ev[sp == 1], minlength=n)
    fb = hist_bins(rows[:, 3], nbins)
    _, fq, fc = event_moments(ev, np.where(fb >= 0, sp * nbins + fb, -1), pps, 2 * nbins, a)
    _, tq, tc = event_moments(ev, sp, pps, 2, a)
    out = {"flux_sq": fq, "flux_xa": fc, "sky_sq": None, "sky_xa": None,
           "totals": np.array([n, a.sum(), (a * a).sum(), tq[0], tq[1], tc[0], tc[1], 0.0], np.float64)}
    if sky_kw is not None:
        size = 2 * sky_kw["n_theta"] * sky_kw["n_phi"] * sky_kw["n_dw"]
        _, out["sky_sq"], out["sky_xa"] = event_moments(ev, sky_bins(rows[:, 2], rows[:, 3], rows[:, 12], rows[:, 1], **sky_kw),
                                                        pps, size, a)
    return out


REPLICATE_KEYS = ("flux", "sky", "totals", "groups")


def rows_replicates(rows, R, nbins, sky_kw=None, attempts=None, event_lo=0, n_events=None) -> dict:
    """art_event_replicates_device's tables in numpy from npy rows (column 7 raw or divided alike: the tables are in
    the powers' own units): the oracle of the device tables, and the path for row files written earlier. The group
    of a row is (column 0 - 1) mod R, its event's 0-based global id mod R (2 <= R <= 64). Returns the raw dict of
    one set (kind "run"): flux (1, R, 2 nbins), sky (1, R, 2, n_theta, n_phi, n_dw; None without sky_kw), totals
    (1, R, 2: Σ power of all axion and photon rows) and groups (R, 3: the events n_g, a_g, 0). attempts (the
    sampler's, of the events event_lo .. event_lo + len(attempts)): a_g = Σ_e (attempts - 1 + the event's photon
    rows), whose sum is the f_inx of these events. attempts=None, for row files, which do not store them: a_e is
    taken constant, as moments_sigma(trials=None) takes it (a_g = n_g; jackknife scales it to f_inx), over the
    events event_lo .. event_lo + n_events (n_events=None: up to the last event that has a row)."""
    rows = np.asarray(rows, np.float64)
    R, nbins, lo = int(R), int(nbins), int(event_lo)
    if not _lib.REPLICATES_MIN_GROUPS <= R <= _lib.REPLICATES_MAX_GROUPS:
        raise ValueError(f"replicates: {_lib.REPLICATES_MIN_GROUPS} to {_lib.REPLICATES_MAX_GROUPS} groups, not {R}")
    gid = np.rint(rows[:, 0]).astype(np.int64) - 1  # the 0-based global id
    if attempts is not None:
        n = len(attempts)
    elif n_events is not None:
        n = int(n_events)
    else:
        n = int(gid.max()) + 1 - lo if len(rows) else 0
    if len(rows) and (gid.min() < lo or gid.max() >= lo + n):
        raise ValueError("rows_replicates: a row's event lies outside event_lo .. event_lo + n_events")
    g = gid % R
    sp = (rows[:, 1] != 0).astype(np.int64)
    p = rows[:, 8] * rows[:, 7]
    ev_g = np.arange(lo, lo + n, dtype=np.int64) % R
    groups = np.zeros((R, len(_lib.REPLICATE_GROUPS)))
    groups[:, 0] = np.bincount(ev_g, minlength=R)
    if attempts is None:
        groups[:, 1] = groups[:, 0]
    else:
        groups[:, 1] = (np.bincount(ev_g, weights=np.asarray(attempts, np.int64) - 1, minlength=R)
                        + np.bincount(g[sp == 1], minlength=R))
    fb = hist_bins(rows[:, 3], nbins) if nbins > 0 else np.full(len(rows), -1)
    labels = [("flux", np.where(fb >= 0, sp * nbins + fb, -1), 2 * nbins, (2 * nbins,)), ("totals", sp, 2, (2,))]
    out = {"kind": "run", "R": R, "sky": None, "groups": groups}
    if sky_kw is not None:
        kw = {k: sky_kw[k] for k in ("n_theta", "n_phi", "n_dw", "theta_axis", "dw_range") if k in sky_kw}
        shape = (2, kw.get("n_theta", 32), kw.get("n_phi", 64), kw.get("n_dw", 1))
        labels.append(("sky", sky_bins(rows[:, 2], rows[:, 3], rows[:, 12], rows[:, 1], **kw), int(np.prod(shape)), shape))
    for name, lab, size, shape in labels:
        keep = lab >= 0
        out[name] = np.bincount(g[keep] * size + lab[keep], weights=p[keep], minlength=R * size).reshape(1, R, *shape)
    return out


def replicates_raw(rep) -> dict:
    """Engine.event_replicates' dict with its tables on the host (numpy): what adds over chunks and ranks"""
    out = {k: (None if rep[k] is None else (rep[k].cpu().numpy() if hasattr(rep[k], "cpu") else np.asarray(rep[k])))
           for k in REPLICATE_KEYS}
    out.update(kind=rep["kind"], R=int(rep["R"]))
    return out


def replicates_pack(raw) -> np.ndarray:
    """A rank's replicate tables (replicates_raw, rows_replicates) as one vector for the run's all-reduce: the tables
    there are, in REPLICATE_KEYS' order"""
    return np.concatenate([np.asarray(raw[k], np.float64).reshape(-1) for k in REPLICATE_KEYS if raw.get(k) is not None])


def replicates_unpack(vec, like) -> dict:
    """replicates_pack's vector back into a dict shaped like `like` (the rank's own raw dict)"""
    out, at = {"kind": like["kind"], "R": like["R"]}, 0
    for k in REPLICATE_KEYS:
        if like.get(k) is None:
            out[k] = None
            continue
        out[k] = np.asarray(vec[at:at + like[k].size], np.float64).reshape(like[k].shape)
        at += like[k].size
    return out


def _replicate_tables(flux, sky, totals, f, squeeze):
    """The normalised tables jackknife hands to fn: flux (K, 2, nbins), sky_map, sum_weight_sln_prob (K, 2), each
    divided by f (NaN where f is 0); squeeze: without the leading axis (the plain run's one set)"""
    with np.errstate(divide="ignore", invalid="ignore"):
        div = (lambda t: t / f) if f != 0 else (lambda t: np.full(t.shape, np.nan))
        t = {"flux": div(flux.reshape(flux.shape[0], 2, flux.shape[-1] // 2)), "sum_weight_sln_prob": div(totals)}
        if sky is not None:
            t["sky_map"] = div(sky)
    return {k: v[0] for k, v in t.items()} if squeeze else t


def replicates_result(raw, f_inx) -> dict:
    """The jackknife replicates of a run from its raw tables (replicates_raw or rows_replicates, summed over the
    ranks) and the run's f_inx: R, kind, n_g and a_g (R), misplaced (records outside their tree's range, which must
    be 0), f_inx, raw, and the full estimates jackknife's fn is handed -- flux (2, nbins), sky_map (with a map) and
    sum_weight_sln_prob (2), the tables summed over the groups and divided by f_inx, with a scan's leading K axis
    where there is one. trees.jackknife(result, fn) gives the value and error of fn of these."""
    groups = np.asarray(raw["groups"], np.float64)
    S = {k: (None if raw.get(k) is None else np.asarray(raw[k], np.float64).sum(axis=1)) for k in ("flux", "sky", "totals")}
    res = {"R": int(raw["R"]), "kind": raw["kind"], "n_g": groups[:, 0].copy(), "a_g": groups[:, 1].copy(),
           "misplaced": int(round(groups[:, 2].sum())), "f_inx": int(f_inx), "raw": raw}
    res.update(_replicate_tables(S["flux"], S["sky"], S["totals"], float(f_inx), raw["kind"] == "run"))
    return res


EXACT_KEYS = ("flux", "sky", "totals", "origin")  # the accumulator tables of an exact dict, each (K, ..., 66) int64
# ("origin": the emission map's, with run_events(origin_map=, exact=True) only; a dict without it packs as before)
EXACT_PARTS = ("run", "coupling", "halo")  # the order of the exact parts of a rank's vector


def _exact_host(fn, *args):
    lib = _lib.load()
    rc = getattr(lib, fn)(*args)
    if rc != 0:
        raise _lib.ArtError(f"{fn}: {lib.art_last_error().decode()}")


def exact_add(values, bins=None, n_bins=1, acc=None):
    """values added exactly to the accumulators bins[i] of n_bins (art_exact_add_host, the host twin of the device
    adds; bins None: all to bin 0; a bin < 0 or >= n_bins is skipped). Returns (acc, nonfinite): acc (n_bins, 66)
    int64, normalised, ACCUMULATED into when given, and the number of NaNs and infinities, which are not added."""
    import ctypes as C
    values = np.ascontiguousarray(values, np.float64)
    if bins is not None:
        bins = np.ascontiguousarray(bins, np.int32)
        if bins.shape != values.shape:
            raise ValueError("exact_add: bins and values must have one length")
    if acc is None:
        acc = np.zeros((int(n_bins), _lib.EXACT_LIMBS), np.int64)
    if acc.shape != (int(n_bins), _lib.EXACT_LIMBS) or acc.dtype != np.int64 or not acc.flags.c_contiguous:
        raise ValueError("exact_add: acc must be a contiguous int64 (n_bins, 66) array")
    bad = C.c_int64(0)
    _exact_host("art_exact_add_host", values.size, None if bins is None else bins.ctypes.data, values.ctypes.data, int(n_bins),
                acc.ctypes.data, C.addressof(bad))
    return acc, int(bad.value)


def exact_normalize(acc):
    """Accumulators (..., 66) int64 carry-propagated in place (art_exact_normalize_host): every limb but the top one in
    [0, 2^32). The value does not change. Returns acc."""
    if acc.dtype != np.int64 or acc.shape[-1] != _lib.EXACT_LIMBS or not acc.flags.c_contiguous:
        raise ValueError("exact_normalize: acc must be a contiguous int64 (..., 66) array")
    _exact_host("art_exact_normalize_host", acc.size // _lib.EXACT_LIMBS, acc.ctypes.data)
    return acc


def exact_round(acc) -> np.ndarray:
    """The correctly rounded float64 sums of accumulators (..., 66) int64 (art_exact_round_host, the host twin of
    art_exact_finish_device): round-to-nearest-even of the exact sum. The accumulators are only read."""
    acc = np.ascontiguousarray(acc, np.int64)
    if acc.shape[-1] != _lib.EXACT_LIMBS:
        raise ValueError("exact_round: acc must be an int64 (..., 66) array")
    out = np.zeros(acc.shape[:-1])
    _exact_host("art_exact_round_host", out.size, acc.ctypes.data, out.ctypes.data)
    return out


def exact_raw(acc) -> dict:
    """Engine.event_exact's dict with its tensors on the host (numpy): what exact_merge adds over chunks and ranks"""
    host = lambda v: None if v is None else (v.cpu().numpy() if hasattr(v, "cpu") else np.asarray(v))  # noqa: E731
    out = {k: host(acc.get(k)) for k in EXACT_KEYS + ("nonfinite", "misplaced")}
    out["kind"] = acc["kind"]
    return out


def exact_merge(accs) -> dict:
    """The accumulator dicts (Engine.event_exact's, run_events' res["exact"]["acc"], rows_exact(acc=True)'s "acc") of
    chunks, ranks or files added limb by limb, in any order, and normalised: the accumulators of all their rows
    together. The dicts must be of one kind and one set of tables. Returns a host dict (exact_raw's)."""
    accs = [exact_raw(a) for a in accs]
    if not accs:
        raise ValueError("exact_merge: nothing to merge")
    first = accs[0]
    out = {"kind": first["kind"]}
    for a in accs[1:]:
        if a["kind"] != first["kind"] or any((a[k] is None) != (first[k] is None) or
                                             (a[k] is not None and a[k].shape != first[k].shape) for k in EXACT_KEYS):
            raise ValueError("exact_merge: the accumulators were made for another kind, other sets or other tables")
    for k in EXACT_KEYS:
        out[k] = None
        if first[k] is not None:
            total = np.zeros(first[k].shape, np.int64)
            for j, a in enumerate(accs):
                total += a[k]  # (normalised limbs: below 2^32 each)
                if j % (1 << 20) == (1 << 20) - 1:
                    exact_normalize(total)
            out[k] = exact_normalize(total)
    for k in ("nonfinite", "misplaced"):
        out[k] = np.sum([np.asarray(a[k], np.float64) for a in accs], axis=0)
    return out


def exact_finish(acc) -> dict:
    """The rounded tables of an accumulator dict on the host, the twin of Engine.exact_finish: flux_raw (K, 2, nbins),
    sky_raw (K, the map's shape; with a map) and totals_raw (K, 2), each entry the correctly rounded exact sum of its
    rows' powers, and nonfinite (K); kind "run": without the leading axis."""
    acc = exact_raw(acc)
    K = acc["flux"].shape[0]
    out = {"flux_raw": exact_round(acc["flux"]).reshape(K, 2, -1), "totals_raw": exact_round(acc["totals"])}
    if acc["sky"] is not None:
        out["sky_raw"] = exact_round(acc["sky"])
    if acc.get("origin") is not None:  # (the emission map's, with run_events(origin_map=, exact=True))
        out["origin_raw"] = exact_round(acc["origin"])
    out["nonfinite"] = np.asarray(acc["nonfinite"], np.float64).copy()
    return {k: v[0] for k, v in out.items()} if acc["kind"] == "run" else out


def exact_result(acc, f_inx) -> dict:
    """run_info["exact"]: exact_finish's tables with flux, sky_map and sum_weight_sln_prob, the raw ones divided by
    f_inx (by 1 when it is 0) with one IEEE division each, and acc, the accumulators themselves (exact_raw's dict).
    A misplaced record is an ArtError, as in the replicates."""
    acc = exact_raw(acc)
    if float(np.sum(acc["misplaced"])) != 0:
        raise _lib.ArtError(f"exact: {int(np.sum(acc['misplaced']))} node records lie in the range of another tree")
    out = exact_finish(acc)
    div = float(f_inx) if f_inx > 0 else 1.0
    out.update(flux=out["flux_raw"] / div, sum_weight_sln_prob=out["totals_raw"] / div)
    if "sky_raw" in out:
        out["sky_map"] = out["sky_raw"] / div
    if "origin_raw" in out:
        out["origin_map"] = out["origin_raw"] / div
    out["acc"] = acc
    return out


def exact_pack(acc) -> np.ndarray:
    """A rank's exact accumulators (exact_raw's dict, normalised) as float64 for the run's all-reduce: the limbs of the
    tables there are, in EXACT_KEYS' order, then nonfinite and misplaced. A normalised limb is an integer below 2^32
    (the top one a small signed one), which float64 holds exactly, as it does their sums over up to 2^21 ranks."""
    limbs = [acc[k].reshape(-1) for k in EXACT_KEYS if acc.get(k) is not None]
    if any(np.abs(v).max(initial=0) >= 2 ** 32 for v in limbs):
        raise ValueError("exact_pack: the accumulators are not normalised, or a sum exceeds 2^1038")
    return np.concatenate([v.astype(np.float64) for v in limbs] + [np.asarray(acc[k], np.float64).reshape(-1)
                                                                   for k in ("nonfinite", "misplaced")])


def exact_unpack(vec, like) -> dict:
    """exact_pack's vector, summed over the ranks, back into a dict shaped like `like` (the rank's own), normalised"""
    out, at = {"kind": like["kind"]}, 0
    for k in EXACT_KEYS:
        out[k] = None
        if like.get(k) is not None:
            out[k] = exact_normalize(np.rint(vec[at:at + like[k].size]).astype(np.int64).reshape(like[k].shape))
            at += like[k].size
    for k in ("nonfinite", "misplaced"):
        n = np.asarray(like[k]).size
        out[k] = np.asarray(vec[at:at + n], np.float64).copy()
        at += n
    return out


def rows_exact(rows, nbins, sky_kw=None, f_inx=None, acc=False) -> dict:
    """The exact tables from npy rows (column 7 raw or divided alike: the tables are in the powers' own units): the
    host oracle of art_event_exact_device, and the exact tables of row files written earlier. Per bin of the flux
    table (hist_bins of column 3 per species), of the sky map (sky_bins, with sky_kw) and per species, math.fsum of
    the rows' powers column 8 * column 7, which is the correctly rounded exact sum. Returns flux_raw (2, nbins),
    sky_raw (2, n_theta, n_phi, n_dw; with sky_kw), totals_raw (2) and nonfinite, the rows whose power is NaN or
    infinite (not added anywhere); with f_inx also flux, sky_map and sum_weight_sln_prob, divided by it; with
    acc=True also "acc", the same sums as accumulators (exact_add), which exact_merge adds to those of other files."""
    import math
    rows = np.asarray(rows, np.float64)
    nbins = int(nbins)
    sp = (rows[:, 1] != 0).astype(np.int64)
    p = rows[:, 8] * rows[:, 7]
    ok = np.isfinite(p)
    fb = hist_bins(rows[:, 3], nbins) if nbins > 0 else np.full(len(rows), -1)
    labels = [("flux", np.where(fb >= 0, sp * nbins + fb, -1), (2, nbins)), ("totals", sp, (2,))]
    if sky_kw is not None:
        kw = {k: sky_kw[k] for k in ("n_theta", "n_phi", "n_dw", "theta_axis", "dw_range") if k in sky_kw}
        shape = (2, kw.get("n_theta", 32), kw.get("n_phi", 64), kw.get("n_dw", 1))
        labels.append(("sky", sky_bins(rows[:, 2], rows[:, 3], rows[:, 12], rows[:, 1], **kw), shape))
    out, accs = {"nonfinite": float(np.count_nonzero(~ok))}, {"kind": "run", "sky": None}
    for name, lab, shape in labels:
        lab = np.where(ok, lab, -1)
        size = int(np.prod(shape))
        keep = lab >= 0
        order = np.argsort(lab[keep], kind="stable")
        cut = np.searchsorted(lab[keep][order], np.arange(size + 1))
        vals = p[keep][order]
        out[name + "_raw"] = np.array([math.fsum(vals[cut[b]:cut[b + 1]]) for b in range(size)]).reshape(shape)
        if acc:
            accs[name] = exact_add(p, lab, size)[0].reshape(1, *(shape if name != "flux" else (2 * nbins,)), _lib.EXACT_LIMBS)
    if f_inx is not None:
        div = float(f_inx) if f_inx > 0 else 1.0
        out.update(flux=out["flux_raw"] / div, sum_weight_sln_prob=out["totals_raw"] / div)
        if "sky_raw" in out:
            out["sky_map"] = out["sky_raw"] / div
    if acc:
        accs.update(nonfinite=np.array([out["nonfinite"]]), misplaced=np.zeros(1))
        out["acc"] = accs
    return out


def jackknife(rep, fn, cov=False) -> dict:
    """The delete-a-group jackknife of fn over a run's replicates (replicates_result's dict: run_events' or run_info's
    "replicates", or a scan's). fn gets a dict of normalised tables -- flux (2, nbins), sky_map (2, n_theta, n_phi,
    n_dw; with a map) and sum_weight_sln_prob (2), with a scan's leading K axis where there is one -- and returns a
    number or an array: a pulse profile summed over Δω, a band power, a ratio of two bins or of two models, the g
    where a curve crosses a threshold. With S a table summed over the groups, T_g its group g, f = f_inx and a_g the
    group's part of it (scaled so that Σ_g a_g = f, which changes nothing when the attempts were counted):
        value   = fn(S / f),      θ_g = fn((S - T_g) / (f - a_g)),
        sigma   = sqrt((R' - 1) / R' Σ_g (θ_g - mean θ)²)    over the R' groups that hold events,
    and with cov the covariance (R' - 1) / R' Σ_g (θ_g - mean)(θ_g - mean)ᵀ of the flattened result, whose diagonal
    is sigma². groups_used is R'. sigma is NaN with R' < 2 and where a leave-out divisor is 0. The two estimates of
    one scatter, this one and moments_sigma's, differ by a relative noise of order sqrt(2 / (R' - 1)); under
    heavy-tailed weights both are biased low alike."""
    raw, f = rep["raw"], float(rep["f_inx"])
    groups = np.asarray(raw["groups"], np.float64)
    n_g, a_g = groups[:, 0], groups[:, 1]
    squeeze = raw["kind"] == "run"
    T = {k: (None if raw.get(k) is None else np.asarray(raw[k], np.float64)) for k in ("flux", "sky", "totals")}
    S = {k: (None if v is None else v.sum(axis=1)) for k, v in T.items()}
    value = np.asarray(fn(_replicate_tables(S["flux"], S["sky"], S["totals"], f, squeeze)), np.float64)
    used = np.flatnonzero(n_g > 0)
    out = {"value": value, "groups_used": int(used.size)}
    a_sum = a_g.sum()
    scale = f / a_sum if a_sum > 0 else 0.0
    theta = []
    for g in used:
        left = {k: (None if v is None else S[k] - v[:, g]) for k, v in T.items()}
        theta.append(np.asarray(fn(_replicate_tables(left["flux"], left["sky"], left["totals"], f - a_g[g] * scale, squeeze)),
                                np.float64).reshape(-1))
    if used.size < 2:
        out["sigma"] = np.full(value.shape, np.nan)
        if cov:
            out["cov"] = np.full((value.size, value.size), np.nan)
        return out
    theta = np.stack(theta)
    d = theta - theta.mean(axis=0)
    c = (used.size - 1.0) / used.size
    out["sigma"] = np.sqrt(c * (d * d).sum(axis=0)).reshape(value.shape)
    if cov:
        out["cov"] = c * (d.T @ d)
    return out


# ---- emission maps: the power over where its event converted, and jointly over where it goes
ORIGIN_KEYS = ("n_r", "n_theta", "n_phi", "theta_axis", "r_range", "frame", "mode")
ORIGIN_FRAMES = ("magnetic", "rotation")


def origin_spec(origin, observer=None, params=None) -> dict:
    """An emission map's keywords completed and checked, the dict Engine.event_origin and the numpy oracle both use:
    origin a dict of n_r, n_theta, n_phi, theta_axis ("cos" | "theta"), r_range, frame ("magnetic" | "rotation") and
    mode (0 or "auto", 1 or "lds", 2 or "global"); {}: 1 x 16 x 32, "cos", "magnetic". observer: None, or a dict of
    n_theta, n_phi, theta_axis ({}: 32 x 64, "cos"), the sky map's first two axes. The spec also holds cm and sm, the
    rotation about y that origin_bins applies: math.cos / math.sin of params.theta_m in frame "magnetic" (params is
    needed there), (1, 0) in frame "rotation"; "shape", the table's (2, obs_theta, obs_phi, n_r, n_theta, n_phi), and
    "observer", the completed dict or None. A dict that origin_spec made (it is marked) is returned after a check that
    its shape still follows from its axes and its mode is 0, 1 or 2; observer= beside it is a ValueError. Unknown keys, an axis
    below 1, n_r > 1 without an r_range and a bad range are a ValueError."""
    if isinstance(origin, dict) and origin.get("_origin_spec") is True:  # (completed here: checked again, cheaply)
        if observer is not None:
            raise ValueError("origin_map: a completed spec holds its observer axes; observer= beside it is refused")
        obs = origin["observer"]
        shape = (2, obs["n_theta"] if obs else 1, obs["n_phi"] if obs else 1, origin["n_r"], origin["n_theta"], origin["n_phi"])
        if tuple(origin["shape"]) != shape or origin["mode"] not in (0, 1, 2) or min(shape) < 1:
            raise ValueError("origin_map: the spec was changed after origin_spec completed it (use origin_spec again)")
        return origin
    kw = {"n_r": 1, "n_theta": 16, "n_phi": 32, "theta_axis": "cos", "r_range": None, "frame": "magnetic", "mode": 0}
    if set(origin) - set(kw):
        raise ValueError(f"origin_map: unknown keys {sorted(set(origin) - set(kw))}")
    kw.update(origin)
    _theta_range(kw["theta_axis"])
    if kw["frame"] not in ORIGIN_FRAMES:
        raise ValueError(f"origin_map: frame must be 'magnetic' or 'rotation', not {kw['frame']!r}")
    kw["mode"] = _lib.ORIGIN_MODES.get(kw["mode"], kw["mode"])
    if kw["mode"] not in (0, 1, 2):
        raise ValueError(f"origin_map: mode must be 0 / 'auto', 1 / 'lds' or 2 / 'global', not {kw['mode']!r}")
    for k in ("n_r", "n_theta", "n_phi"):
        if int(kw[k]) != kw[k] or int(kw[k]) < 1:
            raise ValueError(f"origin_map: {k} must be an integer >= 1, not {kw[k]!r}")
        kw[k] = int(kw[k])
    if kw["r_range"] is None:
        if kw["n_r"] > 1:
            raise ValueError("origin_map: n_r > 1 needs an r_range (a data-dependent range cannot be binned chunk by chunk)")
    else:
        lo, hi = float(kw["r_range"][0]), float(kw["r_range"][1])
        if not (np.isfinite(lo) and np.isfinite(hi) and lo < hi):
            raise ValueError("origin_map: r_range needs finite lo < hi")
        kw["r_range"] = (lo, hi)
    if kw["frame"] == "magnetic":
        if params is None:
            raise ValueError("origin_map: frame 'magnetic' needs the run's params (theta_m)")
        kw["cm"], kw["sm"] = math.cos(params.theta_m), math.sin(params.theta_m)
    else:
        kw["cm"], kw["sm"] = 1.0, 0.0
    obs = None
    if observer is not None:
        obs = {"n_theta": 32, "n_phi": 64, "theta_axis": "cos"}
        if set(observer) - set(obs):
            raise ValueError(f"origin_map: unknown observer keys {sorted(set(observer) - set(obs))}")
        obs.update(observer)
        _theta_range(obs["theta_axis"])
        for k in ("n_theta", "n_phi"):
            if int(obs[k]) != obs[k] or int(obs[k]) < 1:
                raise ValueError(f"origin_map: the observer's {k} must be an integer >= 1, not {obs[k]!r}")
            obs[k] = int(obs[k])
    kw["observer"] = obs
    kw["_origin_spec"] = True
    kw["shape"] = (2, obs["n_theta"] if obs else 1, obs["n_phi"] if obs else 1, kw["n_r"], kw["n_theta"], kw["n_phi"])
    if int(np.prod(kw["shape"], dtype=np.int64)) >= 2 ** 31:
        raise ValueError("origin_map: the table has 2^31 bins or more")
    return kw


def origin_map_edges(spec) -> tuple:
    """The bin edges of an emission map's five axes after the species (np.linspace, as np.histogramdd returns them):
    the observer's cos θf or θf and φf (the whole range in one bin without observer axes), then the origin's r (one
    bin for every finite r without an r_range: edges (0, inf)), cos θ or θ, and φ."""
    obs = spec["observer"] or {"n_theta": 1, "n_phi": 1, "theta_axis": "cos"}
    r_edges = np.array([0.0, np.inf]) if spec["r_range"] is None else np.linspace(*spec["r_range"], spec["n_r"] + 1)
    return (np.linspace(*_theta_range(obs["theta_axis"]), obs["n_theta"] + 1), np.linspace(-np.pi, np.pi, obs["n_phi"] + 1),
            r_edges, np.linspace(*_theta_range(spec["theta_axis"]), spec["n_theta"] + 1),
            np.linspace(-np.pi, np.pi, spec["n_phi"] + 1))


def origin_coordinates(x, y, z, spec) -> tuple:
    """(r, cos θ or θ by the spec's theta_axis, φ) of the points (x, y, z) in the spec's frame, rounded as
    origin_bin_of (art_event_origin.h) rounds them: v = (x cm - z sm, y, x sm + z cm), then _angles' (θ, φ, |v|) and
    cos θ = v_z / |v|."""
    x, y, z = (np.asarray(v, np.float64) for v in (x, y, z))
    cm, sm = spec["cm"], spec["sm"]
    v = np.stack([x * cm - z * sm, y, x * sm + z * cm], axis=-1)
    with np.errstate(invalid="ignore", divide="ignore"):
        th, ph, r = _angles(v)
        return r, (v[..., 2] / r if spec["theta_axis"] == "cos" else th), ph


def origin_bins(x, y, z, spec) -> np.ndarray:
    """The flat origin label (ir n_theta + iθ) n_phi + iφ of each point (x, y, z) -- a row's columns 9 to 11 -- in
    numpy: the oracle of the device's origin_bin_of. Each axis is np.histogram's bin of its closed range (hist_bins);
    without an r_range every finite r is in the one r bin; -1 for a point that a range, or a NaN, drops."""
    r, a, ph = origin_coordinates(x, y, z, spec)
    ia = hist_bins(a, spec["n_theta"], *_theta_range(spec["theta_axis"]))
    ib = hist_bins(ph, spec["n_phi"])
    ir = np.where(np.isfinite(r), 0, -1) if spec["r_range"] is None else hist_bins(r, spec["n_r"], *spec["r_range"])
    flat = (ir * spec["n_theta"] + ia) * spec["n_phi"] + ib
    return np.where((ia >= 0) & (ib >= 0) & (ir >= 0), flat, -1)


def rows_origin(rows, spec, R=None) -> np.ndarray:
    """art_event_origin_device's table in numpy from npy rows (column 7 raw or divided alike: the table is in the
    powers' own units): the oracle of the device table, and the path for row files written earlier. Per row the
    species (column 1), the observer bin of columns 2 and 3 (sky_bins with n_dw = 1: a row with a non-finite column 12
    is dropped, as from the sky map), the origin bin of columns 9 to 11 (origin_bins) and the power column 8 * column
    7. Returns the spec's "shape"; with R (2 to 64) an (R, ...) array, a row in group (column 0 - 1) mod R."""
    rows = np.asarray(rows, np.float64)
    shape = spec["shape"]
    n_origin = shape[3] * shape[4] * shape[5]
    obs = spec["observer"] or {"n_theta": 1, "n_phi": 1, "theta_axis": "cos"}
    sb = sky_bins(rows[:, 2], rows[:, 3], rows[:, 12], rows[:, 1], n_theta=obs["n_theta"], n_phi=obs["n_phi"], n_dw=1,
                  theta_axis=obs["theta_axis"])
    ob = origin_bins(rows[:, 9], rows[:, 10], rows[:, 11], spec)
    keep = (sb >= 0) & (ob >= 0)
    lab = sb[keep] * n_origin + ob[keep]
    size = int(np.prod(shape))
    p = (rows[:, 8] * rows[:, 7])[keep]
    if R is None:
        return np.bincount(lab, weights=p, minlength=size).reshape(shape)
    R = int(R)
    if not _lib.REPLICATES_MIN_GROUPS <= R <= _lib.REPLICATES_MAX_GROUPS:
        raise ValueError(f"replicates: {_lib.REPLICATES_MIN_GROUPS} to {_lib.REPLICATES_MAX_GROUPS} groups, not {R}")
    g = ((np.rint(rows[:, 0]).astype(np.int64) - 1) % R)[keep]
    return np.bincount(g * size + lab, weights=p, minlength=R * size).reshape(R, *shape)


def origin_result(raw, spec, f_inx, misplaced=0.0) -> dict:
    """run_events' and run_info's "origin": map (the raw table divided by f_inx, by 1 when it is 0), raw, edges
    (origin_map_edges), spec and misplaced (records outside their tree's range, which must be 0: an ArtError)."""
    raw = np.asarray(raw, np.float64).reshape(spec["shape"])
    if misplaced != 0:
        raise _lib.ArtError(f"origin_map: {int(misplaced)} node records lie in the range of another tree")
    return {"map": raw / (float(f_inx) if f_inx > 0 else 1.0), "raw": raw, "edges": origin_map_edges(spec), "spec": spec,
            "misplaced": int(misplaced)}


def _origin_solid_angles(n_theta, n_phi, theta_axis):
    """The solid angle of each (θ, φ) bin of a pair of axes, (n_theta, 1): equal with "cos", 2π (cos θ_lo - cos θ_hi) /
    n_phi per row with "theta" (line_profile's ring)"""
    edges = np.linspace(*_theta_range(theta_axis), n_theta + 1)
    ring = 2.0 * np.pi * ((edges[1:] - edges[:-1]) if theta_axis == "cos" else (np.cos(edges[:-1]) - np.cos(edges[1:])))
    return (ring / n_phi)[:, None]


def emission_profile(origin_map, spec, species=PHOTON):
    """Where on the conversion surface the power comes from: the emission map of one species summed over r and the
    observer axes, as power per steradian of ORIGIN direction in the spec's frame (each bin divided by its solid
    angle, as pulse_profile divides). Returns (profile (n_theta, n_phi), the θ-axis bin centres, the φ bin centres)."""
    m = np.asarray(origin_map, np.float64).reshape(spec["shape"])[species].sum(axis=(0, 1, 2))
    e = origin_map_edges(spec)
    return (m / _origin_solid_angles(spec["n_theta"], spec["n_phi"], spec["theta_axis"]), 0.5 * (e[3][:-1] + e[3][1:]),
            0.5 * (e[4][:-1] + e[4][1:]))


def observer_view(origin_map, spec, theta_obs, phase=None, species=PHOTON) -> np.ndarray:
    """What an observer at inclination theta_obs [rad] sees lit up: the origin table (n_r, n_theta, n_phi) of one
    species in the observer row that holds theta_obs (pulse_profile's bin rule), as power per steradian of OBSERVER
    direction: summed over the observer's φ and divided by the row's whole ring (the average over the rotation), or,
    with phase [rad, in [-π, π]], taken in the φ bin that holds it and divided by that bin's solid angle. The map
    needs observer axes."""
    obs = spec["observer"]
    if obs is None:
        raise ValueError("observer_view: the emission map has no observer axes")
    m = np.asarray(origin_map, np.float64).reshape(spec["shape"])[species]
    x = math.cos(theta_obs) if obs["theta_axis"] == "cos" else float(theta_obs)
    row = int(hist_bins(np.array([x]), obs["n_theta"], *_theta_range(obs["theta_axis"]))[0])
    if row < 0:
        raise ValueError(f"theta_obs = {theta_obs} lies outside the map")
    omega = _origin_solid_angles(obs["n_theta"], obs["n_phi"], obs["theta_axis"])[row, 0]
    if phase is None:
        return m[row].sum(axis=0) / (omega * obs["n_phi"])
    col = int(hist_bins(np.array([float(phase)]), obs["n_phi"])[0])
    if col < 0:
        raise ValueError(f"phase = {phase} lies outside [-π, π]")
    return m[row, col] / omega


def origin_jackknife(origin, fn, cov=False) -> dict:
    """The delete-a-group jackknife (jackknife's rule and result) of fn over an emission map's replicates: origin is
    run_events' "origin" dict of a run with replicates=R, and fn gets the NORMALISED map (the spec's shape: the groups'
    sum, or the sum without one group, divided by its part of f_inx) and returns a number or an array, such as
    emission_profile's or observer_view's."""
    rep = origin.get("replicates")
    if rep is None:
        raise ValueError("origin_jackknife: the emission map has no replicates (run_events(replicates=R))")
    T = np.asarray(rep["raw"], np.float64)
    R = T.shape[0]
    groups = np.stack([np.asarray(rep["n_g"], np.float64), np.asarray(rep["a_g"], np.float64), np.zeros(R)], axis=1)
    raw = {"kind": "run", "R": R, "groups": groups, "flux": np.zeros((1, R, 2)), "totals": np.zeros((1, R, 2)), "sky": T[None]}
    return jackknife({"raw": raw, "f_inx": rep["f_inx"]}, lambda t: fn(t["sky_map"]), cov=cov)


def _loglog_crossing(g, P, power):
    """The g at which the curve P(g), given at the points g (any order), first crosses `power` going up the sorted g,
    by linear interpolation of log P in log g; NaN where it does not cross"""
    g, P = np.asarray(g, np.float64), np.asarray(P, np.float64)
    order = np.argsort(g)
    with np.errstate(divide="ignore", invalid="ignore"):
        x, y, y0 = np.log(g[order]), np.log(P[order]), math.log(power)
    for i in range(len(x) - 1):
        lo, hi = sorted((y[i], y[i + 1]))
        if np.isfinite(lo) and np.isfinite(hi) and lo <= y0 <= hi and lo < hi:
            return float(np.exp(x[i] + (y0 - y[i]) / (y[i + 1] - y[i]) * (x[i + 1] - x[i])))
    return float("nan")


def coupling_crossing(scan, power, species=PHOTON) -> dict:
    """The coupling g at which the radiated power of `species` equals `power` (> 0), from a coupling scan made with
    replicates (run_events' or run_info's "coupling_scan"): log-log interpolation of coupling_curve between the two
    neighbouring couplings that bracket it, and its jackknife error. The K points of a scan are reweightings of the
    same events and strongly correlated, so this error cannot be had from the per-point σ. Returns jackknife's dict:
    value (NaN where the curve does not reach `power`), sigma, groups_used."""
    if not (power > 0.0 and math.isfinite(power)):
        raise ValueError("coupling_crossing: power must be finite and > 0")
    if "replicates" not in scan:
        raise ValueError("coupling_crossing: the scan has no replicates (run_events(couplings=, replicates=R))")
    sp = 0 if species == AXION else 1
    g = np.asarray(scan["g"], np.float64)
    return jackknife(scan["replicates"], lambda t: _loglog_crossing(g, t["sum_weight_sln_prob"][:, sp], power))


GRID_KEYS = ("flux", "totals", "flux_rep", "totals_rep", "groups", "moment_totals")


def grid_tables(rows_raw, weights, back, ratio, final_index, nbins, R=None, attempts=None, event_lo=0) -> dict:
    """art_event_grid_device's tables in numpy, the statement of its definition ("Coupling x halo grid"):
    rows_raw, the run's own rows of one chunk (column 7 raw; column 14, τ, is read when there are 29 columns), weights
    (K_g, n_nodes) and back (K_g, n_events), the coupling scan's W and B of the chunk, ratio (K_h, n_events), the halo
    scan's R, and final_index, per row the index of its node record. The power of row r of event e at cell (kg, kh)
    is ((W[kg, final_index[r]] B[kg, e]) [exp(-τ)] sln_prob) * R[kh, e], each product rounded on its own, in the
    rows' own flux bins (hist_bins of column 3). Returns the tables as grid_raw lays them out: flux (K_g, K_h, 2 nbins),
    totals (K_g, K_h, 3: Σ power of the axion and of the photon rows, 0 misplaced records), with R groups
    (g = global event id mod R) flux_rep (K_g, K_h, R, 2 nbins), totals_rep (K_g, K_h, R, 2) and groups (R, 3: n_g,
    a_g, 0), and with attempts (the sampler's, of the events event_lo .. event_lo + n_events) moment_totals
    (K_g, K_h, 8): n, A1, A2, Q and C of the two species from X_{e,s} = Σ power of e's rows of species s in row
    order, 0. attempts=None: a_e counts the photon rows only, as the device does with a NULL attempts, and there is
    no moment_totals."""
    rows = np.asarray(rows_raw, np.float64)
    W, B, Rt = (np.atleast_2d(np.asarray(v, np.float64)) for v in (weights, back, ratio))
    Kg, Kh, n, nbins, lo = W.shape[0], Rt.shape[0], B.shape[1], int(nbins), int(event_lo)
    if B.shape[0] != Kg or Rt.shape[1] != n:
        raise ValueError("grid_tables: weights and back share the couplings, back and ratio the events")
    fi = np.asarray(final_index, np.int64).reshape(-1)
    ev = np.rint(rows[:, 0]).astype(np.int64) - 1 - lo
    sp = (rows[:, 1] != 0).astype(np.int64)
    sln = rows[:, 7]
    absorb = np.exp(-rows[:, 14]) if rows.shape[1] > 14 and rows[:, 14].any() else None
    fb = hist_bins(rows[:, 3], nbins) if nbins > 0 else np.full(len(rows), -1)
    lab = np.where(fb >= 0, sp * nbins + fb, -1)
    keep = lab >= 0
    photons = np.bincount(ev[sp == 1], minlength=n)
    a = photons if attempts is None else np.asarray(attempts, np.int64) - 1 + photons
    out = {"flux": np.zeros((Kg, Kh, 2 * nbins)), "totals": np.zeros((Kg, Kh, len(_lib.GRID_TOTALS)))}
    if R is not None:
        R = int(R)
        g_ev = (lo + np.arange(n, dtype=np.int64)) % R
        g = g_ev[ev]
        out.update(flux_rep=np.zeros((Kg, Kh, R, 2 * nbins)), totals_rep=np.zeros((Kg, Kh, R, 2)),
                   groups=np.stack([np.bincount(g_ev, minlength=R), np.bincount(g_ev, weights=a, minlength=R), np.zeros(R)],
                                   axis=1).astype(np.float64))
    if attempts is not None:
        out["moment_totals"] = np.zeros((Kg, Kh, len(_lib.MOMENT_TOTALS)))
    for kg in range(Kg):
        w = W[kg, fi] * B[kg, ev]
        pg = (w if absorb is None else w * absorb) * sln
        for kh in range(Kh):
            pw = pg * Rt[kh, ev]
            out["flux"][kg, kh] = np.bincount(lab[keep], weights=pw[keep], minlength=2 * nbins)
            out["totals"][kg, kh, :2] = np.bincount(sp, weights=pw, minlength=2)
            if R is not None:
                out["flux_rep"][kg, kh] = np.bincount(g[keep] * 2 * nbins + lab[keep], weights=pw[keep],
                                                      minlength=R * 2 * nbins).reshape(R, 2 * nbins)
                out["totals_rep"][kg, kh] = np.bincount(g * 2 + sp, weights=pw, minlength=2 * R).reshape(R, 2)
            if attempts is not None:
                X = np.bincount(ev * 2 + sp, weights=pw, minlength=2 * n).reshape(n, 2)  # (adds in row order)
                out["moment_totals"][kg, kh] = np.r_[float(n), a.sum(), (a * a).sum(), (X * X).sum(axis=0),
                                                     (X * a[:, None]).sum(axis=0), 0.0]
    return out


def grid_raw(grid) -> dict:
    """Engine.event_grid's dict with its tables on the host (numpy) and the cell axis, which the device keeps last
    (art_event_grid_out's tables are cell-minor), turned into two leading axes: flux (K_g, K_h, 2 nbins), totals
    (K_g, K_h, 3), flux_rep (K_g, K_h, R, 2 nbins), totals_rep (K_g, K_h, R, 2), groups (R, 3), moment_totals
    (K_g, K_h, 8) -- those there are; what adds over chunks and ranks -- then g, models, base, R and n_events."""
    Kg, Kh = len(grid["g"]), len(grid["models"])
    out = {}
    for k in GRID_KEYS:
        v = grid.get(k)
        if v is None:
            continue
        v = v.cpu().numpy() if hasattr(v, "cpu") else np.asarray(v, np.float64)
        out[k] = v.copy() if k == "groups" else np.ascontiguousarray(np.moveaxis(v.reshape(*v.shape[:-1], Kg, Kh), (-2, -1), (0, 1)))
    out.update(g=[float(v) for v in grid["g"]], models=[_halo_of(h) for h in grid["models"]], base=grid["base"],
               R=None if grid.get("R") is None else int(grid["R"]), n_events=int(grid["n_events"]))
    return out


def grid_pack(raw) -> np.ndarray:
    """A rank's grid tables (grid_raw) as one vector for the run's all-reduce: the tables there are, in GRID_KEYS'
    order, then the number of events"""
    parts = [np.asarray(raw[k], np.float64).reshape(-1) for k in GRID_KEYS if raw.get(k) is not None]
    return np.concatenate(parts + [np.array([float(raw["n_events"])])])


def grid_unpack(vec, like) -> dict:
    """grid_pack's vector back into a dict shaped like `like` (the rank's own grid_raw)"""
    out, at = {k: like[k] for k in ("g", "models", "base", "R")}, 0
    for k in GRID_KEYS:
        if like.get(k) is None:
            continue
        out[k] = np.asarray(vec[at:at + like[k].size], np.float64).reshape(like[k].shape)
        at += like[k].size
    out["n_events"] = int(round(vec[at]))
    return out


def grid_result(raw, f_inx) -> dict:
    """The coupling x halo grid of a run from its raw tables (grid_raw, summed over the ranks) and the run's f_inx: g
    (K_g), models (K_h), base, flux (K_g, K_h, 2, nbins) and sum_weight_sln_prob (K_g, K_h, 2), both divided by f_inx,
    misplaced (records outside their tree's range, which must be 0), f_inx, raw; with moment totals
    sum_weight_sln_prob_sigma (K_g, K_h, 2; moments_sigma: a_e and f_inx are the run's own in every cell) and n_eff
    (K_g, K_h) = S_photon² / Q_photon, the Kish effective number of events behind a cell's photon total; with
    replicate tables "replicates": the raw group tables flux (K_g, K_h, R, 2 nbins) and totals (K_g, K_h, R, 2), n_g
    and a_g (R), R and f_inx, which grid_jackknife and limit_band read."""
    f = float(f_inx) if f_inx > 0 else 1.0
    tot = np.asarray(raw["totals"], np.float64)
    Kg, Kh = tot.shape[:2]
    nbins = raw["flux"].shape[-1] // 2
    res = {"g": np.array(raw["g"], np.float64), "models": list(raw["models"]), "base": raw["base"],
           "flux": (raw["flux"] / f).reshape(Kg, Kh, 2, nbins), "sum_weight_sln_prob": tot[:, :, 0:2] / f,
           "misplaced": int(round(tot[0, 0, 2])), "f_inx": int(f_inx), "raw": raw}
    mt = raw.get("moment_totals")
    if mt is not None:
        res["sum_weight_sln_prob_sigma"] = np.stack([np.stack([
            moments_sigma(tot[i, j, 0:2], mt[i, j, 3:5], mt[i, j, 5:7], f_inx, mt[i, j, 2], mt[i, j, 0])
            for j in range(Kh)]) for i in range(Kg)])
        with np.errstate(divide="ignore", invalid="ignore"):
            res["n_eff"] = tot[:, :, 1] * tot[:, :, 1] / mt[:, :, 4]
    if raw.get("groups") is not None:
        groups = np.asarray(raw["groups"], np.float64)
        res["replicates"] = {"R": int(raw["R"]), "flux": raw["flux_rep"], "totals": raw["totals_rep"],
                             "n_g": groups[:, 0].copy(), "a_g": groups[:, 1].copy(), "f_inx": int(f_inx)}
        res["misplaced"] = max(res["misplaced"], int(round(groups[:, 2].sum())))
    return res


def grid_jackknife(grid, fn, cov=False) -> dict:
    """trees.jackknife for the coupling x halo grid (grid_result's dict, made with replicates): fn gets a dict of the
    normalised tables flux (K_g, K_h, 2, nbins) and sum_weight_sln_prob (K_g, K_h, 2) and returns a number or an
    array. The same leave-one-group-out formula, the same NaN rules and the same groups_used as jackknife: value,
    sigma, groups_used and with cov the covariance of the flattened result."""
    rep = grid.get("replicates")
    if rep is None:
        raise ValueError("grid_jackknife: the grid has no replicates (run_events(grid=True, replicates=R))")
    flux, totals = np.asarray(rep["flux"], np.float64), np.asarray(rep["totals"], np.float64)
    Kg, Kh, R = totals.shape[:3]
    groups = np.stack([rep["n_g"], rep["a_g"], np.zeros(R)], axis=1)
    raw = {"kind": "grid", "R": R, "groups": groups, "sky": None, "flux": flux.reshape(Kg * Kh, R, -1),
           "totals": totals.reshape(Kg * Kh, R, 2)}
    cells = lambda t: {k: v.reshape(Kg, Kh, *v.shape[1:]) for k, v in t.items()}  # noqa: E731
    return jackknife({"raw": raw, "f_inx": rep["f_inx"]}, lambda t: fn(cells(t)), cov=cov)


def limit_band(grid, power, species=PHOTON, average=None) -> dict:
    """The limit on g under every halo model of a coupling x halo grid (run_events' or run_info's "grid", made with
    replicates), and the band between the models: per model kh the coupling at which column kh of the grid, the
    radiated power of `species` against g, reaches `power` (> 0), by the log-log interpolation of coupling_crossing,
    with its jackknife error. The models reweight the same events, so their limits are strongly correlated and the
    width of the band has a far smaller error than the quadrature sum of the limits' -- which is what cov is for.
    Returns g and sigma (K_h), cov (K_h, K_h; its diagonal is sigma²), lo, hi (the smallest and the largest limit
    over the models that reach `power`), lo_model, hi_model (their indices, -1 for none), lo_sigma, hi_sigma, ratio =
    hi / lo and ratio_sigma (each leave-one-out estimate takes its own smallest and largest), and groups_used.
    average (a list of model indices, or a vector of K_h weights, normalised to sum 1): also g_avg and sigma_avg, the
    crossing of the correspondingly averaged column. The tables are linear in the halo's velocity distribution, so
    an average over models is the table of the averaged distribution: the way to treat an unknown direction of v_ns.
    NaN where a column does not reach `power`."""
    if not (power > 0.0 and math.isfinite(power)):
        raise ValueError("limit_band: power must be finite and > 0")
    if "replicates" not in grid:
        raise ValueError("limit_band: the grid has no replicates (run_events(grid=True, replicates=R))")
    sp = 0 if species == AXION else 1
    g = np.asarray(grid["g"], np.float64)
    Kh = len(grid["models"])
    w = None
    if average is not None:
        av = np.asarray(average)
        if av.size == 0:
            raise ValueError("limit_band: average is empty")
        if np.issubdtype(av.dtype, np.integer):
            if av.min() < 0 or av.max() >= Kh:
                raise ValueError("limit_band: average names a model outside the grid")
            w = np.bincount(av.reshape(-1), minlength=Kh).astype(np.float64)
        else:
            w = np.asarray(av, np.float64).reshape(-1)
            if w.size != Kh or not np.all(np.isfinite(w)) or np.any(w < 0):
                raise ValueError("limit_band: a weight vector has one finite weight >= 0 per model")
        if not w.sum() > 0:
            raise ValueError("limit_band: the weights sum to 0")
        w = w / w.sum()

    def ends(gh):
        ok = np.isfinite(gh)
        return (float(gh[ok].min()), float(gh[ok].max())) if ok.any() else (float("nan"), float("nan"))

    def fn(t):
        P = t["sum_weight_sln_prob"][:, :, sp]
        gh = np.array([_loglog_crossing(g, P[:, h], power) for h in range(Kh)])
        lo, hi = ends(gh)
        tail = [lo, hi, hi / lo if lo > 0 else float("nan")]
        if w is not None:
            tail.append(_loglog_crossing(g, P @ w, power))
        return np.r_[gh, tail]

    jk = grid_jackknife(grid, fn, cov=True)
    v, s = jk["value"], jk["sigma"]
    gh = v[:Kh]
    ok = np.isfinite(gh)
    out = {"g": gh, "sigma": s[:Kh], "cov": jk["cov"][:Kh, :Kh], "lo": float(v[Kh]), "hi": float(v[Kh + 1]),
           "lo_model": int(np.flatnonzero(ok)[np.argmin(gh[ok])]) if ok.any() else -1,
           "hi_model": int(np.flatnonzero(ok)[np.argmax(gh[ok])]) if ok.any() else -1,
           "lo_sigma": float(s[Kh]), "hi_sigma": float(s[Kh + 1]), "ratio": float(v[Kh + 2]),
           "ratio_sigma": float(s[Kh + 2]), "groups_used": jk["groups_used"]}
    if w is not None:
        out.update(g_avg=float(v[Kh + 3]), sigma_avg=float(s[Kh + 3]), weights=w)
    return out


SPECTRUM_TABLES = ("count", "sum", "sum_sq", "totals")  # what adds; the lists top_power and top_event merge


def spectrum_bins(sub_bits) -> int:
    """The bins of the event power spectrum with sub_bits sub-octave bits: 2047 << sub_bits"""
    return 2047 << int(sub_bits)


def spectrum_bin(x, sub_bits) -> np.ndarray:
    """The bin of each x by art_event_spectrum_device's rule: the top 11 + sub_bits bits of the IEEE-754 pattern,
    x.view(int64) >> (52 - sub_bits), for a finite x > 0; -1 otherwise (0, -0.0, negatives, NaN, inf)"""
    x = np.ascontiguousarray(x, np.float64)
    ok = np.isfinite(x) & (x > 0)
    return np.where(ok, x.view(np.int64) >> (52 - int(sub_bits)), -1)


def spectrum_edges(lo, hi, sub_bits) -> np.ndarray:
    """The lower edges of the bins lo .. hi (hi included: hi - lo + 1 doubles; the edge of bin 2047 << sub_bits, the
    upper edge of the last bin, is inf): the doubles whose pattern is b << (52 - sub_bits)"""
    return (np.arange(int(lo), int(hi) + 1, dtype=np.int64) << (52 - int(sub_bits))).view(np.float64)


def _spectrum_check(sub_bits, top):
    m, T = int(sub_bits), int(top)
    if m != sub_bits or not 0 <= m <= _lib.SPECTRUM_MAX_SUB_BITS:
        raise ValueError(f"spectrum: sub_bits is 0 to {_lib.SPECTRUM_MAX_SUB_BITS}, not {sub_bits!r}")
    if T != top or not 0 <= T <= _lib.SPECTRUM_MAX_TOP:
        raise ValueError(f"spectrum: top is 0 to {_lib.SPECTRUM_MAX_TOP}, not {top!r}")
    return m, T


def spectrum_keywords(spectrum) -> tuple:
    """(sub_bits, top) of a spectrum= keyword ({}: the defaults 3 and 64); unknown keys and values out of range are a
    ValueError"""
    from collections.abc import Mapping
    if not isinstance(spectrum, Mapping):
        raise ValueError(f"spectrum: a dict of sub_bits and top ({{}}: the defaults), not {spectrum!r}")
    extra = set(spectrum) - {"sub_bits", "top"}
    if extra:
        raise ValueError(f"spectrum: unknown keys {sorted(extra)} (sub_bits, top)")
    return _spectrum_check(spectrum.get("sub_bits", 3), spectrum.get("top", 64))


def _spectrum_top(X, ids, T):
    """The list of one (set, species): the T pairs with the largest finite X > 0 by (X descending, id ascending),
    padded with (0.0, -1)"""
    X, ids = np.asarray(X, np.float64), np.asarray(ids, np.int64)
    ok = np.isfinite(X) & (X > 0)
    X, ids = X[ok], ids[ok]
    order = np.lexsort((ids, -X.view(np.int64)))[:T]  # (the pattern of a finite X > 0 is monotone in X)
    tp, te = np.zeros(T), np.full(T, -1, np.int64)
    tp[:len(order)], te[:len(order)] = X[order], ids[order]
    return tp, te


def _spectrum_tables(X, ids, m, T) -> dict:
    """The raw dict of the sets X (K, 2, n): X[k, s, i] the power of species s of the event with the global id ids[i]"""
    K, NB = X.shape[0], spectrum_bins(m)
    out = {"count": np.zeros((K, 2, NB)), "sum": np.zeros((K, 2, NB)), "sum_sq": np.zeros((K, 2, NB)),
           "totals": np.zeros((K, 2, len(_lib.SPECTRUM_TOTALS))), "top_power": np.zeros((K, 2, T)),
           "top_event": np.full((K, 2, T), -1, np.int64)}
    for k in range(K):
        for s in range(2):
            x = np.ascontiguousarray(X[k, s])
            b = spectrum_bin(x, m)
            ok = b >= 0
            xp = x[ok]
            with np.errstate(over="ignore", under="ignore"):
                x2 = xp * xp
            out["count"][k, s] = np.bincount(b[ok], minlength=NB)
            out["sum"][k, s] = np.bincount(b[ok], weights=xp, minlength=NB)
            out["sum_sq"][k, s] = np.bincount(b[ok], weights=x2, minlength=NB)
            zeros = int(np.count_nonzero(x == 0))
            out["totals"][k, s, :6] = (len(x), len(xp), zeros, len(x) - len(xp) - zeros, xp.sum(), x2.sum())
            out["top_power"][k, s], out["top_event"][k, s] = _spectrum_top(x, ids, T)
    return out


def rows_spectrum(rows, sub_bits, top, event_lo=0, n_events=None) -> dict:
    """art_event_spectrum_device's tables in numpy from npy rows (column 7 raw: the tables are in the powers' own
    units), for kind "run": the oracle of the device tables, and the path for row files written earlier. X of an event
    and species is Σ column 8 * column 7 over its rows of that species in row order (np.bincount), its global id is
    column 0 - 1. The events are event_lo .. event_lo + n_events (n_events=None: up to the last event that has a
    row); one without a row of a species has X = 0 and is counted under zeros. Returns the raw dict that
    spectrum_raw returns: kind, sub_bits, top, count, sum, sum_sq (1, 2, 2047 << sub_bits), totals (1, 2, 8:
    _lib.SPECTRUM_TOTALS), top_power (1, 2, top) and top_event (1, 2, top; int64)."""
    m, T = _spectrum_check(sub_bits, top)
    rows = np.asarray(rows, np.float64)
    lo = int(event_lo)
    gid = np.rint(rows[:, 0]).astype(np.int64) - 1
    n = int(n_events) if n_events is not None else (int(gid.max()) + 1 - lo if len(rows) else 0)
    if len(rows) and (gid.min() < lo or gid.max() >= lo + n):
        raise ValueError("rows_spectrum: a row's event lies outside event_lo .. event_lo + n_events")
    sp = rows[:, 1] != 0
    p = rows[:, 8] * rows[:, 7]
    X = np.stack([np.bincount(gid[w] - lo, weights=p[w], minlength=n) if n else np.zeros(0) for w in (~sp, sp)])[None]
    return {"kind": "run", "sub_bits": m, "top": T, **_spectrum_tables(X, np.arange(lo, lo + n, dtype=np.int64), m, T)}


def spectrum_raw(spec) -> dict:
    """Engine.event_spectrum's dict with its tables and lists on the host (numpy): the tables add over chunks and
    ranks, the lists merge (spectrum_merge)"""
    host = lambda v: v.cpu().numpy() if hasattr(v, "cpu") else np.asarray(v)  # noqa: E731
    out = {"kind": spec["kind"], "sub_bits": int(spec["sub_bits"]), "top": int(spec["top"])}
    out.update({k: host(spec[k]).astype(np.float64, copy=False) for k in SPECTRUM_TABLES + ("top_power",)})
    out["top_event"] = host(spec["top_event"]).astype(np.int64, copy=False)
    return out


def spectrum_merge(raws) -> dict:
    """The raw spectrum of several chunks, ranks or files (raw dicts of one kind, sub_bits, top and number of sets):
    the tables summed, the lists merged into the best `top` of all their entries by (X descending, id ascending). The
    lists are a function of the multiset of their entries, so the merge is associative and does not depend on the
    order of `raws`; the tables' sums are float64 adds in the order given."""
    raws = list(raws)
    if not raws:
        raise ValueError("spectrum_merge: nothing to merge")
    a = raws[0]
    for b in raws[1:]:
        if any(b[k] != a[k] for k in ("kind", "sub_bits", "top")) or b["count"].shape != a["count"].shape:
            raise ValueError("spectrum_merge: the spectra were made for another kind, sub_bits, top or number of sets")
    out = {"kind": a["kind"], "sub_bits": a["sub_bits"], "top": a["top"]}
    for k in SPECTRUM_TABLES:
        out[k] = np.asarray(a[k], np.float64).copy()
        for b in raws[1:]:
            out[k] = out[k] + np.asarray(b[k], np.float64)
    K, T = a["count"].shape[0], int(a["top"])
    out["top_power"], out["top_event"] = np.zeros((K, 2, T)), np.full((K, 2, T), -1, np.int64)
    for k in range(K):
        for s in range(2):
            X = np.concatenate([np.asarray(r["top_power"], np.float64)[k, s] for r in raws])
            ids = np.concatenate([np.asarray(r["top_event"], np.int64)[k, s] for r in raws])
            have = ids >= 0
            out["top_power"][k, s], out["top_event"][k, s] = _spectrum_top(X[have], ids[have], T)
    return out


def spectrum_pack(raw, rank=0, world=1) -> np.ndarray:
    """A rank's raw spectrum as one vector for the run's all-reduce: [count | sum | sum_sq | totals | powers | ids].
    A sum cannot merge lists, so powers and ids are zeroed blocks of world x (K 2 top) in which the rank fills slot
    `rank` alone: after the sum slot r holds rank r's list (an id as float64 is exact below 2^53)."""
    tp, te = np.asarray(raw["top_power"], np.float64).reshape(-1), np.asarray(raw["top_event"], np.int64).reshape(-1)
    if te.size and te.max() >= 2 ** 53:
        raise ValueError("spectrum_pack: an event id of 2^53 or more is not exact as float64")
    blocks = np.zeros((2, int(world), tp.size))
    blocks[0, int(rank)], blocks[1, int(rank)] = tp, te
    return np.concatenate([np.asarray(raw[k], np.float64).reshape(-1) for k in SPECTRUM_TABLES] + [blocks.reshape(-1)])


def spectrum_unpack(vec, like, world=1) -> dict:
    """spectrum_pack's vector, summed over the ranks, back into a raw dict shaped like `like` (the rank's own): the
    tables as they are, the `world` lists merged by spectrum_merge"""
    out, at = {"kind": like["kind"], "sub_bits": like["sub_bits"], "top": like["top"]}, 0
    for k in SPECTRUM_TABLES:
        out[k] = np.asarray(vec[at:at + like[k].size], np.float64).reshape(like[k].shape)
        at += like[k].size
    shape, size = like["top_power"].shape, like["top_power"].size
    blocks = np.asarray(vec[at:at + 2 * int(world) * size], np.float64).reshape(2, int(world), size)
    zero = {k: np.zeros_like(out[k]) for k in SPECTRUM_TABLES}
    lists = [{**out, **zero, "top_power": blocks[0, r].reshape(shape), "top_event": np.rint(blocks[1, r]).astype(np.int64).reshape(shape)}
             for r in range(int(world))]
    merged = spectrum_merge(lists)
    out["top_power"], out["top_event"] = merged["top_power"], merged["top_event"]
    return out


def tail_index(top_power, k=None) -> dict:
    """The Hill estimator of the tail index α of P(X > x) ~ x^-α from a top list: over its valid entries
    X_(1) >= X_(2) >= ... (finite, > 0; T' of them), α̂_k = k / Σ_{i<=k} ln(X_(i) / X_(k+1)) with σ = α̂_k / √k.
    Returns alpha and alpha_sigma at k (None: the largest, T' - 1), k, and hill, α̂_k for k = 2 .. T' - 1 (the Hill
    plot: read α where it is flat). NaN below 3 entries, or where the logs sum to 0 (equal entries).
    α <= 2: the variance of X does not exist and no σ of a sum of X means what it says; α <= 1: nor does the mean."""
    x = np.asarray(top_power, np.float64).reshape(-1)
    x = np.sort(x[np.isfinite(x) & (x > 0)])[::-1]
    n = len(x)
    nan = float("nan")
    if n < 3:
        return {"alpha": nan, "alpha_sigma": nan, "k": 0, "hill": np.zeros(0)}
    lg = np.log(x)
    ks = np.arange(2, n)
    sums = np.cumsum(lg)[ks - 1] - ks * lg[ks]  # Σ_{i<=k} ln X_(i) - k ln X_(k+1)
    with np.errstate(divide="ignore", invalid="ignore"):
        hill = np.where(sums > 0, ks / sums, nan)
    kk = n - 1 if k is None else int(k)
    if not 2 <= kk <= n - 1:
        raise ValueError(f"tail_index: k must be in 2 .. {n - 1}, not {k!r}")
    alpha = float(hill[kk - 2])
    return {"alpha": alpha, "alpha_sigma": alpha / np.sqrt(kk), "k": kk, "hill": hill}


def spectrum_result(raw, f_inx) -> dict:
    """The event power spectrum of a run from its raw tables (spectrum_raw, rows_spectrum or spectrum_merge) and the
    run's f_inx. With the leading K axis of a scan's sets (none for kind "run") and then the species axis (0 axion,
    1 photon): bins (the first and last non-empty bin over all sets, or None), edges (the bins' edges, one more than
    bins), counts and power (sum / f_inx) over that span; events, positive, zeros, bad; n_eff = S² / Q, how many
    equal events would scatter as these do; top_event, top_power_raw and top_power (/ f_inx); top_share, the share
    of S in the top 1 .. T events, and max_share, the largest event's; alpha, alpha_sigma and hill (NaN-padded to
    T - 2) by tail_index of each list; misplaced (must be 0); sub_bits, top, kind, f_inx and raw."""
    m, T = int(raw["sub_bits"]), int(raw["top"])
    tot = np.asarray(raw["totals"], np.float64)
    count = np.asarray(raw["count"], np.float64)
    f = float(f_inx)
    S, Q = tot[..., 4], tot[..., 5]
    tp = np.asarray(raw["top_power"], np.float64)
    K = count.shape[0]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        res = {"n_eff": np.where(Q > 0, S * S / Q, np.nan), "top_share": np.cumsum(tp, axis=-1) / S[..., None],
               "top_power": tp / f if f != 0 else np.full(tp.shape, np.nan)}
    res["max_share"] = res["top_share"][..., 0] if T > 0 else np.full(S.shape, np.nan)
    used = np.flatnonzero(count.sum(axis=(0, 1)) > 0)
    if len(used):
        lo, hi = int(used[0]), int(used[-1])
        with np.errstate(divide="ignore", invalid="ignore"):
            power = np.asarray(raw["sum"], np.float64)[..., lo:hi + 1] / f if f != 0 else np.full(count[..., lo:hi + 1].shape, np.nan)
        res.update(bins=(lo, hi), edges=spectrum_edges(lo, hi + 1, m), counts=count[..., lo:hi + 1], power=power)
    else:
        res.update(bins=None, edges=np.zeros(0), counts=count[..., :0], power=count[..., :0])
    res.update(events=tot[..., 0], positive=tot[..., 1], zeros=tot[..., 2], bad=tot[..., 3],
               top_event=np.asarray(raw["top_event"], np.int64), top_power_raw=tp)
    alpha, sigma, hill = np.full((K, 2), np.nan), np.full((K, 2), np.nan), np.full((K, 2, max(T - 2, 0)), np.nan)
    for k in range(K):
        for s in range(2):
            t = tail_index(tp[k, s])
            alpha[k, s], sigma[k, s] = t["alpha"], t["alpha_sigma"]
            hill[k, s, :len(t["hill"])] = t["hill"]
    res.update(alpha=alpha, alpha_sigma=sigma, hill=hill)
    if raw["kind"] == "run":
        res = {k: (v[0] if isinstance(v, np.ndarray) and v.ndim >= 2 and k != "edges" else v) for k, v in res.items()}
    res.update(misplaced=int(round(float(tot[..., 6].sum()))), sub_bits=m, top=T, kind=raw["kind"], f_inx=int(f_inx), raw=raw)
    return res


def pack_totals(flux, f_inx, sum_axion, sum_photon, n_rows, sky=None, moments=None) -> np.ndarray:
    """A rank's part of main_runner_tree's single all-reduce: [flux (2 nbins) | f_inx | Σ weight *
    sln_prob (axions, photons) | rows], then the sky map's table when there is one, then with moments
    (errors=True; a dict of event_moments' tables, all additive over the ranks) [flux_sq | flux_xa |
    sky_sq | sky_xa (with a sky map) | totals (8)]."""
    tot = np.concatenate([flux, [float(f_inx), float(sum_axion), float(sum_photon), float(n_rows)]])
    if sky is not None:
        tot = np.concatenate([tot, np.asarray(sky, np.float64).reshape(-1)])
    if moments is None:
        return tot
    keys = ("flux_sq", "flux_xa") + (("sky_sq", "sky_xa") if sky is not None else ()) + ("totals",)
    return np.concatenate([tot] + [np.asarray(moments[k], np.float64).reshape(-1) for k in keys])


def unpack_totals(tot, nbins, sky_shape=None, moments=False) -> dict:
    """The parts of a pack_totals vector (sky_shape: the map's (2, n_theta, n_phi, n_dw), or None;
    moments: the vector ends with pack_totals' moments part, returned as a dict under "moments")."""
    m = 2 * nbins
    out = {"flux": tot[:m], "f_inx": tot[m], "sum_axion": tot[m + 1], "sum_photon": tot[m + 2], "rows": tot[m + 3]}
    at = m + 4
    ns = 0 if sky_shape is None else int(np.prod(sky_shape))
    if sky_shape is not None:
        out["sky"] = tot[at:at + ns].reshape(sky_shape)
        at += ns
    if moments:
        mo = {"sky_sq": None, "sky_xa": None}
        parts = [("flux_sq", m), ("flux_xa", m)] + ([("sky_sq", ns), ("sky_xa", ns)] if sky_shape is not None else [])
        for k, size in parts + [("totals", len(_lib.MOMENT_TOTALS))]:
            v = tot[at:at + size]
            mo[k] = v.reshape(sky_shape) if k.startswith("sky") else v
            at += size
        out["moments"] = mo
    return out


def _sigma_info(tt, nbins) -> dict:
    """run_info's σ keys from the reduced totals (unpack_totals(moments=True)): the global tables, the
    global f_inx and the global number of events"""
    mo, f = tt["moments"], tt["f_inx"]
    t8 = mo["totals"]
    out = {"flux_sigma": moments_sigma(tt["flux"], mo["flux_sq"], mo["flux_xa"], f, t8[2], t8[0]).reshape(2, nbins),
           "sum_weight_sln_prob_sigma": tuple(float(v) for v in moments_sigma(
               np.array([tt["sum_axion"], tt["sum_photon"]]), t8[3:5], t8[5:7], f, t8[2], t8[0]))}
    if "sky" in tt:
        out["sky_map_sigma"] = moments_sigma(tt["sky"], mo["sky_sq"], mo["sky_xa"], f, t8[2], t8[0])
    return out


REPLICATE_PARTS = ("run", "coupling", "halo")  # the order of the replicate parts of a rank's vector


SPECTRUM_PARTS = ("run", "coupling", "halo")  # the order of the spectrum parts of a rank's vector


def rank_vector(totals, coupling_raw=None, halo_raw=None, *, replicates=None, grid=None, spectrum=None, rank=0, world=1,
                exact=None, origin=None):
    """A rank's vector for main_runner_tree's single all-reduce, [pack_totals | coupling scan | halo scan |
    replicates... | grid]: the rank's pack_totals vector, then scan_pack of its coupling scan's raw tables and
    halo_scan_pack of its halo scan's, each only when there is one, then replicates_pack of each raw dict of
    `replicates` (a dict with the keys "run", "coupling", "halo" there are, in that order; None: none), then grid_pack
    of `grid` (the rank's grid_raw; None: none), so every earlier part keeps its place and its end, and LAST
    spectrum_pack(raw, rank, world) of each raw dict of `spectrum` (a dict with the keys "run", "coupling", "halo"
    there are, in that order; None: none, and the vector is what it is without the keyword); after them exact_pack of
    each raw dict of `exact` (the same keys and order; None: none, and the vector is what it is without the keyword);
    LAST of all `origin`, the rank's raw emission map (an array; None: none, and the vector is what it is without it).
    Returns (the vector, where each of its parts ends)."""
    parts = [totals] + [pack(raw) for pack, raw in ((scan_pack, coupling_raw), (halo_scan_pack, halo_raw)) if raw is not None]
    parts += [replicates_pack(replicates[k]) for k in REPLICATE_PARTS if replicates and replicates.get(k) is not None]
    if grid is not None:
        parts.append(grid_pack(grid))
    parts += [spectrum_pack(spectrum[k], rank, world) for k in SPECTRUM_PARTS if spectrum and spectrum.get(k) is not None]
    parts += [exact_pack(exact[k]) for k in EXACT_PARTS if exact and exact.get(k) is not None]
    if origin is not None:
        parts.append(np.asarray(origin, np.float64).reshape(-1))
    return (np.concatenate(parts) if len(parts) > 1 else totals), np.cumsum([len(v) for v in parts])


def _finish_run(rows, totals, coupling_raw=None, halo_raw=None, *, nbins, sky_kw, errors, world, run_info, events, n_events,
                g0, path, replicates=None, grid=None, spectrum=None, rank=0, exact=None, origin=None):
    """The end of main_runner_tree on every path: the rank's vector (rank_vector of its pack_totals vector and its
    scans' raw tables) summed over the ranks in ONE all-reduce, σ from the reduced tables, column 8 of the rank's
    rows divided by the global f_inx, run_info (a dict or None; events: the rank's (lo, hi), n_events: the run's),
    and with `path` the npy file and, with a sky map, skymap_<its stem>.npz beside it. g0: the run's coupling, the
    coupling scan's base. replicates: the rank's raw replicate tables (rank_vector's keyword), which end the vector
    and come back as run_info["replicates"] and as "replicates" in the scans' dicts. grid: the rank's grid_raw, the
    vector's part after them, which comes back as run_info["grid"] (grid_result). spectrum: the rank's raw spectra
    (rank_vector's keyword; rank: this rank's slot for its lists), the vector's last parts, which come back merged
    over the ranks as run_info["spectrum"] and as "spectrum" in the scans' dicts (spectrum_result). exact: the rank's
    raw exact accumulators (rank_vector's keyword), the parts after those, which come back summed over the ranks as
    run_info["exact"] and as "exact" in the scans' dicts (exact_result). origin: (the rank's raw emission map, its
    origin_spec), the vector's LAST part, which comes back summed over the ranks as run_info["origin"] (origin_result).
    Returns the rows."""
    from .shard import allreduce_sum
    tot, ends = rank_vector(totals, coupling_raw, halo_raw, replicates=replicates, **({} if grid is None else {"grid": grid}),
                            **({} if spectrum is None else {"spectrum": spectrum, "rank": rank, "world": world}),
                            **({} if exact is None else {"exact": exact}),
                            **({} if origin is None else {"origin": origin[0]}))
    n_scans = (coupling_raw is not None) + (halo_raw is not None)
    if world > 1:
        tot = allreduce_sum(tot)
    sky_shape = None if sky_kw is None else (2, sky_kw["n_theta"], sky_kw["n_phi"], sky_kw["n_dw"])
    tt = unpack_totals(tot[:ends[0]], nbins, sky_shape, moments=errors)
    sigma = _sigma_info(tt, nbins) if errors else {}
    f_glob = tt["f_inx"]
    if len(rows):
        rows[:, 7] /= f_glob  # saveAll[:, 8] ./= f_inx (MainRunner.jl:747), the whole run's f_inx
    if run_info is not None:
        run_info.update(f_inx=int(round(f_glob)), flux=(tt["flux"] / f_glob).reshape(2, nbins),
                        sum_weight_sln_prob=(tt["sum_axion"] / f_glob, tt["sum_photon"] / f_glob),
                        rows=int(round(tt["rows"])), events=events, n_events=n_events)
        if sky_kw is not None:
            run_info.update(sky_map=tt["sky"] / f_glob, sky_map_edges=sky_map_edges(**sky_kw))
        run_info.update(sigma)
        if coupling_raw is not None:
            raw = scan_unpack(tot[ends[0]:ends[1]], coupling_raw)
            run_info["coupling_scan"] = scan_result(raw, g0, int(round(f_glob)))
        if halo_raw is not None:
            raw = halo_scan_unpack(tot[ends[n_scans - 1]:ends[n_scans]], halo_raw)
            run_info["halo_scan"] = halo_scan_result(raw, int(round(f_glob)))
        have = [k for k in REPLICATE_PARTS if replicates and replicates.get(k) is not None]
        for j, k in enumerate(have):
            raw = replicates_unpack(tot[ends[n_scans + j]:ends[n_scans + j + 1]], replicates[k])
            where = run_info if k == "run" else run_info[k + "_scan"]
            where["replicates"] = replicates_result(raw, int(round(f_glob)))
        n_rep = len(have)
        if grid is not None:
            at = n_scans + n_rep
            run_info["grid"] = grid_result(grid_unpack(tot[ends[at]:ends[at + 1]], grid), int(round(f_glob)))
        at = n_scans + n_rep + (grid is not None)
        for j, k in enumerate(k for k in SPECTRUM_PARTS if spectrum and spectrum.get(k) is not None):
            raw = spectrum_unpack(tot[ends[at + j]:ends[at + j + 1]], spectrum[k], world)
            where = run_info if k == "run" else run_info[k + "_scan"]
            where["spectrum"] = spectrum_result(raw, int(round(f_glob)))
        at += sum(1 for k in SPECTRUM_PARTS if spectrum and spectrum.get(k) is not None)
        for j, k in enumerate(k for k in EXACT_PARTS if exact and exact.get(k) is not None):
            raw = exact_unpack(tot[ends[at + j]:ends[at + j + 1]], exact[k])
            where = run_info if k == "run" else run_info[k + "_scan"]
            where["exact"] = exact_result(raw, int(round(f_glob)))
        if origin is not None:  # (the vector's last part)
            run_info["origin"] = origin_result(tot[len(tot) - origin[0].size:], origin[1], int(round(f_glob)))
    if path is not None:
        os.makedirs(os.path.dirname(path), exist_ok=True)
        np.save(path, rows)
        if sky_kw is not None:
            te, pe, de = sky_map_edges(**sky_kw)
            stem = os.path.splitext(os.path.basename(path))[0]
            np.savez(os.path.join(os.path.dirname(path), f"skymap_{stem}.npz"), sky_map=tt["sky"] / f_glob,
                     theta_edges=te, phi_edges=pe, dw_edges=de, theta_axis=sky_kw["theta_axis"], f_inx=int(round(f_glob)),
                     **({"sky_map_sigma": sigma["sky_map_sigma"]} if errors else {}))
    return rows


def gather_rank_rows(dir_tag, params: Params, Ntajs, world, file_tag="", ntimes=3, num_cutoff=5, MC_nodes=5,
                     max_nodes=50) -> np.ndarray:
    """The rows of a sharded run: its per-rank files (file_tag + str(rank)) concatenated in rank
    order -- the rows the single-process run writes."""
    return np.concatenate([np.load(tree_file_name(dir_tag, params.mass_a, params.g_agg, params.theta_m,
                                                  params.omega_pul, params.B0, Ntajs, ntimes, num_cutoff, MC_nodes,
                                                  max_nodes, f"{file_tag}{r}")) for r in range(int(world))], axis=0)


def combine_files(Mass_a, Ax_g, θm, ωPul, B0, Ntajs, Nruns, file_tag, ntimes=3, dir_tag="results", num_cutoff=5,
                  MC_nodes=5, max_nodes=50, remove=True):
    """Gen_Samples.jl --run_Combine 1 (combine_files, Gen_Samples.jl:195-239): concatenate the
    npy rows of runs file_tag + "0" .. file_tag + str(Nruns - 1), divide column 8 (1-based,
    sln_prob) by Nruns, write them to dir_tag/<name with Ax_trajs = Ntajs * Nruns>.npy and
    delete the inputs. Returns the combined path."""
    files = [tree_file_name(dir_tag, Mass_a, Ax_g, θm, ωPul, B0, Ntajs, ntimes, num_cutoff, MC_nodes, max_nodes,
                            f"{file_tag}{i}") for i in range(int(Nruns))]
    hold = np.concatenate([np.load(f) for f in files], axis=0)
    hold[:, 7] /= Nruns  # hold[:, 8] ./= Nruns (Julia 1-based, :220)
    name = os.path.basename(tree_file_name(dir_tag, Mass_a, Ax_g, θm, ωPul, B0, Ntajs * Nruns, ntimes, num_cutoff,
                                           MC_nodes, max_nodes, file_tag))
    out = os.path.join(dir_tag, name[len("tree_"):])  # dir_tag/MassAx_... (:223-231)
    np.save(out, hold)
    if remove:
        for f in files:
            os.remove(f)
    return out


def combine_files_py(out_path, files) -> np.ndarray:
    """Combine_Files.py OUT IN... (the reference's Python combine, Combine_Files.py:1-31):
    the row files in the given order, each file's event numbers (column 1) offset by the last
    event number combined so far (:22), and -- its quirk -- column 10 (0-based 9, the sampled
    x position) divided by the number of files (:28). Writes out_path and returns the rows.
    (Gen_Samples.jl --run_Combine divides the sln_prob column instead: combine_files.)"""
    data = None
    for f in files:
        name = os.path.basename(f)
        if not (name[:5] == "tree_" and name[-4:] == ".npy"):
            raise ValueError(f"{f} is not a tree_*.npy row file")
        tmp = np.load(f).T.copy()
        if data is None:
            data = tmp
        else:
            tmp[0, :] += data[0, -1]
            data = np.append(data, tmp, axis=1)
    if data is None:
        raise ValueError("no input files")
    data[9, :] /= len(files)
    np.save(out_path, data.T)
    return data.T

