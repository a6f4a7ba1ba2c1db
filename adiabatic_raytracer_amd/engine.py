"""Device-resident batches: inputs and outputs live in HBM as torch tensors (PyTorch is
plumbing for device memory and streams here); every compute call goes through libart.so
on the caller's current HIP stream."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib
from ._lib import CrossingBuf, CyclotronOut, SegmentOut, check
from .raytracer import Params

F64 = torch.float64


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def nodes_to_numpy(nodes):
    """The records of Engine.grow_trees' `nodes` (a uint8 tensor of whole art_tree_node records),
    copied to the host and viewed as a trees.NODE_DTYPE record array."""
    from .trees import NODE_DTYPE
    return nodes.detach().cpu().contiguous().numpy().reshape(-1).view(NODE_DTYPE)


class Engine:
    def __init__(self, params: Params, device: int | None = None):
        self.lib = _lib.load()
        if not torch.cuda.is_available():
            raise _lib.ArtError("no GPU visible: the engine has no CPU fallback")
        self.device = torch.device("cuda", torch.cuda.current_device() if device is None else device)
        torch.cuda.set_device(self.device)
        check(self.lib.art_set_device(self.device.index))
        self.params = params
        self.cp = params.to_c()

    def empty(self, *shape, dtype=F64):
        return torch.empty(*shape, dtype=dtype, device=self.device)

    # ---- conversion-surface sampler (RayTracer.jl:1480-1653, MainRunner.jl:463-529)
    def sample(self, n: int, seed: int = 1769, ray_offset: int = 0, max_r=None, halo=None) -> dict:
        max_r = self.params.max_r() if max_r is None else max_r
        o = {"x": self.empty(3 * n), "k_init": self.empty(3 * n), "erg": self.empty(n), "vifty": self.empty(3 * n),
             "weights": self.empty(n, dtype=torch.int32), "attempts": self.empty(n, dtype=torch.int32)}
        bufs = [_p(o[k]) for k in ("x", "k_init", "erg", "vifty", "weights", "attempts")]
        if halo is not None:  # (a raytracer.Halo: the halo velocity model, include/art.h)
            check(self.lib.art_sample_conversion_points_halo_device(
                C.byref(self.cp), C.byref(halo.to_c()), float(max_r), int(seed), int(ray_offset), int(n), *bufs,
                _stream()))
            return o
        check(self.lib.art_sample_conversion_points_device(
            C.byref(self.cp), float(max_r), int(seed), int(ray_offset), int(n), *bufs, _stream()))
        return o

    def forward_roots(self, n: int, seed: int = 1769, ray_offset: int = 0, halo=None) -> dict:
        """Segment inputs of the forward-tree roots (MainRunner.jl:653-664 -> :179): photons
        at the sampled conversion points, Δω = -1, ln t0 = -30."""
        s = self.sample(n, seed, ray_offset, halo=halo)
        return {"x0": s["x"], "k0": s["k_init"], "erg": s["erg"],
                "dw": torch.full((n,), -1.0, dtype=F64, device=self.device),
                "ln_t0": torch.full((n,), -30.0, dtype=F64, device=self.device),
                "species": torch.ones(n, dtype=torch.int8, device=self.device), "sample": s}

    def alloc_out(self, n: int, capacity: int = 1) -> dict:
        # crossing slots a ray does not fill stay as allocated (include/art.h): NaN here, once
        nan = lambda m: self.empty(m).fill_(float("nan"))  # noqa: E731
        return {"x_end": self.empty(3 * n), "k_end": self.empty(3 * n), "u7_end": self.empty(n),
                "tau_end": self.empty(n), "status": self.empty(n, dtype=torch.int32),
                "n_accept": self.empty(n, dtype=torch.int32), "n_reject": self.empty(n, dtype=torch.int32),
                "n_cross": self.empty(n, dtype=torch.int32), "xc_pos": nan(3 * capacity * n),
                "xc_k": nan(3 * capacity * n), "xc_t": nan(capacity * n),
                "xc_dw": nan(capacity * n), "xc_p": nan(capacity * n), "capacity": capacity}

    # ---- RT.propagate (RayTracer.jl:171-452), asynchronous on the current stream
    def propagate(self, inp: dict, out: dict | None = None, max_crossings: int = -1, capacity: int = 1,
                  cyclotron: bool = False) -> dict:
        """cyclotron (art_propagate_cyclotron_device, Vern6): also each ray's cyclotron-resonance optical
        depth cyc_tau (n), the number of its crossings of ω_c = ω cyc_count (n), and the first one's
        cyc_pos (3, n) [km] and cyc_ln_t (n), which stay NaN where there is none."""
        n = inp["erg"].numel()
        out = out or self.alloc_out(n, capacity)
        so = SegmentOut(*[out[k].data_ptr() for k in ("x_end", "k_end", "u7_end", "tau_end", "status", "n_accept",
                                                    "n_reject")])
        xb = CrossingBuf(out["capacity"], *[out[k].data_ptr() for k in ("n_cross", "xc_pos", "xc_k", "xc_t", "xc_dw",
                                                                        "xc_p")])
        args = [C.byref(self.cp), n, *[_p(inp[k]) for k in ("x0", "k0", "erg", "dw", "ln_t0", "species")],
                int(max_crossings), C.byref(so), C.byref(xb)]
        if cyclotron:
            if "cyc_tau" not in out:
                out.update(cyc_tau=self.empty(n), cyc_count=self.empty(n, dtype=torch.int32),
                           cyc_pos=self.empty(3, n).fill_(float("nan")), cyc_ln_t=self.empty(n).fill_(float("nan")))
            cy = CyclotronOut(*[out[k].data_ptr() for k in ("cyc_tau", "cyc_count", "cyc_pos", "cyc_ln_t")])
            check(self.lib.art_propagate_cyclotron_device(*args, C.byref(cy), _stream()))
        else:
            check(self.lib.art_propagate_device(*args, _stream()))
        return out

    def set_tail_donation(self, lanes: int) -> None:
        """Tail donation for launches pipelined with others on other streams
        (art_set_tail_donation, include/art.h): a drained wave with <= lanes live rays hands
        them to a continuation launch and retires. Bit-identical results; 0 = off, -1 = the
        library's default by geometry (16 for Schwarzschild batches, else 0)."""
        check(self.lib.art_set_tail_donation(int(lanes)))

    def set_graduation(self, attempts: int) -> None:
        """Graduation of a launch's outlier rays to the one-wave-per-ray tail kernel
        (art_set_graduation, include/art.h): 0 = off (several batches in flight), -1 = the
        default (2048 attempts). Bit-identical results."""
        check(self.lib.art_set_graduation(int(attempts)))

    def set_sampler_waves(self, waves: int) -> None:
        """Waves per SIMD of the sampler (art_set_sampler_waves, include/art.h): 0 = by line
        length (the default), 3 = the 3-wave build for every line (several sampler launches in
        flight). Bit-identical samples."""
        check(self.lib.art_set_sampler_waves(int(waves)))

    def kernel_ms(self) -> float:
        """Duration of the last propagate kernel (HIP events on its stream); synchronizes."""
        check(self.lib.art_synchronize())
        return float(self.lib.art_last_kernel_ms())

    # ---- binned flux (plot/flux.py:38-48)
    def flux_histogram(self, out: dict, species, weights=None, nbins: int = 50, hist=None):
        n = out["status"].numel()
        hist = torch.zeros(2 * nbins, dtype=F64, device=self.device) if hist is None else hist
        check(self.lib.art_flux_histogram_device(C.byref(self.cp), n, _p(out["x_end"]), _p(out["k_end"]),
                                                 _p(out["status"]), _p(species), _p(weights), int(nbins), _p(hist),
                                                 _stream()))
        return hist

    # ---- sky map: flux over (θf | cos θf, φf, Δω) per species (art_sky_map_segments_device)
    def sky_map(self, out: dict, species, weights=None, *, n_theta: int = 32, n_phi: int = 64, n_dw: int = 1,
                theta_axis: str = "cos", dw_range=None, dw_offset=None, hist=None, return_bins: bool = False,
                mode: int = 0):
        """The batch's final segments binned by the direction and line shift of their final momentum,
        on the current stream: a (2, n_theta, n_phi, n_dw) float64 tensor (axions, photons), added to
        `hist` when one is given. theta_axis "cos" bins cos θf over [-1, 1] (equal solid angle),
        "theta" θf over [0, π]; φf over [-π, π]; Δω = u7_end / mass_a + dw_offset over dw_range, which
        n_dw > 1 needs (n_dw = 1 is one bin for every finite Δω). return_bins: also each ray's flat
        bin index (int32, -1 for a ray that is not counted). mode: 0 picks the accumulation path by the
        table's size, 1 forces the block-private LDS table, 2 adds to HBM (include/art.h)."""
        n = out["status"].numel()
        if n_dw > 1 and dw_range is None:
            raise ValueError("sky_map: n_dw > 1 needs dw_range")
        lo, hi = (0.0, 0.0) if dw_range is None else (float(dw_range[0]), float(dw_range[1]))
        spec = _lib.SkySpec(int(n_theta), int(n_phi), int(n_dw), _lib.THETA_AXIS[theta_axis], int(mode), lo, hi)
        if hist is None:
            hist = torch.zeros(2, n_theta, n_phi, n_dw, dtype=F64, device=self.device)
        bins = self.empty(n, dtype=torch.int32) if return_bins else None
        check(self.lib.art_sky_map_segments_device(C.byref(self.cp), C.byref(spec), n, _p(out["x_end"]), _p(out["k_end"]),
                                                   _p(out["u7_end"]), _p(out["status"]), _p(species), _p(weights),
                                                   _p(dw_offset), _p(hist), _p(bins), _stream()))
        return (hist, bins) if return_bins else hist

    # ---- get_Prob_nonAD (MainRunner.jl:67-124)
    def get_prob_nonad(self, pos, kpos, erg_eff, group_start=None):
        nc = erg_eff.numel()
        out = self.empty(nc)
        ng = nc if group_start is None else group_start.numel() - 1
        check(self.lib.art_get_prob_nonad_device(C.byref(self.cp), nc, _p(pos), _p(kpos), _p(erg_eff), ng,
                                                 _p(group_start), _p(out), _stream()))
        return out

    # ---- per-sample event weight (MainRunner.jl:498-557): 5 x n SoA
    def event_weight(self, sample: dict, max_r=None, rho_DM=0.45, n_maxSample=6, halo=None):
        n = sample["erg"].numel()
        max_r = self.params.max_r() if max_r is None else max_r
        out = self.empty(5 * n)
        if halo is not None:  # (the Halo the sample was drawn with)
            check(self.lib.art_event_weight_halo_device(C.byref(self.cp), C.byref(halo.to_c()), float(max_r),
                                                        float(rho_DM), float(n_maxSample), n, _p(sample["x"]),
                                                        _p(sample["k_init"]), _p(sample["vifty"]), _p(out), _stream()))
            return out.view(5, n)
        check(self.lib.art_event_weight_device(C.byref(self.cp), float(max_r), float(rho_DM), float(n_maxSample), n,
                                               _p(sample["x"]), _p(sample["k_init"]), _p(sample["vifty"]), _p(out),
                                               _stream()))
        return out.view(5, n)

    # ---- get_tree (MainRunner.jl:126-352) for n roots, every tree's state in HBM (art_grow_trees_device)
    def grow_trees(self, x0, k0, erg, species, *, num_cutoff=5, mc_nodes=5, max_nodes=50, splittings_cutoff=-1,
                   crossing_cap=64, prob_cutoff=1e-10, seed=1769, tree_offset=0, node_capacity=None) -> dict:
        """The forest of n roots held in HBM -- x0, k0 (3n SoA, float64), erg (n), species (n int8, or
        one ART_AXION / ART_PHOTON for all) -- on the current stream; the options are trees.grow_trees'.
        Returns a dict of device tensors: nodes, uint8 (n_nodes, record size), whole art_tree_node
        records, trees in order and each tree's nodes in the order it processed them (nodes_to_numpy
        views a copy as trees.NODE_DTYPE); node_start int64 (n + 1): tree i owns records
        node_start[i] .. node_start[i + 1]; counts, infos int32 (n): get_tree's count and info; and
        n_nodes (an int). Unlike the other methods it blocks until the forest is done (the driver reads
        the count of active trees between rounds). node_capacity: records to allocate (default: the
        bound n (max_nodes + 2), or n for the backtrace form); a smaller one is grown and the forest
        run again when it does not suffice (ART_E_NOMEM)."""
        from .trees import NODE_DTYPE
        rec = NODE_DTYPE.itemsize
        n = erg.numel()
        x0, k0, erg = (t.to(F64).contiguous() for t in (x0, k0, erg))
        if not torch.is_tensor(species):
            species = torch.full((n,), int(species), dtype=torch.int8, device=self.device)
        species = species.to(torch.int8).contiguous()
        if x0.numel() != 3 * n or k0.numel() != 3 * n or species.numel() != n:
            raise ValueError("grow_trees: x0 and k0 hold 3n values, erg and species n")
        opts = _lib.TreeOpts(num_cutoff, mc_nodes, max_nodes, splittings_cutoff, crossing_cap, int(tree_offset),
                             prob_cutoff, seed)
        per_tree = 1 if (splittings_cutoff > 0 and num_cutoff <= 0) else max_nodes + 2
        cap = max(1, n * per_tree if node_capacity is None else int(node_capacity))
        node_start = self.empty(n + 1, dtype=torch.int64)
        counts, infos = self.empty(n, dtype=torch.int32), self.empty(n, dtype=torch.int32)
        while True:
            nodes = self.empty(cap, rec, dtype=torch.uint8)
            nn = C.c_int64(0)
            rc = self.lib.art_grow_trees_device(C.byref(self.cp), n, _p(x0), _p(k0), _p(erg), _p(species), C.byref(opts),
                                                cap, _p(nodes), _p(node_start), _p(counts), _p(infos), C.byref(nn),
                                                _stream())
            if rc == -3 and nn.value > cap:  # ART_E_NOMEM: the needed count is known now
                cap = nn.value
                continue
            check(rc)
            break
        used = nodes[:nn.value]
        if 2 * nn.value < cap:  # (do not keep the whole bound alive behind a small view)
            used = used.clone()
        return {"nodes": used, "node_start": node_start, "counts": counts, "infos": infos, "n_nodes": int(nn.value)}

    # ---- main_runner_tree's rows, flux and sky map from forests in HBM (art_event_rows_device)
    def _sky_spec(self, sky):
        """(SkySpec, shape, the keywords completed) of a sky-map dict: sky_map()'s keywords n_theta, n_phi,
        n_dw, theta_axis, dw_range, and mode. None (no map): three None."""
        if sky is None:
            return None, None, None
        kw ={"n_theta": 32, "n_phi": 64, "n_dw": 1, "theta_axis": "cos", "dw_range": None, "mode": 0}
        if set(sky) - set(kw):
            raise ValueError(f"sky_map: unknown keys {sorted(set(sky) - set(kw))}")
        kw.update(sky)
        if kw["theta_axis"] not in _lib.THETA_AXIS:
            raise ValueError(f"theta_axis must be 'cos' or 'theta', not {kw['theta_axis']!r}")
        if kw["n_dw"] > 1 and kw["dw_range"] is None:
            raise ValueError("sky_map: n_dw > 1 needs a dw_range (a data-dependent range cannot be binned chunk by chunk)")
        lo, hi = (0.0, 0.0) if kw["dw_range"] is None else (float(kw["dw_range"][0]), float(kw["dw_range"][1]))
        spec = _lib.SkySpec(int(kw["n_theta"]), int(kw["n_phi"]), int(kw["n_dw"]), _lib.THETA_AXIS[kw["theta_axis"]],
                            int(kw["mode"]), lo, hi)
        return spec, (2, int(kw["n_theta"]), int(kw["n_phi"]), int(kw["n_dw"])), kw

    def event_rows(self, sample, weight5, back, forward, *, event_offset=0, saveMode=0, nbins=50, flux=None, sky=None,
                   sky_hist=None, totals=None, rows=True, cyclotron=False, return_bins=False) -> dict:
        """The npy rows of main_runner_tree for one chunk of events whose forests the caller grew, on the
        current stream: sample (Engine.sample's dict), weight5 (Engine.event_weight's (5, n)), back and
        forward (Engine.grow_trees' dicts of the backtrace and of the forward forest). One pass over the
        forward nodes writes the rows of the final ones in node order (13 columns, 29 with saveMode > 0;
        column 7 is the raw sln_prob, NOT yet divided by f_inx) and adds column 8 * column 7 to
        flux (2 nbins; nbins = 0: none), to the sky map sky_hist (sky: a dict of n_theta, n_phi, n_dw,
        theta_axis, dw_range, mode; None: no map) and to totals (6 float64: rows, photon rows,
        Σ weight sln_prob of axions and of photons, Σ (attempts - 1), cyclotron mismatches). flux,
        sky_hist and totals are ACCUMULATED into when given, else start at zero. rows=False only bins.
        cyclotron: the final photon segments run again through art_propagate_cyclotron_device (one count
        comes to the host for it), τ goes into column 14 and exp(-τ) into column 8; a re-run that does
        not reproduce its node's end state is counted in totals[5]. return_bins: also each row's flat
        sky bin (int32, -1 for not counted). Returns a dict: rows ((n_rows, ncols) or None), n_rows
        (an int when rows or bins were asked for, which costs one synchronisation, else None), flux,
        sky_hist, totals, chunk_totals (this call's part of totals), bins, and cyclotron_rerun (the re-run
        this call made, for event_moments of the same chunk; None without cyclotron)."""
        n = sample["erg"].numel()
        nn = int(forward["n_nodes"])
        ncols = 29 if saveMode > 0 else 13
        nbins = int(nbins)
        if flux is None:
            flux = torch.zeros(2 * nbins, dtype=F64, device=self.device)
        spec, shape, _ = self._sky_spec(sky)
        if spec is not None and sky_hist is None:
            sky_hist = torch.zeros(*shape, dtype=F64, device=self.device)
        if return_bins and spec is None:
            raise ValueError("event_rows: return_bins needs a sky map")
        part = torch.zeros(len(_lib.EVENT_TOTALS), dtype=F64, device=self.device)
        out_rows = self.empty(max(nn, 1), ncols) if rows else None
        bins = self.empty(max(nn, 1), dtype=torch.int32) if return_bins else None
        keep = self._cyclotron_rerun(sample, forward, nn, n) if cyclotron else None
        ei = self._event_rows_in(sample, weight5, back, forward, event_offset, keep)
        eo = _lib.EventRowsOut(ncols, nbins, _p(out_rows), nn if (rows or return_bins) else 0, _p(flux),
                               C.pointer(spec) if spec is not None else None, _p(sky_hist), _p(bins), _p(part))
        check(self.lib.art_event_rows_device(C.byref(self.cp), C.byref(ei), C.byref(eo), _stream()))
        if totals is None:
            totals = part
        else:
            totals += part
        n_rows = None
        if rows or return_bins:
            n_rows = int(part[0].item())
            out_rows = out_rows[:n_rows] if rows else None
            bins = bins[:n_rows] if return_bins else None
        return {"rows": out_rows, "n_rows": n_rows, "flux": flux, "sky_hist": sky_hist, "totals": totals,
                "chunk_totals": part, "bins": bins, "cyclotron_rerun": keep}

    def _event_rows_in(self, sample, weight5, back, forward, event_offset, rerun):
        """art_event_rows_in of one chunk (rerun: _cyclotron_rerun's dict, or None)"""
        ei = _lib.EventRowsIn(sample["erg"].numel(), int(event_offset), sample["x"].data_ptr(), sample["k_init"].data_ptr(),
                              sample["attempts"].data_ptr() if sample.get("attempts") is not None else None,
                              weight5.data_ptr(), back["nodes"].data_ptr(), back["counts"].data_ptr(),
                              forward["nodes"].data_ptr(), int(forward["n_nodes"]), forward["counts"].data_ptr(),
                              forward["infos"].data_ptr(), None, 0, None, None)
        if rerun is not None:
            ei.cyc_slot, ei.cyc_n, ei.cyc_tau = rerun["slot"].data_ptr(), rerun["m"], rerun["tau"].data_ptr()
            ei.cyc_end = C.pointer(rerun["end"])
        return ei

    def _zero_moments(self, nbins, shape):
        z = lambda *s: torch.zeros(*s, dtype=F64, device=self.device)  # noqa: E731
        return {"flux_sq": z(2 * nbins), "flux_xa": z(2 * nbins), "sky_sq": z(*shape) if shape else None,
                "sky_xa": z(*shape) if shape else None, "totals": z(len(_lib.MOMENT_TOTALS))}

    def event_moments(self, sample, weight5, back, forward, *, event_offset=0, nbins=50, sky=None, moments=None,
                      cyclotron_rerun=None) -> dict:
        """The second moments of one chunk's binned event power (art_event_moments_device), on the current
        stream and without a synchronisation: the arguments of event_rows for the same chunk, whose bins
        and powers (column 8 * column 7) it takes. Per event e and bin b the content X = Σ power of e's
        final rows in b is formed first; the tables take Q = Σ_e X² and C = Σ_e X a_e with
        a_e = attempts[e] - 1 + e's final photon rows. Returns a dict of device tensors, float64: flux_sq,
        flux_xa (2 nbins), sky_sq, sky_xa (the map's shape; None without sky) and totals (8: events, Σ a_e,
        Σ a_e², Q of axions and photons over all their rows, C of axions and photons, misplaced records,
        which must stay 0). moments: such a dict of an earlier chunk, ACCUMULATED into and returned.
        cyclotron_rerun: event_rows' "cyclotron_rerun" of this chunk, so exp(-τ) is in the powers as it is
        in column 8; nothing is propagated here. trees.moments_sigma turns the tables into errors."""
        nbins = int(nbins)
        spec, shape, _ = self._sky_spec(sky)
        if moments is None:
            moments = self._zero_moments(nbins, shape)
        if moments["flux_sq"].numel() != 2 * nbins or (shape and tuple(moments["sky_sq"].shape) != shape):
            raise ValueError("event_moments: `moments` was made for other tables")
        ei = self._event_rows_in(sample, weight5, back, forward, event_offset, cyclotron_rerun)
        mo = _lib.EventMomentsOut(nbins, 0, _p(moments["flux_sq"]), _p(moments["flux_xa"]),
                                  C.pointer(spec) if spec is not None else None, _p(moments["sky_sq"]) if shape else None,
                                  _p(moments["sky_xa"]) if shape else None, _p(moments["totals"]))
        check(self.lib.art_event_moments_device(C.byref(self.cp), C.byref(ei), _p(forward["node_start"]), C.byref(mo),
                                                _stream()))
        return moments

    def _couplings(self, couplings):
        """The list of a coupling scan as floats, checked as art_event_reweight_device checks it"""
        import math
        g = [float(v) for v in couplings]
        if not 1 <= len(g) <= _lib.REWEIGHT_MAX_COUPLINGS:
            raise ValueError(f"couplings: 1 to {_lib.REWEIGHT_MAX_COUPLINGS} values, not {len(g)}")
        if not all(math.isfinite(v) and v > 0.0 for v in g):
            raise ValueError("couplings: every coupling must be finite and > 0")
        if not (math.isfinite(self.params.g_agg) and self.params.g_agg > 0.0):
            raise ValueError("couplings: the base coupling params.g_agg must be finite and > 0")
        return g

    def _zero_scan(self, K, n_totals, nbins, shape, errors, ident):
        """The zero tables of a scan over K sets (couplings or halo models), its totals n_totals wide. ident: what
        the scan was made for, its first keys ({"g": [...]}, or {"base": ..., "models": [...]})."""
        z = lambda *d: torch.zeros(*d, dtype=F64, device=self.device)  # noqa: E731
        scan = {**ident, "flux": z(K, 2 * nbins), "sky": z(K, *shape) if shape else None, "totals": z(K, n_totals),
                "n_events": 0}
        if errors:
            scan.update(flux_sq=z(K, 2 * nbins), flux_xa=z(K, 2 * nbins), sky_sq=z(K, *shape) if shape else None,
                        sky_xa=z(K, *shape) if shape else None, moment_totals=z(K, len(_lib.MOMENT_TOTALS)))
        return scan

    @staticmethod
    def _scan_fits(scan, ident, nbins, shape, errors):
        """Was `scan` (a _zero_scan, maybe added to since) made for this ident and these tables?"""
        return (all(scan[k] == v for k, v in ident.items()) and scan["flux"].shape[1] == 2 * nbins and
                errors == ("moment_totals" in scan) and
                (None if scan["sky"] is None else tuple(scan["sky"].shape[1:])) == shape)

    @staticmethod
    def _finish_scan(scan, zero, result, counter, what):
        """run_events' last step for a scan: zero tables (zero()) when there were no events, the tables as `result`
        makes them the scan's dict of host arrays, and its integrity counter, which must be 0"""
        out = result(zero() if scan is None else scan)
        if out[counter] != 0:
            raise _lib.ArtError(f"run_events: {out[counter]} node records {what}")
        return out

    @staticmethod
    def _scan_out(scan, nbins, spec, shape):
        """What art_event_reweight_out and art_event_halo_scan_out share: (nbins, reserved, flux, sky, sky_hist,
        totals), the fields after the first, and the five moment tables, the last ones"""
        mo = [_p(scan.get(k)) for k in ("flux_sq", "flux_xa", "sky_sq", "sky_xa", "moment_totals")]
        return (nbins, 0, _p(scan["flux"]), C.pointer(spec) if spec is not None else None,
                _p(scan["sky"]) if shape else None, _p(scan["totals"])), mo

    def event_reweight(self, sample, weight5, back, forward, couplings, *, mc_nodes, event_offset=0, nbins=50, sky=None,
                       errors=False, cyclotron_rerun=None, scan=None, return_weights=False) -> dict:
        """The coupling scan of one chunk (art_event_reweight_device; DESIGN.md §3, "Coupling scan"), on the
        current stream and without a synchronisation: the arguments of event_rows for the same chunk, whose
        forests were grown at the base coupling g0 = params.g_agg, reweighted to every g of `couplings` (1 to
        32 finite, positive values). mc_nodes: the forward forest's (grow_trees' mc_nodes), which says which
        children were Monte-Carlo draws. Returns a dict of device tensors, float64, each with a leading axis
        over the couplings: flux (K, 2 nbins), sky (K, the map's shape; None without sky), totals (K, 6:
        Σ power of axions and of photons, coverage summed over the trees, saturated, unlinked,
        recomputed_differs -- _lib.REWEIGHT_TOTALS), n_events (a number, summed over the chunks), and with
        errors flux_sq, flux_xa, sky_sq, sky_xa and moment_totals (K, 8), art_event_moments_device's tables
        per coupling. scan: such a dict of an earlier chunk, ACCUMULATED into and returned. cyclotron_rerun:
        event_rows' "cyclotron_rerun" of this chunk, so exp(-τ) is in the powers (τ does not depend on g).
        return_weights: also weights (K, n_nodes), W_k of every node record of THIS chunk, back
        (K, n_events), its events' backtrace factors, and back_prob, their first factor 1 - exp(-s x_root)."""
        g = self._couplings(couplings)
        K, nbins = len(g), int(nbins)
        n, nn = sample["erg"].numel(), int(forward["n_nodes"])
        spec, shape, _ = self._sky_spec(sky)
        if scan is None:
            scan = self._zero_scan(K, len(_lib.REWEIGHT_TOTALS), nbins, shape, errors, {"g": list(g)})
        if not self._scan_fits(scan, {"g": g}, nbins, shape, errors):
            raise ValueError("event_reweight: `scan` was made for other couplings or tables")
        # (zeros: a record outside its own tree's range is written by no lane)
        W = torch.zeros(K, max(nn, 1), dtype=F64, device=self.device) if return_weights else None
        B = self.empty(K, max(n, 1)) if return_weights else None
        Bp = self.empty(K, max(n, 1)) if return_weights else None
        ei = self._event_rows_in(sample, weight5, back, forward, event_offset, cyclotron_rerun)
        tables, mo = self._scan_out(scan, nbins, spec, shape)
        ro = _lib.EventReweightOut(_p(sample["erg"]), *tables, _p(W), _p(B), _p(Bp), *mo)
        opts = _lib.TreeOpts(0, int(mc_nodes), 0, -1, 0, 0, 0.0, 0)  # (only mc_nodes is read)
        check(self.lib.art_event_reweight_device(C.byref(self.cp), C.byref(ei), _p(forward["node_start"]), C.byref(opts),
                                                 K, (C.c_double * K)(*g), C.byref(ro), _stream()))
        scan["n_events"] += n
        if return_weights:
            scan["weights"], scan["back"], scan["back_prob"] = W[:, :nn], B[:, :n], Bp[:, :n]
        return scan

    @staticmethod
    def _halo_key(base):
        """(v0, v_ns, the resolved proposal scale) of the base of a halo scan"""
        return float(base.v0), tuple(float(c) for c in base.v_ns), base.vp()

    def event_halo_scan(self, sample, weight5, back, forward, base, halos, *, event_offset=0, nbins=50, sky=None,
                        scan=None, errors=False, return_ratio=False, cyclotron_rerun=None) -> dict:
        """The halo scan of one chunk (art_event_halo_scan_device; DESIGN.md §3, "Halo scan"), on the current
        stream and without a synchronisation: the arguments of event_rows for the same chunk, which was
        sampled and weighted under the raytracer.Halo `base`, reweighted to every model of `halos` (1 to 32
        Halo objects or (v0, v_ns) pairs; v0 at most base.vp(); a model's own v_prop is ignored). Per event
        and model R = F_model / F_base (trees.halo_ratio) multiplies the run's own column 8 * column 7, in the
        run's own bins. Returns a dict of device tensors, float64, each with a leading axis over the models:
        flux (K, 2 nbins), sky (K, the map's shape; None without sky), totals (K, 5: Σ power of axions and of
        photons, Σ_e R, Σ_e R², misplaced records -- _lib.HALO_SCAN_TOTALS), models, base, n_events (a number,
        summed over the chunks), and with errors flux_sq, flux_xa, sky_sq, sky_xa and moment_totals (K, 8),
        art_event_moments_device's tables per model. scan: such a dict of an earlier chunk, ACCUMULATED into
        and returned. cyclotron_rerun: event_rows' "cyclotron_rerun" of this chunk, so exp(-τ) is in the
        powers (τ does not depend on the halo). return_ratio: also ratio (K, n_events), R of THIS chunk."""
        from .trees import halo_scan_models
        models = halo_scan_models(base, halos)
        K, nbins = len(models), int(nbins)
        n = sample["erg"].numel()
        spec, shape, _ = self._sky_spec(sky)
        ident = {"base": self._halo_key(base), "models": list(models)}
        if scan is None:
            scan = self._zero_scan(K, len(_lib.HALO_SCAN_TOTALS), nbins, shape, errors, ident)
        if not self._scan_fits(scan, ident, nbins, shape, errors):
            raise ValueError("event_halo_scan: `scan` was made for another base, other models or other tables")
        R = self.empty(K, max(n, 1)) if return_ratio else None
        ei = self._event_rows_in(sample, weight5, back, forward, event_offset, cyclotron_rerun)
        tables, mo = self._scan_out(scan, nbins, spec, shape)
        ho = _lib.EventHaloScanOut(_p(sample["vifty"]), *tables, _p(R), *mo)
        arr = (_lib.ArtHalo * K)(*[_lib.ArtHalo(v0, (C.c_double * 3)(*v), -1.0) for v0, v in models])
        check(self.lib.art_event_halo_scan_device(C.byref(self.cp), C.byref(ei), _p(forward["node_start"]),
                                                  C.byref(base.to_c()), K, arr, C.byref(ho), _stream()))
        scan["n_events"] += n
        if return_ratio:
            scan["ratio"] = R[:, :n]
        return scan

    # The most bytes the replicate tables of one set of tables (the run's, a coupling scan's or a halo scan's) may take
    REPLICATES_MAX_BYTES = 1 << 30

    @staticmethod
    def _replicates_groups(R):
        """The group count of replicates= as an int, checked as art_event_replicates_device checks it"""
        if int(R) != R or not _lib.REPLICATES_MIN_GROUPS <= int(R) <= _lib.REPLICATES_MAX_GROUPS:
            raise ValueError(f"replicates: {_lib.REPLICATES_MIN_GROUPS} to {_lib.REPLICATES_MAX_GROUPS} groups, not {R!r}")
        return int(R)

    @classmethod
    def _replicates_fit(cls, what, K, R, nbins, shape):
        """ValueError when the replicate tables of K sets and R groups exceed REPLICATES_MAX_BYTES"""
        sky = 1
        for d in shape or (0,):
            sky *= d
        size = 8 * K * R * (2 * nbins + sky + 2)
        if size > cls.REPLICATES_MAX_BYTES:
            raise ValueError(f"replicates: the replicate tables of {what} ({K} sets x {R} groups) would take {size} bytes, "
                             f"more than {cls.REPLICATES_MAX_BYTES}: drop the sky map from the scan or lower R")

    def _zero_replicates(self, kind, K, R, nbins, shape):
        z = lambda *d: torch.zeros(*d, dtype=F64, device=self.device)  # noqa: E731
        return {"kind": kind, "R": R, "flux": z(K, R, 2 * nbins), "sky": z(K, R, *shape) if shape else None,
                "totals": z(K, R, 2), "groups": z(R, len(_lib.REPLICATE_GROUPS))}

    def event_replicates(self, sample, weight5, back, forward, R, *, event_offset=0, nbins=50, sky=None,
                         cyclotron_rerun=None, rep=None, kind="run", node_factor=None, event_factor=None) -> dict:
        """The jackknife replicates of one chunk (art_event_replicates_device; DESIGN.md §3, "Jackknife
        replicates"), on the current stream and without a synchronisation: the arguments of event_rows for the same
        chunk, whose first-moment tables it keeps per group of events, g = (event_offset + tree) mod R (2 <= R <= 64).
        kind "run": the run's own powers, one set. kind "coupling": the powers of a coupling scan, from
        node_factor = event_reweight(return_weights=True)'s "weights" (K, n_nodes) and event_factor = its "back"
        (K, n_events). kind "halo": those of a halo scan, from event_factor = event_halo_scan(return_ratio=True)'s
        "ratio" (K, n_events). Returns a dict of device tensors, float64: flux (K, R, 2 nbins), sky (K, R, the map's
        shape; None without sky), totals (K, R, 2: Σ power of all final axion and photon rows) and groups (R, 3:
        events, a_g = Σ (attempts - 1) + final photon rows, misplaced records -- _lib.REPLICATE_GROUPS), with kind and
        R. rep: such a dict of an earlier chunk, ACCUMULATED into and returned. cyclotron_rerun: event_rows'
        "cyclotron_rerun" of this chunk, so exp(-τ) is in the powers. trees.jackknife turns the tables into errors."""
        R, nbins = self._replicates_groups(R), int(nbins)
        if kind not in _lib.REPLICATE_KINDS:
            raise ValueError(f"event_replicates: kind must be one of {sorted(_lib.REPLICATE_KINDS)}, not {kind!r}")
        if (kind == "coupling" and node_factor is None) or (kind != "run" and event_factor is None):
            raise ValueError(f"event_replicates: kind {kind!r} needs its factor arrays")
        K = 1 if kind == "run" else int(event_factor.shape[0])
        spec, shape, _ = self._sky_spec(sky)
        if rep is None:
            rep = self._zero_replicates(kind, K, R, nbins, shape)
        if (rep["kind"] != kind or tuple(rep["flux"].shape) != (K, R, 2 * nbins) or
                (None if rep["sky"] is None else tuple(rep["sky"].shape[2:])) != shape):
            raise ValueError("event_replicates: `rep` was made for another kind, other groups, sets or tables")
        n, nn = sample["erg"].numel(), int(forward["n_nodes"])
        if kind != "run" and (tuple(event_factor.shape) != (K, n) or not event_factor.is_contiguous()):
            raise ValueError("event_replicates: event_factor must be a contiguous (K, n_events) tensor")
        if kind == "coupling" and (tuple(node_factor.shape) != (K, nn) or (nn > 0 and not node_factor.is_contiguous())):
            raise ValueError("event_replicates: node_factor must be a contiguous (K, n_nodes) tensor")
        ei = self._event_rows_in(sample, weight5, back, forward, event_offset, cyclotron_rerun)
        ro = _lib.EventReplicatesOut(R, _lib.REPLICATE_KINDS[kind], K, nbins, _p(node_factor) if kind == "coupling" else None,
                                     _p(event_factor) if kind != "run" else None, _p(rep["flux"]),
                                     C.pointer(spec) if spec is not None else None, _p(rep["sky"]) if shape else None,
                                     _p(rep["totals"]), _p(rep["groups"]))
        check(self.lib.art_event_replicates_device(C.byref(self.cp), C.byref(ei), _p(forward["node_start"]), C.byref(ro),
                                                   _stream()))
        return rep

    # The most bytes the exact accumulators of one set of tables (the run's, a coupling scan's or a halo scan's) may take
    EXACT_MAX_BYTES = 1 << 30

    @classmethod
    def _exact_fit(cls, what, K, nbins, shape):
        """ValueError when the exact accumulators of K sets exceed EXACT_MAX_BYTES"""
        sky = 1
        for d in shape or (0,):
            sky *= d
        size = 8 * _lib.EXACT_LIMBS * K * (2 * nbins + sky + 2)
        if size > cls.EXACT_MAX_BYTES:
            raise ValueError(f"exact: the accumulators of {what} ({K} sets of {_lib.EXACT_LIMBS} limbs per bin) would take "
                             f"{size} bytes, more than {cls.EXACT_MAX_BYTES}: drop the sky map from the scan, coarsen it or "
                             "scan fewer values")

    def _zero_exact(self, kind, K, nbins, shape):
        z = lambda *d: torch.zeros(*d, _lib.EXACT_LIMBS, dtype=torch.int64, device=self.device)  # noqa: E731
        return {"kind": kind, "flux": z(K, 2 * nbins), "sky": z(K, *shape) if shape else None, "totals": z(K, 2),
                "nonfinite": torch.zeros(K, dtype=F64, device=self.device),
                "misplaced": torch.zeros(1, dtype=F64, device=self.device)}

    def exact_histogram(self, bins, values, n_bins, *, acc=None, nonfinite=None, mode="auto"):
        """values[i] added exactly to accumulator bins[i] of n_bins (art_exact_histogram_device; DESIGN.md §3, "Exact
        tables"), on the current stream: bins an int32 and values a float64 device tensor of one length; a bin < 0 or
        >= n_bins is skipped, a NaN or an infinity is counted and not added. Returns (acc, nonfinite): acc
        (n_bins, 66) int64, normalised limbs, and nonfinite (1) float64; both are ACCUMULATED into when given.
        mode: "auto", "lds" (n_bins <= 124) or "global"; the limbs do not depend on it. exact_round gives the sums."""
        n_bins = int(n_bins)
        if bins.dtype != torch.int32 or values.dtype != F64 or bins.numel() != values.numel():
            raise ValueError("exact_histogram: bins must be int32 and values float64, of one length")
        if acc is None:
            acc = torch.zeros(n_bins, _lib.EXACT_LIMBS, dtype=torch.int64, device=self.device)
        if nonfinite is None:
            nonfinite = torch.zeros(1, dtype=F64, device=self.device)
        if tuple(acc.shape) != (n_bins, _lib.EXACT_LIMBS) or acc.dtype != torch.int64 or not acc.is_contiguous():
            raise ValueError("exact_histogram: acc must be a contiguous int64 (n_bins, 66) tensor")
        check(self.lib.art_exact_histogram_device(values.numel(), _p(bins.contiguous()), _p(values.contiguous()), n_bins,
                                                  _p(acc), _p(nonfinite), _lib.EXACT_MODES[mode], _stream()))
        return acc, nonfinite

    def exact_round(self, acc):
        """The correctly rounded float64 sums of accumulators (..., 66) (art_exact_finish_device), on the current
        stream; the accumulators are only read"""
        if acc.dtype != torch.int64 or acc.shape[-1] != _lib.EXACT_LIMBS or not acc.is_contiguous():
            raise ValueError("exact_round: acc must be a contiguous int64 (..., 66) tensor")
        out = self.empty(*acc.shape[:-1]) if acc.numel() else torch.zeros(*acc.shape[:-1], dtype=F64, device=self.device)
        check(self.lib.art_exact_finish_device(out.numel(), _p(acc), _p(out), _stream()))
        return out

    def event_exact(self, sample, weight5, back, forward, *, event_offset=0, nbins=50, sky=None, cyclotron_rerun=None,
                    acc=None, kind="run", node_factor=None, event_factor=None, mode="auto") -> dict:
        """The exact tables of one chunk (art_event_exact_device; DESIGN.md §3, "Exact tables"), on the current stream
        and without a synchronisation: event_replicates' arguments without the groups, and its kinds -- "run", one
        set; "coupling" from node_factor = event_reweight(return_weights=True)'s "weights" and event_factor = its
        "back"; "halo" from event_factor = event_halo_scan(return_ratio=True)'s "ratio". The powers of the chunk's
        final rows are added to fixed-point accumulators of 66 int64 limbs per bin, so the tables are sums that do not
        depend on the order of the adds. Returns a dict of device tensors: flux (K, 2 nbins, 66), sky (K, the map's
        shape, 66; None without sky) and totals (K, 2, 66), int64 and normalised, nonfinite (K: powers that were NaN or
        infinite and were not added) and misplaced (1), float64, with kind. acc: such a dict of an earlier chunk,
        ACCUMULATED into and returned. mode: "auto", "lds" (totals and flux block-private in LDS; nbins <= 56) or
        "global" (every add to HBM); the limbs do not depend on it. exact_finish gives the rounded tables."""
        nbins = int(nbins)
        if kind not in _lib.REPLICATE_KINDS:
            raise ValueError(f"event_exact: kind must be one of {sorted(_lib.REPLICATE_KINDS)}, not {kind!r}")
        if mode not in _lib.EXACT_MODES:
            raise ValueError(f"event_exact: mode must be one of {sorted(_lib.EXACT_MODES)}, not {mode!r}")
        if (kind == "coupling" and node_factor is None) or (kind != "run" and event_factor is None):
            raise ValueError(f"event_exact: kind {kind!r} needs its factor arrays")
        K = 1 if kind == "run" else int(event_factor.shape[0])
        spec, shape, _ = self._sky_spec(sky)
        if acc is None:
            acc = self._zero_exact(kind, K, nbins, shape)
        if (acc["kind"] != kind or tuple(acc["flux"].shape) != (K, 2 * nbins, _lib.EXACT_LIMBS) or
                (None if acc["sky"] is None else tuple(acc["sky"].shape[1:-1])) != shape):
            raise ValueError("event_exact: `acc` was made for another kind, other sets or other tables")
        n, nn = sample["erg"].numel(), int(forward["n_nodes"])
        if kind != "run" and (tuple(event_factor.shape) != (K, n) or not event_factor.is_contiguous()):
            raise ValueError("event_exact: event_factor must be a contiguous (K, n_events) tensor")
        if kind == "coupling" and (tuple(node_factor.shape) != (K, nn) or (nn > 0 and not node_factor.is_contiguous())):
            raise ValueError("event_exact: node_factor must be a contiguous (K, n_nodes) tensor")
        ei = self._event_rows_in(sample, weight5, back, forward, event_offset, cyclotron_rerun)
        eo = _lib.EventExactOut(_lib.REPLICATE_KINDS[kind], K, nbins, _lib.EXACT_MODES[mode],
                                _p(node_factor) if kind == "coupling" else None, _p(event_factor) if kind != "run" else None,
                                _p(acc["flux"]), C.pointer(spec) if spec is not None else None,
                                _p(acc["sky"]) if shape else None, _p(acc["totals"]), _p(acc["nonfinite"]),
                                _p(acc["misplaced"]))
        check(self.lib.art_event_exact_device(C.byref(self.cp), C.byref(ei), _p(forward["node_start"]), C.byref(eo),
                                              _stream()))
        return acc

    def exact_finish(self, acc, f_inx=None) -> dict:
        """The rounded tables of event_exact's accumulators, on the device (art_exact_finish_device): flux_raw
        (K, 2, nbins), sky_raw (K, the map's shape; with a map) and totals_raw (K, 2), each entry the correctly rounded
        exact sum of its rows' powers, with nonfinite (K) and acc (the accumulators, for trees.exact_merge); kind
        "run": without the leading axis. f_inx: also flux, sky_map and sum_weight_sln_prob, the raw tables divided by
        it (by 1 when it is 0) with the one IEEE division the float tables get."""
        K = acc["flux"].shape[0]
        out = {"flux_raw": self.exact_round(acc["flux"]).view(K, 2, -1), "totals_raw": self.exact_round(acc["totals"])}
        if acc["sky"] is not None:
            out["sky_raw"] = self.exact_round(acc["sky"])
        if acc.get("origin") is not None:  # (the emission map's, with run_events(origin_map=, exact=True))
            out["origin_raw"] = self.exact_round(acc["origin"])
        out["nonfinite"] = acc["nonfinite"]
        if acc["kind"] == "run":
            out = {k: v[0] for k, v in out.items()}
        if f_inx is not None:
            # (a device tensor: torch turns a division by a host scalar into a multiplication by its reciprocal)
            div = torch.full((), float(f_inx) if f_inx > 0 else 1.0, dtype=F64, device=self.device)
            out.update(flux=out["flux_raw"] / div, sum_weight_sln_prob=out["totals_raw"] / div)
            if "sky_raw" in out:
                out["sky_map"] = out["sky_raw"] / div
            if "origin_raw" in out:
                out["origin_map"] = out["origin_raw"] / div
        out["acc"] = acc
        return out

    # The most bytes an emission map may take, the R copies of its replicates included
    ORIGIN_MAX_BYTES = 1 << 30

    @classmethod
    def _origin_fit(cls, spec, R, exact):
        """ValueError when an emission map (with R group copies; R None: none) exceeds ORIGIN_MAX_BYTES, or its exact
        accumulators EXACT_MAX_BYTES or art_exact_histogram_device's 2^24 bins"""
        bins = 1
        for d in spec["shape"]:
            bins *= d
        size = 8 * bins * max(int(R or 1), 1)
        if size > cls.ORIGIN_MAX_BYTES:
            raise ValueError(f"origin_map: the table{' of ' + str(R) + ' groups' if R else ''} would take {size} bytes, more "
                             f"than {cls.ORIGIN_MAX_BYTES}: coarsen it or lower R")
        if exact and (bins > 1 << 24 or 8 * _lib.EXACT_LIMBS * bins > cls.EXACT_MAX_BYTES):
            raise ValueError(f"origin_map: the exact accumulators of {bins} bins ({_lib.EXACT_LIMBS} limbs each) exceed 2^24 "
                             f"bins or {cls.EXACT_MAX_BYTES} bytes: coarsen the map")

    def event_origin(self, sample, weight5, back, forward, origin, *, observer=None, groups=None, event_offset=0, hist=None,
                     cyclotron_rerun=None, return_bins=False) -> dict:
        """The emission map of one chunk (art_event_origin_device; DESIGN.md §3, "Emission maps"), on the current
        stream and without a synchronisation: the arguments of event_rows for the same chunk, whose powers (column
        8 * column 7) it bins per species over WHERE the row's event converted -- (r, cos θ or θ, φ) of the sampled
        point, columns 9 to 11, in the magnetic or the rotation frame -- and, with observer, jointly over the row's
        direction (θf or cos θf, φf), the sky map's bins. origin: a dict of n_r, n_theta, n_phi, theta_axis, r_range,
        frame and mode ({}: 1 x 16 x 32, "cos", "magnetic"), or trees.origin_spec's dict; observer: None or a dict of
        n_theta, n_phi, theta_axis. groups (R, 2 to 64): the table gets a leading group axis and a row goes to group
        (event_offset + tree) mod R. Returns a dict: hist (the spec's shape (2, obs_theta, obs_phi, n_r, n_theta,
        n_phi), or (R, ...)), misplaced (1; must stay 0), spec, groups, and with return_bins bins (n_nodes int32: per
        node record the flat bin without the group, -1 where not counted) and power (n_nodes: the power, 0 where not
        final). hist: such a dict of an earlier chunk, ACCUMULATED into and returned (made for other axes or groups:
        ValueError). cyclotron_rerun: event_rows' "cyclotron_rerun" of this chunk, so exp(-τ) is in the powers."""
        from .trees import origin_spec
        spec = origin_spec(origin, observer, self.params)
        R = None if groups is None else self._replicates_groups(groups)
        shape = spec["shape"] if R is None else (R,) + tuple(spec["shape"])
        self._origin_fit(spec, R, False)
        if hist is None:
            hist = {"hist": torch.zeros(*shape, dtype=F64, device=self.device),
                    "misplaced": torch.zeros(1, dtype=F64, device=self.device), "groups": R}
        keys = ("n_r", "n_theta", "n_phi", "theta_axis", "r_range", "cm", "sm", "observer")
        if (tuple(hist["hist"].shape) != tuple(shape) or hist.get("groups") != R or
                ("spec" in hist and any(hist["spec"][k] != spec[k] for k in keys))):
            raise ValueError("event_origin: `hist` was made for other axes or other groups")
        hist["spec"] = spec
        nn = int(forward["n_nodes"])
        bins = self.empty(max(nn, 1), dtype=torch.int32) if return_bins else None
        power = self.empty(max(nn, 1)) if return_bins else None
        lo, hi = spec["r_range"] or (0.0, 0.0)
        og = _lib.OriginSpec(spec["n_r"], spec["n_theta"], spec["n_phi"], _lib.THETA_AXIS[spec["theta_axis"]], spec["mode"],
                             lo, hi, spec["cm"], spec["sm"])
        obs = spec["observer"]
        sk = None if obs is None else _lib.SkySpec(obs["n_theta"], obs["n_phi"], 1, _lib.THETA_AXIS[obs["theta_axis"]], 0,
                                                   0.0, 0.0)
        ei = self._event_rows_in(sample, weight5, back, forward, event_offset, cyclotron_rerun)
        oo = _lib.EventOriginOut(C.pointer(og), C.pointer(sk) if sk is not None else None, R or 0, _p(hist["hist"]),
                                 _p(bins), _p(power), _p(hist["misplaced"]))
        check(self.lib.art_event_origin_device(C.byref(self.cp), C.byref(ei), _p(forward["node_start"]), C.byref(oo),
                                               _stream()))
        if return_bins:
            hist.update(bins=bins[:nn], power=power[:nn])
        return hist

    # The most bytes the spectrum tables of one set of tables (the run's, a coupling scan's or a halo scan's) may take
    SPECTRUM_MAX_BYTES = 64 << 20

    @classmethod
    def _spectrum_fit(cls, what, K, sub_bits):
        """ValueError when the spectrum tables of K sets exceed SPECTRUM_MAX_BYTES"""
        size = 8 * K * 2 * 3 * (2047 << sub_bits)
        if size > cls.SPECTRUM_MAX_BYTES:
            raise ValueError(f"spectrum: the tables of {what} ({K} sets, sub_bits {sub_bits}) would take {size} bytes, "
                             f"more than {cls.SPECTRUM_MAX_BYTES}: lower sub_bits or the number of sets")

    def _zero_spectrum(self, kind, K, sub_bits, top):
        z = lambda *d: torch.zeros(*d, dtype=F64, device=self.device)  # noqa: E731
        NB = 2047 << sub_bits
        return {"kind": kind, "sub_bits": sub_bits, "top": top, "count": z(K, 2, NB), "sum": z(K, 2, NB), "sum_sq": z(K, 2, NB),
                "totals": z(K, 2, len(_lib.SPECTRUM_TOTALS)), "top_power": z(K, 2, top),
                "top_event": torch.full((K, 2, top), -1, dtype=torch.int64, device=self.device)}

    def event_spectrum(self, sample, weight5, back, forward, *, sub_bits=3, top=64, kind="run", node_factor=None,
                       event_factor=None, event_offset=0, cyclotron_rerun=None, spec=None) -> dict:
        """The event power spectrum of one chunk (art_event_spectrum_device; DESIGN.md §3, "Event power spectrum"), on
        the current stream and without a synchronisation: the arguments of event_rows for the same chunk, of whose
        per-event power X_{e,s} (the moments' X: the powers of e's final rows of species s, summed in node order) it
        keeps the distribution. The sets and their powers by kind are event_replicates': "run", one set; "coupling"
        from node_factor = event_reweight(return_weights=True)'s "weights" and event_factor = its "back"; "halo" from
        event_factor = event_halo_scan(return_ratio=True)'s "ratio". Returns a dict of device tensors: count, sum and
        sum_sq (K, 2, 2047 << sub_bits: the events, Σ X and Σ X² per bin, bin = bits(X) >> (52 - sub_bits), float64),
        totals (K, 2, 8: _lib.SPECTRUM_TOTALS), top_power (K, 2, top) and top_event (K, 2, top; int64, the global
        ids event_offset + tree), the `top` events with the largest X by (X descending, id ascending), padded with
        (0.0, -1), with kind, sub_bits and top. spec: such a dict of an earlier chunk, ACCUMULATED into -- its lists
        are candidates of this call -- and returned. cyclotron_rerun: event_rows' "cyclotron_rerun" of this chunk, so
        exp(-τ) is in the powers. trees.spectrum_result turns the tables into n_eff, shares and the tail index."""
        from .trees import _spectrum_check
        m, T = _spectrum_check(sub_bits, top)
        if kind not in _lib.REPLICATE_KINDS:
            raise ValueError(f"event_spectrum: kind must be one of {sorted(_lib.REPLICATE_KINDS)}, not {kind!r}")
        if (kind == "coupling" and node_factor is None) or (kind != "run" and event_factor is None):
            raise ValueError(f"event_spectrum: kind {kind!r} needs its factor arrays")
        if kind != "run" and not (torch.is_tensor(event_factor) and event_factor.dim() == 2):
            raise ValueError("event_spectrum: event_factor must be a contiguous float64 (K, n_events) tensor on the "
                             "engine's device")
        K = 1 if kind == "run" else int(event_factor.shape[0])
        if spec is None:
            spec = self._zero_spectrum(kind, K, m, T)
        if (spec["kind"] != kind or spec["sub_bits"] != m or spec["top"] != T or
                tuple(spec["count"].shape) != (K, 2, 2047 << m)):
            raise ValueError("event_spectrum: `spec` was made for another kind, other bins, another list or other sets")
        n, nn = sample["erg"].numel(), int(forward["n_nodes"])
        here = lambda t: torch.is_tensor(t) and t.dtype == F64 and t.device == self.device  # noqa: E731
        if kind != "run" and (not here(event_factor) or tuple(event_factor.shape) != (K, n) or
                              not event_factor.is_contiguous()):
            raise ValueError("event_spectrum: event_factor must be a contiguous float64 (K, n_events) tensor on the "
                             "engine's device")
        if kind == "coupling" and (not here(node_factor) or tuple(node_factor.shape) != (K, nn) or
                                   (nn > 0 and not node_factor.is_contiguous())):
            raise ValueError("event_spectrum: node_factor must be a contiguous float64 (K, n_nodes) tensor on the "
                             "engine's device")
        ei = self._event_rows_in(sample, weight5, back, forward, event_offset, cyclotron_rerun)
        so = _lib.EventSpectrumOut(_lib.REPLICATE_KINDS[kind], K, m, T, _p(node_factor) if kind == "coupling" else None,
                                   _p(event_factor) if kind != "run" else None, _p(spec["count"]), _p(spec["sum"]),
                                   _p(spec["sum_sq"]), _p(spec["totals"]), _p(spec["top_power"]) if T else None,
                                   _p(spec["top_event"]) if T else None)
        check(self.lib.art_event_spectrum_device(C.byref(self.cp), C.byref(ei), _p(forward["node_start"]), C.byref(so),
                                                 _stream()))
        return spec

    @classmethod
    def _grid_fit(cls, Kg, Kh, R, nbins, errors):
        """ValueError when the grid's tables -- (1 + R) copies under replicates=R, plus the moment totals -- exceed
        REPLICATES_MAX_BYTES"""
        C_ = Kg * Kh
        size = 8 * (C_ * ((2 * nbins + len(_lib.GRID_TOTALS)) + (R or 0) * (2 * nbins + 2)
                          + (len(_lib.MOMENT_TOTALS) if errors else 0)) + (R or 0) * len(_lib.REPLICATE_GROUPS))
        if size > cls.REPLICATES_MAX_BYTES:
            raise ValueError(f"grid: the tables of {Kg} x {Kh} cells{f' and {R} groups' if R else ''} would take {size} "
                             f"bytes, more than {cls.REPLICATES_MAX_BYTES}: lower nbins, R or the number of cells")

    def _zero_grid(self, g, models, base, R, nbins, errors):
        """The zero tables of a grid, cell-minor as art_event_grid_out takes them (C = K_g K_h cells last)"""
        z = lambda *d: torch.zeros(*d, dtype=F64, device=self.device)  # noqa: E731
        C_ = len(g) * len(models)
        grid = {"g": list(g), "models": list(models), "base": base, "R": R, "flux": z(2 * nbins, C_),
                "totals": z(len(_lib.GRID_TOTALS), C_), "n_events": 0}
        if R is not None:
            grid.update(flux_rep=z(R, 2 * nbins, C_), totals_rep=z(R, 2, C_), groups=z(R, len(_lib.REPLICATE_GROUPS)))
        if errors:
            grid["moment_totals"] = z(len(_lib.MOMENT_TOTALS), C_)
        return grid

    def event_grid(self, sample, weight5, back, forward, *, weights, back_factor, ratio, g, models, base, event_offset=0,
                   nbins=50, replicates=None, errors=False, cyclotron_rerun=None, grid=None) -> dict:
        """The coupling x halo grid of one chunk (art_event_grid_device; DESIGN.md §3, "Coupling x halo grid"), on the
        current stream and without a synchronisation: the arguments of event_rows for the same chunk and the factors
        the two scans hand out for it -- weights (K_g, n_nodes) and back_factor (K_g, n_events), event_reweight(
        return_weights=True)'s "weights" and "back", and ratio (K_h, n_events), event_halo_scan(return_ratio=True)'s
        "ratio" -- with what they were made for: g (the K_g couplings), models (the K_h halo models) and base (the
        raytracer.Halo of the run). At cell (kg, kh) the power of a final row is the coupling scan's at g[kg] times
        ratio[kh] of its event, in the run's own flux bins. Returns a dict of device tensors, float64, CELL-MINOR as
        the kernel adds to them (C = K_g K_h, cell = kg K_h + kh last): flux (2 nbins, C), totals (3, C: Σ power of
        axions and of photons, misplaced records -- _lib.GRID_TOTALS), with replicates=R flux_rep (R, 2 nbins, C),
        totals_rep (R, 2, C) and groups (R, 3, event_replicates'), with errors moment_totals (8, C,
        _lib.MOMENT_TOTALS per cell), and g, models, base, R, n_events. trees.grid_raw brings them to the host with
        (K_g, K_h) leading. grid: such a dict of an earlier chunk, ACCUMULATED into and returned. cyclotron_rerun:
        event_rows' "cyclotron_rerun" of this chunk, so exp(-τ) is in the powers."""
        from .trees import halo_scan_models
        g = self._couplings(g)
        models = halo_scan_models(base, models)
        R = None if replicates is None else self._replicates_groups(replicates)
        Kg, Kh, nbins = len(g), len(models), int(nbins)
        n, nn = sample["erg"].numel(), int(forward["n_nodes"])
        for name, t, shape in (("weights", weights, (Kg, nn)), ("back_factor", back_factor, (Kg, n)), ("ratio", ratio, (Kh, n))):
            if (not torch.is_tensor(t) or t.dtype != F64 or tuple(t.shape) != shape or
                    (t.numel() > 0 and not t.is_contiguous())):
                raise ValueError(f"event_grid: {name} must be a contiguous float64 tensor of shape {shape}")
        key = self._halo_key(base)
        if grid is None:
            grid = self._zero_grid(g, models, key, R, nbins, errors)
        if (grid["g"] != g or grid["models"] != models or grid["base"] != key or grid["R"] != R or
                tuple(grid["flux"].shape) != (2 * nbins, Kg * Kh) or errors != ("moment_totals" in grid)):
            raise ValueError("event_grid: `grid` was made for other couplings, models, groups or tables")
        ei = self._event_rows_in(sample, weight5, back, forward, event_offset, cyclotron_rerun)
        go = _lib.EventGridOut(Kg, Kh, nbins, R or 0, _p(weights), _p(back_factor), _p(ratio), _p(grid["flux"]),
                               _p(grid["totals"]), _p(grid.get("flux_rep")), _p(grid.get("totals_rep")),
                               _p(grid.get("groups")), _p(grid.get("moment_totals")))
        check(self.lib.art_event_grid_device(C.byref(self.cp), C.byref(ei), _p(forward["node_start"]), C.byref(go),
                                             _stream()))
        grid["n_events"] += n
        return grid

    def _cyclotron_rerun(self, sample, forward, nn, n):
        """The final photon segments of a forward forest, packed (art_event_gather_photons_device) and run
        again with the cyclotron observation: slot per node, the batch size m, its tau and end states."""
        cap = max(nn, 1)
        b = {"x0": self.empty(3 * cap), "k0": self.empty(3 * cap), "erg": self.empty(cap), "dw": self.empty(cap),
             "ln_t0": self.empty(cap), "species": self.empty(cap, dtype=torch.int8)}
        slot = self.empty(cap, dtype=torch.int32)
        m = C.c_int64(0)
        check(self.lib.art_event_gather_photons_device(C.byref(self.cp), n, _p(sample["erg"]), nn, _p(forward["nodes"]), cap,
                                                       *[_p(b[k]) for k in ("x0", "k0", "erg", "dw", "ln_t0", "species")],
                                                       _p(slot), C.byref(m), _stream()))
        m = int(m.value)
        if m == 0:
            z = self.empty(1)
            return {"slot": slot, "m": 0, "tau": z, "end": _lib.SegmentOut(), "out": None}
        inp = {k: (v[:3 * m] if k in ("x0", "k0") else v[:m]) for k, v in b.items()}
        out = self.propagate(inp, max_crossings=-1, capacity=1, cyclotron=True)
        end = _lib.SegmentOut(*[out[k].data_ptr() for k in ("x_end", "k_end", "u7_end", "tau_end", "status", "n_accept",
                                                           "n_reject")])
        return {"slot": slot, "m": m, "tau": out["cyc_tau"], "end": end, "out": out, "inp": inp}

    def run_events(self, n_events, *, seed=1769, event_offset=0, chunk=None, saveMode=0, num_cutoff=5, MC_nodes=5,
                   max_nodes=50, prob_cutoff=1e-10, backtrace_cap=256, rho_DM=0.45, n_maxSample=6, nbins=50, sky_map=None,
                   cyclotron=False, rows=True, halo=None, errors=False, couplings=None, halos=None, replicates=None,
                   grid=False, spectrum=None, exact=False, origin_map=None) -> dict:
        """One main_runner_tree run of n_events events (global ids event_offset .. event_offset +
        n_events) with everything in HBM: per chunk of events [lo, hi) the sampler (ray_offset = lo), the
        event weights, the backtrace forest (-k, -B0, axion, num_cutoff = 0, splittings_cutoff = 100000,
        tree_offset = lo), the forward forest (tree_offset = lo) and event_rows (event_offset = lo); flux,
        sky map and totals accumulate on the device and the rows are collected there. The sampler and the
        Monte-Carlo draws are keyed by global ids, so the chunking does not change the rows (the weighted
        tables differ by the order of their adds only; exact=True adds tables that do not). It blocks,
        because grow_trees does.

        chunk: events per chunk (None: one chunk). A chunk of c events holds at most c (max_nodes + 2)
        node records of 264 B for the forward forest (3.4 MB per 250 events at the defaults, 1.8 GB per
        2^17; about 3.5 records per event are used on the flat configuration), the same again while the
        driver's node log is flattened, c records for the backtrace forest with 9 backtrace_cap c doubles
        of crossing slots, and, with rows, ncols doubles per record for the chunk's rows before they are
        cut to the final nodes.

        sky_map: a dict of n_theta, n_phi, n_dw, theta_axis, dw_range, mode ({}: the defaults), or None.
        n_dw > 1 needs a dw_range: ValueError without one. rows=False: no rows, the large-run mode.

        halo (a raytracer.Halo): the sampler draws each event's speed at infinity from the halo model and
        the weights carry its importance ratio; column 12 is u7_end/m_a + |vifty|²/2 of each event
        ("Halo velocity model"). None (the default): the reference's single speed, every
        row as before.

        errors: also the Monte-Carlo standard errors (event_moments per chunk; DESIGN.md §3, "Monte-Carlo
        errors"): flux_sigma (2, nbins), sky_map_sigma (the map's shape, with a sky map) and
        sum_weight_sln_prob_sigma (2), in the units of flux, sky_map and sum_weight_sln_prob, and moments,
        the raw tables and totals for a caller that reduces over ranks first (trees.moments_sigma). The
        events are the independent unit, so this works with rows=False. NaN below two events or with
        f_inx = 0. The bins of one event are correlated: the σ of a sum of bins is NOT the quadrature sum of
        these. False (the default): exactly the keys below.

        couplings (a list of 1 to 32 values of g_agg; DESIGN.md §3, "Coupling scan"): the run's forests, grown
        at params.g_agg, are also reweighted to every coupling of the list (event_reweight per chunk), and
        the result gets "coupling_scan", trees.scan_result's dict of host arrays: g, scale, flux (K, 2, nbins)
        and sky_map (K, the map's shape), both divided by f_inx, sum_weight_sln_prob (K, 2), coverage (K, the
        mean over the events), saturated, unlinked, recomputed_differs, raw (the undivided tables, for a
        caller that reduces over ranks first) and, with errors, flux_sigma, sky_map_sigma and
        sum_weight_sln_prob_sigma per coupling. A record without exactly one parent (unlinked != 0) is an
        ArtError. None (the default): exactly the keys below.

        halos (a list of 1 to 32 raytracer.Halo; needs halo=, the base; DESIGN.md §3, "Halo scan"): the run, sampled
        and weighted under `halo`, is also reweighted to every model of the list (event_halo_scan per chunk: one
        ratio R = F_model / F_halo per event), and the result gets "halo_scan", trees.halo_scan_result's dict of
        host arrays: models, flux (K, 2, nbins) and sky_map (K, the map's shape), both divided by f_inx,
        sum_weight_sln_prob (K, 2), ratio_sum and ratio_sq (K), misplaced, raw (the undivided tables) and, with
        errors, flux_sigma, sky_map_sigma, sum_weight_sln_prob_sigma and n_eff (K) per model. A model's v0 may
        not exceed halo.vp(): choose the base as the widest model, with a v_prop that covers the targets.
        couplings= in the same run scans the couplings at the base halo and the halos at the base coupling.
        None (the default): exactly the keys below.

        replicates (a group count R, 2 to 64; DESIGN.md §3, "Jackknife replicates"): the run's first-moment tables are
        also kept per group of events, g = global event id mod R (event_replicates per chunk), and the result gets
        "replicates", trees.replicates_result's dict of host arrays, from which trees.jackknife gives the value, σ and
        covariance of ANY function of the tables -- a pulse profile summed over Δω, a band power, a ratio. With
        couplings= or halos= the scan's dict gets "replicates" too, with the scan's leading axis (the scans are then
        called with return_weights / return_ratio), so correlated read-offs such as trees.coupling_crossing have an
        error. It needs neither rows nor errors=True. Replicate tables of more than Engine.REPLICATES_MAX_BYTES (1 GiB)
        per set of tables are a ValueError before any work is done. None (the default): exactly the keys below.

        grid (needs couplings=, halos= and halo=; DESIGN.md §3, "Coupling x halo grid"): the two scans are each made at
        the other's base value; with grid=True the run's flux and totals are also formed at every (coupling, halo
        model) cell (event_grid per chunk, from the factors the two scans hand out: nothing is integrated or grown
        again), and the result gets "grid", trees.grid_result's dict of host arrays: g (K_g), models (K_h), base, flux
        (K_g, K_h, 2, nbins) and sum_weight_sln_prob (K_g, K_h, 2), both divided by f_inx, misplaced, raw; with errors
        sum_weight_sln_prob_sigma (K_g, K_h, 2) and n_eff (K_g, K_h); with replicates "replicates", the per-group
        tables from which trees.limit_band reads the limit on g under every halo model, the band between the models
        and their errors. There is no sky map in the grid. Its tables -- (1 + R) copies under replicates=R plus the
        moment totals -- may take at most Engine.REPLICATES_MAX_BYTES: beyond that, or without one of the three
        keywords, a ValueError before any work is done. A misplaced record is an ArtError. False (the default):
        exactly the keys below.

        spectrum ({} or a dict of sub_bits, 0 to 4, default 3, and top, 0 to 256, default 64; DESIGN.md §3, "Event
        power spectrum"): the distribution of the per-event power (event_spectrum per chunk), and the result gets
        "spectrum", trees.spectrum_result's dict of host arrays: the histogram over range-free bins (edges, counts,
        power), events, positive, zeros, bad, n_eff = S² / Q, top_event (global ids: run_events(1, event_offset=id)
        replays one), top_power, top_share, max_share, and the Hill tail index alpha ± alpha_sigma with the Hill plot
        hill. alpha <= 2: the variance does not exist and no σ of this run means what it says; alpha <= 1: nor does
        the mean converge; otherwise read n_eff and top_share. With couplings= or halos= the scan's dict gets
        "spectrum" too, with the scan's leading axis (the scans are then called with return_weights / return_ratio);
        the grid gets none. It needs neither rows, errors nor replicates. Unknown keys, values out of range and tables
        of more than Engine.SPECTRUM_MAX_BYTES (64 MiB) per set of tables are a ValueError before any work is done.
        None (the default): exactly the keys below.

        exact ("Exact tables"): beside the float tables, whose last bits depend on the order of their
        adds, the same tables as the correctly rounded EXACT sums of the same row powers (event_exact per chunk, into
        fixed-point accumulators of 66 int64 limbs per bin), which are identical across runs, chunk sizes,
        event_offset splits and rank counts. The result gets "exact", exact_finish's dict of device tensors: flux
        (2, nbins), sky_map and sum_weight_sln_prob (2), divided by f_inx with the one IEEE division the float tables
        get, the undivided flux_raw, sky_raw and totals_raw, nonfinite (powers that were NaN or infinite: not added)
        and acc, the normalised accumulators, which trees.exact_merge adds over runs. With couplings= or halos= the
        scan's dict gets "exact" too, with the scan's leading axis (the scans are then called with return_weights /
        return_ratio). Not covered: the grid, the second moments and σ, the replicate tables and the spectrum, which
        are what they are without it. Accumulators of more than Engine.EXACT_MAX_BYTES (1 GiB) per set of tables are
        a ValueError before any work is done. False (the default): exactly the keys below.

        origin_map ("Emission maps"; {} or a dict of event_origin's origin keys n_r, n_theta, n_phi,
        theta_axis, r_range, frame, mode, plus an optional observer=dict(n_theta, n_phi, theta_axis)): the power per
        species binned over WHERE its event converted -- the sampled point of columns 9 to 11 in the magnetic or the
        rotation frame -- and with observer jointly over the direction it left in (event_origin per chunk; it needs no
        rows and takes the cyclotron re-run's τ as the other tables do). The result gets "origin", a dict of host
        arrays: map (2, obs_theta, obs_phi, n_r, n_theta, n_phi), divided by f_inx, with size-1 observer axes kept;
        raw, the undivided table; edges (trees.origin_map_edges); spec; misplaced. With replicates=R also
        "replicates": raw (R, ...), the per-group tables of a second launch, with the run's own n_g, a_g, R and f_inx
        (the same events, the same groups), for trees.origin_jackknife. With exact=True "exact" gets origin_map,
        origin_raw and acc["origin"], from the labels and powers the origin kernel hands out through
        exact_histogram. trees.emission_profile and trees.observer_view read the map. The scans (couplings=, halos=),
        grid=, errors=True and spectrum= get NO origin table: the jackknife is its error path. Tables of more than
        Engine.ORIGIN_MAX_BYTES (1 GiB, the R copies included), or exact accumulators of more than EXACT_MAX_BYTES
        or 2^24 bins, are a ValueError before any work is done. None (the default): exactly the keys below.

        Returns a dict of device tensors and numbers: rows ((n_rows, ncols) with column 7 divided by f_inx,
        or None), flux ((2, nbins), divided by f_inx), sky_map and sky_map_edges (numpy) when asked for,
        f_inx, sum_weight_sln_prob, n_rows, n_photon_rows, and the raw, undivided parts for a caller that
        reduces over ranks first: totals (6: rows, photon rows, Σ weight sln_prob of axions and photons,
        Σ (attempts - 1), cyclotron mismatches), flux_raw, sky_raw, rows_raw (column 7 undivided; the
        tensor `rows` is a divided copy of)."""
        from dataclasses import replace
        from .trees import AXION, PHOTON, halo_scan_models, sky_map_edges
        if grid and (couplings is None or halos is None or halo is None):  # (before any work is done)
            raise ValueError("grid: the coupling x halo grid needs couplings=, halos= and halo= (the base)")
        if replicates is not None:
            replicates = Engine._replicates_groups(replicates)  # (before any work is done)
        if spectrum is not None:
            from .trees import spectrum_keywords
            spectrum = spectrum_keywords(spectrum)  # (before any work is done)
        if halos is not None:
            halos = halo_scan_models(halo, halos)  # (before any work is done)
        ospec = None
        if origin_map is not None:  # (before any work is done)
            from .trees import origin_spec
            ospec = origin_spec({k: v for k, v in origin_map.items() if k != "observer"}, origin_map.get("observer"),
                                self.params)
            self._origin_fit(ospec, replicates, exact)
        n_events = int(n_events)
        if n_events < 0:
            raise ValueError("run_events: n_events must be >= 0")
        if couplings is not None:
            couplings = self._couplings(couplings)  # (before any work is done)
        chunk = max(1, n_events) if chunk is None else int(chunk)
        if chunk < 1:
            raise ValueError("run_events: chunk must be >= 1")
        ncols = 29 if saveMode > 0 else 13
        _, shape, sky_kw = self._sky_spec(sky_map)
        if grid:  # (before any work is done)
            self._grid_fit(len(couplings), len(halos), replicates, int(nbins), errors)
        if replicates is not None:  # (before any work is done)
            for what, K in (("the run", 1), ("the coupling scan", couplings and len(couplings)),
                            ("the halo scan", halos and len(halos))):
                if K:
                    self._replicates_fit(what, K, replicates, int(nbins), shape)
        if exact:  # (before any work is done)
            for what, K in (("the run", 1), ("the coupling scan", couplings and len(couplings)),
                            ("the halo scan", halos and len(halos))):
                if K:
                    self._exact_fit(what, K, int(nbins), shape)
        if spectrum is not None:  # (before any work is done)
            for what, K in (("the run", 1), ("the coupling scan", couplings and len(couplings)),
                            ("the halo scan", halos and len(halos))):
                if K:
                    self._spectrum_fit(what, K, spectrum[0])
        sky_hist = torch.zeros(*shape, dtype=F64, device=self.device) if shape else None
        max_r = self.params.max_r()
        if max_r < self.params.rNS:
            raise ValueError("maxR < rNS: this neutron star has no conversion surface (MainRunner.jl:387-396)")
        back_eng = Engine(replace(self.params, B0=-self.params.B0), device=self.device.index)
        flux = torch.zeros(2 * int(nbins), dtype=F64, device=self.device)
        totals = torch.zeros(len(_lib.EVENT_TOTALS), dtype=F64, device=self.device)
        parts = []
        moments = scan = hscan = rep = crep = hrep = cells = spec = cspec = hspec = xacc = cxacc = hxacc = None
        omap = orep = oacc = None
        want = replicates is not None
        factors = want or bool(grid) or spectrum is not None or bool(exact)  # the scans hand out their factors
        for lo in range(int(event_offset), int(event_offset) + n_events, chunk):
            c = min(chunk, int(event_offset) + n_events - lo)
            s = self.sample(c, seed=seed, ray_offset=lo, max_r=max_r, halo=halo)
            w5 = self.event_weight(s, max_r=max_r, rho_DM=rho_DM, n_maxSample=n_maxSample, halo=halo)
            back = back_eng.grow_trees(s["x"], -s["k_init"], s["erg"], AXION, num_cutoff=0, splittings_cutoff=100000,
                                       crossing_cap=backtrace_cap, prob_cutoff=prob_cutoff, seed=seed, tree_offset=lo)
            fwd = self.grow_trees(s["x"], s["k_init"], s["erg"], PHOTON, num_cutoff=num_cutoff, mc_nodes=MC_nodes,
                                  max_nodes=max_nodes, prob_cutoff=prob_cutoff, seed=seed, tree_offset=lo)
            r = self.event_rows(s, w5, back, fwd, event_offset=lo, saveMode=saveMode, nbins=nbins, flux=flux,
                                sky=sky_map, sky_hist=sky_hist, totals=totals, rows=rows, cyclotron=cyclotron)
            if errors:
                moments = self.event_moments(s, w5, back, fwd, event_offset=lo, nbins=nbins, sky=sky_map, moments=moments,
                                             cyclotron_rerun=r["cyclotron_rerun"])
            if couplings is not None:
                scan = self.event_reweight(s, w5, back, fwd, couplings, mc_nodes=MC_nodes, event_offset=lo, nbins=nbins,
                                           sky=sky_map, errors=errors, cyclotron_rerun=r["cyclotron_rerun"], scan=scan,
                                           **({"return_weights": True} if factors else {}))
            if halos is not None:
                hscan = self.event_halo_scan(s, w5, back, fwd, halo, halos, event_offset=lo, nbins=nbins, sky=sky_map,
                                             errors=errors, cyclotron_rerun=r["cyclotron_rerun"], scan=hscan,
                                             **({"return_ratio": True} if factors else {}))
            if grid:
                cells = self.event_grid(s, w5, back, fwd, weights=scan["weights"], back_factor=scan["back"],
                                        ratio=hscan["ratio"], g=couplings, models=halos, base=halo, event_offset=lo,
                                        nbins=nbins, replicates=replicates, errors=errors,
                                        cyclotron_rerun=r["cyclotron_rerun"], grid=cells)
            if want:
                kw = dict(event_offset=lo, nbins=nbins, sky=sky_map, cyclotron_rerun=r["cyclotron_rerun"])
                rep = self.event_replicates(s, w5, back, fwd, replicates, rep=rep, **kw)
                if couplings is not None:
                    crep = self.event_replicates(s, w5, back, fwd, replicates, rep=crep, kind="coupling",
                                                 node_factor=scan["weights"], event_factor=scan["back"], **kw)
                if halos is not None:
                    hrep = self.event_replicates(s, w5, back, fwd, replicates, rep=hrep, kind="halo",
                                                 event_factor=hscan["ratio"], **kw)
            if spectrum is not None:
                kw = dict(sub_bits=spectrum[0], top=spectrum[1], event_offset=lo, cyclotron_rerun=r["cyclotron_rerun"])
                spec = self.event_spectrum(s, w5, back, fwd, spec=spec, **kw)
                if couplings is not None:
                    cspec = self.event_spectrum(s, w5, back, fwd, spec=cspec, kind="coupling", node_factor=scan["weights"],
                                                event_factor=scan["back"], **kw)
                if halos is not None:
                    hspec = self.event_spectrum(s, w5, back, fwd, spec=hspec, kind="halo", event_factor=hscan["ratio"], **kw)
            if exact:
                kw = dict(event_offset=lo, nbins=nbins, sky=sky_map, cyclotron_rerun=r["cyclotron_rerun"])
                xacc = self.event_exact(s, w5, back, fwd, acc=xacc, **kw)
                if couplings is not None:
                    cxacc = self.event_exact(s, w5, back, fwd, acc=cxacc, kind="coupling", node_factor=scan["weights"],
                                             event_factor=scan["back"], **kw)
                if halos is not None:
                    hxacc = self.event_exact(s, w5, back, fwd, acc=hxacc, kind="halo", event_factor=hscan["ratio"], **kw)
            if ospec is not None:
                kw = dict(event_offset=lo, cyclotron_rerun=r["cyclotron_rerun"])
                omap = self.event_origin(s, w5, back, fwd, ospec, hist=omap, return_bins=bool(exact), **kw)
                if want:
                    orep = self.event_origin(s, w5, back, fwd, ospec, groups=replicates, hist=orep, **kw)
                if exact:  # (the labels and powers the kernel handed out: no exact kernel of its own)
                    # (its non-finite count is not kept: the run's own exact tables count the same powers in nonfinite)
                    oacc, _ = self.exact_histogram(omap.pop("bins"), omap.pop("power"), omap["hist"].numel(), acc=oacc)
            if factors:  # (this chunk's factors are not part of the scans' tables)
                for d, keys in ((scan, ("weights", "back", "back_prob")), (hscan, ("ratio",))):
                    for k in keys if d is not None else ():
                        d.pop(k, None)
            if rows:
                parts.append(r["rows"] if len(r["rows"]) * 2 >= fwd["n_nodes"] else r["rows"].clone())
        tot = totals.cpu().numpy()
        if tot[5] != 0:
            raise _lib.ArtError(f"run_events: {int(tot[5])} cyclotron re-runs of final photon segments do not "
                                "reproduce their end states")
        f_inx = int(round(tot[4] + tot[1]))
        # (a device tensor, not a Python number: torch turns a division by a host scalar into a
        # multiplication by its reciprocal, which rounds differently from the host's division)
        div = torch.full((), float(f_inx) if f_inx > 0 else 1.0, dtype=F64, device=self.device)
        rows_raw = rows_div = None
        if rows:
            rows_raw = torch.cat(parts, dim=0) if parts else torch.zeros(0, ncols, dtype=F64, device=self.device)
            rows_div = rows_raw.clone()
            rows_div[:, 7] /= div  # saveAll[:, 8] ./= f_inx (MainRunner.jl:747): one IEEE division
        res = {"rows": rows_div, "flux": (flux / div).view(2, int(nbins)), "f_inx": f_inx,
               "sum_weight_sln_prob": (float(tot[2]) / max(f_inx, 1), float(tot[3]) / max(f_inx, 1)),
               "n_rows": int(round(tot[0])),
               "n_photon_rows": int(round(tot[1])), "totals": totals, "flux_raw": flux, "rows_raw": rows_raw}
        if sky_map is not None:
            ekw = {k: sky_kw[k] for k in ("n_theta", "n_phi", "n_dw", "theta_axis", "dw_range")}
            res.update(sky_map=sky_hist / div, sky_raw=sky_hist, sky_map_edges=sky_map_edges(**ekw))
        if errors:
            from .trees import _sigma_info
            if moments is None:  # (no events)
                moments = self._zero_moments(int(nbins), shape)
            host = {k: None if v is None else v.cpu().numpy() for k, v in moments.items()}
            if host["totals"][7] != 0:
                raise _lib.ArtError(f"run_events: {int(host['totals'][7])} node records lie in the range of another tree")
            # (the tables are small: σ is formed on the host, as main_runner_tree forms it from the reduced ones)
            tt = {"flux": flux.cpu().numpy(), "f_inx": f_inx, "sum_axion": tot[2], "sum_photon": tot[3], "moments": host}
            if shape:
                tt["sky"] = sky_hist.cpu().numpy()
            sig = _sigma_info(tt, int(nbins))
            res.update(flux_sigma=torch.from_numpy(sig["flux_sigma"]).to(self.device), moments=moments,
                       sum_weight_sln_prob_sigma=sig["sum_weight_sln_prob_sigma"])
            if shape:
                res["sky_map_sigma"] = torch.from_numpy(sig["sky_map_sigma"]).to(self.device)
        if couplings is not None:
            from .trees import scan_raw, scan_result
            res["coupling_scan"] = self._finish_scan(
                scan, lambda: self._zero_scan(len(couplings), len(_lib.REWEIGHT_TOTALS), int(nbins), shape, errors,
                                              {"g": list(couplings)}),
                lambda s: scan_result(scan_raw(s), self.params.g_agg, f_inx), "unlinked",
                "of the forward forest have no parent, or more than one")
        if halos is not None:
            from .trees import halo_scan_raw, halo_scan_result
            res["halo_scan"] = self._finish_scan(
                hscan, lambda: self._zero_scan(len(halos), len(_lib.HALO_SCAN_TOTALS), int(nbins), shape, errors,
                                               {"base": self._halo_key(halo), "models": list(halos)}),
                lambda s: halo_scan_result(halo_scan_raw(s), f_inx), "misplaced", "lie in the range of another tree")
        if want:
            from .trees import replicates_raw, replicates_result
            for out, have, kind, K in ((res, rep, "run", 1), (res.get("coupling_scan"), crep, "coupling", len(couplings or ())),
                                       (res.get("halo_scan"), hrep, "halo", len(halos or ()))):
                if out is None:
                    continue
                have = self._zero_replicates(kind, K, replicates, int(nbins), shape) if have is None else have  # (no events)
                out["replicates"] = replicates_result(replicates_raw(have), f_inx)
                if out["replicates"]["misplaced"] != 0:
                    raise _lib.ArtError(f"run_events: {out['replicates']['misplaced']} node records lie in the range of "
                                        "another tree")
        if spectrum is not None:
            from .trees import spectrum_raw, spectrum_result
            for out, have, kind, K in ((res, spec, "run", 1), (res.get("coupling_scan"), cspec, "coupling", len(couplings or ())),
                                       (res.get("halo_scan"), hspec, "halo", len(halos or ()))):
                if out is None:
                    continue
                have = self._zero_spectrum(kind, K, *spectrum) if have is None else have  # (no events)
                out["spectrum"] = spectrum_result(spectrum_raw(have), f_inx)
                if out["spectrum"]["misplaced"] != 0:
                    raise _lib.ArtError(f"run_events: {out['spectrum']['misplaced']} node records lie in the range of "
                                        "another tree")
        if ospec is not None:
            from .trees import origin_result
            zero = np.zeros(ospec["shape"])  # (no events)
            res["origin"] = origin_result(zero if omap is None else omap["hist"].cpu().numpy(), ospec, f_inx,
                                          0.0 if omap is None else float(omap["misplaced"].item()))
            if want:
                rr = res["replicates"]
                res["origin"]["replicates"] = {
                    "raw": np.zeros((replicates,) + ospec["shape"]) if orep is None else orep["hist"].cpu().numpy(),
                    "n_g": rr["n_g"], "a_g": rr["a_g"], "R": replicates, "f_inx": f_inx}
            if exact:
                if xacc is None:  # (no events)
                    xacc = self._zero_exact("run", 1, int(nbins), shape)
                if oacc is None:
                    oacc = torch.zeros(zero.size, _lib.EXACT_LIMBS, dtype=torch.int64, device=self.device)
                xacc["origin"] = oacc.view(1, *ospec["shape"], _lib.EXACT_LIMBS)
        if exact:
            for out, have, kind, K in ((res, xacc, "run", 1), (res.get("coupling_scan"), cxacc, "coupling", len(couplings or ())),
                                       (res.get("halo_scan"), hxacc, "halo", len(halos or ()))):
                if out is None:
                    continue
                have = self._zero_exact(kind, K, int(nbins), shape) if have is None else have  # (no events)
                out["exact"] = self.exact_finish(have, f_inx)
                if float(have["misplaced"].item()) != 0:
                    raise _lib.ArtError(f"run_events: {int(have['misplaced'].item())} node records lie in the range of "
                                        "another tree")
        if grid:
            from .trees import grid_raw, grid_result
            if cells is None:  # (no events)
                cells = self._zero_grid(couplings, halos, self._halo_key(halo), replicates, int(nbins), errors)
            res["grid"] = grid_result(grid_raw(cells), f_inx)
            if res["grid"]["misplaced"] != 0:
                raise _lib.ArtError(f"run_events: {res['grid']['misplaced']} node records lie in the range of another tree")
        return res

    # ---- pointwise physics (parity tests)
    def eval_rhs(self, u, tau, erg, species):
        n = tau.numel()
        du = self.empty(7 * n)
        check(self.lib.art_eval_rhs_device(C.byref(self.cp), n, _p(u), _p(tau), _p(erg), _p(species), _p(du),
                                           _stream()))
        return du

    def eval_hamiltonian(self, x, k, T, E):
        n = T.numel()
        H, gx, gk, gT = self.empty(n), self.empty(3 * n), self.empty(3 * n), self.empty(n)
        check(self.lib.art_eval_hamiltonian_device(C.byref(self.cp), n, _p(x), _p(k), _p(T), _p(E), _p(H), _p(gx),
                                                   _p(gk), _p(gT), _stream()))
        return H, gx, gk, gT

    def eval_cyclotron(self, pos, k, t):
        """ω_c [eV] and a crossing's optical depth at Cartesian pos, k (3n SoA) and time t (n)"""
        n = t.numel()
        wc, tau = self.empty(n), self.empty(n)
        check(self.lib.art_eval_cyclotron_device(C.byref(self.cp), n, _p(pos), _p(k), _p(t), _p(wc), _p(tau),
                                                 _stream()))
        return wc, tau

    def eval_math(self, fn, a, b=None, tu=0):
        """One of art_core.h's hand-written scalar functions at every element of a (and b)
        (art_eval_math_device): fn an ART_MATH_* id or its name ("SINCOS", "EXP", "LOG", "RCP",
        "POW120", "MAX_ABS", "MIN_Q", "MAX_Q", "RCLAMP"); tu the translation unit the kernel was
        compiled in (0 art_kernels.hip, 1 art_kernels_nolicm.hip; art_eval_math.h in each). Returns (sin, cos) for SINCOS,
        else one tensor."""
        fn = _lib.MATH_FN[fn] if isinstance(fn, str) else int(fn)
        n = a.numel()
        out0 = self.empty(n)
        out1 = self.empty(n) if fn == _lib.MATH_FN["SINCOS"] else None
        check(self.lib.art_eval_math_device(fn, int(tu), n, _p(a), _p(b), _p(out0), _p(out1), _stream()))
        return (out0, out1) if out1 is not None else out0

    def eval_condition(self, u, tau):
        n = tau.numel()
        c = self.empty(n)
        check(self.lib.art_eval_condition_device(C.byref(self.cp), n, _p(u), _p(tau), _p(c), _stream()))
        return c
