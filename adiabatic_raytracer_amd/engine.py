"""Device-resident batches: inputs and outputs live in HBM as torch tensors (PyTorch is
plumbing for device memory and streams here); every compute call goes through libart.so
on the caller's current HIP stream."""
from __future__ import annotations

import ctypes as C

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
    def sample(self, n: int, seed: int = 1769, ray_offset: int = 0, max_r=None) -> dict:
        max_r = self.params.max_r() if max_r is None else max_r
        o = {"x": self.empty(3 * n), "k_init": self.empty(3 * n), "erg": self.empty(n), "vifty": self.empty(3 * n),
             "weights": self.empty(n, dtype=torch.int32), "attempts": self.empty(n, dtype=torch.int32)}
        check(self.lib.art_sample_conversion_points_device(
            C.byref(self.cp), float(max_r), int(seed), int(ray_offset), int(n),
            *[_p(o[k]) for k in ("x", "k_init", "erg", "vifty", "weights", "attempts")], _stream()))
        return o

    def forward_roots(self, n: int, seed: int = 1769, ray_offset: int = 0) -> dict:
        """Segment inputs of the forward-tree roots (MainRunner.jl:653-664 -> :179): photons
        at the sampled conversion points, Δω = -1, ln t0 = -30."""
        s = self.sample(n, seed, ray_offset)
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
    def event_weight(self, sample: dict, max_r=None, rho_DM=0.45, n_maxSample=6):
        n = sample["erg"].numel()
        max_r = self.params.max_r() if max_r is None else max_r
        out = self.empty(5 * n)
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
