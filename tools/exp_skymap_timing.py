"""DEV TOOL: kernel times of the sky-map entry points by HIP events (the median of REPS launches
after a warm-up), one JSON line each:

  - art_histogram3_device on ROWS rows with weights (33 B a row) for (1,50,1), (32,64,1) and
    (64,128,16) bins, uniform directions; the yardsticks on the same rows: flux_phi_kernel
    (art_flux_histogram_phi_device, 50 bins) and the HBM read floor;
  - (64,128,16) again on the real, concentrated (cos θf, φf, Δω) of a propagated flat batch;
  - the fused kernel (art_sky_map_segments_device) on that device-resident batch.

    python tools/exp_skymap_timing.py [ROWS] [REPS] [--global-only] >> profiles/NAME.jsonl

--global-only: the launches that add to HBM alone (A/B of builds of that path; ART_LIB names the
library, the "lib" field of every line)."""
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import adiabatic_raytracer_amd as A  # noqa: E402

F64 = torch.float64
LIB_TAG = os.path.basename(os.environ.get("ART_LIB", "libart.so"))


def timed(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return float(np.median(ms)), float(np.min(ms)), float(np.max(ms))


def emit(what, n, t, **kw):
    print(json.dumps({"what": what, "lib": LIB_TAG, "rows": n, "ms_median": t[0], "ms_min": t[1], "ms_max": t[2], **kw}),
          flush=True)


def p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def h3(lib, n, a, b, c, sp, w, shape, ranges, mode, hist):
    A._lib.check(lib.art_histogram3_device(n, p(a), p(b), p(c), p(sp), p(w), (C.c_int32 * 3)(*shape),
                                           (C.c_double * 3)(*[r[0] for r in ranges]),
                                           (C.c_double * 3)(*[r[1] for r in ranges]), mode, p(hist),
                                           C.c_void_p(torch.cuda.current_stream().cuda_stream)))


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    n = int(float(args[0])) if args else 10_000_000
    reps = int(args[1]) if len(args) > 1 else 20
    global_only = "--global-only" in sys.argv
    eng = A.Engine(A.Params(theta_m=0.2, mass_a=1e-5, flat=True))
    lib, dev = eng.lib, eng.device
    g = torch.Generator(device=dev).manual_seed(1)
    shapes = [(64, 128, 16)] if global_only else [(1, 50, 1), (32, 64, 1), (64, 128, 16)]
    floor_ms = n * 33 / 8e12 * 1e3  # 8 TB/s peak HBM

    # ---- uniform directions
    a = torch.rand(n, dtype=F64, device=dev, generator=g) * 2 - 1
    b = (torch.rand(n, dtype=F64, device=dev, generator=g) * 2 - 1) * np.pi
    c = torch.rand(n, dtype=F64, device=dev, generator=g)
    w = torch.rand(n, dtype=F64, device=dev, generator=g) + 0.5
    sp = (torch.rand(n, device=dev, generator=g) < 0.9).to(torch.int8)
    ranges = ((-1.0, 1.0), (-np.pi, np.pi), (0.0, 1.0))
    for shape in shapes:
        hist = torch.zeros(2, *shape, dtype=F64, device=dev)
        t = timed(lambda: h3(lib, n, a, b, c, sp, w, shape, ranges, 0, hist), reps)
        emit("histogram3 uniform", n, t, shape=shape, path="lds" if 2 * np.prod(shape) <= 8192 else "global",
             read_floor_ms=floor_ms, counted=float(hist.sum().item()))
    if not global_only:
        hist = torch.zeros(100, dtype=F64, device=dev)
        t = timed(lambda: A._lib.check(lib.art_flux_histogram_phi_device(
            n, p(b), p(sp), p(w), 50, p(hist), C.c_void_p(torch.cuda.current_stream().cuda_stream))), reps)
        emit("flux_phi_kernel uniform", n, t, shape=(50,), read_floor_ms=n * 17 / 8e12 * 1e3)
    del a, b, c, w, sp

    # ---- a propagated flat batch: its real directions and line shifts
    inp = eng.forward_roots(n, seed=1769)
    out = eng.propagate(inp, max_crossings=-1)
    torch.cuda.synchronize()
    k = out["k_end"].view(3, n)
    a = k[2] / torch.sqrt(k[0] * k[0] + k[1] * k[1] + k[2] * k[2])
    b = torch.atan2(k[1], k[0])
    c = out["u7_end"] / eng.params.mass_a
    fin = torch.isfinite(c)
    dw_range = (float(c[fin].min().item()), float(c[fin].max().item()))
    w = torch.rand(n, dtype=F64, device=dev, generator=g) + 0.5
    sp = inp["species"]
    ranges = ((-1.0, 1.0), (-np.pi, np.pi), dw_range)
    shape = (64, 128, 16)
    hist = torch.zeros(2, *shape, dtype=F64, device=dev)
    t = timed(lambda: h3(lib, n, a, b, c, sp, w, shape, ranges, 0, hist), reps)
    one = torch.zeros(2, *shape, dtype=F64, device=dev)
    h3(lib, n, a, b, c, sp, None, shape, ranges, 0, one)
    occ = one[1].reshape(-1)
    top = torch.sort(occ, descending=True).values
    emit("histogram3 flat batch", n, t, shape=shape, path="global", read_floor_ms=floor_ms, counted=float(occ.sum().item()),
         bins_hit=int((occ > 0).sum().item()), share_of_top_64_bins=float((top[:64].sum() / occ.sum()).item()),
         dw_range=dw_range)
    for shape in shapes:
        if shape == (1, 50, 1):
            continue
        hist = torch.zeros(2, *shape, dtype=F64, device=dev)
        kw = dict(n_theta=shape[0], n_phi=shape[1], n_dw=shape[2], dw_range=dw_range if shape[2] > 1 else None, hist=hist)
        t = timed(lambda: eng.sky_map(out, sp, w, **kw), reps)
        # x_end, k_end (48 B), u7_end, w (16 B), status (4 B), species (1 B)
        emit("sky_map_segments flat batch", n, t, shape=shape, path="lds" if 2 * np.prod(shape) <= 8192 else "global",
             read_floor_ms=n * 69 / 8e12 * 1e3)
    if not global_only:
        hist = torch.zeros(100, dtype=F64, device=dev)
        t = timed(lambda: eng.flux_histogram(out, sp, w, 50, hist=hist), reps)
        emit("flux_kernel flat batch", n, t, shape=(50,), read_floor_ms=n * 61 / 8e12 * 1e3)
