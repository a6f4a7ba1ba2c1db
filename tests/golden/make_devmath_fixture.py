"""True values for the hand-written scalar functions of art_core.h (msincos, exp_fma, log_fma,
frcp, the controller's EEst2^(1/120)): tests/golden/devmath/{sincos,exp,log,rcp,pow120}.npz.

CPU only, mpmath at 256 bits; never run at test time (tests/test_devmath.py and
tests/test_gpu_devmath.py read the files). Regenerate with

    python tests/golden/make_devmath_fixture.py

which rewrites the files byte for byte (seeded default_rng, fixed zip timestamps).

Each file holds the inputs `x`, the true value as a double-double and the sets the inputs are
drawn from (`set_names`, `set_sizes`, in the order of `x`):

    hi      the true value rounded to the nearest double
    lo_ulp  (true value - hi) / spacing(|hi|), float32: the double-double's low part in units of
            hi's ulp, |lo_ulp| <= 0.5

so that the error of a computed y in ulp of the true value is

    |(y - hi) / spacing(|hi|) - lo_ulp|

which is |(y - hi) - lo| / spacing(|hi|) with lo = lo_ulp spacing(|hi|). y - hi is exact for any y
within a factor 2 of hi and the division is by a power of two, so the figure is good to float32's
3e-8 ulp with no high-precision arithmetic at test time. The low part is kept in ulp and not as a
double because a double lo underflows where hi is small (e^-708 = 3.3e-308 has an ulp of 4.9e-324,
the smallest subnormal: lo would round to 0 or a whole ulp), and because five float64 arrays of
sincos's 4076 points would not fit the 128 KB a fixture file may take. sincos.npz holds
sin_hi, sin_lo_ulp, cos_hi, cos_lo_ulp.
"""
import io
import os
import zipfile

import mpmath as mp
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "devmath")
mp.mp.prec = 256
MAX_POINTS, MAX_BYTES = 4096, 128 * 1024


def split(values):
    """mpf values -> (hi float64, lo_ulp float32)"""
    hi = np.array([float(v) for v in values])
    sp = np.spacing(np.abs(hi))
    lo = np.array([float((v - mp.mpf(float(h))) / mp.mpf(float(s))) for v, h, s in zip(values, hi, sp)])
    assert np.all(np.isfinite(hi)) and np.all(hi != 0.0) and np.all(np.abs(lo) <= 0.5)
    return hi, lo.astype(np.float32)


def neighbours(c):
    """every double of c with the one below and the one above it"""
    c = np.asarray(c, np.float64)
    return np.stack([np.nextafter(c, -np.inf), c, np.nextafter(c, np.inf)], axis=1).reshape(-1)


def signs(rng, n):
    return np.where(rng.random(n) < 0.5, -1.0, 1.0)


def write(name, sets, **arrays):
    """tests/golden/devmath/<name>.npz, reproducibly: members in the given order, the zip's
    timestamps fixed"""
    x = np.concatenate([s for _, s in sets])
    assert x.size <= MAX_POINTS and all(a.shape == x.shape for a in arrays.values())
    members = {"x": x, **arrays, "set_names": np.array([n for n, _ in sets]),
               "set_sizes": np.array([s.size for _, s in sets], np.int64)}
    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, name + ".npz")
    with zipfile.ZipFile(path, "w") as z:
        for key, a in members.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(a), allow_pickle=False)
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue(), compresslevel=9)
    size = os.path.getsize(path)
    assert size <= MAX_BYTES, (name, size)
    print(f"{name}: {x.size} points, {size} bytes; " + ", ".join(f"{n} {s.size}" for n, s in sets))


def sincos():
    rng = np.random.default_rng(20260101)
    sets = [("uniform_200", rng.uniform(-200.0, 200.0, 2048)),
            ("pi", rng.uniform(-np.pi, np.pi, 768)),
            ("sampler_2pi", rng.uniform(0.0, 2.0 * np.pi, 384)),
            ("uniform_1e6", rng.uniform(-1e6, 1e6, 512)),
            ("tiny", signs(rng, 64) * 10.0 ** rng.uniform(-300.0, -8.0, 64)),
            # the doubles nearest k π/2, where the reduction cancels most
            ("k_half_pi", neighbours([float(k * mp.pi / 2) for k in range(1, 101)]))]
    x = np.concatenate([s for _, s in sets])
    sh, sl = split([mp.sin(mp.mpf(float(v))) for v in x])
    ch, cl = split([mp.cos(mp.mpf(float(v))) for v in x])
    write("sincos", sets, sin_hi=sh, sin_lo_ulp=sl, cos_hi=ch, cos_lo_ulp=cl)


def exp():
    rng = np.random.default_rng(20260102)
    ks = np.round(np.linspace(-1000, 1000, 250)).astype(int)
    sets = [("uniform_708", rng.uniform(-708.0, 708.0, 1536)),
            ("ln_t", rng.uniform(-30.0, 5.0, 1536)),
            ("small", rng.uniform(-1e-3, 1e-3, 256)),
            # the reduction's rint ties: the doubles nearest (k + 1/2) ln 2
            ("rint_ties", neighbours([float((int(k) + mp.mpf(0.5)) * mp.ln2) for k in ks])),
            ("zeros", np.array([0.0, -0.0]))]
    x = np.concatenate([s for _, s in sets])
    hi, lo = split([mp.exp(mp.mpf(float(v))) for v in x])
    write("exp", sets, hi=hi, lo_ulp=lo)


def log():
    rng = np.random.default_rng(20260103)
    es = np.round(np.linspace(-1020, 1020, 64)).astype(int)
    sub = np.concatenate([[1], np.floor(2.0 ** rng.uniform(0.0, 52.0, 63))]).astype(np.int64)
    sets = [("decades_300", 10.0 ** rng.uniform(-300.0, 300.0, 1280)),
            ("half_to_2", rng.uniform(0.5, 2.0, 1024)),
            ("one_1e-6", 1.0 + rng.uniform(-1e-6, 1e-6, 512)),
            ("one_1e-12", 1.0 + rng.uniform(-1e-12, 1e-12, 256)),
            ("eest2", 10.0 ** rng.uniform(-40.0, 10.0, 256)),
            # where the mantissa is folded: the doubles around √½ 2^e
            ("sqrt_half", neighbours([float(mp.ldexp(mp.sqrt(mp.mpf(0.5)), int(e))) for e in es])),
            ("subnormal", sub.view(np.float64)),
            ("max", np.array([np.finfo(np.float64).max]))]
    x = np.concatenate([s for _, s in sets])
    assert np.all(x > 0.0) and np.all(x != 1.0) and np.all(sets[6][1] < np.finfo(np.float64).tiny)
    hi, lo = split([mp.log(mp.mpf(float(v))) for v in x])
    write("log", sets, hi=hi, lo_ulp=lo)


def rcp():
    rng = np.random.default_rng(20260104)
    k = np.arange(1, 65)
    one = (np.float64(1.0).view(np.int64) + np.concatenate([k, -k])).view(np.float64)  # 1 ± k ulp
    two = (np.float64(2.0).view(np.int64) - k).view(np.float64)  # 2 - k ulp
    near = np.concatenate([one, two])
    p2 = np.ldexp(1.0, np.arange(-1020, 1021, 4))
    sets = [("mantissa_exponent", signs(rng, 2048) * np.ldexp(rng.uniform(1.0, 2.0, 2048), rng.integers(-1000, 1001, 2048))),
            ("near_1_and_2", np.concatenate([near, -near])),
            ("mantissa_near_2", signs(rng, 512) * rng.uniform(1.99, 2.0, 512)),
            ("powers_of_two", np.concatenate([p2, -p2]))]
    x = np.concatenate([s for _, s in sets])
    assert np.all(np.abs(sets[2][1]) < 2.0)
    hi, lo = split([1 / mp.mpf(float(v)) for v in x])
    write("rcp", sets, hi=hi, lo_ulp=lo)


def pow120():
    rng = np.random.default_rng(20260105)
    sets = [("eest2", 10.0 ** rng.uniform(-40.0, 10.0, 2048))]
    hi, lo = split([mp.root(mp.mpf(float(v)), 120) for v in sets[0][1]])
    write("pow120", sets, hi=hi, lo_ulp=lo)


if __name__ == "__main__":
    sincos()
    exp()
    log()
    rcp()
    pow120()
