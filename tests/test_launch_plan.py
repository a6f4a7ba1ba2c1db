"""The launch plan (art_launch_plan.h: which kernels one propagate launch runs), through a host compile
of the header (tools/launchplancheck): the band edges of the small-tail and 1-wave/SIMD thresholds, the
side conditions of graduation, the tail kernel and the hot side launch, the plan against a transcription
of the launch logic as it stood before it became a header, and completeness: over the full input grid
every plan names a build of the instantiation lists, and every listed build is reached. No GPU."""
import os
import random
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import launchplancheck  # noqa: E402

NCU = 256  # the MI355X


def plan(**kw):
    kw.setdefault("ncu", NCU)
    p = launchplancheck.plan(**kw)
    assert p["bulk_exists"] and p["cont_exists"] and p["tail_exists"], p
    return p


def bulk(p):
    return (p["integrator"], p["geom"], p["save"], p["don"], p["wps"], p["cyc"]) if p["bulk"] else None


# ---- band edges, 256 CUs ----

@pytest.mark.parametrize("geom", ["FLAT", "GR"])
@pytest.mark.parametrize("donate", [0, 16])
def test_small_tail_edge(geom, donate):
    """At most 4 x CUs = 1024 Vern6 rays: tail_kernel alone, one wave per ray, whatever the donation says;
    one ray more: the persistent integrator."""
    p = plan(n=1024, geom=geom, donate_device=donate)
    assert p["small_tail"] and not p["bulk"] and not p["cont"] and not p["hot"]
    assert p["tail"] and p["tail_geom"] == geom and p["tail_grid"] == 1024
    assert p["donate"] == 0 and p["ncont"] == 1024 and p["nhot"] == 0 and p["graduate"] == 0
    q = plan(n=1025, geom=geom, donate_device=donate)
    assert not q["small_tail"] and q["bulk"] and q["bulk_grid"] == 5 and q["donate"] == donate
    if donate:
        assert bulk(q) == ("vern6", geom, False, 1, 2, False)
        assert q["cont"] and q["cont_donate"] == 4 and q["tail"] and q["graduate"] == 2048
        assert q["ncont"] == 1025 and q["nhot"] == 1024
        assert q["cont_grid"] == 2  # 5 blocks x 4 waves x 16 lanes = 320 records: two blocks
        assert q["cont_wps"] == (1 if geom == "GR" else 2)
    else:
        assert bulk(q) == ("vern6", geom, False, 0, 1, False)  # the 1-wave/SIMD build
        assert not q["cont"] and not q["tail"] and q["graduate"] == 0 and q["ncont"] == 0


@pytest.mark.parametrize("geom", ["FLAT", "GR"])
@pytest.mark.parametrize("donate", [0, 16])
def test_w1_edge(geom, donate):
    """At most 64 x 4 x CUs = 65 536 rays without donation: the 1-wave/SIMD build, one block per CU; one ray
    more, or any donation: 2 waves/SIMD."""
    p, q = plan(n=65536, geom=geom, donate_device=donate), plan(n=65537, geom=geom, donate_device=donate)
    if donate:
        assert bulk(p) == bulk(q) == ("vern6", geom, False, 1, 2, False)
        assert p["bulk_grid"] == 256 and q["bulk_grid"] == 257
        assert p["ncont"] == 65536 and q["ncont"] == 65537  # (below 256 CUs x 32 waves x 16 lanes)
    else:
        assert bulk(p) == ("vern6", geom, False, 0, 1, False) and p["bulk_grid"] == 256
        assert bulk(q) == ("vern6", geom, False, 0, 2, False) and q["bulk_grid"] == 257
    # the grid follows the occupancy the launch finds for its kernel
    assert plan(n=10 ** 6, geom=geom, donate_device=donate, blocks_per_cu=2)["bulk_grid"] == 512
    assert plan(n=10 ** 6, geom=geom, donate_device=donate, blocks_per_cu=1)["bulk_grid"] == 256


def test_small_tail_and_w1_settings():
    assert not plan(n=512, geom="FLAT", small_tail=0)["small_tail"]  # ART_SMALL_TAIL=0: off
    assert plan(n=5000, geom="FLAT", small_tail=5000)["small_tail"]
    assert plan(n=5000, geom="FLAT", small_tail=5000)["tail_grid"] == 1024  # one wave per SIMD, the rest queue
    assert bulk(plan(n=512, geom="FLAT", small_tail=0, w1=0)) == ("vern6", "FLAT", False, 0, 2, False)
    assert bulk(plan(n=512, geom="GR", small_tail=0, w1=0, donate_device=0)) == ("vern6", "GR", False, 0, 2, False)
    # no 1-wave/SIMD build of the general geometry
    assert bulk(plan(n=512, geom="ANY", small_tail=0)) == ("vern6", "ANY", False, 0, 2, False)


@pytest.mark.parametrize("n", [1, 512, 1024, 2048, 10 ** 6])
def test_general_geometry_never_leaves_the_persistent_integrator(n):
    """There is no tail_kernel<GEOM_ANY> (it did not reproduce propagate_kernel<GEOM_ANY> bit for bit): no
    small-batch tail path, and with donation the packed continuation alone, whatever the settings ask for."""
    for donate in (-1, 0, 16, 63):
        p = plan(n=n, geom="ANY", donate_device=donate, nonblocking=1, graduate_device=1, hot_at_env=16, tail_rays=100000,
                 small_tail=5000)
        lanes = max(donate, 0)
        assert not p["small_tail"] and bulk(p) == ("vern6", "ANY", False, 1 if lanes else 0, 2, False)
        assert p["donate"] == lanes and p["cont"] == bool(lanes) and p["cont_wps"] == (2 if lanes else 0)
        assert not p["tail"] and p["tail_grid"] == 0 and p["cont_donate"] == 0
        assert p["graduate"] == 0 and not p["grad_records"] and not p["hot"] and not p["hot_records"] and not p["sorted"]


def test_default_donation_goes_by_geometry():
    assert plan(n=2048, geom="GR")["donate"] == 16
    assert plan(n=2048, geom="FLAT")["donate"] == 0 and plan(n=2048, geom="ANY")["donate"] == 0
    assert plan(n=2048, geom="GR", integrator="rk4")["donate"] == 0
    assert plan(n=2048, geom="GR", save=1)["donate"] == 0 and plan(n=2048, geom="GR", cyc=1)["donate"] == 0
    # the caller's choice, then the device's
    assert plan(n=2048, geom="GR", donate_device=0)["donate"] == 0
    assert plan(n=2048, geom="GR", donate_device=0, donate_caller=8)["donate"] == 8
    assert plan(n=2048, geom="FLAT", donate_caller=0, donate_device=16)["donate"] == 0


# ---- side conditions ----

@pytest.mark.parametrize("geom", ["FLAT", "GR", "ANY"])
@pytest.mark.parametrize("special", [dict(integrator="rk4"), dict(save=1), dict(cyc=1), dict(integrator="rk4", save=1)])
@pytest.mark.parametrize("n", [512, 2048, 10 ** 6])
def test_rk4_saveat_and_cyclotron_never_graduate_or_leave_the_integrator(geom, special, n):
    for donate in (0, 16):
        p = plan(n=n, geom=geom, donate_device=donate, nonblocking=1, graduate_device=1, hot_at_env=16, **special)
        assert not p["small_tail"] and p["bulk"] and p["wps"] == 2
        assert p["graduate"] == 0 and not p["grad_records"] and not p["tail"] and not p["hot"] and not p["sorted"]
        assert p["hot_at"] == 0 and p["cont_donate"] == 0
        assert p["cont"] == bool(donate) and p["don"] == (1 if donate else 0)
        assert p["cont_wps"] == (2 if donate else 0)  # (the continuation is the bulk build again)
        rk4 = special.get("integrator") == "rk4"
        want_geom = geom if (geom == "FLAT" and not (rk4 and "save" in special)) else ("ANY" if rk4 else geom)
        assert bulk(p) == ("rk4" if rk4 else "vern6", want_geom, "save" in special, 1 if donate else 0, 2, "cyc" in special)


def test_art_tail_0_switches_graduation_and_hot_off():
    on = plan(n=2048, geom="GR", nonblocking=1)
    assert on["tail"] and on["graduate"] == 2048 and on["hot"] and on["hot_at"] == 128 and on["sorted"]
    off = plan(n=2048, geom="GR", nonblocking=1, tail_rays=0)
    assert off["cont"] and bulk(off) == bulk(on)  # the packed continuation alone
    assert not off["tail"] and off["graduate"] == 0 and not off["grad_records"] and not off["hot"] and off["hot_at"] == 0
    assert off["cont_donate"] == 0 and not off["sorted"]
    assert off["bulk_grid"] == on["bulk_grid"] == 8  # (8 blocks: too few to give HOT_BLOCKS of them up)
    k = plan(n=2048, geom="GR", tail_rays=100000)
    assert k["tail"] and k["tail_grid"] == 2 * 4 * 4 + 2048  # second-level lanes + graduation records, below 100 000 waves


def test_hot_needs_a_nonblocking_stream_records_and_graduation():
    base = dict(n=2048, geom="GR")
    assert plan(**base, nonblocking=1)["hot"]
    assert not plan(**base, nonblocking=0)["hot"] and plan(**base, nonblocking=0)["graduate"] == 2048
    assert not plan(**base, nonblocking=1, graduate_device=0)["hot"]  # no graduation, no early graduation
    assert not plan(**base, nonblocking=1, graduate_env=0)["hot"]
    assert not plan(**base, nonblocking=1, hot_at_env=0)["hot"]
    assert not plan(**base, nonblocking=1, donate_device=0)["hot"]  # nhot = 0: no donation records, no hot ones
    assert plan(**base, nonblocking=1, donate_device=0)["nhot"] == 0
    p = plan(**base, nonblocking=1, hot_at_env=16, graduate_device=1)
    assert p["hot"] and p["hot_at"] == 16 and p["graduate"] == 1 and p["nhot"] == 1024
    assert not plan(**base, nonblocking=1, hot_order=0)["sorted"] and plan(**base, nonblocking=1, hot_order=0)["hot"]
    # a large launch gives HOT_BLOCKS = 32 of its blocks to the side launch
    assert plan(n=10 ** 6, geom="GR", nonblocking=1)["bulk_grid"] == 512 - 32
    assert plan(n=10 ** 6, geom="GR", nonblocking=0)["bulk_grid"] == 512


def test_gr_continuation_is_one_wave_per_simd_only_with_w1():
    assert plan(n=2048, geom="GR")["cont_wps"] == 1
    p = plan(n=2048, geom="GR", w1=0)
    assert p["cont_wps"] == 2 and p["cont_geom"] == "GR" and p["cont_don"] == 1
    assert plan(n=2048, geom="FLAT", donate_device=16)["cont_wps"] == 2  # (flat stays at 2: measured slower at 1)
    assert plan(n=2048, geom="ANY", donate_device=16)["cont_wps"] == 2


def test_streamed_plan():
    for geom in ("FLAT", "GR", "ANY"):
        p = launchplancheck.streamed(10 ** 7, geom, 496)
        assert p["streamed"] and bulk(p) == ("vern6", geom, False, 3, 2, False) and p["bulk_grid"] == 496 and p["bulk_exists"]
        assert not p["cont"] and not p["tail"] and not p["hot"] and p["graduate"] == 0
    assert launchplancheck.streamed(2048, "FLAT", 496)["bulk_grid"] == 8


# ---- the plan against the launch logic as it stood in propagate_device_impl and launch_propagate ----

def old_logic(n, integrator, geom, save, cyc, donate_caller, donate_device, graduate_device, graduate_env, tail_rays,
              tail_donate, w1, small_tail_limit, nonblocking, hot_at_env, hot_order, ncu, per_cu):
    """A transcription of the branches of art_device.cpp and art_kernels.hip before the plan became a header."""
    rk4, flat, sch = integrator == "rk4", geom == "FLAT", geom == "GR"
    none = not save and not cyc
    if geom == "ANY":
        # The one rule the plan adds to that logic: the general geometry has no tail kernel (ART_BUILDS_TAIL), so
        # it takes neither the small-batch path nor second-level donation, graduation or the hot side launch --
        # the branches below as ART_TAIL=0 and ART_SMALL_TAIL=0 took them, without the graduation records.
        tail_rays, small_tail_limit, graduate_device = 0, 0, 0
    r = dict(small_tail=none and not rk4 and n <= small_tail_limit)
    if r["small_tail"]:
        r.update(bulk=False, tail=True, tail_grid=min(n, ncu * 4), cont=False, hot=False, graduate=0, sorted=False, hot_at=0)
        return r
    donate = donate_caller if donate_caller >= 0 else (donate_device if donate_device >= 0 else
                                                       (16 if sch and not rk4 and none else 0))
    ncont = min(n, ncu * 32 * donate) if donate > 0 else 0
    nhot = min(ncont, 1024)
    graduate, hot_set, hot_at = 0, False, 0
    grad_ptr = False
    if ncont and none and not rk4:
        grad_ptr = True
        graduate = graduate_device if graduate_device >= 0 else max(0, graduate_env)
        if nhot and graduate > 0 and nonblocking:
            hot_set, hot_at = True, max(0, hot_at_env)
    # launch_propagate
    if not (donate > 0 and tail_rays != 0 and not rk4 and none and ncont):
        grad_ptr, graduate = False, 0
    hot = graduate > 0 and hot_set and hot_at > 0
    if not hot:
        hot_at = 0
    don = 1 if donate > 0 else 0
    if cyc:
        fn = ("vern6", "FLAT" if flat else ("GR" if sch else "ANY"), False, don, 2, True)
    elif save and not rk4 and flat:
        fn = ("vern6", "FLAT", True, don, 2, False)
    elif not save and flat:
        fn = ("rk4" if rk4 else "vern6", "FLAT", False, don, 2, False)
    else:
        fn = ("rk4" if rk4 else "vern6", "GR" if (not rk4 and sch) else "ANY", save, don, 2, False)
    is_w1 = False
    if w1 and donate <= 0 and none and not rk4 and (flat or sch) and n <= ncu * 4 * 64:
        fn, is_w1 = ("vern6", "FLAT" if flat else "GR", False, 0, 1, False), True
    per = per_cu if per_cu > 0 else (1 if is_w1 else 2)
    grid = min((n + 255) // 256, ncu * per)
    if hot and grid > 64:
        grid -= 32
    r.update(bulk=True, build=fn, bulk_grid=grid, cont=donate > 0, hot=hot, graduate=graduate, hot_at=hot_at,
             sorted=hot and hot_order and n < 2 ** 31 - 1, tail=False, tail_grid=0)
    if donate > 0:
        tail = tail_rays != 0 and not rk4 and none and bool(ncont)
        r["cont_donate"] = tail_donate if tail else 0
        cgrid = (grid * 4 * donate + 255) // 256
        r["cont_grid"] = cgrid
        r["cont_build"] = ("vern6", "GR", False, 1, 1, False) if (w1 and sch and not rk4 and none) else fn
        if tail:
            maxc2 = cgrid * 4 * r["cont_donate"] + (min(ncont, 2 ** 31 - 1) if grad_ptr else 0)
            waves = ncu * 4 if tail_rays == 1 else tail_rays
            r["tail_grid"] = min(maxc2, waves)
            r["tail"] = r["tail_grid"] > 0
    return r


def test_plan_equals_the_launch_logic_it_replaced():
    rng = random.Random(1769)
    for _ in range(400):
        integ = rng.choice(["vern6", "vern6", "rk4"])
        mode = rng.choice([0, 0, 1, 2]) if integ == "vern6" else rng.choice([0, 1])
        kw = dict(n=rng.choice([1, 63, 512, 1024, 1025, 2048, 65536, 65537, 10 ** 6, 3 * 10 ** 6]), integrator=integ,
                  geom=rng.choice(["FLAT", "GR", "ANY"]), save=int(mode == 1), cyc=int(mode == 2),
                  donate_caller=rng.choice([-1, -1, 0, 16]), donate_device=rng.choice([-1, 0, 16, 63]),
                  graduate_device=rng.choice([-1, -1, 0, 1, 64]), graduate_env=rng.choice([2048, 0, -5, 100]),
                  tail_rays=rng.choice([1, 1, 0, 7, 100000]), tail_donate=rng.choice([1, 4, 63]), w1=rng.choice([0, 1]),
                  nonblocking=rng.choice([0, 1]), hot_at_env=rng.choice([128, 16, 0, -1]), hot_order=rng.choice([0, 1]),
                  ncu=rng.choice([256, 304, 8]), blocks_per_cu=rng.choice([0, 1, 2]))
        st = rng.choice([None, None, 0, 5000])
        if st is not None:
            kw["small_tail"] = st
        got = launchplancheck.plan(**kw)
        args = dict(kw)
        args.pop("small_tail", None)
        per_cu = args.pop("blocks_per_cu")
        want = old_logic(small_tail_limit=st if st is not None else 4 * kw["ncu"], per_cu=per_cu,
                         **{k: (bool(v) if k in ("save", "cyc", "w1", "nonblocking", "hot_order") else v) for k, v in args.items()})
        assert got["bulk_exists"] and got["cont_exists"] and got["tail_exists"], (kw, got)
        for k in ("small_tail", "bulk", "tail", "tail_grid", "cont", "hot", "graduate", "hot_at", "sorted"):
            assert got[k] == want[k], (k, kw, got, want)
        if want["bulk"]:
            assert bulk(got) == want["build"] and got["bulk_grid"] == want["bulk_grid"], (kw, got, want)
        if want["cont"]:
            assert got["cont_donate"] == want["cont_donate"] and got["cont_grid"] == want["cont_grid"], (kw, got, want)
            assert (got["cont_geom"], got["cont_don"], got["cont_wps"]) == (want["cont_build"][1], want["cont_build"][3],
                                                                             want["cont_build"][4]), (kw, got, want)


# ---- completeness ----

# the instantiations the kernel units compile: 30 integrators and 2 tail kernels
BUILDS = (
    [("propagate", "vern6", "FLAT", False, d, 2, False) for d in (0, 1, 3)] + [("propagate", "vern6", "FLAT", False, 0, 1, False)] +
    [("propagate", "vern6", "FLAT", True, d, 2, False) for d in (0, 1)] +
    [("propagate", "rk4", "FLAT", False, d, 2, False) for d in (0, 1)] +
    [("propagate", "vern6", "FLAT", False, d, 2, True) for d in (0, 1)] +
    [("propagate", "vern6", g, True, d, 2, False) for g in ("GR", "ANY") for d in (0, 1)] +
    [("propagate", "rk4", "ANY", s, d, 2, False) for s in (True, False) for d in (0, 1)] +
    [("propagate", "vern6", g, False, d, 2, False) for g in ("GR", "ANY") for d in (0, 1, 3)] +
    [("propagate", "vern6", "GR", False, d, 1, False) for d in (0, 1)] +
    [("propagate", "vern6", g, False, d, 2, True) for g in ("GR", "ANY") for d in (0, 1)] +
    [("tail", g) for g in ("FLAT", "GR")])


def test_instantiation_lists():
    got = launchplancheck.builds()
    assert len(got) == len(set(got)) == 32  # no build listed twice
    assert set(got) == set(BUILDS)


def test_every_plan_names_a_listed_build_and_every_listed_build_is_reached():
    ok, reached, unreached, text = launchplancheck.sweep()
    assert ok, text  # a plan named a combination nobody instantiated (nl_propagate would answer nullptr)
    assert int(text.splitlines()[0].split()[1]) > 400000  # the grid was swept
    assert unreached == [], unreached  # an instantiation nothing reaches: remove it, or say how it is reached
    assert set(reached) == set(launchplancheck.builds()) == set(BUILDS)
