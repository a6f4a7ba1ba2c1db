"""What the last propagate launch ran (raytracer.last_launch_path), for the GPU tests that compare a
launch with a policy on against one with it off: each asserts the kernels both sides ran, so the
comparison cannot hold because the policy silently stayed off."""


def last():
    import adiabatic_raytracer_amd as A
    return A.raytracer.last_launch_path()


def build(rec):
    """the bulk integrator's instantiation: (integrator, geom, saveat, DON, waves per SIMD, cyclotron); None without one"""
    if not rec["bulk"]:
        return None
    return (rec["integrator"], rec["geom"], rec["save"], rec["don"], rec["wps"], rec["cyc"])


def expect(rec, what, build_is=None, **fields):
    """the record's bulk build and the given fields; prints the record's non-zero fields first"""
    print(what, {k: v for k, v in rec.items() if v not in (0, False)})
    if build_is is not None:
        assert build(rec) == build_is, (what, build(rec), build_is, rec)
    for k, v in fields.items():
        assert rec[k] == v, (what, k, rec[k], v, rec)
    return rec


def persistent(rec, what, **fields):
    """a launch of the persistent integrator alone or first: no small-batch tail path, not the streamed call"""
    return expect(rec, what, small_tail=False, bulk=True, streamed=False, **fields)


def small_tail(rec, what, n):
    """every ray on a wave of its own: tail_kernel alone"""
    return expect(rec, what, small_tail=True, bulk=False, cont=False, tail=True, hot=False, donated=n)
