"""ctypes binding of libart.so (include/art.h). Fails loudly when the library is missing:
there is no CPU fallback anywhere in the product path."""
import ctypes as C
import os

from .build import LIB

ART_VERN6, ART_RK4 = 0, 1
ART_AXION, ART_PHOTON = 0, 1
STATUS_NAMES = {0: "Success", 1: "Terminated(crossing)", 2: "Terminated(hit NS)", 3: "MaxIters", 4: "NonFinite"}


class ArtParams(C.Structure):
    _fields_ = [
        ("theta_m", C.c_double), ("omega_pul", C.c_double), ("B0", C.c_double), ("rNS", C.c_double),
        ("mass_ns", C.c_double), ("mass_a", C.c_double), ("g_agg", C.c_double), ("bndry_lyr", C.c_double),
        ("ln_t_end", C.c_double), ("abstol", C.c_double), ("reltol", C.c_double), ("dtmin", C.c_double),
        ("maxiters", C.c_int64), ("flat", C.c_int32), ("isotropic", C.c_int32), ("melrose", C.c_int32),
        ("integrator", C.c_int32), ("n_fixed", C.c_int32), ("interp_points", C.c_int32),
    ]


class SegmentOut(C.Structure):
    _fields_ = [("x_end", C.c_void_p), ("k_end", C.c_void_p), ("u7_end", C.c_void_p), ("tau_end", C.c_void_p),
                ("status", C.c_void_p), ("n_accept", C.c_void_p), ("n_reject", C.c_void_p)]


class CrossingBuf(C.Structure):
    _fields_ = [("capacity", C.c_int32), ("count", C.c_void_p), ("pos", C.c_void_p), ("k", C.c_void_p),
                ("t", C.c_void_p), ("dw", C.c_void_p), ("p_nonad", C.c_void_p)]


class CyclotronOut(C.Structure):  # include/art.h art_cyclotron_out
    _fields_ = [("tau", C.c_void_p), ("count", C.c_void_p), ("pos", C.c_void_p), ("ln_t", C.c_void_p)]


LAUNCH_PATH_DECISIONS = ("launches", "streamed", "small_tail", "bulk", "integrator", "geom", "save", "don", "wps", "cyc",
                         "bulk_grid", "donate", "cont", "cont_wps", "cont_donate", "tail", "tail_geom", "tail_grid", "hot",
                         "sorted", "graduate", "hot_at")
LAUNCH_PATH_COUNTS = ("donated", "donated2", "grad_count", "grad_cap", "hot_count", "hot_cap", "hot_claimed")


class LaunchPath(C.Structure):  # include/art.h art_launch_path
    _fields_ = [(k, C.c_int32) for k in LAUNCH_PATH_DECISIONS] + [(k, C.c_uint64) for k in LAUNCH_PATH_COUNTS]


class SkySpec(C.Structure):  # include/art.h art_sky_spec
    _fields_ = [("n_theta", C.c_int32), ("n_phi", C.c_int32), ("n_dw", C.c_int32), ("theta_axis", C.c_int32),
                ("mode", C.c_int32), ("dw_lo", C.c_double), ("dw_hi", C.c_double)]


class EventRowsIn(C.Structure):  # include/art.h art_event_rows_in
    _fields_ = [("n_events", C.c_int64), ("event_offset", C.c_int64), ("x", C.c_void_p), ("k_init", C.c_void_p),
                ("attempts", C.c_void_p), ("weight5", C.c_void_p), ("back", C.c_void_p), ("back_counts", C.c_void_p),
                ("nodes", C.c_void_p), ("n_nodes", C.c_int64), ("counts", C.c_void_p), ("infos", C.c_void_p),
                ("cyc_slot", C.c_void_p), ("cyc_n", C.c_int64), ("cyc_tau", C.c_void_p),
                ("cyc_end", C.POINTER(SegmentOut))]


class EventRowsOut(C.Structure):  # include/art.h art_event_rows_out
    _fields_ = [("ncols", C.c_int32), ("nbins", C.c_int32), ("rows", C.c_void_p), ("row_capacity", C.c_int64),
                ("flux", C.c_void_p), ("sky", C.POINTER(SkySpec)), ("sky_hist", C.c_void_p), ("bin_out", C.c_void_p),
                ("totals", C.c_void_p)]


class EventMomentsOut(C.Structure):  # include/art.h art_event_moments_out
    _fields_ = [("nbins", C.c_int32), ("reserved", C.c_int32), ("flux_sq", C.c_void_p), ("flux_xa", C.c_void_p),
                ("sky", C.POINTER(SkySpec)), ("sky_sq", C.c_void_p), ("sky_xa", C.c_void_p), ("totals", C.c_void_p)]


class EventReweightOut(C.Structure):  # include/art.h art_event_reweight_out
    _fields_ = [("erg", C.c_void_p), ("nbins", C.c_int32), ("reserved", C.c_int32), ("flux", C.c_void_p),
                ("sky", C.POINTER(SkySpec)), ("sky_hist", C.c_void_p), ("totals", C.c_void_p), ("weights", C.c_void_p),
                ("back", C.c_void_p), ("back_prob", C.c_void_p), ("flux_sq", C.c_void_p), ("flux_xa", C.c_void_p), ("sky_sq", C.c_void_p),
                ("sky_xa", C.c_void_p), ("moment_totals", C.c_void_p)]


class ArtHalo(C.Structure):  # include/art.h art_halo
    _fields_ = [("v0", C.c_double), ("v_ns", C.c_double * 3), ("v_prop", C.c_double)]


class EventHaloScanOut(C.Structure):  # include/art.h art_event_halo_scan_out
    _fields_ = [("vifty", C.c_void_p), ("nbins", C.c_int32), ("reserved", C.c_int32), ("flux", C.c_void_p),
                ("sky", C.POINTER(SkySpec)), ("sky_hist", C.c_void_p), ("totals", C.c_void_p), ("ratio", C.c_void_p),
                ("flux_sq", C.c_void_p), ("flux_xa", C.c_void_p), ("sky_sq", C.c_void_p), ("sky_xa", C.c_void_p),
                ("moment_totals", C.c_void_p)]


class EventReplicatesOut(C.Structure):  # include/art.h art_event_replicates_out
    _fields_ = [("n_groups", C.c_int32), ("kind", C.c_int32), ("n_sets", C.c_int32), ("nbins", C.c_int32),
                ("node_factor", C.c_void_p), ("event_factor", C.c_void_p), ("flux", C.c_void_p),
                ("sky", C.POINTER(SkySpec)), ("sky_hist", C.c_void_p), ("totals", C.c_void_p), ("groups", C.c_void_p)]


# art_event_replicates_out::groups, per group; its kinds; the range of its group count
REPLICATE_GROUPS = ("events", "a", "misplaced")
REPLICATE_KINDS = {"run": 0, "coupling": 1, "halo": 2}
REPLICATES_MIN_GROUPS, REPLICATES_MAX_GROUPS = 2, 64

class EventGridOut(C.Structure):  # include/art.h art_event_grid_out
    _fields_ = [("n_couplings", C.c_int32), ("n_models", C.c_int32), ("nbins", C.c_int32), ("n_groups", C.c_int32),
                ("node_factor", C.c_void_p), ("back", C.c_void_p), ("ratio", C.c_void_p), ("flux", C.c_void_p),
                ("totals", C.c_void_p), ("flux_rep", C.c_void_p), ("totals_rep", C.c_void_p), ("groups", C.c_void_p),
                ("moment_totals", C.c_void_p)]


# art_event_grid_out::totals, per cell; the limits of its two axes
GRID_TOTALS = ("sum_axion", "sum_photon", "misplaced")
GRID_MAX_COUPLINGS, GRID_MAX_MODELS = 32, 32

class EventSpectrumOut(C.Structure):  # include/art.h art_event_spectrum_out
    _fields_ = [("kind", C.c_int32), ("n_sets", C.c_int32), ("sub_bits", C.c_int32), ("top", C.c_int32),
                ("node_factor", C.c_void_p), ("event_factor", C.c_void_p), ("count", C.c_void_p), ("sum", C.c_void_p),
                ("sum_sq", C.c_void_p), ("totals", C.c_void_p), ("top_power", C.c_void_p), ("top_event", C.c_void_p)]


# art_event_spectrum_out::totals, per set and species; the limits of its bin rule and its list
SPECTRUM_TOTALS = ("events", "positive", "zeros", "bad", "sum", "sum_sq", "misplaced", "reserved")
SPECTRUM_MAX_SUB_BITS, SPECTRUM_MAX_TOP = 4, 256

class EventExactOut(C.Structure):  # include/art.h art_event_exact_out
    _fields_ = [("kind", C.c_int32), ("n_sets", C.c_int32), ("nbins", C.c_int32), ("mode", C.c_int32),
                ("node_factor", C.c_void_p), ("event_factor", C.c_void_p), ("flux_acc", C.c_void_p),
                ("sky", C.POINTER(SkySpec)), ("sky_acc", C.c_void_p), ("totals_acc", C.c_void_p),
                ("nonfinite", C.c_void_p), ("misplaced", C.c_void_p)]


# the exact tables: ART_EXACT_LIMBS, the modes of their accumulation paths, the bins the LDS paths hold
EXACT_LIMBS = 66
EXACT_MODES = {"auto": 0, "lds": 1, "global": 2}
EXACT_LDS_BINS, EXACT_LDS_FLUX_BINS = 124, 56

class OriginSpec(C.Structure):  # include/art.h art_origin_spec
    _fields_ = [("n_r", C.c_int32), ("n_theta", C.c_int32), ("n_phi", C.c_int32), ("theta_axis", C.c_int32),
                ("mode", C.c_int32), ("r_lo", C.c_double), ("r_hi", C.c_double), ("cm", C.c_double), ("sm", C.c_double)]


class EventOriginOut(C.Structure):  # include/art.h art_event_origin_out
    _fields_ = [("origin", C.POINTER(OriginSpec)), ("observer", C.POINTER(SkySpec)), ("groups", C.c_int32),
                ("hist", C.c_void_p), ("bin_out", C.c_void_p), ("power_out", C.c_void_p), ("misplaced", C.c_void_p)]


# the emission maps: the modes of art_origin_spec, the doubles a block-private table may hold
ORIGIN_MODES = {"auto": 0, "lds": 1, "global": 2}
ORIGIN_LDS_DOUBLES = 8192

EVENT_TOTALS = ("rows", "photon_rows", "sum_axion", "sum_photon", "attempts_minus_1", "cyclotron_mismatches")
# art_event_moments_out::totals
MOMENT_TOTALS = ("events", "A1", "A2", "Q_axion", "Q_photon", "C_axion", "C_photon", "bad_nodes")
# art_event_reweight_out::totals, per coupling
REWEIGHT_TOTALS = ("sum_axion", "sum_photon", "coverage", "saturated", "unlinked", "recomputed_differs")
REWEIGHT_MAX_COUPLINGS = 32
# art_event_halo_scan_out::totals, per model
HALO_SCAN_TOTALS = ("sum_axion", "sum_photon", "ratio_sum", "ratio_sq", "misplaced")
HALO_SCAN_MAX_MODELS = 32


# name -> (restype, argtypes); the test suite checks this table against include/art.h
class TreeOpts(C.Structure):  # include/art.h art_tree_opts
    _fields_ = [("num_cutoff", C.c_int32), ("mc_nodes", C.c_int32), ("max_nodes", C.c_int32),
                ("splittings_cutoff", C.c_int32), ("crossing_cap", C.c_int32), ("tree_offset", C.c_int32),
                ("prob_cutoff", C.c_double), ("seed", C.c_uint64)]


class TreeTraj(C.Structure):  # include/art.h art_tree_traj
    _fields_ = [("ntimes", C.c_int32), ("crossing_cap", C.c_int32), ("traj", C.c_void_p), ("times", C.c_void_p),
                ("count", C.c_void_p), ("xc", C.c_void_p)]


_P = C.POINTER(ArtParams)
_v = C.c_void_p
_i64, _i32, _d, _u64 = C.c_int64, C.c_int32, C.c_double, C.c_uint64
_H = C.POINTER(ArtHalo)
SIGNATURES = {
    "art_abi_version": (C.c_int, []),
    "art_last_error": (C.c_char_p, []),
    "art_device_count": (C.c_int, [C.POINTER(C.c_int32)]),
    "art_set_device": (C.c_int, [_i32]),
    "art_synchronize": (C.c_int, []),
    "art_shutdown": (C.c_int, []),
    "art_last_kernel_ms": (C.c_double, []),
    "art_last_stats": (C.c_int, [C.POINTER(C.c_uint64), C.POINTER(C.c_int32)]),
    "art_last_launch_path": (C.c_int, [C.POINTER(LaunchPath)]),
    "art_vern6_tableau": (C.c_int, [_v, _v, _v, _v]),
    "art_find_conversion_surface": (C.c_double, [_P]),
    "art_propagate_host": (C.c_int, [_P, _i64, _v, _v, _v, _v, _v, _v, _i32, C.POINTER(SegmentOut),
                                     C.POINTER(CrossingBuf)]),
    "art_propagate_device": (C.c_int, [_P, _i64, _v, _v, _v, _v, _v, _v, _i32, C.POINTER(SegmentOut),
                                       C.POINTER(CrossingBuf), _v]),
    "art_propagate_host_flux": (C.c_int, [_P, _i64, _v, _v, _v, _v, _v, _v, _i32, C.POINTER(SegmentOut),
                                          C.POINTER(CrossingBuf), _i32, _v]),
    "art_propagate_host_flux_async": (C.c_int, [_P, _i64, _v, _v, _v, _v, _v, _v, _i32, C.POINTER(SegmentOut),
                                                C.POINTER(CrossingBuf), _i32, _v, C.POINTER(C.c_int64)]),
    "art_host_wait": (C.c_int, [C.c_int64]),
    "art_host_path_counters": (C.c_int, [_v, _i32, _i32]),
    "art_propagate_traj_host": (C.c_int, [_P, _i64, _v, _v, _v, _v, _v, _v, _i32, C.POINTER(SegmentOut),
                                          C.POINTER(CrossingBuf), _i32, _v, _v, _v]),
    "art_propagate_traj_device": (C.c_int, [_P, _i64, _v, _v, _v, _v, _v, _v, _i32, C.POINTER(SegmentOut),
                                            C.POINTER(CrossingBuf), _i32, _v, _v, _v, _v]),
    "art_get_prob_nonad_host": (C.c_int, [_P, _i64, _v, _v, _v, _i64, _v, _v]),
    "art_get_prob_nonad_device": (C.c_int, [_P, _i64, _v, _v, _v, _i64, _v, _v, _v]),
    "art_sample_conversion_points_host": (C.c_int, [_P, _d, _u64, _i64, _i64, _v, _v, _v, _v, _v, _v]),
    "art_sample_conversion_points_device": (C.c_int, [_P, _d, _u64, _i64, _i64, _v, _v, _v, _v, _v, _v, _v]),
    "art_sample_conversion_points_halo_host": (C.c_int, [_P, _H, _d, _u64, _i64, _i64, _v, _v, _v, _v, _v, _v]),
    "art_sample_conversion_points_halo_device": (C.c_int, [_P, _H, _d, _u64, _i64, _i64, _v, _v, _v, _v, _v, _v, _v]),
    "art_flux_histogram_device": (C.c_int, [_P, _i64, _v, _v, _v, _v, _v, _i32, _v, _v]),
    "art_grow_trees": (C.c_int, [_P, _i64, _v, _v, _v, _v, C.POINTER(TreeOpts), _i64, _v, C.POINTER(_i64), _v, _v]),
    "art_grow_trees_traj": (C.c_int, [_P, _i64, _v, _v, _v, _v, C.POINTER(TreeOpts), _i64, _v, C.POINTER(_i64), _v,
                                      _v, C.POINTER(TreeTraj)]),
    "art_grow_trees_device": (C.c_int, [_P, _i64, _v, _v, _v, _v, C.POINTER(TreeOpts), _i64, _v, _v, _v, _v,
                                        C.POINTER(_i64), _v]),
    "art_event_weight_host": (C.c_int, [_P, _d, _d, _d, _i64, _v, _v, _v, _v]),
    "art_event_weight_device": (C.c_int, [_P, _d, _d, _d, _i64, _v, _v, _v, _v, _v]),
    "art_event_weight_halo_host": (C.c_int, [_P, _H, _d, _d, _d, _i64, _v, _v, _v, _v]),
    "art_event_weight_halo_device": (C.c_int, [_P, _H, _d, _d, _d, _i64, _v, _v, _v, _v, _v]),
    "art_recent_kernel_ms": (C.c_int, [_i32, _v]),
    "art_recent_kernel_span_ms": (C.c_int, [_i32, _v]),
    "art_set_tail_donation": (C.c_int, [_i32]),
    "art_set_graduation": (C.c_int, [_i32]),
    "art_set_sampler_waves": (C.c_int, [_i32]),
    "art_flux_histogram_phi_device": (C.c_int, [_i64, _v, _v, _v, _i32, _v, _v]),
    "art_flux_histogram_phi_range_device": (C.c_int, [_i64, _v, _v, _v, _i32, _d, _d, _v, _v]),
    "art_histogram3_device": (C.c_int, [_i64, _v, _v, _v, _v, _v, C.POINTER(_i32), C.POINTER(_d), C.POINTER(_d), _i32, _v,
                                        _v]),
    "art_sky_map_segments_device": (C.c_int, [_P, C.POINTER(SkySpec), _i64, _v, _v, _v, _v, _v, _v, _v, _v, _v, _v]),
    "art_event_rows_device": (C.c_int, [_P, C.POINTER(EventRowsIn), C.POINTER(EventRowsOut), _v]),
    "art_event_gather_photons_device": (C.c_int, [_P, _i64, _v, _i64, _v, _i64, _v, _v, _v, _v, _v, _v, _v,
                                                  C.POINTER(_i64), _v]),
    "art_event_moments_device": (C.c_int, [_P, C.POINTER(EventRowsIn), _v, C.POINTER(EventMomentsOut), _v]),
    "art_event_reweight_device": (C.c_int, [_P, C.POINTER(EventRowsIn), _v, C.POINTER(TreeOpts), _i32, C.POINTER(_d),
                                            C.POINTER(EventReweightOut), _v]),
    "art_event_halo_scan_device": (C.c_int, [_P, C.POINTER(EventRowsIn), _v, _H, _i32, _H, C.POINTER(EventHaloScanOut), _v]),
    "art_event_replicates_device": (C.c_int, [_P, C.POINTER(EventRowsIn), _v, C.POINTER(EventReplicatesOut), _v]),
    "art_event_grid_device": (C.c_int, [_P, C.POINTER(EventRowsIn), _v, C.POINTER(EventGridOut), _v]),
    "art_event_spectrum_device": (C.c_int, [_P, C.POINTER(EventRowsIn), _v, C.POINTER(EventSpectrumOut), _v]),
    "art_exact_histogram_device": (C.c_int, [_i64, _v, _v, _i32, _v, _v, _i32, _v]),
    "art_exact_finish_device": (C.c_int, [_i64, _v, _v, _v]),
    "art_exact_add_host": (C.c_int, [_i64, _v, _v, _i32, _v, _v]),
    "art_exact_normalize_host": (C.c_int, [_i64, _v]),
    "art_exact_round_host": (C.c_int, [_i64, _v, _v]),
    "art_event_exact_device": (C.c_int, [_P, C.POINTER(EventRowsIn), _v, C.POINTER(EventExactOut), _v]),
    "art_event_origin_device": (C.c_int, [_P, C.POINTER(EventRowsIn), _v, C.POINTER(EventOriginOut), _v]),
    "art_comm_unique_id": (C.c_int, [_v]),
    "art_comm_init": (C.c_int, [_i32, _i32, _v]),
    "art_flux_allreduce": (C.c_int, [_v, _i64, _v]),
    "art_flux_allreduce_host": (C.c_int, [_v, _i64]),
    "art_comm_destroy": (C.c_int, []),
    "art_eval_rhs_device": (C.c_int, [_P, _i64, _v, _v, _v, _v, _v, _v]),
    "art_eval_hamiltonian_device": (C.c_int, [_P, _i64, _v, _v, _v, _v, _v, _v, _v, _v, _v]),
    "art_eval_condition_device": (C.c_int, [_P, _i64, _v, _v, _v, _v]),
    "art_propagate_cyclotron_host": (C.c_int, [_P, _i64, _v, _v, _v, _v, _v, _v, _i32, C.POINTER(SegmentOut),
                                               C.POINTER(CrossingBuf), C.POINTER(CyclotronOut)]),
    "art_propagate_cyclotron_device": (C.c_int, [_P, _i64, _v, _v, _v, _v, _v, _v, _i32, C.POINTER(SegmentOut),
                                                 C.POINTER(CrossingBuf), C.POINTER(CyclotronOut), _v]),
    "art_eval_cyclotron_device": (C.c_int, [_P, _i64, _v, _v, _v, _v, _v, _v]),
    "art_eval_math_device": (C.c_int, [_i32, _i32, _i64, _v, _v, _v, _v, _v]),
}
# include/art.h ART_MATH_*: the function ids of art_eval_math_device
MATH_FN = {"SINCOS": 0, "EXP": 1, "LOG": 2, "RCP": 3, "POW120": 4, "MAX_ABS": 5, "MIN_Q": 6, "MAX_Q": 7, "RCLAMP": 8}

# the sky maps' θ axis (art_sky_spec.theta_axis) and its range
THETA_AXIS = {"theta": 0, "cos": 1}

_lib = None


class ArtError(RuntimeError):
    pass


def load(path=None):
    """Load libart.so; raise if it is absent (build it with `python -m adiabatic_raytracer_amd.build`)."""
    global _lib
    if _lib is not None:
        return _lib
    path = path or os.environ.get("ART_LIB", LIB)
    if not os.path.exists(path):
        raise ArtError(f"libart.so not found at {path}: the HIP engine must be built "
                       f"(python -m adiabatic_raytracer_amd.build); there is no CPU fallback")
    # PyTorch ships its own HIP runtime under the same soname (libamdhip64.so.7). Whichever is
    # loaded first serves the whole process; torch refuses a foreign one ("No HIP GPUs are
    # available"), so when torch is present it is imported first and libart binds to torch's.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = C.CDLL(path)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(rc):
    if rc != 0:
        raise ArtError(f"libart error {rc}: {load().art_last_error().decode()}")
    return rc
