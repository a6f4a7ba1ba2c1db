// art_launch_plan.h -- which kernels one propagate launch runs, as arithmetic that needs no HIP: the
// small-batch tail path, the bulk integrator's instantiation and grid, the packed continuation, the
// tail kernel, graduation and early ("hot") graduation, from the batch, the caller's, the device's
// and the environment's settings and the device's size. propagate_device_impl (art_device.cpp) fills
// the inputs and lays out the scratch from the plan, launch_propagate (art_kernels.hip) launches what
// the plan names, and the plan's record half is what art_last_launch_path reports. The instantiation
// lists below are the only place that says which propagate_kernel / tail_kernel builds exist: the
// kernel units turn them into their lookup functions, tools/launchplancheck.cpp into data. Plain C++
// like art_host_plan.h: that tool compiles it with the host compiler (tests/test_launch_plan.py).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "../../include/art.h"

namespace art {

// The geometry a kernel is instantiated for (the GEOM_* of art_step.h, the same numbers;
// art_kernels.hip checks that they agree).
enum { LP_GEOM_ANY = ART_GEOM_ANY, LP_GEOM_FLAT = ART_GEOM_FLAT, LP_GEOM_GR = ART_GEOM_GR };
constexpr int LP_WPS = 2;        // the integrator's waves per SIMD by default (ART_WAVES_PER_SIMD)
constexpr int LP_BLOCK = 256;    // the integrator's block (BLOCK of art_step.h)
constexpr int LP_HOT_BLOCKS = 32;    // HOT_BLOCKS of art_internal.h
constexpr int64_t LP_HOT_CAP = 1024;  // early-graduation records of one launch (SegOut::hot)

// ---- the instantiation lists: X(integrator, geometry, saveat, DON, waves per SIMD, cyclotron) ----
// flat space, compiled in art_kernels.hip (with MachineLICM)
#define ART_BUILDS_FLAT(X)                                                                             \
  X(ART_VERN6, ART_GEOM_FLAT, false, 0, 2, false) X(ART_VERN6, ART_GEOM_FLAT, false, 1, 2, false)     \
  X(ART_VERN6, ART_GEOM_FLAT, false, 3, 2, false) X(ART_VERN6, ART_GEOM_FLAT, false, 0, 1, false)     \
  X(ART_VERN6, ART_GEOM_FLAT, true, 0, 2, false) X(ART_VERN6, ART_GEOM_FLAT, true, 1, 2, false)       \
  X(ART_RK4, ART_GEOM_FLAT, false, 0, 2, false) X(ART_RK4, ART_GEOM_FLAT, false, 1, 2, false)         \
  X(ART_VERN6, ART_GEOM_FLAT, false, 0, 2, true) X(ART_VERN6, ART_GEOM_FLAT, false, 1, 2, true)
// every other geometry, compiled in art_kernels_nolicm.hip (nl_propagate, nl_propagate_cyc)
#define ART_BUILDS_NL(X)                                                                               \
  X(ART_VERN6, ART_GEOM_GR, true, 0, 2, false) X(ART_VERN6, ART_GEOM_GR, true, 1, 2, false)           \
  X(ART_VERN6, ART_GEOM_ANY, true, 0, 2, false) X(ART_VERN6, ART_GEOM_ANY, true, 1, 2, false)         \
  X(ART_RK4, ART_GEOM_ANY, true, 0, 2, false) X(ART_RK4, ART_GEOM_ANY, true, 1, 2, false)             \
  X(ART_RK4, ART_GEOM_ANY, false, 0, 2, false) X(ART_RK4, ART_GEOM_ANY, false, 1, 2, false)           \
  X(ART_VERN6, ART_GEOM_GR, false, 0, 2, false) X(ART_VERN6, ART_GEOM_GR, false, 1, 2, false)         \
  X(ART_VERN6, ART_GEOM_GR, false, 3, 2, false)                                                       \
  X(ART_VERN6, ART_GEOM_ANY, false, 0, 2, false) X(ART_VERN6, ART_GEOM_ANY, false, 1, 2, false)       \
  X(ART_VERN6, ART_GEOM_ANY, false, 3, 2, false)                                                      \
  X(ART_VERN6, ART_GEOM_GR, false, 0, 1, false) X(ART_VERN6, ART_GEOM_GR, false, 1, 1, false)
#define ART_BUILDS_NL_CYC(X)                                                                           \
  X(ART_VERN6, ART_GEOM_GR, false, 0, 2, true) X(ART_VERN6, ART_GEOM_GR, false, 1, 2, true)           \
  X(ART_VERN6, ART_GEOM_ANY, false, 0, 2, true) X(ART_VERN6, ART_GEOM_ANY, false, 1, 2, true)
// tail_kernel: X(geometry). None for the general geometry: its right-hand side (rhs_photon) keeps
// the backend's cross-statement FMA fusion (ART_FP_FAST), whose choices depend on the site it is inlined
// into, and tail_kernel<GEOM_ANY> did not reproduce propagate_kernel<GEOM_ANY> bit for bit (350 of 512
// boundary-layer rays ended with other step counts; built without that fusion the two agree, DESIGN.md
// "Launch paths"). A launch in the general geometry therefore never leaves the persistent integrator
// and its packed continuation (lp_tail_kernel).
#define ART_BUILDS_TAIL(X) X(ART_GEOM_FLAT) X(ART_GEOM_GR)

// one propagate_kernel instantiation
struct LaunchBuild {
  int integrator, geom;
  bool save;
  int don, wps;
  bool cyc;
};
inline bool operator==(const LaunchBuild& a, const LaunchBuild& b) {
  return a.integrator == b.integrator && a.geom == b.geom && a.save == b.save && a.don == b.don && a.wps == b.wps &&
         a.cyc == b.cyc;
}
inline bool build_exists(const LaunchBuild& b) {
#define ART_LP_HAS(I, G, S, D, W, C) \
  if (b == LaunchBuild{I, G, S, D, W, C}) return true;
  ART_BUILDS_FLAT(ART_LP_HAS) ART_BUILDS_NL(ART_LP_HAS) ART_BUILDS_NL_CYC(ART_LP_HAS)
#undef ART_LP_HAS
  return false;
}

// ---- the inputs of one launch's plan ----
struct LaunchPlanIn {
  int64_t n = 0;
  int integrator = ART_VERN6;
  int geom = LP_GEOM_ANY;  // geom_of the launch's parameters
  bool save = false;       // saveat (ntimes >= 2)
  bool cyc = false;        // the cyclotron observation
  // tail donation: the caller's lanes (LaunchOpts::donate), the device's (art_set_tail_donation); -1: unset
  int donate_caller = -1, donate_device = -1;
  // graduation: the device's attempts (art_set_graduation; -1: unset) and the environment's (ART_GRADUATE, 2048)
  int graduate_device = -1, graduate_env = 2048;
  int tail_rays = 1;    // ART_TAIL: 0 no tail kernel, 1 one wave per SIMD, k: k waves
  int tail_donate = 4;  // ART_TAIL_DONATE: lanes a drained continuation wave hands to the tail kernel
  bool w1 = true;       // ART_W1: the 1-wave/SIMD builds
  bool small_tail_set = false;  // ART_SMALL_TAIL given ...
  int64_t small_tail_max = 0;   // ... and its value (else one ray per SIMD of the device)
  bool nonblocking = false;     // the launch's stream is a non-blocking one (not the null stream)
  int hot_at_env = 128;         // ART_HOT_AT
  bool hot_order = true;        // ART_HOT_ORDER
  int ncu = 0;                  // the device's compute units
  // resident blocks of the bulk kernel per CU (the occupancy query); <= 0: the build's design value
  int blocks_per_cu = 0;
};

// ---- the plan: the record's decisions, and what the two executors need beside them ----
struct LaunchPlan {
  bool small_tail = false;
  int donate = 0;          // first-level donation lanes
  size_t ncont = 0;        // donation records of one level (small tail: one per ray)
  size_t nhot = 0;         // early-graduation records
  bool bulk = false;       // the persistent integrator runs
  LaunchBuild bulk_build{ART_VERN6, LP_GEOM_ANY, false, 0, LP_WPS, false};
  int bulk_grid = 0;
  bool cont = false;       // the packed continuation
  LaunchBuild cont_build{ART_VERN6, LP_GEOM_ANY, false, 0, LP_WPS, false};
  int cont_grid = 0;
  int cont_donate = 0;     // its own donation lanes (the second level)
  bool tail = false;       // tail_kernel is launched (after the continuation, or alone for a small batch)
  int tail_geom = LP_GEOM_ANY;
  int tail_grid = 0, tail_waves = 0;
  bool grad_records = false;  // SegOut::grad is laid out and handed to the kernels
  int graduate = 0;           // the effective graduate threshold (0: off)
  int grad_cap = 0;
  bool hot_records = false;   // SegOut::hot_ready ... are laid out (the side stream exists)
  bool hot = false;           // the hot side launch runs
  int hot_at = 0;             // the effective hot_at (0: off)
  int hot_cap = 0;
  bool sorted = false;        // the bulk pass claims its rays in sorted order
};

// tail_kernel serves Vern6 without saveat or the cyclotron observation, in flat space and Schwarzschild
// (ART_BUILDS_TAIL): the small-batch path, second-level donation, graduation and the hot side launch need it.
inline bool lp_tail_kernel(const LaunchPlanIn& in) {
  return !in.save && !in.cyc && in.integrator == ART_VERN6 && in.geom != LP_GEOM_ANY;
}
// A small batch that tail_kernel serves runs every ray on a wave of its own.
inline int64_t lp_small_tail_limit(const LaunchPlanIn& in) { return in.small_tail_set ? in.small_tail_max : (int64_t)in.ncu * 4; }
inline bool lp_small_tail(const LaunchPlanIn& in) {
  return lp_tail_kernel(in) && in.n <= lp_small_tail_limit(in);
}
// Tail donation: the caller's choice, else the device's setting, else by geometry (16 lanes for a
// Schwarzschild Vern6 batch without saveat or the cyclotron observation, 0 otherwise).
inline int lp_donate(const LaunchPlanIn& in) {
  if (in.donate_caller >= 0) return in.donate_caller;
  if (in.donate_device >= 0) return in.donate_device;
  return (in.geom == LP_GEOM_GR && in.integrator == ART_VERN6 && !in.save && !in.cyc) ? 16 : 0;
}
// donation records of one level: at most (resident waves) x donate; a small-tail batch: one per ray
inline size_t lp_ncont(int64_t n, int ncu, int donate, bool small_tail) {
  if (small_tail) return (size_t)n;
  return donate > 0 ? std::min((size_t)n, (size_t)ncu * 32 * (size_t)donate) : 0;
}
inline size_t lp_nhot(size_t ncont, bool small_tail) { return small_tail ? 0 : std::min(ncont, (size_t)LP_HOT_CAP); }

// the bulk integrator's instantiation for a launch that donates `donate` lanes
inline LaunchBuild lp_bulk_build(const LaunchPlanIn& in, int donate, bool* w1_out) {
  const bool rk4 = in.integrator == ART_RK4, flat = in.geom == LP_GEOM_FLAT, sch = in.geom == LP_GEOM_GR;
  const bool plain = !in.save && !in.cyc;
  const int don = donate > 0 ? 1 : 0;
  LaunchBuild b;
  if (in.cyc)  // (Vern6 without saveat: the entry points refuse the rest)
    b = LaunchBuild{ART_VERN6, flat ? LP_GEOM_FLAT : (sch ? LP_GEOM_GR : LP_GEOM_ANY), false, don, LP_WPS, true};
  else if (flat && !(in.save && rk4))
    b = LaunchBuild{rk4 ? ART_RK4 : ART_VERN6, LP_GEOM_FLAT, in.save, don, LP_WPS, false};
  else  // (RK4 has the general geometry's builds only, flat RK4 with saveat among them)
    b = LaunchBuild{rk4 ? ART_RK4 : ART_VERN6, (!rk4 && sch) ? LP_GEOM_GR : LP_GEOM_ANY, in.save, don, LP_WPS, false};
  // a batch that fits one ray per lane of 1 wave per SIMD runs the 1-wave/SIMD build (no spills)
  *w1_out = in.w1 && donate <= 0 && plain && !rk4 && (flat || sch) && in.n <= (int64_t)in.ncu * 4 * 64;
  if (*w1_out) b = LaunchBuild{ART_VERN6, flat ? LP_GEOM_FLAT : LP_GEOM_GR, false, 0, 1, false};
  return b;
}

inline LaunchPlan plan_launch(const LaunchPlanIn& in) {
  LaunchPlan P;
  const bool rk4 = in.integrator == ART_RK4, sch = in.geom == LP_GEOM_GR;
  const bool plain = !in.save && !in.cyc;
  P.small_tail = lp_small_tail(in);
  P.donate = P.small_tail ? 0 : lp_donate(in);
  P.ncont = lp_ncont(in.n, in.ncu, P.donate, P.small_tail);
  P.nhot = lp_nhot(P.ncont, P.small_tail);
  P.tail_geom = in.geom;
  if (P.small_tail) {  // pack_fresh_kernel, then tail_kernel alone
    P.tail = true;
    P.tail_waves = (int)std::min(in.n, (int64_t)in.ncu * 4);
    P.tail_grid = P.tail_waves;
    return P;
  }
  // the tail kernel after the continuation: second-level donation, graduation and the hot side launch need it
  const bool tail_on = P.donate > 0 && P.ncont > 0 && in.tail_rays != 0 && lp_tail_kernel(in);
  const bool grad_laid = P.ncont > 0 && lp_tail_kernel(in);  // (the records' place in the scratch)
  const int grad_setting = grad_laid ? (in.graduate_device >= 0 ? in.graduate_device : std::max(0, in.graduate_env)) : 0;
  P.grad_records = grad_laid && tail_on;
  P.graduate = P.grad_records ? grad_setting : 0;
  P.grad_cap = grad_laid ? (int)std::min(P.ncont, (size_t)INT32_MAX) : 0;
  // early graduation: with graduation only, and with the side stream, which a blocking stream cannot have
  P.hot_records = P.nhot > 0 && grad_setting > 0 && in.nonblocking;
  P.hot_cap = P.hot_records ? (int)P.nhot : 0;
  const int hot_at = P.hot_records ? std::max(0, in.hot_at_env) : 0;
  P.hot = P.graduate > 0 && P.hot_records && hot_at > 0;
  P.hot_at = P.hot ? hot_at : 0;
  P.sorted = P.hot && in.hot_order && in.n > 0 && in.n < INT32_MAX;

  bool w1 = false;
  P.bulk = true;
  P.bulk_build = lp_bulk_build(in, P.donate, &w1);
  // (the integrator's blocks per CU by design: its waves per SIMD, 4 waves a block)
  const int per_cu = in.blocks_per_cu > 0 ? in.blocks_per_cu : (w1 ? 1 : LP_WPS * 4 / (LP_BLOCK / 64));
  const int64_t need = (in.n + LP_BLOCK - 1) / LP_BLOCK, full = (int64_t)in.ncu * per_cu;
  int grid = (int)std::min(need, full);
  // the hot rays' launch takes HOT_BLOCKS block slots beside the bulk pass
  if (P.hot) grid = grid > 2 * LP_HOT_BLOCKS ? grid - LP_HOT_BLOCKS : grid;
  P.bulk_grid = grid;
  if (P.donate > 0) {
    P.cont = true;
    // GR continuations at 1 wave/SIMD (no spills); every other one is the bulk build again
    P.cont_build = (in.w1 && sch && !rk4 && plain) ? LaunchBuild{ART_VERN6, LP_GEOM_GR, false, 1, 1, false} : P.bulk_build;
    P.cont_donate = tail_on ? in.tail_donate : 0;
    const int64_t maxc = (int64_t)grid * (LP_BLOCK / 64) * P.donate;
    P.cont_grid = (int)((maxc + LP_BLOCK - 1) / LP_BLOCK);
    if (tail_on) {
      const int64_t maxc2 = (int64_t)P.cont_grid * (LP_BLOCK / 64) * P.cont_donate + (P.grad_records ? (int64_t)P.grad_cap : 0);
      P.tail_waves = in.tail_rays == 1 ? in.ncu * 4 : in.tail_rays;
      P.tail_grid = (int)std::min(maxc2, (int64_t)P.tail_waves);
      P.tail = P.tail_grid > 0;
    }
  }
  return P;
}

// The streamed host call's integrator: DON = 3, at most `blocks` persistent blocks.
inline LaunchPlan plan_streamed(int64_t n, int geom, int blocks) {
  LaunchPlan P;
  P.bulk = true;
  P.bulk_build = LaunchBuild{ART_VERN6, geom, false, 3, LP_WPS, false};
  P.bulk_grid = (int)std::min((n + LP_BLOCK - 1) / LP_BLOCK, (int64_t)blocks);
  P.tail_geom = geom;
  return P;
}

// The record's decision half (art_launch_path of include/art.h) from a plan; the counts stay zero.
inline art_launch_path plan_record(const LaunchPlan& P, bool streamed) {
  art_launch_path r{};
  r.launches = 1;
  r.streamed = streamed ? 1 : 0;
  r.small_tail = P.small_tail ? 1 : 0;
  r.bulk = P.bulk ? 1 : 0;
  r.integrator = P.bulk_build.integrator;
  r.geom = P.bulk ? P.bulk_build.geom : P.tail_geom;
  r.save = P.bulk_build.save ? 1 : 0;
  r.don = P.bulk ? P.bulk_build.don : 0;
  r.wps = P.bulk ? P.bulk_build.wps : 0;
  r.cyc = P.bulk_build.cyc ? 1 : 0;
  r.bulk_grid = P.bulk_grid;
  r.cont = P.cont ? 1 : 0;
  r.cont_wps = P.cont ? P.cont_build.wps : 0;
  r.cont_donate = P.cont ? P.cont_donate : 0;
  r.tail = P.tail ? 1 : 0;
  r.tail_geom = P.tail_geom;
  r.tail_grid = P.tail ? P.tail_grid : 0;
  r.hot = P.hot ? 1 : 0;
  r.sorted = P.sorted ? 1 : 0;
  r.graduate = P.graduate;
  r.hot_at = P.hot_at;
  r.donate = P.donate;
  return r;
}

}  // namespace art
