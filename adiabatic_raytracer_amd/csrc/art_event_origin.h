// art_event_origin.h -- the emission maps (art_event_origin_device): the power of a chunk's final rows binned over
// WHERE their event converted, the sampled point of columns 9 to 11, and optionally jointly over the direction the
// row left in,
//   hist[species][obs_theta][obs_phi][r][origin_theta][origin_phi]     (C order; [group] in front with groups = R).
// The origin's coordinates are written once, below, as __host__ __device__ functions: event_origin_kernel and a
// host build for the CPU tests (tools/eventorigin.cpp) compile the same source, as with art_event_rows.h.
//
// THE ORIGIN BIN. (x, y, z) is the event's sampled point, EventLoad::x. It is turned about y,
//   v = (x cm - z sm, y, x sm + z cm),
// with cm, sm the caller's: (cos θm, sin θm) makes the magnetic axis (sin θm, 0, cos θm) the pole, (1, 0) leaves
// v = (x, y, z). No contraction: two rounded products and one rounded add or subtract, as numpy rounds
// rows[:, 9] * cm - rows[:, 11] * sm. Then (θ, φ, r) = event_angles(v), cos θ = v_z / r, and every axis goes through
// np_hist_bin over its closed range: cos θ over [-1, 1] or θ over [0, π], φ over [-π, π], r over [r_lo, r_hi] --
// or, r_all, one bin that holds every finite r (sky_bin_of's c_all rule). A NaN, or a value outside a range on any
// axis, gives -1: the row is dropped from this table only.
#pragma once
#include "art_core.h"
#include "art_event_rows.h"
#include "art_internal.h"  // OriginAxes, beside SkyAxes
#include "art_ray_io.h"    // np_hist_bin

namespace art {

// the flat origin bin (ir n_theta + iθ) n_phi + iφ of the point (x, y, z), -1 for none
__host__ __device__ inline int origin_bin_of(const OriginAxes& O, double x, double y, double z) {
#pragma clang fp contract(off)
  const double xc = x * O.cm, zs = z * O.sm, xs = x * O.sm, zc = z * O.cm;
  const double v[3] = {xc - zs, y, xs + zc};
  double theta, phi, r;
  event_angles(v, theta, phi, r);
  const int ia = O.theta_axis ? np_hist_bin(v[2] / r, O.n[1], -1.0, 1.0) : np_hist_bin(theta, O.n[1], 0.0, PI);
  const int ib = np_hist_bin(phi, O.n[2]);
  const int ir = O.r_all ? ((r - r == 0.0) ? 0 : -1) : np_hist_bin(r, O.n[0], O.r_lo, O.r_hi);
  if ((ia | ib | ir) < 0) return -1;
  return (ir * O.n[1] + ia) * O.n[2] + ib;
}

}  // namespace art

#ifdef ART_EVENT_KERNELS
namespace art {

// One lane per node record (sky_accumulate's grid-stride loop over n_nodes). A record is taken through event_record:
// a final one of its own range gives its power and its observer bin sb, the sky map's ((species, θf, φf) of the
// caller's SkyAxes with c_all), and its event's point gives the origin bin ob; the row goes to bin
// sb n_origin + ob of its group's table (group replicate_group(event_offset + tree, R) with n_groups = R > 0).
// bin_out / power_out (may be null): per record, that bin without the group (-1: not counted) and the power (0
// where not final). Misplaced records are skipped and counted, summed per lane, then per wave.
// LDS: the whole (R-fold) table block-private, of lds_table doubles.
template <bool LDS>
__global__ __launch_bounds__(256) void event_origin_kernel(const EventRowsArgs a, const EventOriginArgs r, const SkyAxes A,
                                                             const int cos_axis, const OriginAxes O, const int lds_table) {
  extern __shared__ __attribute__((aligned(16))) double sh[];
  double misplaced = 0.0;
  sky_accumulate<LDS>(a.n_nodes, LDS ? lds_table : 0, r.hist, sh, [&](int64_t i, double& v) {
    const EventRecord rec = event_record(a, r.node_start, i, 0, true, A, cos_axis);
    if (rec.state == RECORD_MISPLACED) misplaced += 1.0;
    int idx = -1;
    if (rec.state == RECORD_FINAL) {
      v = rec.power;
      if (rec.sb >= 0) {
        const EventLoad E{a, rec.e};
        const int ob = origin_bin_of(O, E.x(0), E.x(1), E.x(2));
        if (ob >= 0) idx = rec.sb * r.n_origin + ob;
      }
    }
    if (r.bin_out) r.bin_out[i] = idx;
    if (r.power_out) r.power_out[i] = v;
    if (idx >= 0 && r.n_groups > 0) idx += (int)(replicate_group(a.event_offset + rec.e, r.n_groups) * r.table);
    return idx;
  });
  wave_add(r.misplaced, misplaced);
}

// sky_launch's rule at 256 threads whatever the table (with an acos and an atan2 more than the sky kernels the lanes
// need more than the 128 registers a block of 1024 leaves them). On the LDS path every block pays for zeroing and
// flushing its table, so no more blocks are launched than are resident at once: what the runtime says fit a CU beside
// each other with this build's registers and this table (2 to 3 at 165 to 181 VGPRs; fewer with a table over 40 KiB),
// times the device's CUs. Every thread takes at least 4 records.
hipError_t launch_event_origin(const EventRowsArgs& a, const EventOriginArgs& r, const SkyAxes& A, int cos_axis,
                               const OriginAxes& O, int mode, hipStream_t s) {
  if (a.n_nodes <= 0) return hipSuccess;
  const int64_t total = (int64_t)(r.n_groups > 0 ? r.n_groups : 1) * r.table;  // every group's table
  const bool lds = mode == 1 || (mode == 0 && total <= SKY_LDS_DOUBLES);
  const size_t shmem = lds ? (size_t)total * sizeof(double) : 0;
  const auto fn = lds ? &event_origin_kernel<true> : &event_origin_kernel<false>;
  // (asked once per device and table size: the callers hold the library's mutex)
  static int have_dev = -1, cus = 0, per_cu = 0;
  static size_t have_shmem = 0;
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return e;
  if (dev != have_dev || shmem != have_shmem) {
    have_dev = -1;
    if ((e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, 256, shmem)) != hipSuccess) return e;
    if ((e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev)) != hipSuccess) return e;
    if (per_cu < 1) per_cu = 1;
    have_dev = dev;
    have_shmem = shmem;
  }
  int64_t grid = (a.n_nodes + 4 * 256 - 1) / (4 * 256);
  if (grid > (int64_t)cus * per_cu) grid = (int64_t)cus * per_cu;
  hipLaunchKernelGGL(fn, dim3((unsigned)grid), dim3(256), shmem, s, a, r, A, cos_axis, O, (int)total);
  return hipGetLastError();
}

}  // namespace art
#endif  // ART_EVENT_KERNELS
