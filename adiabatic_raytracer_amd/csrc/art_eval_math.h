// art_eval_math.h -- eval_math_kernel: the scalar functions of art_core.h, one instantiation per translation unit.
#pragma once
#include <hip/hip_runtime.h>

#include "art_core.h"
#include "art_internal.h"

namespace art {

// ---------------------------------------------------------------------------
// The hand-written scalar functions of art_core.h themselves (art_eval_math_device): operands
// loaded from memory, the function called, the result stored -- one thread per element, no
// restatement of any of them. Compiled in both translation units (TU = 0 here, TU = 1
// art_kernels_nolicm.hip), each with its unit's flags: the functions must round alike in both.
template <int TU, int FN>
__global__ __launch_bounds__(256) void eval_math_kernel(const int64_t n, const double* __restrict__ a,
                                                        const double* __restrict__ b, double* __restrict__ out0,
                                                        double* __restrict__ out1) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double x = a[i];
  double y0 = 0.0, y1 = 0.0;
  if constexpr (FN == ART_MATH_SINCOS) msincos(x, y0, y1);
  else if constexpr (FN == ART_MATH_EXP) y0 = fexp(x);
  else if constexpr (FN == ART_MATH_LOG) y0 = flog(x);
  else if constexpr (FN == ART_MATH_RCP) y0 = frcp(x);
  else if constexpr (FN == ART_MATH_POW120) y0 = fexp(flog(x) * (1.0 / 120.0));
  else if constexpr (FN == ART_MATH_MAX_ABS) y0 = fmax_abs(x, b[i]);
  else if constexpr (FN == ART_MATH_MIN_Q) y0 = fmin_q(x, b[i]);
  else if constexpr (FN == ART_MATH_MAX_Q) y0 = fmax_q(x, b[i]);
  else y0 = rclamp(x, b[i]);
  if (out0) out0[i] = y0;
  if (FN == ART_MATH_SINCOS && out1) out1[i] = y1;
}
template <int TU>
MFn pick_eval_math(int fn) {
  switch (fn) {
    case ART_MATH_SINCOS: return eval_math_kernel<TU, ART_MATH_SINCOS>;
    case ART_MATH_EXP: return eval_math_kernel<TU, ART_MATH_EXP>;
    case ART_MATH_LOG: return eval_math_kernel<TU, ART_MATH_LOG>;
    case ART_MATH_RCP: return eval_math_kernel<TU, ART_MATH_RCP>;
    case ART_MATH_POW120: return eval_math_kernel<TU, ART_MATH_POW120>;
    case ART_MATH_MAX_ABS: return eval_math_kernel<TU, ART_MATH_MAX_ABS>;
    case ART_MATH_MIN_Q: return eval_math_kernel<TU, ART_MATH_MIN_Q>;
    case ART_MATH_MAX_Q: return eval_math_kernel<TU, ART_MATH_MAX_Q>;
    case ART_MATH_RCLAMP: return eval_math_kernel<TU, ART_MATH_RCLAMP>;
  }
  return nullptr;
}

}  // namespace art
