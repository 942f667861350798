// The Keys cubic (a = -0.5, GDAL's "cubic") as the warps of hsr_coreg.hip and hsr_reproject.hip evaluate it: one definition, so
// that both give the same bits on the same taps (include/hsr_coreg.h states the polynomials).
#pragma once
#include <hip/hip_runtime.h>

namespace hsr {

__device__ __forceinline__ void keys_weights(double t, double (&wt)[4]) {
  wt[0] = ((-0.5 * t + 1.0) * t - 0.5) * t;
  wt[1] = ((1.5 * t - 2.5) * t) * t + 1.0;
  wt[2] = ((-1.5 * t + 2.0) * t + 0.5) * t;
  wt[3] = ((0.5 * t - 0.5) * t) * t;
}

__device__ __forceinline__ int clamp_to_int(double v, int lo, int hi) {
  return v >= (double)hi ? hi : (v > (double)lo ? (int)v : lo);   // NaN -> lo
}

}  // namespace hsr
