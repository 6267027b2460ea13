// Coordinate and weight arithmetic that the resampling kernels share (sliding.hip, augment.hip, preprocess.hip): scipy.ndimage's
// zoom(grid_mode=True) coordinates and its order-3 B-spline weights.  Every including file is built with -ffp-contract=off.
#pragma once
#include <hip/hip_runtime.h>

namespace e2e {
namespace rs {

// weights of the four taps floor(x) - 1 .. floor(x) + 2 of the cubic B-spline at offset t = x - floor(x)
__device__ __forceinline__ void bspline3_weights(double t, double (&w)[4]) {
  const double u = 1.0 - t;
  w[0] = u * u * u / 6.0;
  w[1] = (3.0 * t * t * t - 6.0 * t * t + 4.0) / 6.0;
  w[2] = (-3.0 * t * t * t + 3.0 * t * t + 3.0 * t + 1.0) / 6.0;
  w[3] = t * t * t / 6.0;
}

// order 1 (NI_ZoomShift): coordinate (o + 0.5) * (in / out) - 0.5 in double, clamped to [0, in - 1]; taps i0, i1 and fraction t
__device__ __forceinline__ void lin_coord(int o, int n_in, int n_out, int& i0, int& i1, double& t) {
  double c = ((double)o + 0.5) * ((double)n_in / (double)n_out) - 0.5;
  if (c < 0.0) c = 0.0;
  if (c > (double)(n_in - 1)) c = (double)(n_in - 1);
  const double f = floor(c);
  i0 = (int)f;
  t = c - f;
  i1 = i0 + 1 < n_in ? i0 + 1 : n_in - 1;
}
// order 0 (map_coordinates(order=0, mode='nearest')): floor(c + 0.5) of the clamped coordinate
__device__ __forceinline__ int near_coord(int o, int n_in, int n_out) {
  double c = ((double)n_in / (double)n_out) * ((double)o + 0.5) - 0.5;
  if (c < 0.0) c = 0.0;
  if (c > (double)(n_in - 1)) c = (double)(n_in - 1);
  return (int)floor(c + 0.5);
}

}  // namespace rs
}  // namespace e2e
