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
// The 2 x 2 x 2 taps of one output voxel of the order-1 resize (sliding.hip's resample_linear, cascade.hip's fused argmax): set up
// once per voxel, evaluated once per class.  lowres = 0..2 picks that axis by nearest neighbour, -1 interpolates all three; an axis
// whose size does not change has coordinate o exactly (weight 1 on tap 0).
struct Lin3 {
  int i0[3], i1[3];
  double w0[3], w1[3];
};
__device__ __forceinline__ void lin3_setup(Lin3& L, const int (&o)[3], const int (&n_in)[3], const int (&n_out)[3], int lowres);
// the value at the voxel: taps visited last axis fastest, the coefficient multiplied by the axis weights in axis order and added to
// a double sum (scipy's NI_ZoomShift; the including file is built with -ffp-contract=off), cast to float32
__device__ __forceinline__ float lin3_eval(const Lin3& L, const float* __restrict__ sp, const long long (&st)[3]) {
  double acc = 0.0;
#pragma unroll
  for (int ta = 0; ta < 2; ++ta)
#pragma unroll
    for (int tb = 0; tb < 2; ++tb)
#pragma unroll
      for (int tc = 0; tc < 2; ++tc) {
        const double wa = ta ? L.w1[0] : L.w0[0], wb = tb ? L.w1[1] : L.w0[1], wc = tc ? L.w1[2] : L.w0[2];
        if (wa == 0.0 || wb == 0.0 || wc == 0.0) continue;       // (taps scipy does not visit: nearest axis, unchanged axis)
        double coeff = (double)sp[(ta ? L.i1[0] : L.i0[0]) * st[0] + (tb ? L.i1[1] : L.i0[1]) * st[1] + (tc ? L.i1[2] : L.i0[2]) * st[2]];
        coeff *= wa;
        coeff *= wb;
        coeff *= wc;
        acc += coeff;
      }
  return (float)acc;
}
// order 0 (map_coordinates(order=0, mode='nearest')): floor(c + 0.5) of the clamped coordinate
__device__ __forceinline__ int near_coord(int o, int n_in, int n_out) {
  double c = ((double)n_in / (double)n_out) * ((double)o + 0.5) - 0.5;
  if (c < 0.0) c = 0.0;
  if (c > (double)(n_in - 1)) c = (double)(n_in - 1);
  return (int)floor(c + 0.5);
}
__device__ __forceinline__ void lin3_setup(Lin3& L, const int (&o)[3], const int (&n_in)[3], const int (&n_out)[3], int lowres) {
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    if (d == lowres || n_in[d] == n_out[d]) {
      L.i0[d] = L.i1[d] = (d == lowres) ? near_coord(o[d], n_in[d], n_out[d]) : o[d];
      L.w0[d] = 1.0; L.w1[d] = 0.0;
    } else {
      double t;
      lin_coord(o[d], n_in[d], n_out[d], L.i0[d], L.i1[d], t);
      L.w0[d] = 1.0 - t; L.w1[d] = t;
    }
  }
}

}  // namespace rs
}  // namespace e2e
