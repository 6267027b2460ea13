// P2: preprocessing of a raw case on the device (gfx950): crop to the non-zero region, resample to the plans' spacing, normalise.
// Reference: e2enet/preprocessing/cropping.py (create_nonzero_mask, get_bbox_from_mask, crop_to_nonzero) and
// e2enet/preprocessing/preprocessing.py (resample_data_or_seg, GenericPreprocessor.resample_and_normalize), which run
// scipy.ndimage.binary_fill_holes, one fp64 skimage.transform.resize per modality (or per slice) and per label, and numpy masked
// statistics on the CPU.
//
//   e2e_pp_nonzero_mask   mask = OR over the modalities of x != 0 (a NaN is non-zero), then binary_fill_holes with its default
//                         6-neighbour structure: the background is labelled with the union-find of e2e_unionfind.h and every
//                         background component without a voxel on a face of the volume becomes mask
//   e2e_pp_bbox           [lo, hi) per axis of the voxels != outside_value, and their number (integer atomics)
//   e2e_pp_crop           the cropped modalities and the cropped seg (-1 where seg == 0 off the mask; without a seg -1 off / 0 on)
//   e2e_pp_label_hist     histogram of the whole-number labels -256 .. 255 (np.unique of a seg); optionally seg[seg < -1] = 0
//   e2e_pp_nan_to_zero    data[isnan(data)] = 0
//   e2e_pp_minmax         clip range of the cubic resize: per modality, or per (modality, slice) across a separate axis
//   e2e_pp_pad_edge       edge padding (scipy's pre-padding by 12 for mode 'nearest') of a strided source into a contiguous buffer;
//                         the prefilter that follows is e2e_aug_bspline_prefilter_axis, as it is
//   e2e_pp_resize_cubic   scipy.ndimage.zoom(order=3, mode='nearest', grid_mode=True) clipped to the range (what
//                         skimage.transform.resize(order=3, mode='edge', anti_aliasing=False, clip=True) evaluates); along a separate
//                         low-resolution axis order 0 (map_coordinates(order=0, mode='nearest')) of the per-slice 2-D resize
//   e2e_pp_resize_seg     batchgenerators' resize_segmentation(order=1): per label the linear interpolation of its binary mask
//                         (the arithmetic of e2e_resample_linear), the label written where it is >= 0.5, labels ascending, so the
//                         largest label that reaches 0.5 wins; one gather, no mask per label: only the labels at a voxel's (up to
//                         eight) taps can reach 0.5 there.  Labels < -1 are written as 0.
//   e2e_pp_norm_stats / e2e_pp_normalize   the four normalisation schemes; mean and np.std (ddof 0) of a case in two passes, fp64
//                         on per-block records folded in a fixed order: no floating-point atomics, the same bits on every run
// All of them are HBM streaming kernels except the union-find's merge.
#include "e2e_common.h"
#include "e2e_resample.h"
#include "e2e_unionfind.h"

namespace {

using e2e::uf::NONE;
enum { R_LO0 = 0, R_HI0 = 1, R_GIVEUP = 6, R_COUNT = 7 };        // the eight result words: lo, hi per axis; give-up; voxel count

// ---- non-zero mask and hole filling ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void pp_mask_kernel(const float* __restrict__ x, unsigned char* __restrict__ mask, int C, unsigned V,
                                                      unsigned* __restrict__ result) {
  if (blockIdx.x == 0 && threadIdx.x == 0) result[R_GIVEUP] = 0u;
  const unsigned long long i = (unsigned long long)blockIdx.x * 256ull + threadIdx.x;
  if (i >= V) return;
  bool m = false;
  for (int c = 0; c < C; ++c) m |= x[(unsigned long long)c * V + i] != 0.f;
  mask[i] = m ? 1 : 0;
}

// background runs; outside[i] = 0
__global__ __launch_bounds__(256) void pp_bg_init_kernel(const unsigned char* __restrict__ mask, unsigned* __restrict__ parent,
                                                         unsigned char* __restrict__ outside, unsigned V, unsigned W) {
  e2e::uf::init_runs([&](unsigned j) { return mask[j] == 0; }, parent, V, W);
  const unsigned long long i = (unsigned long long)blockIdx.x * 256ull + threadIdx.x;
  if (i < V) outside[i] = 0;
}

__global__ __launch_bounds__(256) void pp_bg_merge_kernel(unsigned* parent, unsigned* result, unsigned V, unsigned W, unsigned HW) {
  e2e::uf::merge_back(parent, &result[R_GIVEUP], V, W, HW);
}

// parent[i] = root(i); a background voxel on a face of the volume marks its root as connected to the outside
__global__ __launch_bounds__(256) void pp_bg_flatten_kernel(unsigned* parent, unsigned char* outside, unsigned* result, unsigned V,
                                                            unsigned D, unsigned H, unsigned W) {
  const unsigned long long i64 = (unsigned long long)blockIdx.x * 256ull + threadIdx.x;
  if (i64 >= V) return;
  const unsigned i = (unsigned)i64;
  if (parent[i] == NONE) return;
  unsigned budget = V + 64u;
  const unsigned root = e2e::uf::find_root(parent, i, budget, &result[R_GIVEUP]);
  if (root == NONE) return;
  parent[i] = root;                                            // (roots keep parent[r] == r; a racing reader sees an ancestor)
  const unsigned w = i % W, h = (i / W) % H, d = i / (W * H);
  if (w == 0u || w == W - 1u || h == 0u || h == H - 1u || d == 0u || d == D - 1u) outside[root] = 1;
}

__global__ __launch_bounds__(256) void pp_fill_kernel(unsigned char* __restrict__ mask, const unsigned* __restrict__ parent,
                                                      const unsigned char* __restrict__ outside, unsigned V) {
  const unsigned long long i = (unsigned long long)blockIdx.x * 256ull + threadIdx.x;
  if (i >= V) return;
  const unsigned p = parent[i];                                // (i's root after the flatten pass)
  if (p != NONE && p < V && outside[p] == 0) mask[i] = 1;
}

// ---- bounding box ------------------------------------------------------------------------------------------------------------
__global__ void pp_bbox_init_kernel(unsigned* result) {
  if (threadIdx.x < 6) result[threadIdx.x] = (threadIdx.x & 1u) ? 0u : 0xFFFFFFFFu;
  if (threadIdx.x == 6) result[R_COUNT] = 0u;
}
__global__ __launch_bounds__(256) void pp_bbox_kernel(const unsigned char* __restrict__ mask, int outside_value, unsigned V, unsigned H,
                                                      unsigned W, unsigned* result) {
  const unsigned long long i64 = (unsigned long long)blockIdx.x * 256ull + threadIdx.x;
  const unsigned i = (unsigned)i64;
  const bool m = i64 < V && (int)mask[i] != outside_value;
  unsigned lo[3] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu}, hi[3] = {0u, 0u, 0u};
  if (m) {
    const unsigned c[3] = {i / (W * H), (i / W) % H, i % W};
#pragma unroll
    for (int a = 0; a < 3; ++a) { lo[a] = c[a]; hi[a] = c[a] + 1u; }
  }
  const unsigned long long bits = __ballot(m);
  if (bits == 0ull) return;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1)
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const unsigned l = __shfl_xor(lo[a], off, 64), h = __shfl_xor(hi[a], off, 64);
      lo[a] = l < lo[a] ? l : lo[a];
      hi[a] = h > hi[a] ? h : hi[a];
    }
  if ((threadIdx.x & 63u) == 0u) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      atomicMin(&result[R_LO0 + 2 * a], lo[a]);
      atomicMax(&result[R_HI0 + 2 * a], hi[a]);
    }
    atomicAdd(&result[R_COUNT], (unsigned)__popcll(bits));
  }
}

// ---- crop --------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void pp_crop_kernel(const float* __restrict__ data, const float* __restrict__ seg,
                                                      const unsigned char* __restrict__ mask, float* __restrict__ out_data,
                                                      float* __restrict__ out_seg, int C, int S, int H, int W, long long V, int z0, int y0,
                                                      int x0, int d, int h, int w, float nonzero_label) {
  const long long v = (long long)d * h * w;
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= v) return;
  const int ox = (int)(idx % w), oy = (int)((idx / w) % h), oz = (int)(idx / ((long long)w * h));
  const long long src = ((long long)(z0 + oz) * H + (y0 + oy)) * W + (x0 + ox);
  for (int c = 0; c < C; ++c) out_data[(long long)c * v + idx] = data[(long long)c * V + src];
  const bool on = mask[src] != 0;
  if (seg == nullptr) {
    out_seg[idx] = on ? 0.f : nonzero_label;
    return;
  }
  for (int s = 0; s < S; ++s) {
    const float l = seg[(long long)s * V + src];
    out_seg[(long long)s * v + idx] = (l == 0.f && !on) ? nonzero_label : l;
  }
}

// ---- label histogram ---------------------------------------------------------------------------------------------------------
constexpr int HIST_LO = -256, HIST_BINS = 513;                 // bins for -256 .. 255 and one for everything else
__global__ __launch_bounds__(256) void pp_label_hist_kernel(float* __restrict__ seg, long long n, unsigned* __restrict__ hist,
                                                            int fix_below) {
  __shared__ unsigned local[HIST_BINS];
  for (int b = threadIdx.x; b < HIST_BINS; b += 256) local[b] = 0u;
  __syncthreads();
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    const float v = seg[i];
    int bin = HIST_BINS - 1;
    if (v >= (float)HIST_LO && v <= 255.f && v == floorf(v)) bin = (int)v - HIST_LO;
    atomicAdd(&local[bin], 1u);
    if (fix_below && v < -1.f) seg[i] = 0.f;
  }
  __syncthreads();
  for (int b = threadIdx.x; b < HIST_BINS; b += 256)
    if (local[b]) atomicAdd(&hist[b], local[b]);
}

__global__ __launch_bounds__(256) void pp_nan_to_zero_kernel(float* __restrict__ x, long long n) {
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    const float v = x[i];
    if (v != v) x[i] = 0.f;
  }
}

// ---- clip range of the cubic resize ------------------------------------------------------------------------------------------
// group g = k (lowres < 0: the whole modality) or k * n[lowres] + slice; part[(g * chunks + chunk) * 2] = (min, max)
struct Dims3 { int n[3]; long long st[3]; };

__global__ __launch_bounds__(256) void pp_minmax_kernel(const float* __restrict__ src, long long kstride, Dims3 g, int lowres, int chunks,
                                                        double* __restrict__ part) {
  const int grp = blockIdx.y;
  const int nslice = lowres < 0 ? 1 : g.n[lowres];
  const int k = grp / nslice, fixed = grp - k * nslice;
  const int p = lowres == 0 ? 1 : 0, q = lowres == 2 ? 1 : 2;  // the two free axes of a slice (lowres >= 0)
  const long long cnt = lowres < 0 ? (long long)g.n[0] * g.n[1] * g.n[2] : (long long)g.n[p] * g.n[q];
  const float* base = src + (long long)k * kstride + (lowres < 0 ? 0 : (long long)fixed * g.st[lowres]);
  const long long per = e2e::cdivll(cnt, chunks);
  const long long lo = (long long)blockIdx.x * per, hi = lo + per < cnt ? lo + per : cnt;
  float mn = INFINITY, mx = -INFINITY;
  for (long long e = lo + threadIdx.x; e < hi; e += 256) {
    long long off;
    if (lowres < 0) {
      const long long bc = (long long)g.n[1] * g.n[2];
      const long long a = e / bc, r = e - a * bc;
      off = a * g.st[0] + (r / g.n[2]) * g.st[1] + (r % g.n[2]) * g.st[2];
    } else {
      off = (e / g.n[q]) * g.st[p] + (e % g.n[q]) * g.st[q];
    }
    const float v = base[off];
    mn = fminf(mn, v);
    mx = fmaxf(mx, v);
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) { mn = fminf(mn, __shfl_xor(mn, off, 64)); mx = fmaxf(mx, __shfl_xor(mx, off, 64)); }
  __shared__ float sh[4][2];
  if ((threadIdx.x & 63) == 0) { sh[threadIdx.x >> 6][0] = mn; sh[threadIdx.x >> 6][1] = mx; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int i = 1; i < 4; ++i) { mn = fminf(mn, sh[i][0]); mx = fmaxf(mx, sh[i][1]); }
    double* o = part + ((long long)grp * chunks + blockIdx.x) * 2;
    o[0] = (double)mn; o[1] = (double)mx;
  }
}
__global__ void pp_minmax_final_kernel(const double* __restrict__ part, double* __restrict__ out, int chunks, int groups) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= groups) return;
  const double* p = part + (long long)g * chunks * 2;
  double a = p[0], b = p[1];
  for (int i = 1; i < chunks; ++i) { a = fmin(a, p[2 * i]); b = fmax(b, p[2 * i + 1]); }
  out[2 * g] = a; out[2 * g + 1] = b;
}

// ---- edge padding ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void pp_pad_edge_kernel(const float* __restrict__ src, float* __restrict__ dst, long long kstride, Dims3 g,
                                                          int pa, int pb, int pc) {
  const int PA = g.n[0] + 2 * pa, PB = g.n[1] + 2 * pb, PC = g.n[2] + 2 * pc;
  const long long pvol = (long long)PA * PB * PC;
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= pvol) return;
  int c = (int)(idx % PC) - pc, b = (int)((idx / PC) % PB) - pb, a = (int)(idx / ((long long)PC * PB)) - pa;
  a = a < 0 ? 0 : (a >= g.n[0] ? g.n[0] - 1 : a);
  b = b < 0 ? 0 : (b >= g.n[1] ? g.n[1] - 1 : b);
  c = c < 0 ? 0 : (c >= g.n[2] ? g.n[2] - 1 : c);
  dst[(long long)blockIdx.y * pvol + idx] = src[(long long)blockIdx.y * kstride + a * g.st[0] + b * g.st[1] + c * g.st[2]];
}

// ---- cubic gather ------------------------------------------------------------------------------------------------------------
// coef: [K, n0 + 2 p0, n1 + 2 p1, n2 + 2 p2] B-spline coefficients with p = pad on the interpolated axes and 0 on the separate one
__global__ __launch_bounds__(256) void pp_resize_cubic_kernel(const float* __restrict__ coef, float* __restrict__ dst,
                                                              const double* __restrict__ minmax, int K, int A, int B, int C, int OA,
                                                              int OB, int OC, int pad, int lowres) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long ovol = (long long)OA * OB * OC;
  if (idx >= ovol) return;
  const int o[3] = {(int)(idx / ((long long)OC * OB)), (int)((idx / OC) % OB), (int)(idx % OC)};
  const int n_in[3] = {A, B, C}, n_out[3] = {OA, OB, OC};
  int P[3], nt[3], tap[3][4];
  double wt[3][4];
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    if (d == lowres) {
      P[d] = n_in[d];
      nt[d] = 1;
      tap[d][0] = e2e::rs::near_coord(o[d], n_in[d], n_out[d]);
      wt[d][0] = 1.0;
    } else {
      P[d] = n_in[d] + 2 * pad;
      nt[d] = 4;
      const double c = ((double)o[d] + 0.5) * ((double)n_in[d] / (double)n_out[d]) - 0.5 + pad;
      const double f = floor(c);
      e2e::rs::bspline3_weights(c - f, wt[d]);
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int i = (int)f - 1 + t;                          // inside [0, P) for pad >= 2; the clamp keeps a bad call in bounds
        tap[d][t] = i < 0 ? 0 : (i >= P[d] ? P[d] - 1 : i);
      }
    }
  }
  const long long pvol = (long long)P[0] * P[1] * P[2];
  const int slice = lowres < 0 ? 0 : tap[lowres][0], nslice = lowres < 0 ? 1 : n_in[lowres];
  for (int k = 0; k < K; ++k) {
    const float* cf = coef + (long long)k * pvol;
    double acc = 0.0;
    for (int a = 0; a < nt[0]; ++a) {
      double sa = 0.0;
      for (int b = 0; b < nt[1]; ++b) {
        const float* row = cf + ((long long)tap[0][a] * P[1] + tap[1][b]) * P[2];
        double sb = 0.0;
        for (int e = 0; e < nt[2]; ++e) sb += wt[2][e] * (double)row[tap[2][e]];
        sa += wt[1][b] * sb;
      }
      acc += wt[0][a] * sa;
    }
    const double* mm = minmax + 2 * ((long long)k * nslice + slice);
    const float f = (float)acc, mn = (float)mm[0], mx = (float)mm[1];
    dst[(long long)k * ovol + idx] = f < mn ? mn : (f > mx ? mx : f);
  }
}

// ---- segmentation resize -----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void pp_resize_seg_kernel(const float* __restrict__ src, float* __restrict__ dst, int K, long long kstride,
                                                            Dims3 g, int OA, int OB, int OC, int lowres) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long ovol = (long long)OA * OB * OC;
  if (idx >= ovol) return;
  const int o[3] = {(int)(idx / ((long long)OC * OB)), (int)((idx / OC) % OB), (int)(idx % OC)};
  const int n_out[3] = {OA, OB, OC};
  int i0[3], i1[3];
  double w0[3], w1[3];
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    if (d == lowres || g.n[d] == n_out[d]) {
      i0[d] = i1[d] = (d == lowres) ? e2e::rs::near_coord(o[d], g.n[d], n_out[d]) : o[d];
      w0[d] = 1.0; w1[d] = 0.0;
    } else {
      double t;
      e2e::rs::lin_coord(o[d], g.n[d], n_out[d], i0[d], i1[d], t);
      w0[d] = 1.0 - t; w1[d] = t;
    }
  }
  for (int k = 0; k < K; ++k) {
    const float* sp = src + (long long)k * kstride;
    // the taps in resample_linear's order, each with the product it adds for a label whose mask is 1 there
    float lab[8];
    double wgt[8];
    int nt = 0;
#pragma unroll
    for (int ta = 0; ta < 2; ++ta)
#pragma unroll
      for (int tb = 0; tb < 2; ++tb)
#pragma unroll
        for (int tc = 0; tc < 2; ++tc) {
          const double wa = ta ? w1[0] : w0[0], wb = tb ? w1[1] : w0[1], wc = tc ? w1[2] : w0[2];
          const bool live = !(wa == 0.0 || wb == 0.0 || wc == 0.0);
          double coeff = 1.0;
          coeff *= wa;
          coeff *= wb;
          coeff *= wc;
          lab[nt] = live ? sp[(ta ? i1[0] : i0[0]) * g.st[0] + (tb ? i1[1] : i0[1]) * g.st[1] + (tc ? i1[2] : i0[2]) * g.st[2]] : 0.f;
          wgt[nt] = live ? coeff : -1.0;                       // (-1: a tap resample_linear does not visit)
          ++nt;
        }
    float best = 0.f;
    bool have = false;
#pragma unroll
    for (int t = 0; t < 8; ++t) {
      if (wgt[t] < 0.0) continue;
      double acc = 0.0;
#pragma unroll
      for (int u = 0; u < 8; ++u)
        if (wgt[u] >= 0.0 && lab[u] == lab[t]) acc += wgt[u];
      if (acc >= 0.5 && (!have || lab[t] > best)) { best = lab[t]; have = true; }
    }
    dst[(long long)k * ovol + idx] = best < -1.f ? 0.f : best;
  }
}

// ---- normalisation -----------------------------------------------------------------------------------------------------------
// prm[c * 8 ..]: scheme (0 default, 1 CT, 2 CT2, 3 noNorm), lower bound, upper bound, mean, sd (CT: the plans' constants),
// use_nonzero_mask.  stats[c * 4 ..]: voxels counted, mean, std of the case (schemes 0 and 2).
enum { S_DEFAULT = 0, S_CT = 1, S_CT2 = 2, S_NONORM = 3 };

__device__ __forceinline__ bool norm_counts(int scheme, bool use_mask, double lb, double ub, float v, const float* seg, long long i) {
  if (scheme == S_CT2) return (double)v > lb && (double)v < ub;
  return !use_mask || seg[i] >= 0.f;
}

// pass 0: part = (count, sum); pass 1: part = (count, sum of (x - mean)^2)
__global__ __launch_bounds__(256) void pp_norm_stats_kernel(const float* __restrict__ x, const float* __restrict__ seg,
                                                            const double* __restrict__ prm, const double* __restrict__ stats,
                                                            double* __restrict__ part, long long vol, int chunks, int pass) {
  const int c = blockIdx.y;
  const double* q = prm + (long long)c * 8;
  const int scheme = (int)q[0];
  if (scheme != S_DEFAULT && scheme != S_CT2) return;
  const bool use_mask = q[5] != 0.0 && seg != nullptr;
  const double lb = q[1], ub = q[2], mean = pass ? stats[c * 4 + 1] : 0.0;
  const float* p = x + (long long)c * vol;
  const long long per = e2e::cdivll(vol, chunks);
  const long long lo = (long long)blockIdx.x * per, hi = lo + per < vol ? lo + per : vol;
  double n = 0.0, s = 0.0;
  for (long long i = lo + threadIdx.x; i < hi; i += 256) {
    const float v = p[i];
    if (!norm_counts(scheme, use_mask, lb, ub, v, seg, i)) continue;
    const double dv = (double)v - mean;
    n += 1.0;
    s += pass ? dv * dv : dv;
  }
  n = e2e::wave_sum_d(n);
  s = e2e::wave_sum_d(s);
  __shared__ double sh[4][2];
  if ((threadIdx.x & 63) == 0) { sh[threadIdx.x >> 6][0] = n; sh[threadIdx.x >> 6][1] = s; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int i = 1; i < 4; ++i) { n += sh[i][0]; s += sh[i][1]; }
    double* o = part + ((long long)c * chunks + blockIdx.x) * 2;
    o[0] = n; o[1] = s;
  }
}
__global__ void pp_norm_stats_final_kernel(const double* __restrict__ part, const double* __restrict__ prm, double* __restrict__ stats,
                                           int chunks, int C, int pass) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  const int scheme = (int)prm[(long long)c * 8];
  if (scheme != S_DEFAULT && scheme != S_CT2) return;
  const double* p = part + (long long)c * chunks * 2;
  double n = p[0], s = p[1];
  for (int i = 1; i < chunks; ++i) { n += p[2 * i]; s += p[2 * i + 1]; }
  if (pass == 0) { stats[c * 4] = n; stats[c * 4 + 1] = s / n; }      // (an empty selection: 0 / 0 = NaN, like numpy's mean)
  else stats[c * 4 + 2] = sqrt(s / n);
}

__global__ __launch_bounds__(256) void pp_normalize_kernel(float* __restrict__ x, const float* __restrict__ seg,
                                                           const double* __restrict__ prm, const double* __restrict__ stats, long long vol) {
  const int c = blockIdx.y;
  const double* q = prm + (long long)c * 8;
  const int scheme = (int)q[0];
  if (scheme == S_NONORM) return;
  const bool use_mask = q[5] != 0.0 && seg != nullptr;
  const double lb = q[1], ub = q[2];
  const double mean = scheme == S_CT ? q[3] : stats[c * 4 + 1];
  const double sd = scheme == S_CT ? q[4] : (scheme == S_CT2 ? stats[c * 4 + 2] : stats[c * 4 + 2] + 1e-8);
  float* p = x + (long long)c * vol;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < vol; i += (long long)gridDim.x * 256) {
    if (use_mask && seg[i] < 0.f) { p[i] = 0.f; continue; }
    double v = (double)p[i];
    if (scheme != S_DEFAULT) v = v < lb ? lb : (v > ub ? ub : v);
    p[i] = (float)((v - mean) / sd);
  }
}

bool pp_dims_ok(const char* what, int D, int H, int W, int* rc) {
  if (D < 1 || H < 1 || W < 1) {
    e2e::set_error("%s: every axis needs at least one voxel (got %d x %d x %d)", what, D, H, W);
    *rc = E2E_ERR_ARG;
    return false;
  }
  if ((long long)D * H * W > e2e::uf::MAX_VOXELS) {
    e2e::set_error("%s: %d x %d x %d is more than the 2^31 - 2 voxels a 32-bit index serves", what, D, H, W);
    *rc = E2E_ERR_UNSUPPORTED;
    return false;
  }
  return true;
}

inline unsigned stream_blocks(long long n) {
  long long b = e2e::cdivll(n, 256 * 4);
  return (unsigned)(b > 4096 ? 4096 : (b < 1 ? 1 : b));
}
inline int minmax_chunks(long long per_group) {
  const long long c = e2e::cdivll(per_group, 16384);
  return (int)(c > 64 ? 64 : (c < 1 ? 1 : c));
}
constexpr int NORM_CHUNKS = 128;

}  // namespace

extern "C" long long e2e_pp_nonzero_ws_bytes(int D, int H, int W) {
  int rc;
  if (!pp_dims_ok("pp_nonzero_ws_bytes", D, H, W, &rc)) return 0;
  return (5ll * D * H * W + 15) / 16 * 16;
}

extern "C" int e2e_pp_nonzero_mask(const float* data, int C, int D, int H, int W, unsigned char* mask, void* ws, unsigned* result,
                                   void* stream) {
  int rc;
  if (!pp_dims_ok("pp_nonzero_mask", D, H, W, &rc)) return rc;
  E2E_REQUIRE(data && mask && ws && result && C > 0, "pp_nonzero_mask: bad arguments");
  hipStream_t st = (hipStream_t)stream;
  const unsigned V = (unsigned)((long long)D * H * W), HW = (unsigned)((long long)H * W);
  unsigned* parent = (unsigned*)ws;
  unsigned char* outside = (unsigned char*)(parent + V);
  const dim3 grid((unsigned)e2e::cdivll((long long)V, 256)), block(256);
  hipLaunchKernelGGL(pp_mask_kernel, grid, block, 0, st, data, mask, C, V, result);
  if (int e = e2e::check_launch("pp_mask_kernel")) return e;
  hipLaunchKernelGGL(pp_bg_init_kernel, grid, block, 0, st, mask, parent, outside, V, (unsigned)W);
  hipLaunchKernelGGL(pp_bg_merge_kernel, grid, block, 0, st, parent, result, V, (unsigned)W, HW);
  hipLaunchKernelGGL(pp_bg_flatten_kernel, grid, block, 0, st, parent, outside, result, V, (unsigned)D, (unsigned)H, (unsigned)W);
  hipLaunchKernelGGL(pp_fill_kernel, grid, block, 0, st, mask, parent, outside, V);
  return e2e::check_launch("pp_fill_kernel");
}

extern "C" int e2e_pp_bbox(const unsigned char* mask, int outside_value, int D, int H, int W, unsigned* result, void* stream) {
  int rc;
  if (!pp_dims_ok("pp_bbox", D, H, W, &rc)) return rc;
  E2E_REQUIRE(mask && result, "pp_bbox: null pointer");
  hipStream_t st = (hipStream_t)stream;
  const unsigned V = (unsigned)((long long)D * H * W);
  hipLaunchKernelGGL(pp_bbox_init_kernel, dim3(1), dim3(64), 0, st, result);
  hipLaunchKernelGGL(pp_bbox_kernel, dim3((unsigned)e2e::cdivll((long long)V, 256)), dim3(256), 0, st, mask, outside_value, V, (unsigned)H,
                     (unsigned)W, result);
  return e2e::check_launch("pp_bbox_kernel");
}

extern "C" int e2e_pp_crop(const float* data, const float* seg, const unsigned char* mask, float* out_data, float* out_seg, int C, int S,
                           int D, int H, int W, int z0, int y0, int x0, int d, int h, int w, float nonzero_label, void* stream) {
  int rc;
  if (!pp_dims_ok("pp_crop", D, H, W, &rc)) return rc;
  E2E_REQUIRE(data && mask && out_data && out_seg && C > 0 && (seg == nullptr || S > 0), "pp_crop: bad arguments");
  E2E_REQUIRE(z0 >= 0 && y0 >= 0 && x0 >= 0 && d > 0 && h > 0 && w > 0 && z0 + d <= D && y0 + h <= H && x0 + w <= W,
              "pp_crop: the box [%d:%d, %d:%d, %d:%d] is outside the volume %d x %d x %d", z0, z0 + d, y0, y0 + h, x0, x0 + w, D, H, W);
  hipLaunchKernelGGL(pp_crop_kernel, dim3((unsigned)e2e::cdivll((long long)d * h * w, 256)), dim3(256), 0, (hipStream_t)stream, data, seg,
                     mask, out_data, out_seg, C, S, H, W, (long long)D * H * W, z0, y0, x0, d, h, w, nonzero_label);
  return e2e::check_launch("pp_crop_kernel");
}

extern "C" int e2e_pp_label_hist_bins(void) { return HIST_BINS; }

extern "C" int e2e_pp_label_hist(float* seg, long long n, unsigned* hist, int fix_below, void* stream) {
  E2E_REQUIRE(seg && hist && n > 0, "pp_label_hist: bad arguments");
  hipLaunchKernelGGL(pp_label_hist_kernel, dim3(stream_blocks(n)), dim3(256), 0, (hipStream_t)stream, seg, n, hist, fix_below);
  return e2e::check_launch("pp_label_hist_kernel");
}

extern "C" int e2e_pp_nan_to_zero(float* x, long long n, void* stream) {
  E2E_REQUIRE(x && n > 0, "pp_nan_to_zero: bad arguments");
  hipLaunchKernelGGL(pp_nan_to_zero_kernel, dim3(stream_blocks(n)), dim3(256), 0, (hipStream_t)stream, x, n);
  return e2e::check_launch("pp_nan_to_zero_kernel");
}

#define PP_REQUIRE_GRID(what)                                                                                                        \
  E2E_REQUIRE(src && dst && src != dst && K > 0 && K <= 65535 && A > 0 && B > 0 && C > 0, what ": bad arguments");                  \
  E2E_REQUIRE(lowres_axis >= -1 && lowres_axis <= 2, what ": lowres_axis must be -1 (none) or 0..2")

extern "C" long long e2e_pp_minmax_ws_bytes(int K, int A, int B, int C, int lowres_axis) {
  if (K < 1 || A < 1 || B < 1 || C < 1 || lowres_axis < -1 || lowres_axis > 2) return 0;
  const int n[3] = {A, B, C};
  const long long groups = (long long)K * (lowres_axis < 0 ? 1 : n[lowres_axis]);
  return groups * 64 * 2 * (long long)sizeof(double);
}

extern "C" int e2e_pp_minmax(const float* src, double* dst, void* ws, int K, long long kstride, int A, int B, int C, long long sa, long long sb,
                             long long sc, int lowres_axis, void* stream) {
  E2E_REQUIRE(src && dst && ws && K > 0 && A > 0 && B > 0 && C > 0, "pp_minmax: bad arguments");
  E2E_REQUIRE(lowres_axis >= -1 && lowres_axis <= 2, "pp_minmax: lowres_axis must be -1 (none) or 0..2");
  const Dims3 g = {{A, B, C}, {sa, sb, sc}};
  const long long vol = (long long)A * B * C;
  const long long groups = (long long)K * (lowres_axis < 0 ? 1 : g.n[lowres_axis]);
  E2E_REQUIRE(groups <= 65535, "pp_minmax: more than 65535 (modality, slice) groups");
  const int chunks = minmax_chunks(lowres_axis < 0 ? vol : vol / g.n[lowres_axis]);
  hipLaunchKernelGGL(pp_minmax_kernel, dim3(chunks, (unsigned)groups), dim3(256), 0, (hipStream_t)stream, src, kstride, g, lowres_axis,
                     chunks, (double*)ws);
  hipLaunchKernelGGL(pp_minmax_final_kernel, dim3((unsigned)e2e::cdivll(groups, 64)), dim3(64), 0, (hipStream_t)stream, (const double*)ws,
                     dst, chunks, (int)groups);
  return e2e::check_launch("pp_minmax_kernel");
}

extern "C" int e2e_pp_pad_edge(const float* src, float* dst, int K, long long kstride, int A, int B, int C, long long sa, long long sb,
                               long long sc, int pa, int pb, int pc, void* stream) {
  E2E_REQUIRE(src && dst && src != dst && K > 0 && K <= 65535 && A > 0 && B > 0 && C > 0, "pp_pad_edge: bad arguments");
  E2E_REQUIRE(pa >= 0 && pb >= 0 && pc >= 0, "pp_pad_edge: negative padding");
  const Dims3 g = {{A, B, C}, {sa, sb, sc}};
  const long long pvol = (long long)(A + 2 * pa) * (B + 2 * pb) * (C + 2 * pc);
  hipLaunchKernelGGL(pp_pad_edge_kernel, dim3((unsigned)e2e::cdivll(pvol, 256), K), dim3(256), 0, (hipStream_t)stream, src, dst, kstride, g,
                     pa, pb, pc);
  return e2e::check_launch("pp_pad_edge_kernel");
}

extern "C" int e2e_pp_resize_cubic(const float* src, float* dst, const double* minmax, int K, int A, int B, int C, int OA, int OB, int OC,
                                   int pad, int lowres_axis, void* stream) {
  PP_REQUIRE_GRID("pp_resize_cubic");
  E2E_REQUIRE(minmax && OA > 0 && OB > 0 && OC > 0 && pad >= 2, "pp_resize_cubic: bad arguments (the padding is at least 2)");
  hipLaunchKernelGGL(pp_resize_cubic_kernel, dim3((unsigned)e2e::cdivll((long long)OA * OB * OC, 256)), dim3(256), 0, (hipStream_t)stream,
                     src, dst, minmax, K, A, B, C, OA, OB, OC, pad, lowres_axis);
  return e2e::check_launch("pp_resize_cubic_kernel");
}

extern "C" int e2e_pp_resize_seg(const float* src, float* dst, int K, long long kstride, int A, int B, int C, long long sa, long long sb,
                                 long long sc, int OA, int OB, int OC, int lowres_axis, void* stream) {
  PP_REQUIRE_GRID("pp_resize_seg");
  E2E_REQUIRE(OA > 0 && OB > 0 && OC > 0, "pp_resize_seg: bad output shape");
  const Dims3 g = {{A, B, C}, {sa, sb, sc}};
  hipLaunchKernelGGL(pp_resize_seg_kernel, dim3((unsigned)e2e::cdivll((long long)OA * OB * OC, 256)), dim3(256), 0, (hipStream_t)stream, src,
                     dst, K, kstride, g, OA, OB, OC, lowres_axis);
  return e2e::check_launch("pp_resize_seg_kernel");
}

extern "C" long long e2e_pp_norm_ws_bytes(int C) { return C < 1 ? 0 : (long long)C * NORM_CHUNKS * 2 * (long long)sizeof(double); }

extern "C" int e2e_pp_norm_stats(const float* x, const float* seg, const double* prm, double* stats, void* ws, int C, long long vol,
                                 void* stream) {
  E2E_REQUIRE(x && prm && stats && ws && C > 0 && C <= 65535 && vol > 0, "pp_norm_stats: bad arguments");
  hipStream_t st = (hipStream_t)stream;
  for (int pass = 0; pass < 2; ++pass) {
    hipLaunchKernelGGL(pp_norm_stats_kernel, dim3(NORM_CHUNKS, C), dim3(256), 0, st, x, seg, prm, stats, (double*)ws, vol, NORM_CHUNKS, pass);
    hipLaunchKernelGGL(pp_norm_stats_final_kernel, dim3(e2e::cdiv(C, 64)), dim3(64), 0, st, (const double*)ws, prm, stats, NORM_CHUNKS, C,
                       pass);
  }
  return e2e::check_launch("pp_norm_stats_kernel");
}

extern "C" int e2e_pp_normalize(float* x, const float* seg, const double* prm, const double* stats, int C, long long vol, void* stream) {
  E2E_REQUIRE(x && prm && stats && C > 0 && C <= 65535 && vol > 0, "pp_normalize: bad arguments");
  hipLaunchKernelGGL(pp_normalize_kernel, dim3(stream_blocks(vol), C), dim3(256), 0, (hipStream_t)stream, x, seg, prm, stats, vol);
  return e2e::check_launch("pp_normalize_kernel");
}
