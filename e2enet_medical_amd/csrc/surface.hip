// K10: surface-distance scoring (gfx950): border mask of one label (or one set of labels) read straight from the uint8 label volume, exact squared
// Euclidean distance transform with per-axis spacing, and the reductions behind Hausdorff / HD95 / ASD / ASSD / NSD.
// Reference: medpy's __surface_distances as called by e2enet/evaluation/metrics.py:792-861 and surface_dice.py:20-56
// (binary_erosion with the 6-neighbour cross, distance_transform_edt(~border, sampling)).
//
// Shape of the code: every loop's trip count is fixed by the arguments, no workgroup waits on another, atomics are histogram
// and counter increments on integers only -- so every result, the fp64 sums included, is the same bits on every run.
#include "e2e_select.h"
#include <cmath>

namespace {

namespace sel = e2e::select;

constexpr int MAX_LINE = 960;          // longest axis an EDT pass stages: MAX_LINE * (16 + 1) floats fit 64 KiB of LDS
constexpr int LDS_FLOATS = 16384;      // 64 KiB

// ws of e2e_surface_distances_stats
struct StatsWs {
  double part[sel::SWEEP_BLOCKS][2][4];      // per workgroup and direction: count, sum d, max d2, count d <= threshold
  sel::State<2> select;                      // the two ranks of the concatenated distances, on the d2 bit patterns
};

// the two membership tests a border is taken of: one label value, or a set of values (bit v of eight words)
struct IsLabel {
  int label;
  __device__ __forceinline__ bool operator()(unsigned char v) const { return (int)v == label; }
};
struct InSet {
  unsigned w0, w1, w2, w3, w4, w5, w6, w7;
  __device__ __forceinline__ bool operator()(unsigned char v) const {
    const unsigned q = v >> 5;
    const unsigned w = q == 0u ? w0 : q == 1u ? w1 : q == 2u ? w2 : q == 3u ? w3 : q == 4u ? w4 : q == 5u ? w5 : q == 6u ? w6 : w7;
    return (w >> (v & 31u)) & 1u;
  }
};

// border(m) = m & ~erode(m), m = member(x), 6-neighbour cross, outside the volume = 0; count += number of border voxels
template <class Member>
__global__ __launch_bounds__(256) void border_kernel(const unsigned char* __restrict__ x, Member member, unsigned char* __restrict__ border,
                                                     unsigned long long* __restrict__ count, int D, int H, int W) {
  const long long n = (long long)D * H * W, hw = (long long)H * W;
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  bool b = false;
  if (i < n) {
    const int w = (int)(i % W), h = (int)((i / W) % H), d = (int)(i / hw);
    if (member(x[i])) {
      const bool inner = d > 0 && d < D - 1 && h > 0 && h < H - 1 && w > 0 && w < W - 1 &&
                         member(x[i - hw]) && member(x[i + hw]) && member(x[i - W]) &&
                         member(x[i + W]) && member(x[i - 1]) && member(x[i + 1]);
      b = !inner;
    }
    border[i] = b ? 1 : 0;
  }
  const unsigned long long votes = __ballot(b);
  if ((threadIdx.x & 63) == 0 && votes != 0ull) atomicAdd(count, (unsigned long long)__popcll(votes));
}

// tab[k] = ((k s)^2 in fp64) rounded once to fp32: the one rounding a pass adds to a term
__device__ __forceinline__ void fill_term_table(float* tab, int n, double s) {
  for (int k = threadIdx.x; k < n; k += 256) {
    const double t = (double)k * s;
    tab[k] = (float)(t * t);
  }
}

// One EDT pass along an axis that is NOT the contiguous one: out[i] = min_j g[j] + ((i - j) s)^2 over lines of n elements
// `stride` apart.  A workgroup stages tw neighbouring lines (threads across W: coalesced) of outer index blockIdx.y in LDS and
// writes them back in place.  FROM_MASK: g = 0 at set voxels of `mask`, +inf elsewhere (the first pass).
template <bool FROM_MASK>
__global__ __launch_bounds__(256) void edt_pass_strided_kernel(const unsigned char* __restrict__ mask, float* g, int n, long long stride,
                                                               long long outer_stride, int W, int tw, double s) {
  extern __shared__ float lds[];
  float* tab = lds;            // [n]
  float* col = lds + n;        // [n][tw]
  const int tx = threadIdx.x % tw, ty = threadIdx.x / tw, rows = 256 / tw;
  const int w = blockIdx.x * tw + tx;
  const long long base = (long long)blockIdx.y * outer_stride + w;
  fill_term_table(tab, n, s);
  if (w < W) {
    for (int j = ty; j < n; j += rows) {
      const long long a = base + (long long)j * stride;
      col[j * tw + tx] = FROM_MASK ? (mask[a] ? 0.f : INFINITY) : g[a];
    }
  }
  __syncthreads();
  if (w < W) {
    for (int i = ty; i < n; i += rows) {
      float m = INFINITY;
      for (int j = 0; j < n; ++j) {
        const int k = i > j ? i - j : j - i;
        m = fminf(m, col[j * tw + tx] + tab[k]);
      }
      g[base + (long long)i * stride] = m;
    }
  }
}

// The pass along the contiguous axis: a workgroup stages R whole rows (R * n consecutive floats) and writes them back in place
__global__ __launch_bounds__(256) void edt_pass_rows_kernel(float* g, int n, long long nrows, int R, double s) {
  extern __shared__ float lds[];
  float* tab = lds;            // [n]
  float* row = lds + n;        // [R][n]
  const long long r0 = (long long)blockIdx.x * R;
  const long long left = nrows - r0;
  const int items = (int)(left < R ? left : R) * n;
  float* p = g + r0 * n;
  fill_term_table(tab, n, s);
  for (int t = threadIdx.x; t < items; t += 256) row[t] = p[t];
  __syncthreads();
  for (int t = threadIdx.x; t < items; t += 256) {
    const int r = t / n, i = t - r * n;
    const float* line = row + r * n;
    float m = INFINITY;
    for (int j = 0; j < n; ++j) {
      const int k = i > j ? i - j : j - i;
      m = fminf(m, line[j] + tab[k]);
    }
    p[t] = m;
  }
}

// direction 0: d2 = dt2_b at border(a);  direction 1: d2 = dt2_a at border(b)
__global__ __launch_bounds__(sel::SWEEP_THREADS) void stats_partial_kernel(const unsigned char* __restrict__ border_a, const float* __restrict__ dt2_b,
                                                                     const unsigned char* __restrict__ border_b, const float* __restrict__ dt2_a,
                                                                     long long n, double thr, StatsWs* ws) {
  __shared__ double red[sel::SWEEP_THREADS][2][4];
  double acc[2][4] = {{0., 0., 0., 0.}, {0., 0., 0., 0.}};
  for (long long i = (long long)blockIdx.x * sel::SWEEP_THREADS + threadIdx.x; i < n; i += (long long)gridDim.x * sel::SWEEP_THREADS) {
#pragma unroll
    for (int dir = 0; dir < 2; ++dir) {
      if ((dir == 0 ? border_a : border_b)[i]) {
        const double d2 = (double)(dir == 0 ? dt2_b : dt2_a)[i];
        const double d = sqrt(d2);
        acc[dir][0] += 1.;
        acc[dir][1] += d;
        acc[dir][2] = fmax(acc[dir][2], d2);
        acc[dir][3] += d <= thr ? 1. : 0.;
      }
    }
  }
  for (int q = 0; q < 8; ++q) red[threadIdx.x][q >> 2][q & 3] = acc[q >> 2][q & 3];
  __syncthreads();
  for (int half = sel::SWEEP_THREADS / 2; half > 0; half >>= 1) {      // a fixed tree: the same association order on every run
    if ((int)threadIdx.x < half) {
      for (int dir = 0; dir < 2; ++dir) {
        red[threadIdx.x][dir][0] += red[threadIdx.x + half][dir][0];
        red[threadIdx.x][dir][1] += red[threadIdx.x + half][dir][1];
        red[threadIdx.x][dir][2] = fmax(red[threadIdx.x][dir][2], red[threadIdx.x + half][dir][2]);
        red[threadIdx.x][dir][3] += red[threadIdx.x + half][dir][3];
      }
    }
    __syncthreads();
  }
  if (threadIdx.x < 8) ws->part[blockIdx.x][threadIdx.x >> 2][threadIdx.x & 3] = red[0][threadIdx.x >> 2][threadIdx.x & 3];
}

// out[0..7] = per direction: count, sum d, max d, count d <= threshold; the partials are added in workgroup order
__global__ void stats_final_kernel(const StatsWs* ws, int nblocks, double* out) {
  if (threadIdx.x >= 2) return;
  const int dir = threadIdx.x;
  double c = 0., s = 0., m = 0., le = 0.;
  for (int b = 0; b < nblocks; ++b) {
    c += ws->part[b][dir][0];
    s += ws->part[b][dir][1];
    m = fmax(m, ws->part[b][dir][2]);
    le += ws->part[b][dir][3];
  }
  out[dir * 4 + 0] = c;
  out[dir * 4 + 1] = s;
  out[dir * 4 + 2] = sqrt(m);
  out[dir * 4 + 3] = le;
}

// One sweep of the radix select (e2e_select.h) over the concatenation of both directions.  Non-negative floats order like their bit
// patterns and sqrt is monotone, so the select runs on the raw bits of d2.
__global__ __launch_bounds__(sel::SWEEP_THREADS) void select_hist_kernel(const unsigned char* __restrict__ border_a, const float* __restrict__ dt2_b,
                                                                        const unsigned char* __restrict__ border_b, const float* __restrict__ dt2_a,
                                                                        long long n, int pass, StatsWs* ws) {
  __shared__ unsigned bins[2][256];
  const sel::Sweep<2> sw = sel::sweep_begin(bins, &ws->select, 2);
  for (long long i = (long long)blockIdx.x * sel::SWEEP_THREADS + threadIdx.x; i < n; i += (long long)gridDim.x * sel::SWEEP_THREADS) {
#pragma unroll
    for (int dir = 0; dir < 2; ++dir)
      if ((dir == 0 ? border_a : border_b)[i]) sel::sweep_add(bins, sw, pass, __float_as_uint((dir == 0 ? dt2_b : dt2_a)[i]));
  }
  sel::sweep_flush(bins, &ws->select, pass);
}

struct SqrtOfBits {                    // the distance behind the decided bits of a d2
  __device__ __forceinline__ double operator()(unsigned bits) const { return sqrt((double)__uint_as_float(bits)); }
};

bool dims_ok(const char* what, int D, int H, int W) {
  if (D < 1 || H < 1 || W < 1) {
    e2e::set_error("%s: every axis needs at least one voxel (got %d x %d x %d)", what, D, H, W);
    return false;
  }
  return true;
}

template <class Member>
int launch_border(const char* what, const unsigned char* labels, Member member, unsigned char* border, long long* count, int D, int H, int W,
                  void* stream) {
  if (!dims_ok(what, D, H, W)) return E2E_ERR_ARG;
  E2E_REQUIRE(labels && border && count, "%s: null pointer", what);
  const long long n = (long long)D * H * W;
  E2E_REQUIRE(e2e::cdivll(n, 256) <= 0x7FFFFFFFll, "%s: volume too large (%lld voxels)", what, n);
  hipStream_t st = (hipStream_t)stream;
  e2e::zero_async(count, 8, st);
  hipLaunchKernelGGL(border_kernel<Member>, dim3((unsigned)e2e::cdivll(n, 256)), dim3(256), 0, st, labels, member, border,
                     (unsigned long long*)count, D, H, W);
  return e2e::check_launch("border_kernel");
}

}  // namespace

extern "C" int e2e_surface_border(const unsigned char* labels, int label, unsigned char* border, long long* count, int D, int H,
                                  int W, void* stream) {
  E2E_REQUIRE(label >= 0 && label <= 255, "surface_border: label %d is outside a uint8 volume's range", label);
  return launch_border("surface_border", labels, IsLabel{label}, border, count, D, H, W, stream);
}

extern "C" int e2e_surface_border_set(const unsigned char* labels, const unsigned* members, unsigned char* border, long long* count, int D,
                                      int H, int W, void* stream) {
  E2E_REQUIRE(members, "surface_border_set: null pointer");
  const InSet set{members[0], members[1], members[2], members[3], members[4], members[5], members[6], members[7]};
  return launch_border("surface_border_set", labels, set, border, count, D, H, W, stream);
}

extern "C" int e2e_surface_max_line(void) { return MAX_LINE; }

extern "C" int e2e_distance_transform_edt_sq(const unsigned char* mask, float* dt2, int D, int H, int W, double sd, double sh,
                                             double sw, void* stream) {
  if (!dims_ok("distance_transform_edt_sq", D, H, W)) return E2E_ERR_ARG;
  E2E_REQUIRE(mask && dt2, "distance_transform_edt_sq: null pointer");
  E2E_REQUIRE(std::isfinite(sd) && std::isfinite(sh) && std::isfinite(sw) && sd > 0. && sh > 0. && sw > 0.,
              "distance_transform_edt_sq: spacing must be positive and finite (got %g %g %g)", sd, sh, sw);
  if (D > MAX_LINE || H > MAX_LINE || W > MAX_LINE) {
    e2e::set_error("distance_transform_edt_sq: an axis of %d x %d x %d is longer than the %d voxels a pass stages in LDS", D, H, W,
                   MAX_LINE);
    return E2E_ERR_UNSUPPORTED;
  }
  hipStream_t st = (hipStream_t)stream;
  const long long hw = (long long)H * W;
  auto tile_w = [](int n) { return n * (64 + 1) <= LDS_FLOATS ? 64 : n * (32 + 1) <= LDS_FLOATS ? 32 : 16; };
  {  // along D, from the mask
    const int tw = tile_w(D);
    hipLaunchKernelGGL(edt_pass_strided_kernel<true>, dim3((unsigned)e2e::cdiv(W, tw), (unsigned)H), dim3(256),
                       (size_t)D * (tw + 1) * sizeof(float), st, mask, dt2, D, hw, (long long)W, W, tw, sd);
    if (int rc = e2e::check_launch("edt_pass_strided_kernel<mask>")) return rc;
  }
  if (H > 1) {
    const int tw = tile_w(H);
    hipLaunchKernelGGL(edt_pass_strided_kernel<false>, dim3((unsigned)e2e::cdiv(W, tw), (unsigned)D), dim3(256),
                       (size_t)H * (tw + 1) * sizeof(float), st, mask, dt2, H, (long long)W, hw, W, tw, sh);
    if (int rc = e2e::check_launch("edt_pass_strided_kernel")) return rc;
  }
  if (W > 1) {
    const long long nrows = (long long)D * H;
    const int R = 4096 / W > 1 ? 4096 / W : 1;
    hipLaunchKernelGGL(edt_pass_rows_kernel, dim3((unsigned)e2e::cdivll(nrows, R)), dim3(256), (size_t)(R + 1) * W * sizeof(float), st,
                       dt2, W, nrows, R, sw);
    if (int rc = e2e::check_launch("edt_pass_rows_kernel")) return rc;
  }
  return E2E_OK;
}

extern "C" long long e2e_surface_distances_ws_bytes(void) { return (long long)sizeof(StatsWs); }

extern "C" int e2e_surface_distances_stats(const unsigned char* border_a, const float* dt2_b, const unsigned char* border_b,
                                           const float* dt2_a, long long n, double threshold, long long rank_lo, long long rank_hi,
                                           double* out, void* ws, void* stream) {
  E2E_REQUIRE(border_a && dt2_b && border_b && dt2_a && out && ws, "surface_distances_stats: null pointer");
  E2E_REQUIRE(n > 0, "surface_distances_stats: need at least one voxel (got %lld)", n);
  E2E_REQUIRE(rank_lo >= 0 && rank_hi >= rank_lo && rank_hi <= 2 * n - 1,
              "surface_distances_stats: need 0 <= rank_lo <= rank_hi < 2 n (got %lld, %lld, n %lld)", rank_lo, rank_hi, n);
  E2E_REQUIRE(!(threshold != threshold), "surface_distances_stats: threshold is NaN");
  hipStream_t st = (hipStream_t)stream;
  StatsWs* w = (StatsWs*)ws;
  const int nb = sel::sweep_blocks(n);
  sel::start(&w->select, sel::Ranks<2>{{(unsigned long long)rank_lo, (unsigned long long)rank_hi}}, st);
  hipLaunchKernelGGL(stats_partial_kernel, dim3(nb), dim3(sel::SWEEP_THREADS), 0, st, border_a, dt2_b, border_b, dt2_a, n, threshold, w);
  hipLaunchKernelGGL(stats_final_kernel, dim3(1), dim3(64), 0, st, w, nb, out);
  if (int rc = e2e::check_launch("stats_kernels")) return rc;
  for (int pass = 0; pass < sel::PASSES; ++pass) {
    hipLaunchKernelGGL(select_hist_kernel, dim3(nb), dim3(sel::SWEEP_THREADS), 0, st, border_a, dt2_b, border_b, dt2_a, n, pass, w);
    sel::step(&w->select, pass, 2, SqrtOfBits{}, out + 8, st);
  }
  return e2e::check_launch("select_kernels");
}
