// P4: the dataset fingerprint of a cropped training folder on the device (gfx950).
// Reference: e2enet/experiment_planning/DatasetAnalyzer.py:161-179.  _get_voxels_in_foreground keeps every tenth foreground voxel of a
// case in raster order (modality[seg > 0][::10]); _compute_stats takes median, mean, sd, min, max and two percentiles of such a
// sample, or of all cases' samples behind one another.  The cropped case [C + 1, X, Y, Z] (seg last) is where the upload left it.
//
// The raster rank of a foreground voxel comes from e2e_rank.h, with one count row; the order statistics from e2e_select.h.
//
//   e2e_fingerprint_sample_count    a workgroup writes how many voxels of its chunk are > 0; one workgroup then scans the per-chunk
//                                   counts into exclusive 64-bit offsets and the total n_fg
//   e2e_fingerprint_sample_gather   a workgroup whose [offset, offset + count) holds no multiple of the stride leaves before it
//                                   reads a voxel.  Otherwise every foreground voxel recomputes its raster rank r and, where
//                                   r % stride == 0, copies all C modalities to column r / stride: the seg is read once for all
//   e2e_fingerprint_stats           NaN count, min, max and the fp64 sum in one sweep, the fp64 sum of (x - mean)^2 in a second, from
//                                   fixed per-workgroup partials added in workgroup order; then the radix select on the
//                                   order-preserving key of the fp32 bit pattern, four sweeps for up to 8 ranks at once
// Every loop's trip count is fixed by the arguments, every output element has one writer, atomics are histogram increments on
// integers only: the same bits on every run.  All indices, offsets and counts are 64-bit.
#include "e2e_rank.h"
#include "e2e_select.h"
#include <cmath>

namespace {

namespace rk = e2e::rank;
namespace sel = e2e::select;

constexpr int FP_MAX_STRIDE = 1 << 30;                         // rank arithmetic inside a chunk stays 32-bit
constexpr int FP_MAX_RANKS = 8;
constexpr long long FP_MAX_VALUES = 0xFFFFFFFFll;              // a histogram bin is 32 bits wide

// ws of e2e_fingerprint_stats
struct FpStatsWs {
  double part[sel::SWEEP_BLOCKS][4];           // per workgroup: NaN count, min, max, sum; second sweep: [0] = sum of (x - mean)^2
  double mean;
  sel::State<FP_MAX_RANKS> select;
};

struct IsForeground {                  // seg > 0 (a NaN is not)
  __device__ __forceinline__ bool operator()(float v) const { return v > 0.f; }
};

// counts[chunk] = foreground voxels of the chunk
__global__ __launch_bounds__(rk::THREADS) void fp_count_kernel(const float* __restrict__ seg, long long n, unsigned* __restrict__ counts) {
  const long long blk = blockIdx.x;
  float v[rk::ITERS];
  rk::load_chunk(seg, n, blk * rk::CHUNK, v);
  const unsigned tot = rk::wave_matches(v, IsForeground{});
  __shared__ unsigned sh[rk::WAVES];
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = tot;
  __syncthreads();
  if (threadIdx.x == 0) counts[blk] = sh[0] + sh[1] + sh[2] + sh[3];
}

// out[c * out_len + r / stride] = data[c * n + voxel] for the foreground voxel of raster rank r, r % stride == 0
__global__ __launch_bounds__(rk::THREADS) void fp_gather_kernel(const float* __restrict__ data, const float* __restrict__ seg, int C, long long n,
                                                               unsigned stride, long long out_len, const unsigned* __restrict__ counts,
                                                               const unsigned long long* __restrict__ offsets, float* __restrict__ out) {
  const long long blk = blockIdx.x;
  const unsigned cnt = counts[blk];
  if (cnt == 0u) return;                                       // (the same for the whole workgroup, like every return below)
  const unsigned long long lo = offsets[blk];
  const unsigned long long q0 = lo / stride;
  const unsigned rem0 = (unsigned)(lo - q0 * stride);
  if ((rem0 == 0u ? 0u : stride - rem0) >= cnt) return;        // the chunk's first sampled rank lies behind its last voxel
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  float v[rk::ITERS];
  rk::load_chunk(seg, n, blk * rk::CHUNK, v);
  __shared__ unsigned wtot[rk::ITERS * rk::WAVES];
  const unsigned ex = rk::matches_before(v, IsForeground{}, wtot, lane, wave);
#pragma unroll
  for (int it = 0; it < rk::ITERS; ++it) {
    const bool m = IsForeground{}(v[it]);
    const unsigned long long bits = __ballot(m);
    const unsigned local = rem0 + rk::rank_in_chunk(ex, it, wave, bits, lane);   // < stride + CHUNK: 32 bits
    if (!m) continue;
    const unsigned q = local / stride;
    if (local - q * stride != 0u) continue;
    const long long slot = (long long)q0 + (long long)q;
    if (slot >= out_len) continue;                             // (an out_len below ceil(n_fg / stride): a bad call writes less)
    const long long idx = blk * rk::CHUNK + (long long)(it * rk::THREADS + t);
    for (int c = 0; c < C; ++c) out[(long long)c * out_len + slot] = data[(long long)c * n + idx];
  }
}

// SWEEP 0: NaN count, min, max, sum (the NaNs left out);  SWEEP 1: sum of (x - mean)^2
template <int SWEEP>
__global__ __launch_bounds__(sel::SWEEP_THREADS) void fp_partial_kernel(const float* __restrict__ x, long long n, FpStatsWs* ws) {
  __shared__ double red[sel::SWEEP_THREADS][4];
  double nan = 0., mn = INFINITY, mx = -INFINITY, sum = 0.;
  const double mean = SWEEP == 1 ? ws->mean : 0.;
  for (long long i = (long long)blockIdx.x * sel::SWEEP_THREADS + threadIdx.x; i < n; i += (long long)gridDim.x * sel::SWEEP_THREADS) {
    const double v = (double)x[i];
    if (SWEEP == 0) {
      if (v != v) { nan += 1.; continue; }
      mn = fmin(mn, v);
      mx = fmax(mx, v);
      sum += v;
    } else {
      const double d = v - mean;
      sum += d * d;
    }
  }
  red[threadIdx.x][0] = nan; red[threadIdx.x][1] = mn; red[threadIdx.x][2] = mx; red[threadIdx.x][3] = sum;
  __syncthreads();
  for (int half = sel::SWEEP_THREADS / 2; half > 0; half >>= 1) {      // a fixed tree: the same association order on every run
    if ((int)threadIdx.x < half) {
      red[threadIdx.x][0] += red[threadIdx.x + half][0];
      red[threadIdx.x][1] = fmin(red[threadIdx.x][1], red[threadIdx.x + half][1]);
      red[threadIdx.x][2] = fmax(red[threadIdx.x][2], red[threadIdx.x + half][2]);
      red[threadIdx.x][3] += red[threadIdx.x + half][3];
    }
    __syncthreads();
  }
  if (SWEEP == 0) {
    if (threadIdx.x < 4) ws->part[blockIdx.x][threadIdx.x] = red[0][threadIdx.x];
  } else {
    if (threadIdx.x == 0) ws->part[blockIdx.x][0] = red[0][3];
  }
}

// the partials added in workgroup order.  SWEEP 0: out[0..3] = NaN count, min, max, sum and ws->mean = sum / n;  SWEEP 1: out[4]
template <int SWEEP>
__global__ void fp_final_kernel(FpStatsWs* ws, int nblocks, double n, double* out) {
  if (threadIdx.x != 0) return;
  if (SWEEP == 0) {
    double nan = 0., mn = INFINITY, mx = -INFINITY, sum = 0.;
    for (int b = 0; b < nblocks; ++b) {
      nan += ws->part[b][0];
      mn = fmin(mn, ws->part[b][1]);
      mx = fmax(mx, ws->part[b][2]);
      sum += ws->part[b][3];
    }
    out[0] = nan; out[1] = mn; out[2] = mx; out[3] = sum;
    ws->mean = sum / n;
  } else {
    double sum = 0.;
    for (int b = 0; b < nblocks; ++b) sum += ws->part[b][0];
    out[4] = sum;
    out[5] = out[6] = out[7] = 0.;
  }
}

// One sweep of the radix select: x is a flat array, every value takes part under its order-preserving key
__global__ __launch_bounds__(sel::SWEEP_THREADS) void fp_select_hist_kernel(const float* __restrict__ x, long long n, int pass, int nr, FpStatsWs* ws) {
  __shared__ unsigned bins[FP_MAX_RANKS][256];
  const sel::Sweep<FP_MAX_RANKS> sw = sel::sweep_begin(bins, &ws->select, nr);
  for (long long i = (long long)blockIdx.x * sel::SWEEP_THREADS + threadIdx.x; i < n; i += (long long)gridDim.x * sel::SWEEP_THREADS)
    sel::sweep_add(bins, sw, pass, sel::key(x[i]));
  sel::sweep_flush(bins, &ws->select, pass);
}

struct Unkeyed {                       // the order statistic behind a decided key
  __device__ __forceinline__ double operator()(unsigned k) const { return (double)sel::unkey(k); }
};

}  // namespace

extern "C" int e2e_fingerprint_sample_chunk(void) { return rk::CHUNK; }

extern "C" long long e2e_fingerprint_sample_ws_bytes(long long n) {
  if (n < 1 || rk::chunks(n) > rk::MAX_CHUNKS) return 0;
  return rk::ws_bytes(rk::chunks(n), 1);
}

extern "C" int e2e_fingerprint_sample_count(const float* seg, long long n, long long* n_fg, void* ws, void* stream) {
  E2E_REQUIRE(seg && n_fg && ws && n > 0, "fingerprint_sample_count: bad arguments");
  if (int e = rk::check_voxels("fingerprint_sample_count", n)) return e;
  const long long nb = rk::chunks(n);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(fp_count_kernel, dim3((unsigned)nb), dim3(rk::THREADS), 0, st, seg, n, (unsigned*)ws);
  if (int e = e2e::check_launch("fp_count_kernel")) return e;
  return rk::launch_scan(ws, nb, 1, n_fg, st);
}

extern "C" int e2e_fingerprint_sample_gather(const float* data, const float* seg, int C, long long n, int stride, float* out,
                                             long long out_len, const void* ws, void* stream) {
  E2E_REQUIRE(data && seg && ws && n > 0, "fingerprint_sample_gather: bad arguments");
  E2E_REQUIRE(C >= 1, "fingerprint_sample_gather: %d modalities, need at least one", C);
  E2E_REQUIRE(stride >= 1 && stride <= FP_MAX_STRIDE, "fingerprint_sample_gather: stride %d is outside 1 .. %d", stride, FP_MAX_STRIDE);
  E2E_REQUIRE(out_len >= 0 && (out || out_len == 0), "fingerprint_sample_gather: out_len %lld without an output", out_len);
  if (int e = rk::check_voxels("fingerprint_sample_gather", n)) return e;
  if (out_len == 0) return E2E_OK;                             // no foreground: nothing to write
  const long long nb = rk::chunks(n);
  hipLaunchKernelGGL(fp_gather_kernel, dim3((unsigned)nb), dim3(rk::THREADS), 0, (hipStream_t)stream, data, seg, C, n, (unsigned)stride,
                     out_len, (const unsigned*)ws, (const unsigned long long*)rk::ws_offsets(ws, nb, 1), out);
  return e2e::check_launch("fp_gather_kernel");
}

extern "C" int e2e_fingerprint_stats_max_ranks(void) { return FP_MAX_RANKS; }
extern "C" long long e2e_fingerprint_stats_ws_bytes(void) { return (long long)sizeof(FpStatsWs); }

extern "C" int e2e_fingerprint_stats(const float* x, long long n, const long long* ranks, int num_ranks, double* out, void* ws,
                                     void* stream) {
  E2E_REQUIRE(x && ranks && out && ws, "fingerprint_stats: null pointer");
  E2E_REQUIRE(n > 0, "fingerprint_stats: need at least one value (got %lld)", n);
  E2E_REQUIRE(num_ranks >= 1 && num_ranks <= FP_MAX_RANKS, "fingerprint_stats: %d ranks, one call serves 1 .. %d", num_ranks, FP_MAX_RANKS);
  if (n > FP_MAX_VALUES) {
    e2e::set_error("fingerprint_stats: %lld values are more than the %lld a 32-bit histogram bin counts", n, FP_MAX_VALUES);
    return E2E_ERR_UNSUPPORTED;
  }
  sel::Ranks<FP_MAX_RANKS> rk8 = {};
  for (int r = 0; r < num_ranks; ++r) {
    E2E_REQUIRE(ranks[r] >= 0 && ranks[r] < n, "fingerprint_stats: rank %lld is outside 0 .. n - 1 (n %lld)", ranks[r], n);
    rk8.k[r] = (unsigned long long)ranks[r];
  }
  hipStream_t st = (hipStream_t)stream;
  FpStatsWs* w = (FpStatsWs*)ws;
  const int nb = sel::sweep_blocks(n);
  sel::start(&w->select, rk8, st);
  hipLaunchKernelGGL(fp_partial_kernel<0>, dim3(nb), dim3(sel::SWEEP_THREADS), 0, st, x, n, w);
  hipLaunchKernelGGL(fp_final_kernel<0>, dim3(1), dim3(64), 0, st, w, nb, (double)n, out);
  hipLaunchKernelGGL(fp_partial_kernel<1>, dim3(nb), dim3(sel::SWEEP_THREADS), 0, st, x, n, w);
  hipLaunchKernelGGL(fp_final_kernel<1>, dim3(1), dim3(64), 0, st, w, nb, (double)n, out);
  if (int rc = e2e::check_launch("fingerprint_stats reductions")) return rc;
  for (int pass = 0; pass < sel::PASSES; ++pass) {
    hipLaunchKernelGGL(fp_select_hist_kernel, dim3(nb), dim3(sel::SWEEP_THREADS), 0, st, x, n, pass, num_ranks, w);
    sel::step(&w->select, pass, num_ranks, Unkeyed{}, out + 8, st);
  }
  return e2e::check_launch("fingerprint_stats select");
}
