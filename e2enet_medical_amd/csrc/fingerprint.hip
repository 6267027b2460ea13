// P4: the dataset fingerprint of a cropped training folder on the device (gfx950).
// Reference: e2enet/experiment_planning/DatasetAnalyzer.py:161-179.  _get_voxels_in_foreground keeps every tenth foreground voxel of a
// case in raster order (modality[seg > 0][::10]); _compute_stats takes median, mean, sd, min, max and two percentiles of such a
// sample, or of all cases' samples behind one another.  The cropped case [C + 1, X, Y, Z] (seg last) is where the upload left it.
//
//   e2e_fingerprint_sample_count    a workgroup owns FP_CHUNK consecutive voxels of the flat seg and writes how many of them are
//                                   > 0 (one 64-bit ballot and a popcount per 64 voxels); one workgroup then scans the per-chunk
//                                   counts into exclusive 64-bit offsets and the total n_fg
//   e2e_fingerprint_sample_gather   a workgroup whose [offset, offset + count) holds no multiple of the stride leaves before it
//                                   reads a voxel.  Otherwise every foreground voxel recomputes its raster rank r (ballot + popcount
//                                   inside a wave, wave totals through LDS) and, where r % stride == 0, copies all C modalities to
//                                   column r / stride: the seg is read once for all of them
//   e2e_fingerprint_stats           NaN count, min, max and the fp64 sum in one sweep, the fp64 sum of (x - mean)^2 in a second, from
//                                   fixed per-workgroup partials added in workgroup order; then a byte-wise radix select on the
//                                   order-preserving key of the fp32 bit pattern, four sweeps for up to 8 ranks at once
// Every loop's trip count is fixed by the arguments, every output element has one writer, atomics are histogram increments on
// integers only: the same bits on every run.  All indices, offsets and counts are 64-bit.
#include "e2e_common.h"
#include <cmath>

namespace {

constexpr int FP_THREADS = 256, FP_ITERS = 16, FP_WAVES = FP_THREADS / 64;
constexpr int FP_CHUNK = FP_THREADS * FP_ITERS;                // voxels per workgroup; wave w of pass `it` owns 64 consecutive ones
constexpr long long FP_MAX_BLOCKS = (1ll << 24) - 1;           // most chunks of one launch: 2^36 - 4096 voxels
constexpr int FP_MAX_STRIDE = 1 << 30;                         // rank arithmetic inside a chunk stays 32-bit
constexpr int SCAN_STEP = 256;                                 // chunks per iteration of the offset scan
constexpr int STAT_BLOCKS = 1024;                              // most workgroups of a reduction (fixed by n alone)
constexpr int STAT_THREADS = 256;
constexpr int FP_MAX_RANKS = 8;
constexpr long long FP_MAX_VALUES = 0xFFFFFFFFll;              // a histogram bin is 32 bits wide

// ws of e2e_fingerprint_stats
struct FpStatsWs {
  double part[STAT_BLOCKS][4];                 // per workgroup: NaN count, min, max, sum; second sweep: [0] = sum of (x - mean)^2
  double mean;
  unsigned hist[4][FP_MAX_RANKS][256];         // per select pass and rank: byte histogram of the keys that match the rank's prefix
  unsigned prefix[FP_MAX_RANKS];               // bits of the rank's order statistic decided so far
  unsigned long long k[FP_MAX_RANKS];          // rank inside the prefix's bucket
  int rep[FP_MAX_RANKS];                       // first rank with the same prefix: ranks that agree so far share its histogram
};

// voxel base + it * 256 + thread; 0 (background) behind the end of the volume
__device__ __forceinline__ void fp_load(const float* __restrict__ seg, long long n, long long base, float v[FP_ITERS]) {
#pragma unroll
  for (int it = 0; it < FP_ITERS; ++it) {
    const long long i = base + (long long)(it * FP_THREADS + (int)threadIdx.x);
    v[it] = i < n ? seg[i] : 0.f;
  }
}

// counts[chunk] = voxels of the chunk with seg > 0 (a NaN is not)
__global__ __launch_bounds__(FP_THREADS) void fp_count_kernel(const float* __restrict__ seg, long long n, unsigned* __restrict__ counts) {
  const long long blk = blockIdx.x;
  float v[FP_ITERS];
  fp_load(seg, n, blk * FP_CHUNK, v);
  unsigned tot = 0u;
#pragma unroll
  for (int it = 0; it < FP_ITERS; ++it) tot += (unsigned)__popcll(__ballot(v[it] > 0.f));
  __shared__ unsigned sh[FP_WAVES];
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = tot;
  __syncthreads();
  if (threadIdx.x == 0) counts[blk] = sh[0] + sh[1] + sh[2] + sh[3];
}

// inclusive sum over the lanes of a wave
template <typename T>
__device__ __forceinline__ T fp_wave_scan(T x, int lane) {
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const T y = __shfl_up(x, off, 64);
    if (lane >= off) x += y;
  }
  return x;
}

// one workgroup: offsets[chunk] = foreground voxels in front of the chunk, *total = all of them
__global__ __launch_bounds__(SCAN_STEP) void fp_scan_kernel(const unsigned* __restrict__ counts, unsigned long long* __restrict__ offsets,
                                                            long long nb, long long* __restrict__ total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __shared__ unsigned long long wsum[SCAN_STEP / 64];
  unsigned long long carry = 0ull;
  for (long long b0 = 0; b0 < nb; b0 += SCAN_STEP) {
    const long long b = b0 + threadIdx.x;
    const unsigned long long x = b < nb ? (unsigned long long)counts[b] : 0ull;
    const unsigned long long inc = fp_wave_scan(x, lane);
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    unsigned long long before = 0ull, all = 0ull;
#pragma unroll
    for (int w = 0; w < SCAN_STEP / 64; ++w) {
      const unsigned long long s = wsum[w];
      before += w < wave ? s : 0ull;
      all += s;
    }
    if (b < nb) offsets[b] = carry + before + inc - x;
    carry += all;
    __syncthreads();                                           // wsum is rewritten by the next step
  }
  if (threadIdx.x == 0) *total = (long long)carry;
}

// out[c * out_len + r / stride] = data[c * n + voxel] for the foreground voxel of raster rank r, r % stride == 0
__global__ __launch_bounds__(FP_THREADS) void fp_gather_kernel(const float* __restrict__ data, const float* __restrict__ seg, int C, long long n,
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
  float v[FP_ITERS];
  fp_load(seg, n, blk * FP_CHUNK, v);
  // foreground voxels per (pass, wave), in raster order at wtot[it * 4 + wave]
  __shared__ unsigned wtot[FP_ITERS * FP_WAVES];
  unsigned mine = 0u;
#pragma unroll
  for (int it = 0; it < FP_ITERS; ++it) {
    const unsigned tot = (unsigned)__popcll(__ballot(v[it] > 0.f));
    if (lane == it) mine = tot;
  }
  if (lane < FP_ITERS) wtot[lane * FP_WAVES + wave] = mine;
  __syncthreads();
  const unsigned x = wtot[lane];                               // (64 entries: one per lane)
  const unsigned ex = fp_wave_scan(x, lane) - x;               // lane it * 4 + w: the chunk's foreground voxels in front of (it, w)
#pragma unroll
  for (int it = 0; it < FP_ITERS; ++it) {
    const bool m = v[it] > 0.f;
    const unsigned long long bits = __ballot(m);
    const unsigned base = __shfl(ex, it * FP_WAVES + wave, 64);
    if (!m) continue;
    const unsigned local = rem0 + base + (unsigned)__popcll(bits & ((1ull << lane) - 1ull));   // < stride + FP_CHUNK: 32 bits
    const unsigned q = local / stride;
    if (local - q * stride != 0u) continue;
    const long long slot = (long long)q0 + (long long)q;
    if (slot >= out_len) continue;                             // (an out_len below ceil(n_fg / stride): a bad call writes less)
    const long long idx = blk * FP_CHUNK + (long long)(it * FP_THREADS + t);
    for (int c = 0; c < C; ++c) out[(long long)c * out_len + slot] = data[(long long)c * n + idx];
  }
}

// bit pattern -> unsigned key that orders like the floats: all bits of a negative flipped, the sign bit of the others
__device__ __forceinline__ unsigned fp_key(float x) {
  const unsigned b = __float_as_uint(x);
  return (b & 0x80000000u) ? ~b : b ^ 0x80000000u;
}
__device__ __forceinline__ float fp_unkey(unsigned k) { return __uint_as_float((k & 0x80000000u) ? k ^ 0x80000000u : ~k); }

// SWEEP 0: NaN count, min, max, sum (the NaNs left out);  SWEEP 1: sum of (x - mean)^2
template <int SWEEP>
__global__ __launch_bounds__(STAT_THREADS) void fp_partial_kernel(const float* __restrict__ x, long long n, FpStatsWs* ws) {
  __shared__ double red[STAT_THREADS][4];
  double nan = 0., mn = INFINITY, mx = -INFINITY, sum = 0.;
  const double mean = SWEEP == 1 ? ws->mean : 0.;
  for (long long i = (long long)blockIdx.x * STAT_THREADS + threadIdx.x; i < n; i += (long long)gridDim.x * STAT_THREADS) {
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
  for (int half = STAT_THREADS / 2; half > 0; half >>= 1) {      // a fixed tree: the same association order on every run
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

struct FpRanks { unsigned long long k[FP_MAX_RANKS]; };

__global__ void fp_select_init_kernel(FpStatsWs* ws, FpRanks ranks) {
  if (threadIdx.x < FP_MAX_RANKS) {
    ws->prefix[threadIdx.x] = 0u;
    ws->k[threadIdx.x] = ranks.k[threadIdx.x];
    ws->rep[threadIdx.x] = 0;                                  // nothing is decided: one histogram serves every rank
  }
}

// One pass of the byte-wise radix select (the scheme of surface.hip's select_hist_kernel, for up to 8 ranks): histogram of byte
// (24 - 8 pass) of the keys whose higher bytes equal a rank's prefix.  Ranks whose prefixes agree share the histogram of the first
// of them, so the first pass, where every key matches every rank, costs one increment per value.
__global__ __launch_bounds__(STAT_THREADS) void fp_select_hist_kernel(const float* __restrict__ x, long long n, int pass, int nr, FpStatsWs* ws) {
  __shared__ unsigned hist[FP_MAX_RANKS][256];
#pragma unroll
  for (int r = 0; r < FP_MAX_RANKS; ++r) hist[r][threadIdx.x] = 0u;
  __syncthreads();
  const int sft = 24 - 8 * pass;
  const unsigned mask = pass == 0 ? 0u : 0xFFFFFFFFu << (sft + 8);
  unsigned prefix[FP_MAX_RANKS];
  bool own[FP_MAX_RANKS];
#pragma unroll
  for (int r = 0; r < FP_MAX_RANKS; ++r) {
    prefix[r] = ws->prefix[r];
    own[r] = r < nr && ws->rep[r] == r;
  }
  for (long long i = (long long)blockIdx.x * STAT_THREADS + threadIdx.x; i < n; i += (long long)gridDim.x * STAT_THREADS) {
    const unsigned key = fp_key(x[i]);
    const unsigned byte = (key >> sft) & 255u;
#pragma unroll
    for (int r = 0; r < FP_MAX_RANKS; ++r)
      if (own[r] && (key & mask) == prefix[r]) atomicAdd(&hist[r][byte], 1u);
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < FP_MAX_RANKS; ++r)
    if (hist[r][threadIdx.x]) atomicAdd(&ws->hist[pass][r][threadIdx.x], hist[r][threadIdx.x]);
}

// picks the bucket of each rank from the pass's histogram; after the last pass out[8 + r] = the rank's order statistic
__global__ void fp_select_step_kernel(FpStatsWs* ws, int pass, int nr, double* out) {
  const int r = threadIdx.x;
  const int sft = 24 - 8 * pass;
  if (r < nr) {
    const int h = ws->rep[r];
    unsigned long long kk = ws->k[r], cum = 0ull;
    int b = 0;
    for (; b < 256; ++b) {
      const unsigned long long c = ws->hist[pass][h][b];
      if (cum + c > kk) break;
      cum += c;
    }
    if (b > 255) b = 255;
    ws->k[r] = kk - cum;
    const unsigned prefix = ws->prefix[r] | ((unsigned)b << sft);
    ws->prefix[r] = prefix;
    if (pass == 3) out[8 + r] = (double)fp_unkey(prefix);
  } else if (r < FP_MAX_RANKS && pass == 3) {
    out[8 + r] = 0.;
  }
  __syncthreads();                                             // every rank has read its histogram's owner and written its prefix
  if (r == 0) {
    for (int a = 0; a < nr; ++a) {
      int first = a;
      for (int c = a - 1; c >= 0; --c)
        if (ws->prefix[c] == ws->prefix[a]) first = c;
      ws->rep[a] = first;
    }
  }
}

inline long long fp_blocks(long long n) { return e2e::cdivll(n, FP_CHUNK); }
inline long long fp_counts_bytes(long long nb) { return (nb * 4 + 15) / 16 * 16; }

int fp_stat_blocks(long long n) {
  const long long b = e2e::cdivll(n, STAT_THREADS);
  return (int)(b < STAT_BLOCKS ? b : STAT_BLOCKS);
}

}  // namespace

extern "C" int e2e_fingerprint_sample_chunk(void) { return FP_CHUNK; }

extern "C" long long e2e_fingerprint_sample_ws_bytes(long long n) {
  if (n < 1 || fp_blocks(n) > FP_MAX_BLOCKS) return 0;
  const long long nb = fp_blocks(n);
  return fp_counts_bytes(nb) + nb * 8;
}

extern "C" int e2e_fingerprint_sample_count(const float* seg, long long n, long long* n_fg, void* ws, void* stream) {
  E2E_REQUIRE(seg && n_fg && ws && n > 0, "fingerprint_sample_count: bad arguments");
  const long long nb = fp_blocks(n);
  if (nb > FP_MAX_BLOCKS) {
    e2e::set_error("fingerprint_sample_count: %lld voxels are more than the %lld one launch covers", n, FP_MAX_BLOCKS * FP_CHUNK);
    return E2E_ERR_UNSUPPORTED;
  }
  unsigned* cnt = (unsigned*)ws;
  unsigned long long* offs = (unsigned long long*)((char*)ws + fp_counts_bytes(nb));
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(fp_count_kernel, dim3((unsigned)nb), dim3(FP_THREADS), 0, st, seg, n, cnt);
  if (int e = e2e::check_launch("fp_count_kernel")) return e;
  hipLaunchKernelGGL(fp_scan_kernel, dim3(1), dim3(SCAN_STEP), 0, st, (const unsigned*)cnt, offs, nb, n_fg);
  return e2e::check_launch("fp_scan_kernel");
}

extern "C" int e2e_fingerprint_sample_gather(const float* data, const float* seg, int C, long long n, int stride, float* out,
                                             long long out_len, const void* ws, void* stream) {
  E2E_REQUIRE(data && seg && ws && n > 0, "fingerprint_sample_gather: bad arguments");
  E2E_REQUIRE(C >= 1, "fingerprint_sample_gather: %d modalities, need at least one", C);
  E2E_REQUIRE(stride >= 1 && stride <= FP_MAX_STRIDE, "fingerprint_sample_gather: stride %d is outside 1 .. %d", stride, FP_MAX_STRIDE);
  E2E_REQUIRE(out_len >= 0 && (out || out_len == 0), "fingerprint_sample_gather: out_len %lld without an output", out_len);
  const long long nb = fp_blocks(n);
  if (nb > FP_MAX_BLOCKS) {
    e2e::set_error("fingerprint_sample_gather: %lld voxels are more than the %lld one launch covers", n, FP_MAX_BLOCKS * FP_CHUNK);
    return E2E_ERR_UNSUPPORTED;
  }
  if (out_len == 0) return E2E_OK;                             // no foreground: nothing to write
  const unsigned* cnt = (const unsigned*)ws;
  const unsigned long long* offs = (const unsigned long long*)((const char*)ws + fp_counts_bytes(nb));
  hipLaunchKernelGGL(fp_gather_kernel, dim3((unsigned)nb), dim3(FP_THREADS), 0, (hipStream_t)stream, data, seg, C, n, (unsigned)stride,
                     out_len, cnt, offs, out);
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
  FpRanks rk = {};
  for (int r = 0; r < num_ranks; ++r) {
    E2E_REQUIRE(ranks[r] >= 0 && ranks[r] < n, "fingerprint_stats: rank %lld is outside 0 .. n - 1 (n %lld)", ranks[r], n);
    rk.k[r] = (unsigned long long)ranks[r];
  }
  hipStream_t st = (hipStream_t)stream;
  FpStatsWs* w = (FpStatsWs*)ws;
  const int nb = fp_stat_blocks(n);
  e2e::zero_async(&w->hist[0][0][0], sizeof(w->hist), st);
  hipLaunchKernelGGL(fp_select_init_kernel, dim3(1), dim3(64), 0, st, w, rk);
  hipLaunchKernelGGL(fp_partial_kernel<0>, dim3(nb), dim3(STAT_THREADS), 0, st, x, n, w);
  hipLaunchKernelGGL(fp_final_kernel<0>, dim3(1), dim3(64), 0, st, w, nb, (double)n, out);
  hipLaunchKernelGGL(fp_partial_kernel<1>, dim3(nb), dim3(STAT_THREADS), 0, st, x, n, w);
  hipLaunchKernelGGL(fp_final_kernel<1>, dim3(1), dim3(64), 0, st, w, nb, (double)n, out);
  if (int rc = e2e::check_launch("fingerprint_stats reductions")) return rc;
  for (int pass = 0; pass < 4; ++pass) {
    hipLaunchKernelGGL(fp_select_hist_kernel, dim3(nb), dim3(STAT_THREADS), 0, st, x, n, pass, num_ranks, w);
    hipLaunchKernelGGL(fp_select_step_kernel, dim3(1), dim3(64), 0, st, w, pass, num_ranks, out);
  }
  return e2e::check_launch("fingerprint_stats select");
}
