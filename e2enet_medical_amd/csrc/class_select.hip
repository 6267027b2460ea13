// P3: the class-location sampling of a preprocessed training case on the device (gfx950).
// Reference: e2enet/preprocessing/preprocessing.py:343-361 (GenericPreprocessor._run_internal): per class np.argwhere(seg == c), which
// lists the class's voxels in raster order, then RandomState(1234).choice(n, t, replace=False) rows of it.  The label volume is
// where resample_and_normalize left it, on the device; only the K class totals go down and only the drawn ranks come up.
//
//   e2e_pp_select_count    a workgroup owns SEL_CHUNK consecutive voxels of the flat fp32 volume and writes how many of them equal
//                          each class (one 64-bit ballot and a popcount per class and 64 voxels); one workgroup per class then scans
//                          the per-chunk counts into exclusive 64-bit offsets and the class total
//   e2e_pp_select_coords   the host has drawn ranks into the raster order of each class and sorted them.  A workgroup looks up which
//                          of a class's ranks fall into its own [offset, offset + count); without any it leaves before it reads a
//                          voxel.  Otherwise it recomputes the rank of its matching voxels (ballot + popcount inside a wave, wave
//                          totals through LDS) and every voxel whose rank was drawn writes its (i, j, k) into the row of the draw
// Every output row has exactly one writer and nothing is accumulated with atomics: the same bits on every run.  The volume is read
// once per pass whatever K is; all indices, offsets and counts are 64-bit.
#include "e2e_common.h"

namespace {

constexpr int SEL_THREADS = 256, SEL_ITERS = 16;
constexpr int SEL_CHUNK = SEL_THREADS * SEL_ITERS;             // voxels per workgroup; wave w of pass `it` owns 64 consecutive ones
constexpr int SEL_MAX_CLASSES = 64;                            // one lane per class holds its count
constexpr long long SEL_MAX_BLOCKS = (1ll << 24) - 1;          // grid limit of a 256-thread launch: 2^36 - 4096 voxels
constexpr int SCAN_STEP = 256;                                 // chunks per iteration of the offset scan

struct SelClasses { float c[SEL_MAX_CLASSES]; };
struct SelOffsets { long long o[SEL_MAX_CLASSES + 1]; };       // class k's ranks, slots and output rows are [o[k], o[k + 1])

// voxel base + it * 256 + thread; NaN (equal to no class) behind the end of the volume
__device__ __forceinline__ void sel_load(const float* __restrict__ seg, long long n, long long base, float v[SEL_ITERS]) {
#pragma unroll
  for (int it = 0; it < SEL_ITERS; ++it) {
    const long long i = base + (long long)(it * SEL_THREADS + (int)threadIdx.x);
    v[it] = i < n ? seg[i] : __builtin_nanf("");
  }
}

// counts[k * nb + chunk]
__global__ __launch_bounds__(SEL_THREADS) void pp_select_count_kernel(const float* __restrict__ seg, long long n, SelClasses cls, int K,
                                                                      long long nb, unsigned* __restrict__ counts) {
  const long long blk = blockIdx.x;
  float v[SEL_ITERS];
  sel_load(seg, n, blk * SEL_CHUNK, v);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned mine = 0u;                                          // lane k: this wave's voxels of class k
  for (int k = 0; k < K; ++k) {
    const float c = cls.c[k];
    unsigned tot = 0u;
#pragma unroll
    for (int it = 0; it < SEL_ITERS; ++it) tot += (unsigned)__popcll(__ballot(v[it] == c));
    if (lane == k) mine = tot;
  }
  __shared__ unsigned sh[SEL_THREADS / 64][SEL_MAX_CLASSES];
  sh[wave][lane] = mine;
  __syncthreads();
  const int t = threadIdx.x;
  if (t < K) counts[(long long)t * nb + blk] = sh[0][t] + sh[1][t] + sh[2][t] + sh[3][t];
}

// inclusive sum over the lanes of a wave
__device__ __forceinline__ unsigned long long wave_scan_u64(unsigned long long x, int lane) {
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const unsigned long long y = __shfl_up(x, off, 64);
    if (lane >= off) x += y;
  }
  return x;
}

// one workgroup per class: offsets[k * nb + chunk] = number of the class's voxels in front of the chunk, totals[k] = all of them
__global__ __launch_bounds__(SCAN_STEP) void pp_select_scan_kernel(const unsigned* __restrict__ counts, unsigned long long* __restrict__ offsets,
                                                                   long long nb, long long* __restrict__ totals) {
  const unsigned* c = counts + (long long)blockIdx.x * nb;
  unsigned long long* o = offsets + (long long)blockIdx.x * nb;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __shared__ unsigned long long wsum[SCAN_STEP / 64];
  unsigned long long carry = 0ull;
  for (long long b0 = 0; b0 < nb; b0 += SCAN_STEP) {
    const long long b = b0 + threadIdx.x;
    const unsigned long long x = b < nb ? (unsigned long long)c[b] : 0ull;
    const unsigned long long inc = wave_scan_u64(x, lane);
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    unsigned long long before = 0ull, all = 0ull;
#pragma unroll
    for (int w = 0; w < SCAN_STEP / 64; ++w) {
      const unsigned long long s = wsum[w];
      before += w < wave ? s : 0ull;
      all += s;
    }
    if (b < nb) o[b] = carry + before + inc - x;
    carry += all;
    __syncthreads();                                           // wsum is rewritten by the next step
  }
  if (threadIdx.x == 0) totals[blockIdx.x] = (long long)carry;
}

// first p in [lo, hi) with a[p] >= x, or hi
__device__ __forceinline__ long long sel_lower_bound(const long long* __restrict__ a, long long lo, long long hi, long long x) {
  while (lo < hi) {
    const long long mid = lo + ((hi - lo) >> 1);
    if (a[mid] < x) lo = mid + 1; else hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(SEL_THREADS) void pp_select_coords_kernel(const float* __restrict__ seg, long long n, long long HW, long long W,
                                                                       SelClasses cls, SelOffsets off, int K, long long nb,
                                                                       const unsigned* __restrict__ counts,
                                                                       const unsigned long long* __restrict__ offsets,
                                                                       const long long* __restrict__ ranks, const long long* __restrict__ slots,
                                                                       long long* __restrict__ out) {
  const long long blk = blockIdx.x;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  __shared__ long long p_lo[SEL_MAX_CLASSES], p_hi[SEL_MAX_CLASSES], first[SEL_MAX_CLASSES];
  __shared__ unsigned wtot[SEL_ITERS * (SEL_THREADS / 64)];
  __shared__ int any;
  if (t == 0) any = 0;
  __syncthreads();
  if (t < K) {                                                 // thread k: the drawn ranks of class k that lie in this chunk
    long long a = 0, b = 0, lo = 0;
    const unsigned cnt = counts[(long long)t * nb + blk];
    if (cnt != 0u) {
      lo = (long long)offsets[(long long)t * nb + blk];
      a = sel_lower_bound(ranks, off.o[t], off.o[t + 1], lo);
      b = sel_lower_bound(ranks, a, off.o[t + 1], lo + (long long)cnt);
      if (b > a) any = 1;                                      // (every writer writes 1)
    }
    p_lo[t] = a; p_hi[t] = b; first[t] = lo;
  }
  __syncthreads();
  if (any == 0) return;
  float v[SEL_ITERS];
  sel_load(seg, n, blk * SEL_CHUNK, v);
  for (int k = 0; k < K; ++k) {
    const long long a = p_lo[k], b = p_hi[k];
    if (b <= a) continue;                                      // (the same for the whole workgroup)
    const float c = cls.c[k];
    // matching voxels per (pass, wave), in raster order at wtot[it * 4 + wave]
    unsigned mine = 0u;
#pragma unroll
    for (int it = 0; it < SEL_ITERS; ++it) {
      const unsigned tot = (unsigned)__popcll(__ballot(v[it] == c));
      if (lane == it) mine = tot;
    }
    if (lane < SEL_ITERS) wtot[lane * (SEL_THREADS / 64) + wave] = mine;
    __syncthreads();
    const unsigned long long x = wtot[lane];                   // (64 entries: one per lane)
    const unsigned long long ex = wave_scan_u64(x, lane) - x;  // lane it * 4 + w: the class's voxels of this chunk in front of (it, w)
    __syncthreads();                                           // wtot is rewritten for the next class
    const long long row0 = off.o[k], rows = off.o[k + 1] - off.o[k], lo = first[k];
#pragma unroll
    for (int it = 0; it < SEL_ITERS; ++it) {
      const bool m = v[it] == c;
      const unsigned long long bits = __ballot(m);
      const unsigned long long base = __shfl(ex, it * (SEL_THREADS / 64) + wave, 64);
      if (!m) continue;
      const long long r = lo + (long long)base + (long long)__popcll(bits & ((1ull << lane) - 1ull));
      const long long p = sel_lower_bound(ranks, a, b, r);
      if (p >= b || ranks[p] != r) continue;
      const long long slot = slots[p];
      if (slot < 0 || slot >= rows) continue;                  // (a slot outside the class's rows: a bad call writes nothing)
      const long long idx = blk * SEL_CHUNK + (long long)(it * SEL_THREADS + t);
      const long long i = idx / HW, rem = idx - i * HW, j = rem / W;
      long long* o = out + (row0 + slot) * 3;
      o[0] = i; o[1] = j; o[2] = rem - j * W;
    }
  }
}

inline long long sel_blocks(long long n) { return e2e::cdivll(n, SEL_CHUNK); }
inline long long sel_counts_bytes(long long nb, int K) { return ((long long)K * nb * 4 + 15) / 16 * 16; }

}  // namespace

extern "C" int e2e_pp_select_chunk(void) { return SEL_CHUNK; }
extern "C" int e2e_pp_select_max_classes(void) { return SEL_MAX_CLASSES; }

extern "C" long long e2e_pp_select_ws_bytes(long long n, int K) {
  if (n < 1 || K < 1 || K > SEL_MAX_CLASSES || sel_blocks(n) > SEL_MAX_BLOCKS) return 0;
  const long long nb = sel_blocks(n);
  return sel_counts_bytes(nb, K) + (long long)K * nb * 8;
}

extern "C" int e2e_pp_select_count(const float* seg, long long n, const float* classes, int K, long long* counts, void* ws, void* stream) {
  E2E_REQUIRE(seg && classes && counts && ws && n > 0, "pp_select_count: bad arguments");
  E2E_REQUIRE(K >= 1 && K <= SEL_MAX_CLASSES, "pp_select_count: %d classes, one call serves 1 .. %d", K, SEL_MAX_CLASSES);
  const long long nb = sel_blocks(n);
  if (nb > SEL_MAX_BLOCKS) {
    e2e::set_error("pp_select_count: %lld voxels are more than the %lld one launch covers", n, SEL_MAX_BLOCKS * SEL_CHUNK);
    return E2E_ERR_UNSUPPORTED;
  }
  SelClasses cls = {};
  for (int k = 0; k < K; ++k) cls.c[k] = classes[k];
  unsigned* cnt = (unsigned*)ws;
  unsigned long long* offs = (unsigned long long*)((char*)ws + sel_counts_bytes(nb, K));
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(pp_select_count_kernel, dim3((unsigned)nb), dim3(SEL_THREADS), 0, st, seg, n, cls, K, nb, cnt);
  if (int e = e2e::check_launch("pp_select_count_kernel")) return e;
  hipLaunchKernelGGL(pp_select_scan_kernel, dim3((unsigned)K), dim3(SCAN_STEP), 0, st, (const unsigned*)cnt, offs, nb, counts);
  return e2e::check_launch("pp_select_scan_kernel");
}

extern "C" int e2e_pp_select_coords(const float* seg, int D, int H, int W, const float* classes, int K, const long long* ranks,
                                    const long long* slots, const long long* class_offsets, long long* out, const void* ws, void* stream) {
  E2E_REQUIRE(seg && classes && ranks && slots && class_offsets && out && ws, "pp_select_coords: null pointer");
  E2E_REQUIRE(D > 0 && H > 0 && W > 0, "pp_select_coords: every axis needs at least one voxel (got %d x %d x %d)", D, H, W);
  E2E_REQUIRE(K >= 1 && K <= SEL_MAX_CLASSES, "pp_select_coords: %d classes, one call serves 1 .. %d", K, SEL_MAX_CLASSES);
  const long long n = (long long)D * H * W, nb = sel_blocks(n);
  if (nb > SEL_MAX_BLOCKS) {
    e2e::set_error("pp_select_coords: %lld voxels are more than the %lld one launch covers", n, SEL_MAX_BLOCKS * SEL_CHUNK);
    return E2E_ERR_UNSUPPORTED;
  }
  SelClasses cls = {};
  SelOffsets off = {};
  E2E_REQUIRE(class_offsets[0] >= 0, "pp_select_coords: class_offsets[0] is negative");
  for (int k = 0; k < K; ++k) {
    E2E_REQUIRE(class_offsets[k + 1] >= class_offsets[k], "pp_select_coords: class_offsets must not decrease (class %d)", k);
    cls.c[k] = classes[k];
  }
  for (int k = 0; k <= SEL_MAX_CLASSES; ++k) off.o[k] = class_offsets[k < K ? k : K];
  if (class_offsets[K] == class_offsets[0]) return E2E_OK;     // nothing was drawn
  const unsigned* cnt = (const unsigned*)ws;
  const unsigned long long* offs = (const unsigned long long*)((const char*)ws + sel_counts_bytes(nb, K));
  hipLaunchKernelGGL(pp_select_coords_kernel, dim3((unsigned)nb), dim3(SEL_THREADS), 0, (hipStream_t)stream, seg, n, (long long)H * W,
                     (long long)W, cls, off, K, nb, cnt, offs, ranks, slots, out);
  return e2e::check_launch("pp_select_coords_kernel");
}
