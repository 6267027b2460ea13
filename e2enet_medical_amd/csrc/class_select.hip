// P3: the class-location sampling of a preprocessed training case on the device (gfx950).
// Reference: e2enet/preprocessing/preprocessing.py:343-361 (GenericPreprocessor._run_internal): per class np.argwhere(seg == c), which
// lists the class's voxels in raster order, then RandomState(1234).choice(n, t, replace=False) rows of it.  The label volume is
// where resample_and_normalize left it, on the device; only the K class totals go down and only the drawn ranks come up.
//
// The raster rank of a class's voxels comes from e2e_rank.h (chunks, counts, offset scan, rank inside a chunk), one count row per class.
//
//   e2e_pp_select_count    a workgroup writes how many voxels of its chunk equal each class; one workgroup per class then scans the
//                          per-chunk counts into exclusive 64-bit offsets and the class total
//   e2e_pp_select_coords   the host has drawn ranks into the raster order of each class and sorted them.  A workgroup looks up which
//                          of a class's ranks fall into its own [offset, offset + count); without any it leaves before it reads a
//                          voxel.  Otherwise it recomputes the rank of its matching voxels and every voxel whose rank was drawn
//                          writes its (i, j, k) into the row of the draw
// Every output row has exactly one writer and nothing is accumulated with atomics: the same bits on every run.  The volume is read
// once per pass whatever K is; all indices, offsets and counts are 64-bit.
#include "e2e_rank.h"

namespace {

namespace rk = e2e::rank;

constexpr int SEL_MAX_CLASSES = 64;                            // one lane per class holds its count

struct SelClasses { float c[SEL_MAX_CLASSES]; };
struct SelOffsets { long long o[SEL_MAX_CLASSES + 1]; };       // class k's ranks, slots and output rows are [o[k], o[k + 1])

struct IsClass {
  float c;
  __device__ __forceinline__ bool operator()(float v) const { return v == c; }
};

// counts[k * nb + chunk]
__global__ __launch_bounds__(rk::THREADS) void pp_select_count_kernel(const float* __restrict__ seg, long long n, SelClasses cls, int K,
                                                                      long long nb, unsigned* __restrict__ counts) {
  const long long blk = blockIdx.x;
  float v[rk::ITERS];
  rk::load_chunk(seg, n, blk * rk::CHUNK, v);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned mine = 0u;                                          // lane k: this wave's voxels of class k
  for (int k = 0; k < K; ++k) {
    const unsigned tot = rk::wave_matches(v, IsClass{cls.c[k]});
    if (lane == k) mine = tot;
  }
  __shared__ unsigned sh[rk::WAVES][SEL_MAX_CLASSES];
  sh[wave][lane] = mine;
  __syncthreads();
  const int t = threadIdx.x;
  if (t < K) counts[(long long)t * nb + blk] = sh[0][t] + sh[1][t] + sh[2][t] + sh[3][t];
}

// first p in [lo, hi) with a[p] >= x, or hi
__device__ __forceinline__ long long sel_lower_bound(const long long* __restrict__ a, long long lo, long long hi, long long x) {
  while (lo < hi) {
    const long long mid = lo + ((hi - lo) >> 1);
    if (a[mid] < x) lo = mid + 1; else hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(rk::THREADS) void pp_select_coords_kernel(const float* __restrict__ seg, long long n, long long HW, long long W,
                                                                       SelClasses cls, SelOffsets off, int K, long long nb,
                                                                       const unsigned* __restrict__ counts,
                                                                       const unsigned long long* __restrict__ offsets,
                                                                       const long long* __restrict__ ranks, const long long* __restrict__ slots,
                                                                       long long* __restrict__ out) {
  const long long blk = blockIdx.x;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  __shared__ long long p_lo[SEL_MAX_CLASSES], p_hi[SEL_MAX_CLASSES], first[SEL_MAX_CLASSES];
  __shared__ unsigned wtot[rk::ITERS * rk::WAVES];
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
  float v[rk::ITERS];
  rk::load_chunk(seg, n, blk * rk::CHUNK, v);
  for (int k = 0; k < K; ++k) {
    const long long a = p_lo[k], b = p_hi[k];
    if (b <= a) continue;                                      // (the same for the whole workgroup)
    const IsClass is_class{cls.c[k]};
    const unsigned ex = rk::matches_before(v, is_class, wtot, lane, wave);
    __syncthreads();                                           // wtot is rewritten for the next class
    const long long row0 = off.o[k], rows = off.o[k + 1] - off.o[k], lo = first[k];
#pragma unroll
    for (int it = 0; it < rk::ITERS; ++it) {
      const bool m = is_class(v[it]);
      const unsigned long long bits = __ballot(m);
      const long long r = lo + (long long)rk::rank_in_chunk(ex, it, wave, bits, lane);
      if (!m) continue;
      const long long p = sel_lower_bound(ranks, a, b, r);
      if (p >= b || ranks[p] != r) continue;
      const long long slot = slots[p];
      if (slot < 0 || slot >= rows) continue;                  // (a slot outside the class's rows: a bad call writes nothing)
      const long long idx = blk * rk::CHUNK + (long long)(it * rk::THREADS + t);
      const long long i = idx / HW, rem = idx - i * HW, j = rem / W;
      long long* o = out + (row0 + slot) * 3;
      o[0] = i; o[1] = j; o[2] = rem - j * W;
    }
  }
}

}  // namespace

extern "C" int e2e_pp_select_chunk(void) { return rk::CHUNK; }
extern "C" int e2e_pp_select_max_classes(void) { return SEL_MAX_CLASSES; }

extern "C" long long e2e_pp_select_ws_bytes(long long n, int K) {
  if (n < 1 || K < 1 || K > SEL_MAX_CLASSES || rk::chunks(n) > rk::MAX_CHUNKS) return 0;
  return rk::ws_bytes(rk::chunks(n), K);
}

extern "C" int e2e_pp_select_count(const float* seg, long long n, const float* classes, int K, long long* counts, void* ws, void* stream) {
  E2E_REQUIRE(seg && classes && counts && ws && n > 0, "pp_select_count: bad arguments");
  E2E_REQUIRE(K >= 1 && K <= SEL_MAX_CLASSES, "pp_select_count: %d classes, one call serves 1 .. %d", K, SEL_MAX_CLASSES);
  if (int e = rk::check_voxels("pp_select_count", n)) return e;
  const long long nb = rk::chunks(n);
  SelClasses cls = {};
  for (int k = 0; k < K; ++k) cls.c[k] = classes[k];
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(pp_select_count_kernel, dim3((unsigned)nb), dim3(rk::THREADS), 0, st, seg, n, cls, K, nb, (unsigned*)ws);
  if (int e = e2e::check_launch("pp_select_count_kernel")) return e;
  return rk::launch_scan(ws, nb, K, counts, st);
}

extern "C" int e2e_pp_select_coords(const float* seg, int D, int H, int W, const float* classes, int K, const long long* ranks,
                                    const long long* slots, const long long* class_offsets, long long* out, const void* ws, void* stream) {
  E2E_REQUIRE(seg && classes && ranks && slots && class_offsets && out && ws, "pp_select_coords: null pointer");
  E2E_REQUIRE(D > 0 && H > 0 && W > 0, "pp_select_coords: every axis needs at least one voxel (got %d x %d x %d)", D, H, W);
  E2E_REQUIRE(K >= 1 && K <= SEL_MAX_CLASSES, "pp_select_coords: %d classes, one call serves 1 .. %d", K, SEL_MAX_CLASSES);
  const long long n = (long long)D * H * W, nb = rk::chunks(n);
  if (int e = rk::check_voxels("pp_select_coords", n)) return e;
  SelClasses cls = {};
  SelOffsets off = {};
  E2E_REQUIRE(class_offsets[0] >= 0, "pp_select_coords: class_offsets[0] is negative");
  for (int k = 0; k < K; ++k) {
    E2E_REQUIRE(class_offsets[k + 1] >= class_offsets[k], "pp_select_coords: class_offsets must not decrease (class %d)", k);
    cls.c[k] = classes[k];
  }
  for (int k = 0; k <= SEL_MAX_CLASSES; ++k) off.o[k] = class_offsets[k < K ? k : K];
  if (class_offsets[K] == class_offsets[0]) return E2E_OK;     // nothing was drawn
  hipLaunchKernelGGL(pp_select_coords_kernel, dim3((unsigned)nb), dim3(rk::THREADS), 0, (hipStream_t)stream, seg, n, (long long)H * W,
                     (long long)W, cls, off, K, nb, (const unsigned*)ws, (const unsigned long long*)rk::ws_offsets(ws, nb, K),
                     ranks, slots, out);
  return e2e::check_launch("pp_select_coords_kernel");
}
