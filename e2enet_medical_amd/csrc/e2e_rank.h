// Raster rank of the voxels of a flat fp32 volume that match a predicate, without listing them: what class_select.hip (seg == c,
// per class) and fingerprint.hip (seg > 0) share.  A workgroup of THREADS threads owns CHUNK consecutive voxels; wave w of pass
// `it` holds the 64 consecutive voxels behind chunk base + it * THREADS + w * 64, one per lane.
//
//   count pass    wave_matches: one 64-bit ballot and a popcount per 64 voxels; the caller adds its waves and writes counts[row][chunk]
//   scan_kernel   workgroup `row` turns counts[row][0 .. nb) into exclusive 64-bit offsets[row][..] and totals[row]
//   rank pass     a chunk that holds a wanted rank loads its voxels again; a matching voxel's rank is
//                 offsets[row][chunk] + rank_in_chunk(matches_before(..), it, wave, ballot, lane)
// Invariants.
//   * load_chunk pads behind the end of the volume with NaN; a predicate must be false for NaN (== c and > 0 are).
//   * A chunk holds at most CHUNK matches, so everything inside a chunk is 32-bit; a rank is 64-bit once the chunk's offset is added.
//   * matches_before holds the one __syncthreads() that orders its writes of `wtot` before its reads, so every thread of the
//     workgroup calls it.  A caller that calls it again on the same table (class_select, once per class) owns the __syncthreads()
//     that orders those reads before the next writes; a caller that calls it once (fingerprint) needs none.
//   * Nothing is accumulated with atomics and every offset has one writer: the same bits on every run.
#pragma once
#include "e2e_common.h"

namespace e2e::rank {

constexpr int THREADS = 256, ITERS = 16, WAVES = THREADS / 64;
constexpr int CHUNK = THREADS * ITERS;                         // voxels per workgroup
constexpr long long MAX_CHUNKS = (1ll << 24) - 1;              // grid limit of a 256-thread launch: 2^36 - 4096 voxels
constexpr int SCAN_STEP = 256;                                 // chunks per iteration of the offset scan
static_assert(ITERS * WAVES == 64, "the (pass, wave) totals of a chunk are scanned by the 64 lanes of one wave");

// voxel base + it * THREADS + thread; NaN behind the end of the volume
__device__ __forceinline__ void load_chunk(const float* __restrict__ seg, long long n, long long base, float v[ITERS]) {
#pragma unroll
  for (int it = 0; it < ITERS; ++it) {
    const long long i = base + (long long)(it * THREADS + (int)threadIdx.x);
    v[it] = i < n ? seg[i] : __builtin_nanf("");
  }
}

// inclusive sum over the lanes of a wave
template <typename T>
__device__ __forceinline__ T wave_scan(T x, int lane) {
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const T y = __shfl_up(x, off, 64);
    if (lane >= off) x += y;
  }
  return x;
}

// how many of this wave's ITERS * 64 voxels match (the same in every lane)
template <class Pred>
__device__ __forceinline__ unsigned wave_matches(const float v[ITERS], Pred pred) {
  unsigned tot = 0u;
#pragma unroll
  for (int it = 0; it < ITERS; ++it) tot += (unsigned)__popcll(__ballot(pred(v[it])));
  return tot;
}

// lane it * WAVES + w: the chunk's matching voxels in front of (pass it, wave w), through the 64 words of LDS at wtot
template <class Pred>
__device__ __forceinline__ unsigned matches_before(const float v[ITERS], Pred pred, unsigned* wtot, int lane, int wave) {
  unsigned mine = 0u;
#pragma unroll
  for (int it = 0; it < ITERS; ++it) {
    const unsigned tot = (unsigned)__popcll(__ballot(pred(v[it])));
    if (lane == it) mine = tot;
  }
  if (lane < ITERS) wtot[lane * WAVES + wave] = mine;          // raster order: wtot[it * WAVES + wave]
  __syncthreads();
  const unsigned x = wtot[lane];
  return wave_scan(x, lane) - x;
}

// the chunk's matches in front of this lane's voxel of pass `it`, from matches_before's result and the pass's ballot; all lanes call it
__device__ __forceinline__ unsigned rank_in_chunk(unsigned ex, int it, int wave, unsigned long long bits, int lane) {
  return __shfl(ex, it * WAVES + wave, 64) + (unsigned)__popcll(bits & ((1ull << lane) - 1ull));
}

// workgroup `row`: offsets[row * nb + chunk] = matches of the row in front of the chunk, totals[row] = all of them
__global__ inline __launch_bounds__(SCAN_STEP) void scan_kernel(const unsigned* __restrict__ counts, unsigned long long* __restrict__ offsets,
                                                                long long nb, long long* __restrict__ totals) {
  const unsigned* c = counts + (long long)blockIdx.x * nb;
  unsigned long long* o = offsets + (long long)blockIdx.x * nb;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __shared__ unsigned long long wsum[SCAN_STEP / 64];
  unsigned long long carry = 0ull;
  for (long long b0 = 0; b0 < nb; b0 += SCAN_STEP) {
    const long long b = b0 + threadIdx.x;
    const unsigned long long x = b < nb ? (unsigned long long)c[b] : 0ull;
    const unsigned long long inc = wave_scan(x, lane);
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

// ---- host side: the workspace of `rows` count rows over nb chunks is counts[rows][nb] (rounded up to 16 bytes), then offsets[rows][nb]
inline long long chunks(long long n) { return cdivll(n, CHUNK); }
inline long long counts_bytes(long long nb, int rows) { return ((long long)rows * nb * 4 + 15) / 16 * 16; }
inline long long ws_bytes(long long nb, int rows) { return counts_bytes(nb, rows) + (long long)rows * nb * 8; }
inline unsigned long long* ws_offsets(const void* ws, long long nb, int rows) { return (unsigned long long*)((char*)ws + counts_bytes(nb, rows)); }

// E2E_OK, or the refusal of a volume of more chunks than one launch has workgroups, under the caller's name
inline int check_voxels(const char* who, long long n) {
  if (chunks(n) <= MAX_CHUNKS) return E2E_OK;
  set_error("%s: %lld voxels are more than the %lld one launch covers", who, n, MAX_CHUNKS * CHUNK);
  return E2E_ERR_UNSUPPORTED;
}

// the counts of the workspace are written: offsets and totals follow
inline int launch_scan(void* ws, long long nb, int rows, long long* totals, hipStream_t st) {
  hipLaunchKernelGGL(scan_kernel, dim3((unsigned)rows), dim3(SCAN_STEP), 0, st, (const unsigned*)ws, ws_offsets(ws, nb, rows), nb, totals);
  return check_launch("rank::scan_kernel");
}

}  // namespace e2e::rank
