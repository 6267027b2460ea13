// Exact order statistics of fp32 values by a byte-wise radix select on 32-bit keys, without sorting: what dsff.hip (one rank, one
// workgroup, all passes in one kernel), surface.hip (two ranks over two masked arrays) and fingerprint.hip (up to eight ranks over
// a flat array) share.  Pass p = 0 .. 3 takes the histogram of byte (3 - p) of the keys whose higher bytes equal the prefix decided
// so far, walks the 256 bins to the bucket that holds the rank, and appends the bucket to the prefix; after four passes the prefix
// is the key of the order statistic.
// Contract and invariants.
//   * Keys order like the values.  key()/unkey() serve every float; non-negative values may use the raw bit pattern
//     (__float_as_uint), which orders the same way.  A select uses one of the two throughout.
//   * A rank is 0-based into the ascending order and below the number of keys.  Should the bins hold fewer keys than the rank
//     says, the walk ends in bucket 255.  A histogram bin is 32 bits wide: a select takes at most 2^32 - 1 keys.
//   * State<R> serves up to R ranks at once.  rep[r] is the first rank whose prefix equals rank r's: ranks that agree so far share
//     that rank's histogram, so every key costs one increment per distinct prefix (one in the first pass, whatever R is).
//   * A sweep is one kernel of sweep_blocks(n) workgroups of SWEEP_THREADS threads, a grid fixed by n alone, so that fp64 sums
//     on the same grid stay reproducible.  Each file writes its own sweep loop, because what it walks differs: sweep_begin, one
//     sweep_add per key, sweep_flush.  sweep_begin and sweep_flush hold a __syncthreads(): every thread calls them.
//   * Atomics are integer increments only: the same bits on every run.
#pragma once
#include "e2e_common.h"

namespace e2e::select {

constexpr int PASSES = 4;
constexpr int SWEEP_BLOCKS = 1024;     // most workgroups of a sweep
constexpr int SWEEP_THREADS = 256;     // one thread per histogram bin
inline int sweep_blocks(long long n) {
  const long long b = cdivll(n, SWEEP_THREADS);
  return (int)(b < SWEEP_BLOCKS ? b : SWEEP_BLOCKS);
}

// bit pattern -> unsigned key that orders like the floats: all bits of a negative flipped, the sign bit of the others
__device__ __forceinline__ unsigned key(float x) {
  const unsigned b = __float_as_uint(x);
  return (b & 0x80000000u) ? ~b : b ^ 0x80000000u;
}
__device__ __forceinline__ float unkey(unsigned k) { return __uint_as_float((k & 0x80000000u) ? k ^ 0x80000000u : ~k); }

// the byte a pass histograms is (key >> pass_shift) & 255; a key takes part where (key & pass_mask) == prefix
__device__ __forceinline__ int pass_shift(int pass) { return 24 - 8 * pass; }
__device__ __forceinline__ unsigned pass_mask(int pass) { return pass == 0 ? 0u : 0xFFFFFFFFu << (pass_shift(pass) + 8); }

// the bucket of rank k in 256 bins (LDS or global); k becomes the rank inside that bucket
template <typename Count>
__device__ __forceinline__ int pick_bucket(const unsigned* bins, Count& k) {
  Count cum = 0;
  int b = 0;
  for (; b < 256; ++b) {
    const Count c = bins[b];
    if (cum + c > k) break;
    cum += c;
  }
  if (b > 255) b = 255;
  k -= cum;
  return b;
}

// all zero: nothing is decided and one histogram, rank 0's, serves every rank
template <int R>
struct State {
  unsigned hist[PASSES][R][256];       // per pass and rank: byte histogram of the keys that match the rank's prefix
  unsigned prefix[R];                  // bits of the rank's order statistic decided so far
  unsigned long long k[R];             // rank inside the prefix's bucket
  int rep[R];                          // first rank with the same prefix: the owner of the histogram this rank reads
};
template <int R> struct Ranks { unsigned long long k[R]; };

template <int R>
__global__ void init_kernel(State<R>* s, Ranks<R> ranks) {
  if (threadIdx.x < R) s->k[threadIdx.x] = ranks.k[threadIdx.x];
}

// picks the bucket of each of the nr ranks from the pass's histogram and renews the owners; after the last pass
// out[r] = finish(key of rank r's order statistic), and 0 for the ranks nr .. R - 1
template <int R, class Finish>
__global__ void step_kernel(State<R>* s, int pass, int nr, Finish finish, double* out) {
  const int r = threadIdx.x;
  if (r < nr) {
    unsigned long long kk = s->k[r];
    const int b = pick_bucket(s->hist[pass][s->rep[r]], kk);
    s->k[r] = kk;
    const unsigned prefix = s->prefix[r] | ((unsigned)b << pass_shift(pass));
    s->prefix[r] = prefix;
    if (pass == PASSES - 1) out[r] = finish(prefix);
  } else if (r < R && pass == PASSES - 1) {
    out[r] = 0.;
  }
  __syncthreads();                                             // every rank has read its histogram's owner and written its prefix
  if (r == 0) {
    for (int a = 0; a < nr; ++a) {
      int first = a;
      for (int c = a - 1; c >= 0; --c)
        if (s->prefix[c] == s->prefix[a]) first = c;
      s->rep[a] = first;
    }
  }
}

// a workgroup's view of one sweep: per rank the prefix and whether the rank owns a histogram
template <int R>
struct Sweep {
  unsigned prefix[R];
  bool own[R];
};
// clears the workgroup's bins[R][256] in LDS and reads the state
template <int R>
__device__ __forceinline__ Sweep<R> sweep_begin(unsigned (*bins)[256], const State<R>* s, int nr) {
  Sweep<R> sw;
#pragma unroll
  for (int r = 0; r < R; ++r) {
    bins[r][threadIdx.x] = 0u;
    sw.prefix[r] = s->prefix[r];
    sw.own[r] = r < nr && s->rep[r] == r;
  }
  __syncthreads();
  return sw;
}
template <int R>
__device__ __forceinline__ void sweep_add(unsigned (*bins)[256], const Sweep<R>& sw, int pass, unsigned key) {
  const unsigned byte = (key >> pass_shift(pass)) & 255u;
#pragma unroll
  for (int r = 0; r < R; ++r)
    if (sw.own[r] && (key & pass_mask(pass)) == sw.prefix[r]) atomicAdd(&bins[r][byte], 1u);
}
// adds the workgroup's non-zero bins to the pass's histograms
template <int R>
__device__ __forceinline__ void sweep_flush(unsigned (*bins)[256], State<R>* s, int pass) {
  __syncthreads();
#pragma unroll
  for (int r = 0; r < R; ++r)
    if (bins[r][threadIdx.x]) atomicAdd(&s->hist[pass][r][threadIdx.x], bins[r][threadIdx.x]);
}

// ---- host side: start, then per pass the file's own sweep kernel followed by step
template <int R>
inline void start(State<R>* s, const Ranks<R>& ranks, hipStream_t st) {
  zero_async(s, sizeof(*s), st);
  hipLaunchKernelGGL(init_kernel<R>, dim3(1), dim3(64), 0, st, s, ranks);
}
template <int R, class Finish>
inline void step(State<R>* s, int pass, int nr, Finish finish, double* out, hipStream_t st) {
  hipLaunchKernelGGL((step_kernel<R, Finish>), dim3(1), dim3(64), 0, st, s, pass, nr, finish, out);
}

}  // namespace e2e::select
