// P1: "remove all but the largest connected component" on the uint8 label volume (gfx950).
// Reference: remove_all_but_the_largest_connected_component, e2enet/postprocessing/connected_components.py:50-107 (one
// scipy.ndimage.label over the whole volume per class entry plus one (lmap == id).sum() per object).
//
// The mask of a class entry is never materialised: it is set[x >> 5] >> (x & 31) & 1 of a 256-bit class set, formed on load, so a
// joint region such as (1, 2, 3) costs what one class costs.  Connectivity is the 6-neighbour cross (scipy's default structure):
// voxels that touch only diagonally are separate, and the last voxel of a row is no neighbour of the first voxel of the next row.
//
// Method: union-find on a 32-bit parent array, four passes over the volume, no workgroup waits on another.
//   init     parent[i] = flat index of the first voxel of i's run along W (a segmented scan inside the row), NONE off the mask
//   merge    every mask voxel unites with its mask neighbours at i - W and i - H W: find both roots, atomicMin(&parent[larger
//            root], smaller root), and go on from the returned value when another thread linked that root first
//   flatten  parent[i] = root(i); size[root] += 1 (one atomicAdd per run of equal roots in a wave); the value an add returns plus
//            what it added is a partial size and the last add on a root returns its full size, so the atomicMax of those values is
//            the largest size; roots are counted
//   remove   a mask voxel of a component with size != max, and (size * volume_per_voxel < min_valid when a minimum is given), is
//            written as 0; every component whose size equals the maximum is kept (the reference's object_sizes[id] != maximum_size)
//
// Invariants.
//   * parent[i] <= i at all times, equality exactly at roots: a link is only ever written by atomicMin with a smaller index, so every
//     find walks strictly decreasing indices and ends.  A value read late (before another thread's link) is still an ancestor of
//     the same component, so a find may return a former root; the atomicMin on it then returns the link and the union goes on.
//   * A union retries only after another thread's successful atomicMin on the root it tried to link; each retry lowers the larger
//     of the two indices.
//   * Every find and union loop also carries a step budget of V + 64, and a find refuses a link that does not point downwards.
//     When either trips, the thread sets the give-up word, stops looping, and the kernel runs to its end; result[3] reports it.
//     This is a backstop for a broken invariant, never a path a valid input takes.
//   * All atomics are integer min / max / add: every output, the volume and the result words, is the same bits on every run.
#include "e2e_common.h"
#include <cmath>

namespace {

constexpr unsigned NONE = 0xFFFFFFFFu;
constexpr long long MAX_VOXELS = 0x7FFFFFFFll - 1;      // indices and sizes stay below NONE and inside an int
constexpr int WS_WORDS = 16;                            // result words behind the two arrays (64 bytes)
enum { W_ROOTS = 0, W_MAX = 1, W_REMOVED = 2, W_GIVEUP = 3 };

struct ClassSet { unsigned w[8]; };

__device__ __forceinline__ bool in_set(const ClassSet& s, unsigned v) { return (s.w[v >> 5] >> (v & 31)) & 1u; }

__device__ __forceinline__ unsigned load_parent(const unsigned* parent, unsigned i) {
  return __hip_atomic_load(parent + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// root of i, or NONE after setting the give-up word
__device__ __forceinline__ unsigned find_root(const unsigned* parent, unsigned i, unsigned& budget, unsigned* words) {
  for (;;) {
    const unsigned p = load_parent(parent, i);
    if (p == i) return i;
    if (p > i || budget == 0u) {
      atomicOr(&words[W_GIVEUP], 1u);
      return NONE;
    }
    --budget;
    i = p;
  }
}

__device__ __forceinline__ void unite(unsigned* parent, unsigned i, unsigned j, unsigned& budget, unsigned* words) {
  unsigned a = find_root(parent, i, budget, words), b = find_root(parent, j, budget, words);
  while (a != NONE && b != NONE && a != b) {
    if (a < b) {
      const unsigned t = a;
      a = b;
      b = t;
    }
    const unsigned old = atomicMin(&parent[a], b);
    if (old == a) return;                     // a was a root and now hangs under b
    if (budget == 0u) {                       // (another thread linked a first: old < a)
      atomicOr(&words[W_GIVEUP], 1u);
      return;
    }
    --budget;
    a = find_root(parent, old, budget, words);
    b = find_root(parent, b, budget, words);
  }
}

// parent[i] = first voxel of i's run of mask voxels along W; size[i] = 0; workgroup 0 clears the result words
__global__ __launch_bounds__(256) void cc_init_kernel(const unsigned char* __restrict__ x, ClassSet set, unsigned* __restrict__ parent,
                                                      unsigned* __restrict__ size, unsigned* __restrict__ words, unsigned V, unsigned W) {
  if (blockIdx.x == 0 && threadIdx.x < WS_WORDS) words[threadIdx.x] = 0u;
  const unsigned lane = threadIdx.x & 63u;
  const unsigned long long i64 = (unsigned long long)blockIdx.x * 256ull + threadIdx.x;
  const bool live = i64 < V;
  const unsigned i = (unsigned)i64;
  const unsigned base = i - lane;                              // the wave's first voxel (< V whenever any lane is live)
  const bool m = live && in_set(set, x[i]);
  const unsigned long long bits = __ballot(m);
  // where the run that reaches lane 0 begins: the wave steps left through lane 0's row, 64 voxels at a time
  unsigned start0 = base;
  if (bits & 1ull) {
    const unsigned row0 = base - base % W;
    while (start0 > row0) {
      const bool valid = start0 - row0 >= 64u - lane;          // start0 - 64 + lane >= row0
      const bool mm = valid && in_set(set, x[start0 - 64u + lane]);
      const unsigned long long inv = ~__ballot(mm);
      if (inv == 0ull) {
        start0 -= 64u;
        continue;
      }
      start0 -= (unsigned)__clzll(inv);                        // mask voxels directly left of start0
      break;
    }
  }
  if (live) {
    unsigned p = NONE;
    if (m) {
      const unsigned w = i % W;
      const unsigned l0 = w >= lane ? 0u : lane - w;           // lane at which this voxel's row begins inside the wave
      const unsigned long long below = (1ull << lane) - 1ull, row = ~((1ull << l0) - 1ull);
      const unsigned long long gaps = ~bits & below & row;     // non-mask voxels of the row left of this one, inside the wave
      if (gaps) p = base + 64u - (unsigned)__clzll(gaps);      // one past the nearest gap
      else p = l0 ? base + l0 : start0;
    }
    parent[i] = p;
    size[i] = 0u;
  }
}

// Unite with the neighbours one row and one plane back.  The union with (i - s) is implied, and skipped, when i - 1 and i - s - 1
// are both in the mask: i ~ i - 1 and i - s ~ i - s - 1 by their runs, and i - 1 ~ i - s - 1 by the same rule one voxel to the left.
__global__ __launch_bounds__(256) void cc_merge_kernel(unsigned* parent, unsigned* words, unsigned V, unsigned W, unsigned HW) {
  const unsigned long long i64 = (unsigned long long)blockIdx.x * 256ull + threadIdx.x;
  if (i64 >= V) return;
  const unsigned i = (unsigned)i64;
  if (parent[i] == NONE) return;                               // (NONE never changes after init)
  unsigned budget = V + 64u;
  const unsigned w = i % W;
  const bool left = w > 0u && parent[i - 1u] != NONE;
  if (i % HW >= W && parent[i - W] != NONE && !(left && parent[i - W - 1u] != NONE)) unite(parent, i, i - W, budget, words);
  if (i >= HW && parent[i - HW] != NONE && !(left && parent[i - HW - 1u] != NONE)) unite(parent, i, i - HW, budget, words);
}

__global__ __launch_bounds__(256) void cc_flatten_count_kernel(unsigned* parent, unsigned* size, unsigned* words, unsigned V) {
  __shared__ unsigned wave_max[4];
  const unsigned lane = threadIdx.x & 63u;
  const unsigned long long i64 = (unsigned long long)blockIdx.x * 256ull + threadIdx.x;
  const unsigned i = (unsigned)i64;
  unsigned root = NONE;
  if (i64 < V && parent[i] != NONE) {
    unsigned budget = V + 64u;
    root = find_root(parent, i, budget, words);
    if (root != NONE) parent[i] = root;                        // (roots keep parent[r] == r; a racing reader sees an ancestor)
  }
  const bool m = root != NONE;
  // runs of equal roots in the wave add once: a lane leads when it has a root and the lane before has another (or none)
  const unsigned prev = __shfl_up(root, 1, 64);
  const bool brk = lane == 0u || !m || prev != root;
  const unsigned long long brks = __ballot(brk);
  unsigned seen = 0u;
  if (m && brk) {
    const unsigned long long rest = lane == 63u ? 0ull : brks >> (lane + 1u);
    const unsigned len = rest ? (unsigned)__builtin_ctzll(rest) + 1u : 64u - lane;
    seen = atomicAdd(&size[root], len) + len;
  }
  const unsigned long long roots = __ballot(m && root == i);
  if (lane == 0u && roots) atomicAdd(&words[W_ROOTS], (unsigned)__popcll(roots));
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const unsigned o = __shfl_xor(seen, off, 64);
    seen = o > seen ? o : seen;
  }
  if (lane == 0u) wave_max[threadIdx.x >> 6] = seen;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned mx = wave_max[0];
    for (int k = 1; k < 4; ++k) mx = wave_max[k] > mx ? wave_max[k] : mx;
    // (the load only filters: W_MAX never decreases, so skipping a value it already covers changes nothing)
    if (mx > __hip_atomic_load(&words[W_MAX], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(&words[W_MAX], mx);
  }
}

__global__ __launch_bounds__(256) void cc_remove_kernel(unsigned char* x, const unsigned* __restrict__ parent, const unsigned* __restrict__ size,
                                                        unsigned* words, unsigned V, double volume_per_voxel, double min_valid) {
  const unsigned lane = threadIdx.x & 63u;
  const unsigned long long i64 = (unsigned long long)blockIdx.x * 256ull + threadIdx.x;
  const unsigned i = (unsigned)i64;
  unsigned removed = 0u;
  if (i64 < V && words[W_GIVEUP] == 0u) {                        // (a given-up labelling removes nothing)
    const unsigned p = parent[i];
    if (p != NONE) {                                           // (p is i's root after the flatten pass)
      const unsigned s = size[p];
      if (s != words[W_MAX] && (min_valid < 0. || (double)s * volume_per_voxel < min_valid)) {
        x[i] = 0;
        removed = s;
      }
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const unsigned o = __shfl_xor(removed, off, 64);
    removed = o > removed ? o : removed;
  }
  if (lane == 0u && removed > __hip_atomic_load(&words[W_REMOVED], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
    atomicMax(&words[W_REMOVED], removed);
}

__global__ void cc_result_kernel(const unsigned* words, unsigned long long* result) {
  if (threadIdx.x < 4) result[threadIdx.x] = words[threadIdx.x];
}

bool cc_dims_ok(const char* what, int D, int H, int W, int* rc) {
  if (D < 1 || H < 1 || W < 1) {
    e2e::set_error("%s: every axis needs at least one voxel (got %d x %d x %d)", what, D, H, W);
    *rc = E2E_ERR_ARG;
    return false;
  }
  if ((long long)D * H * W > MAX_VOXELS) {
    e2e::set_error("%s: %d x %d x %d is more than the 2^31 - 2 voxels a 32-bit parent array indexes", what, D, H, W);
    *rc = E2E_ERR_UNSUPPORTED;
    return false;
  }
  return true;
}

}  // namespace

extern "C" long long e2e_cc_ws_bytes(int D, int H, int W) {
  int rc;
  if (!cc_dims_ok("cc_ws_bytes", D, H, W, &rc)) return 0;
  return 8ll * D * H * W + 4ll * WS_WORDS;
}

extern "C" int e2e_cc_remove_all_but_largest(unsigned char* volume, int D, int H, int W, const unsigned* class_words,
                                             double volume_per_voxel, double min_valid, void* ws, unsigned long long* result,
                                             void* stream) {
  int rc;
  if (!cc_dims_ok("cc_remove_all_but_largest", D, H, W, &rc)) return rc;
  E2E_REQUIRE(volume && class_words && ws && result, "cc_remove_all_but_largest: null pointer");
  ClassSet set;
  unsigned any = 0u;
  for (int k = 0; k < 8; ++k) any |= (set.w[k] = class_words[k]);
  E2E_REQUIRE(any != 0u, "cc_remove_all_but_largest: the class set is empty");
  E2E_REQUIRE((set.w[0] & 1u) == 0u, "cc_remove_all_but_largest: class 0 is in the set: cannot remove background");
  E2E_REQUIRE(std::isfinite(volume_per_voxel) && volume_per_voxel > 0.,
              "cc_remove_all_but_largest: volume_per_voxel must be positive and finite (got %g)", volume_per_voxel);
  E2E_REQUIRE(!(min_valid != min_valid), "cc_remove_all_but_largest: the minimum valid object size is NaN (negative = none)");
  hipStream_t st = (hipStream_t)stream;
  const unsigned V = (unsigned)((long long)D * H * W), HW = (unsigned)((long long)H * W);
  unsigned* parent = (unsigned*)ws;
  unsigned* size = parent + V;
  unsigned* words = size + V;
  const dim3 grid((unsigned)e2e::cdivll((long long)V, 256)), block(256);
  hipLaunchKernelGGL(cc_init_kernel, grid, block, 0, st, volume, set, parent, size, words, V, (unsigned)W);
  if (int e = e2e::check_launch("cc_init_kernel")) return e;
  hipLaunchKernelGGL(cc_merge_kernel, grid, block, 0, st, parent, words, V, (unsigned)W, HW);
  hipLaunchKernelGGL(cc_flatten_count_kernel, grid, block, 0, st, parent, size, words, V);
  hipLaunchKernelGGL(cc_remove_kernel, grid, block, 0, st, volume, parent, size, words, V, volume_per_voxel, min_valid);
  hipLaunchKernelGGL(cc_result_kernel, dim3(1), dim3(64), 0, st, words, result);
  return e2e::check_launch("cc_kernels");
}
