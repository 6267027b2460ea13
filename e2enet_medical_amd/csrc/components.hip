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
// The union-find itself (init_runs, merge_back, find_root), its invariants and its step-budget backstop are e2e_unionfind.h,
// shared with the hole filling of preprocess.hip; result[3] reports the give-up word.  All atomics are integer min / max /
// add / or: every output, the volume and the result words, is the same bits on every run.
#include "e2e_common.h"
#include "e2e_unionfind.h"
#include <cmath>

namespace {

using e2e::uf::NONE;
using e2e::uf::MAX_VOXELS;
using e2e::uf::find_root;
constexpr int WS_WORDS = 16;                            // result words behind the two arrays (64 bytes)
enum { W_ROOTS = 0, W_MAX = 1, W_REMOVED = 2, W_GIVEUP = 3 };

struct ClassSet { unsigned w[8]; };

__device__ __forceinline__ bool in_set(const ClassSet& s, unsigned v) { return (s.w[v >> 5] >> (v & 31)) & 1u; }

// parent[i] = first voxel of i's run of mask voxels along W; size[i] = 0; workgroup 0 clears the result words
__global__ __launch_bounds__(256) void cc_init_kernel(const unsigned char* __restrict__ x, ClassSet set, unsigned* __restrict__ parent,
                                                      unsigned* __restrict__ size, unsigned* __restrict__ words, unsigned V, unsigned W) {
  if (blockIdx.x == 0 && threadIdx.x < WS_WORDS) words[threadIdx.x] = 0u;
  e2e::uf::init_runs([&](unsigned j) { return in_set(set, x[j]); }, parent, V, W);
  const unsigned long long i64 = (unsigned long long)blockIdx.x * 256ull + threadIdx.x;
  if (i64 < V) size[i64] = 0u;
}

__global__ __launch_bounds__(256) void cc_merge_kernel(unsigned* parent, unsigned* words, unsigned V, unsigned W, unsigned HW) {
  e2e::uf::merge_back(parent, &words[W_GIVEUP], V, W, HW);
}

__global__ __launch_bounds__(256) void cc_flatten_count_kernel(unsigned* parent, unsigned* size, unsigned* words, unsigned V) {
  __shared__ unsigned wave_max[4];
  const unsigned lane = threadIdx.x & 63u;
  const unsigned long long i64 = (unsigned long long)blockIdx.x * 256ull + threadIdx.x;
  const unsigned i = (unsigned)i64;
  unsigned root = NONE;
  if (i64 < V && parent[i] != NONE) {
    unsigned budget = V + 64u;
    root = find_root(parent, i, budget, &words[W_GIVEUP]);
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
