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
//
// P5, further down: the component table of a prediction against its ground truth (e2e_ct_label, e2e_ct_emit), from which the
// post-processing search takes every confusion count it needs without removing anything.
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

// ---- P5: the component table of a prediction (every class of the set labelled in one union-find, sizes and true positives) ---
// Workspace: parent_fg[V] size_fg[V] parent_cl[V] size_cl[V] tp_cl[V] words_fg[16] words_cl[16], 32-bit words: 20 bytes per voxel.
// The foreground half (x in S as one mask) is the three kernels above; the class half unites equal values only.
enum { W_SLOTS = 4 };                                   // emit: records handed out so far (W_ROOTS .. W_GIVEUP as above)

struct CtWs {
  unsigned *parent_fg, *size_fg, *parent_cl, *size_cl, *tp_cl, *words_fg, *words_cl;
};

CtWs ct_ws(void* ws, unsigned V) {
  unsigned* p = (unsigned*)ws;
  return CtWs{p, p + V, p + 2ull * V, p + 3ull * V, p + 4ull * V, p + 5ull * V, p + 5ull * V + WS_WORDS};
}

__device__ __forceinline__ unsigned set_value(const ClassSet& s, unsigned v) { return in_set(s, v) ? v : 0u; }

__global__ __launch_bounds__(256) void ct_init_kernel(const unsigned char* __restrict__ x, ClassSet set, unsigned* __restrict__ parent,
                                                      unsigned* __restrict__ size, unsigned* __restrict__ tp, unsigned* __restrict__ words,
                                                      unsigned V, unsigned W) {
  if (blockIdx.x == 0 && threadIdx.x < WS_WORDS) words[threadIdx.x] = 0u;
  e2e::uf::init_runs_labelled([&](unsigned j) { return set_value(set, x[j]); }, parent, V, W);
  const unsigned long long i64 = (unsigned long long)blockIdx.x * 256ull + threadIdx.x;
  if (i64 < V) size[i64] = tp[i64] = 0u;
}

__global__ __launch_bounds__(256) void ct_merge_kernel(const unsigned char* __restrict__ x, ClassSet set, unsigned* parent, unsigned* words,
                                                       unsigned V, unsigned W, unsigned HW) {
  e2e::uf::merge_back_labelled([&](unsigned j) { return set_value(set, x[j]); }, parent, &words[W_GIVEUP], V, W, HW);
}

// parent[i] = root(i); size[root] += 1 and tp[root] += (g[i] == x[i]), one atomicAdd each per run of equal roots in a wave
__global__ __launch_bounds__(256) void ct_flatten_count_kernel(const unsigned char* __restrict__ x, const unsigned char* __restrict__ g,
                                                               unsigned* parent, unsigned* size, unsigned* tp, unsigned* words, unsigned V) {
  const unsigned lane = threadIdx.x & 63u;
  const unsigned long long i64 = (unsigned long long)blockIdx.x * 256ull + threadIdx.x;
  const unsigned i = (unsigned)i64;
  unsigned root = NONE;
  bool hit = false;
  if (i64 < V && parent[i] != NONE) {
    unsigned budget = V + 64u;
    root = find_root(parent, i, budget, &words[W_GIVEUP]);
    if (root != NONE) {
      parent[i] = root;
      hit = g[i] == x[i];
    }
  }
  const bool m = root != NONE;
  const unsigned prev = __shfl_up(root, 1, 64);
  const bool brk = lane == 0u || !m || prev != root;
  const unsigned long long brks = __ballot(brk), hits = __ballot(hit);
  if (m && brk) {
    const unsigned long long rest = lane == 63u ? 0ull : brks >> (lane + 1u);
    const unsigned len = rest ? (unsigned)__builtin_ctzll(rest) + 1u : 64u - lane;
    const unsigned mine = (unsigned)__popcll((hits >> lane) & (~0ull >> (64u - len)));      // (1 <= len <= 64 - lane)
    atomicAdd(&size[root], len);
    if (mine) atomicAdd(&tp[root], mine);
  }
  const unsigned long long roots = __ballot(m && root == i);
  if (lane == 0u && roots) atomicAdd(&words[W_ROOTS], (unsigned)__popcll(roots));
}

__global__ void ct_result_kernel(const unsigned* words_fg, const unsigned* words_cl, unsigned long long* result) {
  if (threadIdx.x == 0) {
    result[0] = words_cl[W_ROOTS];
    result[1] = words_fg[W_ROOTS];
    result[2] = words_fg[W_GIVEUP] | words_cl[W_GIVEUP];
    result[3] = 0ull;
  }
}

__global__ void ct_emit_reset_kernel(unsigned* words_fg, unsigned* words_cl) {
  if (threadIdx.x == 0) words_fg[W_SLOTS] = words_cl[W_SLOTS] = 0u;
}

// the slot of this lane's record when `is_root`: one atomicAdd per wave hands out a block of slots, the lanes take them in order
__device__ __forceinline__ unsigned ct_slot(bool is_root, unsigned* counter, unsigned lane) {
  const unsigned long long bits = __ballot(is_root);
  unsigned first = 0u;
  if (lane == 0u && bits) first = atomicAdd(counter, (unsigned)__popcll(bits));
  return __shfl(first, 0, 64) + (unsigned)__popcll(bits & ((1ull << lane) - 1ull));
}

// one record per root: class (first, label, size, tp, first voxel of its foreground component), foreground (first, size).  A slot at
// or past the capacity is not written (the entry point refuses such a call; this is the bound the kernel itself keeps).
__global__ __launch_bounds__(256) void ct_emit_kernel(const unsigned char* __restrict__ x, CtWs ws, unsigned* __restrict__ class_rec,
                                                      unsigned class_cap, unsigned* __restrict__ fg_rec, unsigned fg_cap, unsigned V) {
  const unsigned lane = threadIdx.x & 63u;
  const unsigned long long i64 = (unsigned long long)blockIdx.x * 256ull + threadIdx.x;
  const unsigned i = (unsigned)i64;
  const bool live = i64 < V;
  const bool cl = live && ws.parent_cl[i] == i, fg = live && ws.parent_fg[i] == i;
  const unsigned cs = ct_slot(cl, &ws.words_cl[W_SLOTS], lane), fs = ct_slot(fg, &ws.words_fg[W_SLOTS], lane);
  if (cl && cs < class_cap) {
    unsigned* r = class_rec + 5ull * cs;
    r[0] = i;
    r[1] = x[i];
    r[2] = ws.size_cl[i];
    r[3] = ws.tp_cl[i];
    r[4] = ws.parent_fg[i];
  }
  if (fg && fs < fg_cap) {
    fg_rec[2ull * fs] = i;
    fg_rec[2ull * fs + 1ull] = ws.size_fg[i];
  }
}

bool ct_class_set(const char* what, const unsigned* class_words, ClassSet* set, int* rc) {
  unsigned any = 0u;
  for (int k = 0; k < 8; ++k) any |= (set->w[k] = class_words[k]);
  *rc = E2E_ERR_ARG;
  if (any == 0u) {
    e2e::set_error("%s: the class set is empty", what);
    return false;
  }
  if (set->w[0] & 1u) {
    e2e::set_error("%s: class 0 is in the set: background has no components", what);
    return false;
  }
  return true;
}

}  // namespace

extern "C" long long e2e_ct_ws_bytes(int D, int H, int W) {
  int rc;
  if (!cc_dims_ok("ct_ws_bytes", D, H, W, &rc)) return 0;
  return 20ll * D * H * W + 8ll * WS_WORDS;
}

extern "C" int e2e_ct_label(const unsigned char* pred, const unsigned char* gt, int D, int H, int W, const unsigned* class_words, void* ws,
                            unsigned long long* result, void* stream) {
  int rc;
  if (!cc_dims_ok("ct_label", D, H, W, &rc)) return rc;
  E2E_REQUIRE(pred && gt && class_words && ws && result, "ct_label: null pointer");
  ClassSet set;
  if (!ct_class_set("ct_label", class_words, &set, &rc)) return rc;
  hipStream_t st = (hipStream_t)stream;
  const unsigned V = (unsigned)((long long)D * H * W), HW = (unsigned)((long long)H * W);
  const CtWs a = ct_ws(ws, V);
  const dim3 grid((unsigned)e2e::cdivll((long long)V, 256)), block(256);
  hipLaunchKernelGGL(cc_init_kernel, grid, block, 0, st, pred, set, a.parent_fg, a.size_fg, a.words_fg, V, (unsigned)W);
  if (int e = e2e::check_launch("cc_init_kernel")) return e;
  hipLaunchKernelGGL(ct_init_kernel, grid, block, 0, st, pred, set, a.parent_cl, a.size_cl, a.tp_cl, a.words_cl, V, (unsigned)W);
  hipLaunchKernelGGL(cc_merge_kernel, grid, block, 0, st, a.parent_fg, a.words_fg, V, (unsigned)W, HW);
  hipLaunchKernelGGL(ct_merge_kernel, grid, block, 0, st, pred, set, a.parent_cl, a.words_cl, V, (unsigned)W, HW);
  hipLaunchKernelGGL(cc_flatten_count_kernel, grid, block, 0, st, a.parent_fg, a.size_fg, a.words_fg, V);
  hipLaunchKernelGGL(ct_flatten_count_kernel, grid, block, 0, st, pred, gt, a.parent_cl, a.size_cl, a.tp_cl, a.words_cl, V);
  hipLaunchKernelGGL(ct_result_kernel, dim3(1), dim3(64), 0, st, a.words_fg, a.words_cl, result);
  return e2e::check_launch("ct_label kernels");
}

extern "C" int e2e_ct_emit(const unsigned char* pred, int D, int H, int W, void* ws, unsigned* class_records, long long class_capacity,
                           long long class_count, unsigned* fg_records, long long fg_capacity, long long fg_count, void* stream) {
  int rc;
  if (!cc_dims_ok("ct_emit", D, H, W, &rc)) return rc;
  const long long V = (long long)D * H * W;
  E2E_REQUIRE(pred && ws, "ct_emit: null pointer");
  E2E_REQUIRE(class_count >= 0 && fg_count >= 0 && class_count <= V && fg_count <= class_count,
              "ct_emit: %lld class and %lld foreground components are no counts ct_label reports for %lld voxels", class_count, fg_count, V);
  E2E_REQUIRE(class_capacity >= class_count && fg_capacity >= fg_count,
              "ct_emit: room for %lld class and %lld foreground records, %lld and %lld are needed: nothing is truncated",
              class_capacity, fg_capacity, class_count, fg_count);
  E2E_REQUIRE((class_records || class_count == 0) && (fg_records || fg_count == 0), "ct_emit: null record buffer");
  if (class_count == 0) return E2E_OK;                  // (no class component: no foreground component either)
  hipStream_t st = (hipStream_t)stream;
  const CtWs a = ct_ws(ws, (unsigned)V);
  hipLaunchKernelGGL(ct_emit_reset_kernel, dim3(1), dim3(64), 0, st, a.words_fg, a.words_cl);
  if (int e = e2e::check_launch("ct_emit_reset_kernel")) return e;
  // (the capacities the kernel keeps are the counts: a buffer is never written past what the caller read from ct_label)
  hipLaunchKernelGGL(ct_emit_kernel, dim3((unsigned)e2e::cdivll(V, 256)), dim3(256), 0, st, pred, a, class_records, (unsigned)class_count,
                     fg_records, (unsigned)fg_count, (unsigned)V);
  return e2e::check_launch("ct_emit_kernel");
}

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
