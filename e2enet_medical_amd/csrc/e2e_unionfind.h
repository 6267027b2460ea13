// Lock-free union-find over the voxels of a [D, H, W] volume: the 6-neighbour labelling that components.hip (connected components
// of a class set) and preprocess.hip (background components, for binary_fill_holes) share, and its 26-neighbour form for
// cascade.hip.  The mask is a predicate on the flat voxel index, formed on load, so no user materialises one for it.
//
//   init_runs   parent[i] = flat index of the first voxel of i's run of mask voxels along W (a segmented scan inside the row),
//               NONE off the mask
//   merge_back  every mask voxel unites with its mask neighbours at i - W and i - H W: find both roots, atomicMin(&parent[larger
//               root], smaller root), and go on from the returned value when another thread linked that root first
//   merge_back26  the same with the 13 neighbours that precede a voxel in raster order (full connectivity)
//   find_root   after merge_back has run to its end (a kernel boundary), the root of i is its component's smallest voxel
//   init_runs_labelled, merge_back_labelled (at the end of the file): the same two passes where voxels belong together only when
//               they carry the same non-zero value, so that every class of a set is labelled at once (components.hip, P5)
//
// Invariants.
//   * parent[i] <= i at all times, equality exactly at roots: a link is only ever written by atomicMin with a smaller index, so every
//     find walks strictly decreasing indices and ends.  A value read late (before another thread's link) is still an ancestor of
//     the same component, so a find may return a former root; the atomicMin on it then returns the link and the union goes on.
//   * A union retries only after another thread's successful atomicMin on the root it tried to link; each retry lowers the larger
//     of the two indices.
//   * Every find and union loop also carries a step budget (the callers give V + 64), and a find refuses a link that does not
//     point downwards.  When either trips, the thread sets the give-up word, stops looping, and the kernel runs to its end; the
//     caller reports the word as an error.  This is a backstop for a broken invariant, never a path a valid input takes, and it
//     is never retried.
//   * All atomics are integer min / or: the labelling is the same bits on every run.
#pragma once
#include <hip/hip_runtime.h>

namespace e2e {
namespace uf {

constexpr unsigned NONE = 0xFFFFFFFFu;
constexpr long long MAX_VOXELS = 0x7FFFFFFFll - 1;      // indices and sizes stay below NONE and inside an int

__device__ __forceinline__ unsigned load_parent(const unsigned* parent, unsigned i) {
  return __hip_atomic_load(parent + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// root of i, or NONE after setting the give-up word
__device__ __forceinline__ unsigned find_root(const unsigned* parent, unsigned i, unsigned& budget, unsigned* giveup) {
  for (;;) {
    const unsigned p = load_parent(parent, i);
    if (p == i) return i;
    if (p > i || budget == 0u) {
      atomicOr(giveup, 1u);
      return NONE;
    }
    --budget;
    i = p;
  }
}

__device__ __forceinline__ void unite(unsigned* parent, unsigned i, unsigned j, unsigned& budget, unsigned* giveup) {
  unsigned a = find_root(parent, i, budget, giveup), b = find_root(parent, j, budget, giveup);
  while (a != NONE && b != NONE && a != b) {
    if (a < b) {
      const unsigned t = a;
      a = b;
      b = t;
    }
    const unsigned old = atomicMin(&parent[a], b);
    if (old == a) return;                     // a was a root and now hangs under b
    if (budget == 0u) {                       // (another thread linked a first: old < a)
      atomicOr(giveup, 1u);
      return;
    }
    --budget;
    a = find_root(parent, old, budget, giveup);
    b = find_root(parent, b, budget, giveup);
  }
}

// parent[i] = first voxel of i's run of mask voxels along W, for the voxel i = blockIdx.x * 256 + threadIdx.x of a 256-thread
// block.  Every thread of the block calls it (it votes across the wave); in_mask(j) is asked only for j < V.
template <class Pred>
__device__ __forceinline__ void init_runs(Pred in_mask, unsigned* __restrict__ parent, unsigned V, unsigned W) {
  const unsigned lane = threadIdx.x & 63u;
  const unsigned long long i64 = (unsigned long long)blockIdx.x * 256ull + threadIdx.x;
  const bool live = i64 < V;
  const unsigned i = (unsigned)i64;
  const unsigned base = i - lane;                              // the wave's first voxel (< V whenever any lane is live)
  const bool m = live && in_mask(i);
  const unsigned long long bits = __ballot(m);
  // where the run that reaches lane 0 begins: the wave steps left through lane 0's row, 64 voxels at a time
  unsigned start0 = base;
  if (bits & 1ull) {
    const unsigned row0 = base - base % W;
    while (start0 > row0) {
      const bool valid = start0 - row0 >= 64u - lane;          // start0 - 64 + lane >= row0
      const bool mm = valid && in_mask(start0 - 64u + lane);
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
  }
}

// Unite voxel i = blockIdx.x * 256 + threadIdx.x with the neighbours one row and one plane back.  The union with (i - s) is
// implied, and skipped, when i - 1 and i - s - 1 are both in the mask: i ~ i - 1 and i - s ~ i - s - 1 by their runs, and
// i - 1 ~ i - s - 1 by the same rule one voxel to the left.
__device__ __forceinline__ void merge_back(unsigned* parent, unsigned* giveup, unsigned V, unsigned W, unsigned HW) {
  const unsigned long long i64 = (unsigned long long)blockIdx.x * 256ull + threadIdx.x;
  if (i64 >= V) return;
  const unsigned i = (unsigned)i64;
  if (parent[i] == NONE) return;                               // (NONE never changes after init)
  unsigned budget = V + 64u;
  const unsigned w = i % W;
  const bool left = w > 0u && parent[i - 1u] != NONE;
  if (i % HW >= W && parent[i - W] != NONE && !(left && parent[i - W - 1u] != NONE)) unite(parent, i, i - W, budget, giveup);
  if (i >= HW && parent[i - HW] != NONE && !(left && parent[i - HW - 1u] != NONE)) unite(parent, i, i - HW, budget, giveup);
}

// The 26-neighbour form of merge_back (skimage's label(), scipy's label(structure=np.ones((3, 3, 3))): cascade.hip): voxel
// i = blockIdx.x * 256 + threadIdx.x unites with the mask voxels among the 13 neighbours that precede it in raster order.  The left
// neighbour is implied by the run.  The other 12 lie in four rows (same plane one row back; the plane before, rows y - 1, y, y + 1),
// at x - 1, x, x + 1 of each.  Per row:
//   * x in the mask: x - 1 and x + 1, where in the mask, belong to x's run, so one union with x serves all three.  It is implied, and
//     skipped, when i - 1 is in the mask: i ~ i - 1 by the run, and voxel i - 1 is a neighbour of both x - 1 and x of that row, so its
//     own thread unites it with that run (directly, or by this rule one voxel further left; the run's first voxel has no left
//     neighbour and always unites).
//   * x not in the mask: x - 1 and x + 1 are separate runs.  The union with x - 1 is skipped when i - 1 is in the mask (x - 1 is the
//     voxel straight across from i - 1: the case above for that thread); the union with x + 1 is always made.
// find_root, unite, the invariants, the step budget and the give-up word are the ones above.
__device__ __forceinline__ void merge_back26(unsigned* parent, unsigned* giveup, unsigned V, unsigned W, unsigned H) {
  const unsigned long long i64 = (unsigned long long)blockIdx.x * 256ull + threadIdx.x;
  if (i64 >= V) return;
  const unsigned i = (unsigned)i64;
  if (parent[i] == NONE) return;                               // (NONE never changes after init)
  unsigned budget = V + 64u;
  const unsigned HW = H * W;
  const unsigned x = i % W, y = i / W % H, z = i / HW;
  const bool left = x > 0u && parent[i - 1u] != NONE;
  for (int dz = -1; dz <= 0; ++dz) {
    if (dz < 0 && z == 0u) continue;
    for (int dy = -1; dy <= (dz < 0 ? 1 : -1); ++dy) {
      if ((dy < 0 && y == 0u) || (dy > 0 && y + 1u == H)) continue;
      const unsigned r = (unsigned)((long long)i + (long long)dz * HW + (long long)dy * W);      // (x, the row's voxel across)
      if (parent[r] != NONE) {
        if (!left) unite(parent, i, r, budget, giveup);
        continue;
      }
      if (!left && x > 0u && parent[r - 1u] != NONE) unite(parent, i, r - 1u, budget, giveup);
      if (x + 1u < W && parent[r + 1u] != NONE) unite(parent, i, r + 1u, budget, giveup);
    }
  }
}

// ---- labelled variants: every value of a class set is labelled in the same pass (the component table of components.hip) -----
// value(j) is the voxel's label when it is in the class set and 0 when it is not (0 is never in a set); two voxels belong together
// only when both carry the same non-zero value.  find_root and unite are the ones above: the invariants hold unchanged, because a
// link is still only ever written by atomicMin with a smaller index of the same component.

// parent[i] = first voxel of i's run of EQUAL non-zero values along W, NONE where value is 0.  Every thread of the 256-thread block
// calls it (it votes across the wave); value(j) is asked only for j < V.
template <class Val>
__device__ __forceinline__ void init_runs_labelled(Val value, unsigned* __restrict__ parent, unsigned V, unsigned W) {
  const unsigned lane = threadIdx.x & 63u;
  const unsigned long long i64 = (unsigned long long)blockIdx.x * 256ull + threadIdx.x;
  const bool live = i64 < V;
  const unsigned i = (unsigned)i64;
  const unsigned base = i - lane;                              // the wave's first voxel (< V whenever any lane is live)
  const unsigned v = live ? value(i) : 0u;
  const unsigned left = __shfl_up(v, 1, 64);
  // a run begins where the row begins or the voxel to the left carries another value; lane 0 always cuts, its run is traced below
  const unsigned long long cuts = __ballot(lane == 0u || i % W == 0u || left != v);
  const unsigned v0 = __shfl(v, 0, 64);
  // where the run that reaches lane 0 begins: the wave steps left through lane 0's row, 64 voxels at a time
  unsigned start0 = base;
  if (v0 != 0u) {
    const unsigned row0 = base - base % W;
    while (start0 > row0) {
      const bool valid = start0 - row0 >= 64u - lane;          // start0 - 64 + lane >= row0
      const bool same = valid && value(start0 - 64u + lane) == v0;
      const unsigned long long inv = ~__ballot(same);
      if (inv == 0ull) {
        start0 -= 64u;
        continue;
      }
      start0 -= (unsigned)__clzll(inv);                        // voxels of lane 0's value directly left of start0
      break;
    }
  }
  if (live) {
    unsigned p = NONE;
    if (v != 0u) {
      const unsigned long long upto = cuts & (~0ull >> (63u - lane));     // cuts at or left of this lane; bit 0 is always set
      const unsigned c = 63u - (unsigned)__clzll(upto);
      p = c ? base + c : start0;
    }
    parent[i] = p;
  }
}

// Unite voxel i = blockIdx.x * 256 + threadIdx.x with the neighbours one row and one plane back that carry i's value.  With
// x[i] == x[i - s], the union with (i - s) is implied, and skipped, when x[i - 1] == x[i] and x[i - s - 1] == x[i - s] (all four in
// the set): i ~ i - 1 and i - s ~ i - s - 1 by their runs of equal values, and i - 1 ~ i - s - 1 by the same rule one voxel to
// the left, where the four values are again equal.
template <class Val>
__device__ __forceinline__ void merge_back_labelled(Val value, unsigned* parent, unsigned* giveup, unsigned V, unsigned W, unsigned HW) {
  const unsigned long long i64 = (unsigned long long)blockIdx.x * 256ull + threadIdx.x;
  if (i64 >= V) return;
  const unsigned i = (unsigned)i64;
  const unsigned v = value(i);
  if (v == 0u) return;
  unsigned budget = V + 64u;
  const bool left = i % W > 0u && value(i - 1u) == v;
  if (i % HW >= W && value(i - W) == v && !(left && value(i - W - 1u) == v)) unite(parent, i, i - W, budget, giveup);
  if (i >= HW && value(i - HW) == v && !(left && value(i - HW - 1u) == v)) unite(parent, i, i - HW, budget, giveup);
}

}  // namespace uf
}  // namespace e2e
