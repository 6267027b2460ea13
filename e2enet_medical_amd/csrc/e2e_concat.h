// The plane addressing of the virtual concat (include/e2e_hip.h: e2e_in_chan_t, e2e_out_chan_t): what a depth shift does to a
// load and to a store, and who zero-fills.  Every 1x3x3 conv kernel that reads or writes through those tables takes the
// arithmetic from here (K1 conv133.hip, K1s conv133_sparse.hip, K1m conv133_mm.hip, conv133_dense.hip, the weight gradients
// conv133_wgrad.hip and conv133_wgrad_bf3.hip); storage (scalar registers, LDS tables) and any pre-scaling stay with the
// kernels.  The host reaches the store rule through e2e_diag_concat_slice
// (tests/test_host_cpu.py::test_concat_store_slices_partition_the_volume).
#pragma once
#include "e2e_common.h"

namespace e2e {

// ---- load side ------------------------------------------------------------------------------------------------------------------
// Virtual-concat channel c at depth d of a conv with depth stride sd is plane `ptr` of its source at depth d * sd - dshift, zero
// outside [0, Di); the value read goes through lrelu(a * v + b) (in_act), with a = 1, b = 0, slope = 1 for a raw source.

// one input channel resolved for batch item n
struct ConcatChan {
  const float* base;   // element [n, this channel, 0, 0, 0] of the source
  float a, b, slope;
  int dshift;
};

__device__ __forceinline__ ConcatChan concat_chan(const e2e_in_chan_t& ch, int n) {
  ConcatChan r;
  r.base = ch.ptr + (long long)n * ch.nstride;
  r.a = 1.f; r.b = 0.f; r.slope = 1.f;
  r.dshift = ch.dshift;
  if (ch.scale != nullptr) {
    r.a = ch.scale[(long long)n * ch.ab_nstride];
    r.b = ch.shift[(long long)n * ch.ab_nstride];
    r.slope = ch.slope;
  }
  return r;
}

// A kernel that stages whole blocks of channels meets channels beyond Cin.  They resolve to channel 0, which is always
// dereferenceable, with valid = false; the caller masks every element it stages from such a channel.
__device__ __forceinline__ ConcatChan concat_chan_or_first(const e2e_in_chan_t* chans, int c, int Cin, int n, bool& valid) {
  valid = c < Cin;
  return concat_chan(chans[valid ? c : 0], n);
}

// the source slice behind depth d; takes the shift, not the table entry, so that a kernel which keeps resolved channels in a
// record of its own (ChanRec, scalar registers) asks the same question
struct ConcatDepth {
  int din;
  bool valid;
};

__device__ __forceinline__ ConcatDepth concat_depth(int d, int sd, int dshift, int Di) {
  ConcatDepth r;
  r.din = d * sd - dshift;
  r.valid = (unsigned)r.din < (unsigned)Di;
  return r;
}

// wave-uniform description of one staged input plane at one (n, depth), kept in LDS by K1 and K1s
struct PlaneDesc {
  gfloat_p base;      // plane origin; always dereferenceable
  float a, b, slope;  // normalise-on-load coefficients
  int valid;
};

// ---- store side -----------------------------------------------------------------------------------------------------------------
// A data gradient un-shifts on store: the gradient of virtual-concat channel c computed at (shifted) depth d belongs to slice
// dd = d - s of the channel's source, s = dshift.  The depths whose d - s falls outside [0, D) computed nothing the source ever
// read; there are exactly as many of them as there are source slices that receive nothing, so each such workgroup is handed one
// of those slices instead:
//   s > 0:  d in [0, min(s, D))       ->  dd = max(D - s, 0) + d      (the slices [max(D - s, 0), D) receive nothing)
//   s < 0:  d in [max(D + s, 0), D)   ->  dd = d - max(D + s, 0)      (the slices [0, min(-s, D)) receive nothing)
// The first writer of a gradient buffer (accumulate == 0) zero-fills that slice, so the buffer needs no memset.  A later writer
// (accumulate != 0) adds where it computed something and must leave the other slices alone: they hold the final values of the
// earlier writers, and dd still names the slice for a kernel that has more to do with it (K1s sums it for the InstanceNorm
// backward).
// d -> dd is a bijection of [0, D) for every D >= 1 and every s.  s >= 0: the in-range depths [s, D) go to [0, D - s) in order
// (none if s >= D), the other min(s, D) depths go in order to [max(D - s, 0), D), which is [D - s, D) for s < D and [0, D) for
// s >= D: the two images are disjoint and cover [0, D).  s < 0 is the mirror image: [0, D + s) goes to [-s, D), the rest to
// [0, min(-s, D)).  So every slice is written by exactly one depth's workgroups and no launch needs to order its stores.
enum ConcatAction { CONCAT_STORE = 0, CONCAT_ADD = 1, CONCAT_ZERO_FILL = 2, CONCAT_SKIP = 3 };

struct ConcatSlice {
  int dd;       // destination slice, in [0, D) for d in [0, D)
  int action;   // ConcatAction
};

__host__ __device__ __forceinline__ ConcatSlice concat_store_slice(int d, int dshift, int D, int accumulate) {
  ConcatSlice r;
  r.dd = d - dshift;
  bool zero_fill = false;
  if (r.dd < 0) {
    const int lo = D - dshift > 0 ? D - dshift : 0;
    r.dd = lo + d;
    zero_fill = true;
  } else if (r.dd >= D) {
    const int lo = D + dshift > 0 ? D + dshift : 0;
    r.dd = d - lo;
    zero_fill = true;
  }
  r.action = zero_fill ? (accumulate ? CONCAT_SKIP : CONCAT_ZERO_FILL) : (accumulate ? CONCAT_ADD : CONCAT_STORE);
  return r;
}

}  // namespace e2e
