// The tile walk and the slab layout of the weight gradients: how the host cuts the pixel tiles of a launch into chunks, which
// tiles the workgroup of a chunk walks, where a tile sits in the output volume, and which slab of the workspace the workgroup
// writes.  Host plan (plan_wgrad in conv133_wgrad.hip, the transposed-conv plan in convt.hip) and kernels (conv133_wgrad.hip,
// conv133_wgrad_bf3.hip) take all of it from here: the entry points take a bare workspace pointer, and what keeps a kernel
// inside it is that the slab count of the size query and the slab index of every store come from the same functions.  LDS
// images, staging pipelines and MFMA schedules stay with the kernels.  The host reaches the walk through e2e_diag_wgrad_walk
// (tests/test_host_cpu.py::test_wgrad_chunks_partition_the_tiles_and_the_slabs).
#pragma once
#include "e2e_common.h"
#include "e2e_split.h"
#include "e2e_concat.h"

namespace e2e {

// one plan, one struct: every kernel body of both files takes it by value
struct WgParams {
  const e2e_in_chan_t* chans;
  const float* dy;
  float* slab;                 // [slabs][Cout][Cin][9]
  int B, Cin, Cout, Di, Hi, Wi, Do, Ho, Wo, sd;
  int tiles_x, tiles_y, tiles_d, tiles_per_n;
  long long total_tiles;
  int tiles_per_chunk;
  int cblocks;                 // input-channel blocks of a workgroup's width across Cin
  int segs;                    // per-item walk: chunks per batch item
  int geom;                    // split-operand kernel: 0 4 x 32-pixel tiles, 1 8 x 16-pixel tiles (planes 16..31 wide)
  int h2;                      // split-operand kernel: 1 fp16 two-piece operands, three products; 0 bf16 three-piece, six products
  const unsigned* dy_absmax;   // h2: bit pattern of max |dy| over the tensor (device; nullptr: dy is taken unscaled)
  const unsigned* x_absmax;    // h2: bit pattern of (a bound of) max |x| over the input planes after normalise-on-load (nullptr: fixed 2^3)
};

// conv133_wgrad_bf3.hip: dense weight gradient on the bf16 / fp16 matrix pipe with fp32-exact split operands; planned and
// dispatched by e2e_conv133_wgrad (conv133_wgrad.hip)
int launch_wgrad_bf3(const WgParams& p, int nchunks, int pairs, hipStream_t st);
// conv133_wgrad.hip (wgrad_slab_reduce_kernel): dw[e] = sum of the nslabs slabs of numel floats, in a fixed order.  The last step of
// every weight gradient of both conv families; call it only after the main launch passed check_launch
int reduce_slabs(const float* slab, float* dw, long long numel, int nslabs, hipStream_t st);

// ---- host: tiles -> chunks -------------------------------------------------------------------------------------------------------
// A workgroup walks one chunk of pixel tiles: `total` tiles in chunks of equal size for about target_wgs workgroups over `pairs`
// channel-block pairs, at least min_tiles tiles per chunk (every chunk is a slab the reduction has to read).  Returns the number
// of chunks.
inline int split_tiles(long long total, int pairs, int target_wgs, int min_tiles, int* tiles_per_chunk) {
  long long want = target_wgs / (pairs > 0 ? pairs : 1);
  if (want < 1) want = 1;
  long long tpc = cdivll(total, want);
  if (tpc < min_tiles) tpc = min_tiles;
  if (tpc > total) tpc = total;
  *tiles_per_chunk = (int)tpc;
  return (int)cdivll(total, tpc);
}
// The same where chunks never cross a batch item: `*segs` runs of *tiles_per_chunk tiles per item; returns segs * B chunks.
inline int split_tiles_per_item(int tiles_per_n, int B, int pairs, int target_wgs, int min_tiles, int* tiles_per_chunk, int* segs) {
  long long want = target_wgs / (pairs > 0 ? pairs : 1);
  if (want < B) want = B;
  int tpc = cdiv(tiles_per_n, (int)(want / B));
  if (tpc < min_tiles) tpc = min_tiles;
  if (tpc > tiles_per_n) tpc = tiles_per_n;
  *tiles_per_chunk = tpc;
  *segs = cdiv(tiles_per_n, tpc);
  return *segs * B;
}

// ---- host and device: chunk -> tiles ---------------------------------------------------------------------------------------------
// split_tiles: chunk k walks the tiles [lo, hi) of the launch's total_tiles, across batch items where they meet
struct WgTiles {
  long long lo, hi;
};
__host__ __device__ __forceinline__ WgTiles chunk_tiles(const WgParams& p, int chunk) {
  WgTiles r;
  r.lo = (long long)chunk * p.tiles_per_chunk;
  r.hi = r.lo + p.tiles_per_chunk;
  if (r.hi > p.total_tiles) r.hi = p.total_tiles;
  return r;
}
// split_tiles_per_item: chunk k = (batch item n, run `seg` of it) walks the tiles [lo, hi) of that item's tiles_per_n
struct WgItemTiles {
  int n, lo, hi;
};
__host__ __device__ __forceinline__ WgItemTiles chunk_tiles_per_item(const WgParams& p, int chunk) {
  WgItemTiles r;
  r.n = chunk / p.segs;
  r.lo = (chunk - r.n * p.segs) * p.tiles_per_chunk;
  r.hi = r.lo + p.tiles_per_chunk;
  if (r.hi > p.tiles_per_n) r.hi = p.tiles_per_n;
  return r;
}

// ---- host and device: tile -> origin ---------------------------------------------------------------------------------------------
// tiles run x fastest, then y, then depth, then batch item; a tile of nd x th x tw output pixels starts at (d0, h0, w0)
struct WgOrigin {
  int n, d0, h0, w0;
};
__host__ __device__ __forceinline__ WgOrigin tile_origin_in_item(const WgParams& p, int n, int t, int nd, int th, int tw) {
  WgOrigin r;
  r.n = n;
  const int tx = t % p.tiles_x;
  t /= p.tiles_x;
  const int ty = t % p.tiles_y;
  r.d0 = (t / p.tiles_y) * nd;
  r.h0 = ty * th;
  r.w0 = tx * tw;
  return r;
}
template <int ND, int TH, int TW>
__host__ __device__ __forceinline__ WgOrigin tile_origin_in_item(const WgParams& p, int n, int t) {
  return tile_origin_in_item(p, n, t, ND, TH, TW);
}
__host__ __device__ __forceinline__ WgOrigin tile_origin(const WgParams& p, long long tile, int nd, int th, int tw) {
  const int n = (int)((unsigned)tile / (unsigned)p.tiles_per_n);      // (fewer than 2^31 tiles: 32-bit division)
  return tile_origin_in_item(p, n, (int)tile - n * p.tiles_per_n, nd, th, tw);
}
template <int ND, int TH, int TW>
__host__ __device__ __forceinline__ WgOrigin tile_origin(const WgParams& p, long long tile) {
  return tile_origin(p, tile, ND, TH, TW);
}

// ---- host and device: workgroup -> slab ------------------------------------------------------------------------------------------
// The workgroup of chunk `block` writes slabs_per_wg slabs, one per `sub`: 1 everywhere but in the kernels whose two wave groups
// split the tile rows (v3<1,1,2>, smallc) and keep a slab each.  The plan's slab count is the index after the last workgroup's
// last slab.
constexpr int WG_ROW_HALVES = 2;
__host__ __device__ __forceinline__ long long wg_slab_index(int block, int sub, int slabs_per_wg) {
  return (long long)block * slabs_per_wg + sub;
}
inline int wg_slab_count(int chunks, int slabs_per_wg) { return (int)wg_slab_index(chunks - 1, slabs_per_wg - 1, slabs_per_wg) + 1; }
__device__ __forceinline__ float* wg_slab(const WgParams& p, long long index) { return p.slab + index * p.Cout * p.Cin * 9; }

// one 16 x 16 block of a slab from the fp32 MFMA accumulators of its nine taps, D[i = o][j = c]: column = lane & 15 -> c0 + c,
// row = (lane >> 4) * 4 + register -> o0 + o
__device__ __forceinline__ void store_slab_block16(const WgParams& p, long long index, int o0, int c0, int lane, const f32x4_t (&acc)[9]) {
  float* sp = wg_slab(p, index);
  const int c = c0 + (lane & 15);
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int o = o0 + (lane >> 4) * 4 + r;
    if (o < p.Cout && c < p.Cin) {
      float* dst = sp + ((long long)o * p.Cin + c) * 9;
#pragma unroll
      for (int t = 0; t < 9; ++t) dst[t] = acc[t][r];
    }
  }
}

// ---- device: wave-uniform channel descriptors ------------------------------------------------------------------------------------
// The XCW consecutive input channels a wave stages, resolved for one batch item.  Lives in scalar registers: every loop over it is
// fully unrolled and nothing takes the address of a member.
template <int XCW>
struct WaveChans {
  gfloat_p base[XCW];
  float a[XCW], b[XCW], slope[XCW];
  int dshift[XCW];
  bool valid[XCW];
  __device__ __forceinline__ void load(const WgParams& p, int first_channel, int n) {
#pragma unroll
    for (int k = 0; k < XCW; ++k) {
      const ConcatChan chd = concat_chan_or_first(p.chans, first_channel + k, p.Cin, n, valid[k]);
      dshift[k] = chd.dshift;
      base[k] = (gfloat_p)chd.base;
      a[k] = chd.a; b[k] = chd.b; slope[k] = chd.slope;
    }
  }
};

}  // namespace e2e
