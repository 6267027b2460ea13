// K3: transposed convolution with kernel == stride (non-overlapping up-sampling), forward / data gradient /
// weight gradient, gfx950.  Reference: nn.ConvTranspose3d(Cin, Cout, k, k, bias=False) built at
// unetpp_d.py:521-522, DSFF-masked on (Cin, Cout) pairs (core_channel.py:324: names containing 'up').
//
//   y[n,o,kd*d+i,kh*h+j,kw*w+k] = sum_c z[n,c,d,h,w] * W[c,o,i,j,k],   z = lrelu(scale*x + shift)
//
// The op is a per-voxel [Cin] x [Cin, Cout*KT] product.  Three families of kernels, chosen by the plans at the end of the file:
//   * any kernel in {1,2}^3, small planes: forward and data gradient in gather form straight from global memory (the re-reads
//     of z / dy are L2 hits, weights as wave-uniform scalars, DSFF liveness bits walked with scalar bit ops), weight gradient v1
//     on the fp32 MFMA;
//   * kw == 2, even W: the three GEMMs on the matrix pipe with split fp32-exact operands (*_bf3_kernel: fp16 two-piece or bf16
//     three-piece), the default;
//   * the same shapes on fp32 matrix instructions (convT_wgrad_v2, convT_dgrad_v3): E2E_CT_BF3=0, and the data gradient where
//     W is no multiple of 32.
// The gradient GEMMs take their dy addresses from DyTile.
#include "e2e_common.h"
#include "e2e_split.h"
#include "e2e_wgrad.h"
#include <cstdlib>
#include <type_traits>

namespace {

using namespace e2e;

// flat voxel index inside one sample -> (d, h, w).  A sample has fewer than 2^31 voxels (checked by the entry points),
// so this is 32-bit unsigned arithmetic: the 64-bit `%` and `/` the index types would imply cost ~100 vector
// instructions each and used to dominate the staging code of these kernels.
__device__ __forceinline__ void decode_dhw(long long v, int W, int H, int& dv, int& hv, int& wv) {
  const unsigned u = (unsigned)v;
  const unsigned r = u / (unsigned)W;
  wv = (int)(u - r * (unsigned)W);
  const unsigned d = r / (unsigned)H;
  hv = (int)(r - d * (unsigned)H);
  dv = (int)d;
}

__device__ __forceinline__ void tap_ijk(int t, int kh, int kw, int& i, int& j, int& k) {
  k = t % kw;
  const int r = t / kw;
  j = r % kh;
  i = r / kh;
}

// ---- forward: one thread = VPL input voxels of one output channel --------------------------------------------
template <int KT, int VPL>
__global__ __launch_bounds__(256) void convT_fwd_kernel(const float* __restrict__ x, const float* __restrict__ scale,
                                                        const float* __restrict__ shift, float slope,
                                                        const float* __restrict__ w, const unsigned* __restrict__ live,
                                                        float* __restrict__ y, int Cin, int Cout, int D, int H, int W,
                                                        int kd, int kh, int kw) {
  const int o = blockIdx.y, n = blockIdx.z;
  const long long spatial = (long long)D * H * W;
  const long long v0 = ((long long)blockIdx.x * 256 + threadIdx.x) * VPL;   // VPL consecutive voxels (same row if W % VPL == 0)
  float acc[VPL][KT];
#pragma unroll
  for (int v = 0; v < VPL; ++v)
#pragma unroll
    for (int t = 0; t < KT; ++t) acc[v][t] = 0.f;
  const int words = e2e::cdiv(Cin, 32);
  const bool vec_ok = (VPL == 1) || (spatial % VPL == 0);
  for (int wd = 0; wd < words; ++wd) {
    unsigned bits = live ? live[(long long)o * words + wd] : 0xffffffffu;
    const int remain = Cin - wd * 32;
    if (remain < 32) bits &= (1u << remain) - 1u;
    bits = __builtin_amdgcn_readfirstlane(bits);
    // two-level summation (as in conv133_kernel): the live planes of one 32-plane word form a partial sum that is flushed
    // into the outer accumulator -- one fp32 chain over up to 320 planes is noisier than the CPU path's blocked sum
    float part[VPL][KT];
#pragma unroll
    for (int v = 0; v < VPL; ++v)
#pragma unroll
      for (int t = 0; t < KT; ++t) part[v][t] = 0.f;
    while (bits) {
      const int c = wd * 32 + __builtin_ctz(bits);
      bits &= bits - 1;
      const float* wp = w + ((long long)c * Cout + o) * KT;
      float wt[KT];
#pragma unroll
      for (int t = 0; t < KT; ++t) wt[t] = wp[t];
      float a = 1.f, b = 0.f, sl = 1.f;
      if (scale) { a = scale[(long long)n * Cin + c]; b = shift[(long long)n * Cin + c]; sl = slope; }
      const float* xp = x + ((long long)n * Cin + c) * spatial;
      float xv[VPL];
      if (VPL == 4 && vec_ok && v0 + 3 < spatial) {
        const float4 q = *reinterpret_cast<const float4*>(xp + v0);
        xv[0] = q.x; xv[1 % VPL] = q.y; xv[2 % VPL] = q.z; xv[3 % VPL] = q.w;
      } else {
#pragma unroll
        for (int v = 0; v < VPL; ++v) xv[v] = (v0 + v < spatial) ? xp[v0 + v] : 0.f;
      }
#pragma unroll
      for (int v = 0; v < VPL; ++v) {
        const float z = e2e::in_act(xv[v], a, b, sl);
#pragma unroll
        for (int t = 0; t < KT; ++t) part[v][t] = fmaf(wt[t], z, part[v][t]);
      }
    }
#pragma unroll
    for (int v = 0; v < VPL; ++v)
#pragma unroll
      for (int t = 0; t < KT; ++t) acc[v][t] += part[v][t];
  }
  const int Ho = H * kh, Wo = W * kw;
  float* yp = y + ((long long)n * Cout + o) * spatial * KT;
  if (VPL == 2 && kw == 2 && (W % 2) == 0 && v0 + 1 < spatial) {
    int dv, hv, wv;
    decode_dhw(v0, W, H, dv, hv, wv);
#pragma unroll
    for (int t = 0; t < KT; t += 2) {
      int i, j, k;
      tap_ijk(t, kh, kw, i, j, k);
      *reinterpret_cast<float4*>(yp + ((long long)(dv * kd + i) * Ho + (hv * kh + j)) * Wo + wv * 2) =
          make_float4(acc[0][t], acc[0][(t + 1) % KT], acc[1 % VPL][t], acc[1 % VPL][(t + 1) % KT]);
    }
    return;
  }
#pragma unroll
  for (int v = 0; v < VPL; ++v) {
    const long long vi = v0 + v;
    if (vi >= spatial) continue;
    int dv, hv, wv;
    decode_dhw(vi, W, H, dv, hv, wv);
#pragma unroll
    for (int t = 0; t < KT; ++t) {
      int i, j, k;
      tap_ijk(t, kh, kw, i, j, k);
      yp[((long long)(dv * kd + i) * Ho + (hv * kh + j)) * Wo + (wv * kw + k)] = acc[v][t];
    }
  }
}

// ---- data gradient: one thread = one input voxel of one input channel ---------------------------------------
template <int KT>
__global__ __launch_bounds__(256) void convT_dgrad_kernel(const float* __restrict__ dy, const float* __restrict__ w,
                                                          const unsigned* __restrict__ live_t, float* __restrict__ dx,
                                                          int accumulate, int Cin, int Cout, int D, int H, int W, int kd,
                                                          int kh, int kw) {
  const int c = blockIdx.y, n = blockIdx.z;
  const long long spatial = (long long)D * H * W;
  const long long vi = (long long)blockIdx.x * 256 + threadIdx.x;
  const bool in = vi < spatial;
  const long long vv = in ? vi : 0;
  int dv, hv, wv;
  decode_dhw(vv, W, H, dv, hv, wv);
  const int Ho = H * kh, Wo = W * kw;
  long long offs[KT];
#pragma unroll
  for (int t = 0; t < KT; ++t) {
    int i, j, k;
    tap_ijk(t, kh, kw, i, j, k);
    offs[t] = ((long long)(dv * kd + i) * Ho + (hv * kh + j)) * Wo + (wv * kw + k);
  }
  float acc = 0.f;
  const int words = e2e::cdiv(Cout, 32);
  for (int wd = 0; wd < words; ++wd) {
    unsigned bits = live_t ? live_t[(long long)c * words + wd] : 0xffffffffu;
    const int remain = Cout - wd * 32;
    if (remain < 32) bits &= (1u << remain) - 1u;
    bits = __builtin_amdgcn_readfirstlane(bits);
    while (bits) {
      const int o = wd * 32 + __builtin_ctz(bits);
      bits &= bits - 1;
      const float* wp = w + ((long long)c * Cout + o) * KT;
      const float* dyp = dy + ((long long)n * Cout + o) * spatial * KT;
#pragma unroll
      for (int t = 0; t < KT; ++t) acc = fmaf(wp[t], dyp[offs[t]], acc);
    }
  }
  if (in) {
    float* dst = dx + ((long long)n * Cin + c) * spatial + vi;
    if (accumulate) *dst += acc;
    else *dst = acc;
  }
}

// ---- weight gradient (dense) on the fp32 MFMA ------------------------------------------------------------------
// dW[c, o, t] = sum_{n, v} z[n, c, v] * dy[n, o, out(v, t)].
// One workgroup = (32 input channels) x (32 output channels) x all KT taps over a chunk of voxel tiles.
// Wave (ch, oh) owns the 16 x 16 sub-block (c half, o half): KT accumulator tiles of v_mfma_f32_16x16x4_f32
// (exact fp32 fma chain, so the sum is a plain fp32 accumulation like the reference's).  The reduction index is
// the voxel: it lives inside the MFMA K dimension and in the loop, so no cross-lane reduction is needed.
// Partial sums per chunk go to a slab; a second kernel adds the slabs in fixed order (deterministic).

constexpr int WG_TV = 64;                 // voxels staged per step
constexpr int WG_ZS = WG_TV + 2;          // channel stride in LDS, == 2 (mod 32): conflict-free A/B fragment reads

template <int KT>
__global__ __launch_bounds__(256) void convT_wgrad_kernel(const float* __restrict__ x, const float* __restrict__ scale,
                                                          const float* __restrict__ shift, float slope,
                                                          const float* __restrict__ dy, float* __restrict__ slab, int B,
                                                          int Cin, int Cout, int D, int H, int W, int kd, int kh, int kw,
                                                          int tiles_per_chunk, int nchunks) {
  __shared__ float zs[32 * WG_ZS];
  __shared__ float ds[32 * KT * WG_ZS];
  const int chunk = blockIdx.x;
  const int cblocks = e2e::cdiv(Cin, 32);
  const int cb = blockIdx.y % cblocks, ob = blockIdx.y / cblocks;
  const long long spatial = (long long)D * H * W;
  const long long tiles_per_n = e2e::cdivll(spatial, WG_TV);
  const long long total_tiles = tiles_per_n * B;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ch = wave & 1, oh = wave >> 1;
  const int Ho = H * kh, Wo = W * kw;

  f32x4_t acc[KT];
#pragma unroll
  for (int t = 0; t < KT; ++t) acc[t] = f32x4_t{0.f, 0.f, 0.f, 0.f};

  for (int ti = 0; ti < tiles_per_chunk; ++ti) {
    const long long tile = (long long)chunk * tiles_per_chunk + ti;
    if (tile >= total_tiles) break;
    const int n = (int)((unsigned)tile / (unsigned)tiles_per_n);
    const long long vbase = (tile - (long long)n * tiles_per_n) * WG_TV;
    // stage z[32 c][64 v]
    for (int idx = tid; idx < 32 * WG_TV; idx += 256) {
      const int cl = idx / WG_TV, pv = idx - cl * WG_TV;
      const int c = cb * 32 + cl;
      const long long vi = vbase + pv;
      float val = 0.f;
      if (c < Cin && vi < spatial) {
        val = x[((long long)n * Cin + c) * spatial + vi];
        if (scale) val = e2e::in_act(val, scale[(long long)n * Cin + c], shift[(long long)n * Cin + c], slope);
      }
      zs[cl * WG_ZS + pv] = val;
    }
    // stage dy[32 o][KT][64 v]
    for (int idx = tid; idx < 32 * KT * WG_TV; idx += 256) {
      const int pv = idx % WG_TV;
      const int rest = idx / WG_TV;
      const int t = rest % KT, ol = rest / KT;
      const int o = ob * 32 + ol;
      const long long vi = vbase + pv;
      float val = 0.f;
      if (o < Cout && vi < spatial) {
        int dv, hv, wv;
        decode_dhw(vi, W, H, dv, hv, wv);
        int i, j, k;
        tap_ijk(t, kh, kw, i, j, k);
        val = dy[((long long)n * Cout + o) * spatial * KT + ((long long)(dv * kd + i) * Ho + (hv * kh + j)) * Wo + (wv * kw + k)];
      }
      ds[(ol * KT + t) * WG_ZS + pv] = val;
    }
    __syncthreads();
    const int li = lane & 15, lk = lane >> 4;
    const float* ap = zs + (ch * 16 + li) * WG_ZS + lk;
    const float* bp = ds + ((oh * 16 + li) * KT) * WG_ZS + lk;
#pragma unroll 4
    for (int k0 = 0; k0 < WG_TV; k0 += 4) {
      const float a = ap[k0];
#pragma unroll
      for (int t = 0; t < KT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, bp[t * WG_ZS + k0], acc[t], 0, 0, 0);
    }
    __syncthreads();
  }
  // D[i = c][j = o]: col = lane & 15 -> o, row = (lane >> 4) * 4 + reg -> c
  float* sp = slab + (long long)chunk * Cin * Cout * KT;
  const int o = ob * 32 + oh * 16 + (lane & 15);
#pragma unroll
  for (int t = 0; t < KT; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int c = cb * 32 + ch * 16 + (lane >> 4) * 4 + r;
      if (c < Cin && o < Cout) sp[((long long)c * Cout + o) * KT + t] = acc[t][r];
    }
}

// ---- where the dy of one tile lives (kw == 2, even W): every matrix-pipe kernel that reads dy asks here -------------------
// A tile is TV consecutive input voxels of one sample, starting at vbase.  Its dy is fetched as aligned float4 "units": unit
// (rr, vp) of an output channel = output row rr = i * kh + j of the KDH = kd * kh rows an input row produces, voxel pair vp.
// The float4 holds taps (rr, k = 0), (rr, k = 1) of voxel 2 vp and then of voxel 2 vp + 1.  A channel has UPC units, vp
// fastest, so consecutive units are consecutive float4 of one output row.
template <int KDH, int TV>
struct DyTile {
  static constexpr int KT = 2 * KDH;
  static constexpr int VP = TV / 2;
  static constexpr int UPC = KDH * VP;
  struct Unit { int rr, vp; };
  int Cout, H, W, kd, kh, Ho, Wo;
  long long spatial, ospatial;                           // voxels of an input / output channel

  __device__ __forceinline__ DyTile(int Cout_, int D, int H_, int W_, int kd_, int kh_)
      : Cout(Cout_), H(H_), W(W_), kd(kd_), kh(kh_), Ho(H_ * kh_), Wo(W_ * 2), spatial((long long)D * H_ * W_), ospatial(spatial * KT) {}

  // r-th unit of a channel (in the caller's index type: signed or unsigned division, as the caller's other arithmetic is)
  template <class I>
  static __device__ __forceinline__ Unit unit(I r) { return Unit{(int)(r / VP), (int)(r % VP)}; }

  // W % TV == 0: a tile never crosses an input row, and spatial % TV == 0, so there is no ragged last tile.  Then a unit's
  // offset is row_base (wave uniform, changes with the tile) + chan_off + row_off (per thread, never change), and every
  // voxel of the tile exists: chan_ok alone decides whether the unit is read.
  __device__ __forceinline__ bool row_tiles() const { return (W % TV) == 0; }
  // A thread's offsets from its row_base span fewer than 64 channel planes of `spatial` floats in any of these kernels, so
  // below 2^24 voxels they fit 32 bits as BYTE offsets (64 x 2^24 x 4 B = 2^32).
  __device__ __forceinline__ bool byte_offsets_fit_32() const { return spatial < (1ll << 24); }
  // channel o0 + ol (a block's first channel + the caller's place in it) of sample n
  __device__ __forceinline__ long long row_base(int n, int o0, int ol, long long vbase) const {
    int dv, hv, w0;
    decode_dhw(vbase, W, H, dv, hv, w0);
    return ((long long)n * Cout + o0 + ol) * ospatial + ((long long)dv * kd * Ho + (long long)hv * kh) * Wo + 2 * w0;
  }
  __device__ __forceinline__ long long chan_off(int ol) const { return (long long)ol * ospatial; }      // ol channels further on
  __device__ __forceinline__ long long row_off(Unit u) const {
    const int ii = u.rr / kh, jj = u.rr - ii * kh;
    return ((long long)ii * Ho + jj) * Wo + 4 * u.vp;
  }
  // the validity rule: the channel exists and so do both voxels of the pair (spatial is even: a pair is never half inside)
  __device__ __forceinline__ bool chan_ok(int o) const { return o < Cout; }
  __device__ __forceinline__ bool valid(int o, long long vbase, Unit u) const { return o < Cout && vbase + 2 * u.vp + 1 < spatial; }
  // any tile: the offset in dy of the unit of channel o, or 0 (a readable address whose value the commit drops) where it is not valid
  __device__ __forceinline__ long long offset(int n, int o, long long vbase, Unit u) const {
    const long long vi = vbase + 2 * u.vp;
    const bool ok = o < Cout && vi + 1 < spatial;
    long long off = 0;
    if (ok) {
      int dv, hv, wv;
      decode_dhw(vi, W, H, dv, hv, wv);
      const int ii = u.rr / kh, jj = u.rr - ii * kh;
      off = ((long long)n * Cout + o) * ospatial + ((long long)(dv * kd + ii) * Ho + (hv * kh + jj)) * Wo + 2 * wv;
    }
    return off;
  }
  // where the unit's values go in an LDS image of 32 channels, as an index into it (ol = the channel's place in the image,
  // EPV = index steps per staged value, STRIDE = index steps per row):
  //   [tap][channel][voxel]: tap (rr, K) of voxels 2 vp, 2 vp + 1 (adjacent)
  template <int K, int STRIDE, int EPV>
  static __device__ __forceinline__ int tap_major(int ol, Unit u) { return ((u.rr * 2 + K) * 32 + ol) * STRIDE + 2 * EPV * u.vp; }
  //   [voxel][channel x KT taps]: taps (rr, 0), (rr, 1) (adjacent) of voxel 2 vp; voxel 2 vp + 1 one row on
  template <int STRIDE, int EPV>
  static __device__ __forceinline__ int voxel_major(int ol, Unit u) { return (2 * u.vp) * STRIDE + (ol * KT + 2 * u.rr) * EPV; }
};

// ---- v2 (kw == 2, even W): software-pipelined staging ---------------------------------------------------------------
// The op is HBM-bound when every byte is read once (25.6 FLOP/B at 64 -> 32 channels), so the workgroup covers NCB
// blocks of 32 input channels against one block of 32 output channels and stages the dy tile once for all of them.
// A tile = 64 consecutive input voxels.  dy arrives as aligned float4 = (k=0,1) x (voxel pair) of one output row and
// is scattered to an LDS image [tap][o][voxel] whose channel stride == 2 (mod 32): conflict-free B fragments.  Loads
// of tile t+1 are issued into registers before the MFMA phase of tile t and committed after it.

template <int KDH, int NCB>     // KDH = kd * kh (output rows per input voxel row), KT = 2 * KDH
__global__ __launch_bounds__(256 * NCB) void convT_wgrad_v2_kernel(const float* __restrict__ x, const float* __restrict__ scale,
                                                                   const float* __restrict__ shift, float slope,
                                                                   const float* __restrict__ dy, float* __restrict__ slab,
                                                                   int B, int Cin, int Cout, int D, int H, int W, int kd, int kh,
                                                                   int tiles_per_chunk, int cgroups) {
  constexpr int KT = 2 * KDH;
  constexpr int TS = WG_TV + 2;                       // 66 == 2 (mod 32)
  constexpr int YCW = 32 / (4 * NCB);                  // dy channels staged per wave
  using Tile = DyTile<KDH, WG_TV>;
  constexpr int YIT = Tile::UPC / 64;                  // wave iterations per dy channel
  static_assert(KDH == 2 || KDH == 4, "kd*kh in {2,4}");
  __shared__ __attribute__((aligned(16))) float zs[NCB * 32 * TS];
  __shared__ __attribute__((aligned(16))) float ds[KT * 32 * TS];

  const int chunk = blockIdx.x;
  const int cg = blockIdx.y % cgroups, ob = blockIdx.y / cgroups;
  const long long spatial = (long long)D * H * W;
  const long long tiles_per_n = e2e::cdivll(spatial, WG_TV);
  const long long total_tiles = tiles_per_n * B;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int cbl = wave >> 2, ch = wave & 1, oh = (wave >> 1) & 1;
  const Tile yt(Cout, D, H, W, kd, kh);
  const int cbase = cg * NCB * 32;

  f32x4_t acc[KT];
#pragma unroll
  for (int t = 0; t < KT; ++t) acc[t] = f32x4_t{0.f, 0.f, 0.f, 0.f};

  const long long tile_lo = (long long)chunk * tiles_per_chunk;
  long long tile_hi = tile_lo + tiles_per_chunk;
  if (tile_hi > total_tiles) tile_hi = total_tiles;

  // z: each wave stages 8 channels x 64 voxels = 128 float4 -> 2 iterations; lane -> (channel k = g / 16, group g % 16)
  f32x4_t vz[2], vy[YCW][YIT];
  float za[2], zb[2];
  const bool row_tiles = yt.row_tiles();
  long long yoff[YIT];
#pragma unroll
  for (int it = 0; it < YIT; ++it) yoff[it] = yt.row_off(Tile::unit(lane + 64u * it));
  auto prefetch = [&](long long tile) {
    const int n = (int)((unsigned)tile / (unsigned)tiles_per_n);
    const long long vbase = (tile - (long long)n * tiles_per_n) * WG_TV;
#pragma unroll
    for (int it = 0; it < 2; ++it) {
      const int g = lane + 64 * it;
      const int c = cbase + wave * 8 + (g >> 4);
      const long long vi = vbase + (g & 15) * 4;
      const bool ok = c < Cin && vi + 3 < spatial;
      const long long off = ok ? ((long long)n * Cin + c) * spatial + vi : 0;
      vz[it] = *reinterpret_cast<gf4_p>((gfloat_p)x + off);
      za[it] = 1.f; zb[it] = 0.f;
      if (scale != nullptr && c < Cin) { za[it] = scale[(long long)n * Cin + c]; zb[it] = shift[(long long)n * Cin + c]; }
    }
    if (row_tiles) {
      const long long tbase = yt.row_base(n, ob * 32, wave * YCW, vbase);
      const int yo0 = ob * 32 + wave * YCW;            // this wave fetches dy channels yo0 .. yo0 + YCW
#pragma unroll
      for (int k = 0; k < YCW; ++k)
#pragma unroll
        for (int it = 0; it < YIT; ++it)
          vy[k][it] = *reinterpret_cast<gf4_p>((gfloat_p)dy + (yt.chan_ok(yo0 + k) ? tbase + yt.chan_off(k) + yoff[it] : 0));
      return;
    }
#pragma unroll
    for (int k = 0; k < YCW; ++k) {
      const int o = ob * 32 + wave * YCW + k;
#pragma unroll
      for (int it = 0; it < YIT; ++it) vy[k][it] = *reinterpret_cast<gf4_p>((gfloat_p)dy + yt.offset(n, o, vbase, Tile::unit(lane + 64u * it)));
    }
  };
  auto commit = [&](long long tile) {
    const int n = (int)((unsigned)tile / (unsigned)tiles_per_n);
    const long long vbase = (tile - (long long)n * tiles_per_n) * WG_TV;
#pragma unroll
    for (int it = 0; it < 2; ++it) {
      const int g = lane + 64 * it;
      const int cl = wave * 8 + (g >> 4);
      const long long vi = vbase + (g & 15) * 4;
      const bool ok = cbase + cl < Cin && vi + 3 < spatial;
      float2* dst = reinterpret_cast<float2*>(zs + cl * TS + (g & 15) * 4);
      float v[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float t = vz[it][j];
        if (scale != nullptr) t = e2e::in_act(t, za[it], zb[it], slope);
        v[j] = ok ? t : 0.f;
      }
      dst[0] = make_float2(v[0], v[1]);
      dst[1] = make_float2(v[2], v[3]);
    }
#pragma unroll
    for (int k = 0; k < YCW; ++k) {
      const int ol = wave * YCW + k;
#pragma unroll
      for (int it = 0; it < YIT; ++it) {
        const typename Tile::Unit u = Tile::unit(lane + 64u * it);
        const bool ok = yt.valid(ob * 32 + ol, vbase, u);
        const f32x4_t q = vy[k][it];
        float2* d0 = reinterpret_cast<float2*>(ds + Tile::template tap_major<0, TS, 1>(ol, u));
        float2* d1 = reinterpret_cast<float2*>(ds + Tile::template tap_major<1, TS, 1>(ol, u));
        *d0 = ok ? make_float2(q[0], q[2]) : make_float2(0.f, 0.f);
        *d1 = ok ? make_float2(q[1], q[3]) : make_float2(0.f, 0.f);
      }
    }
  };

  if (tile_lo < tile_hi) {
    prefetch(tile_lo);
    for (long long tile = tile_lo; tile < tile_hi; ++tile) {
      commit(tile);
      __syncthreads();
      if (tile + 1 < tile_hi) prefetch(tile + 1);
      const int li = lane & 15, lk = lane >> 4;
      const float* ap = zs + (cbl * 32 + ch * 16 + li) * TS + lk;
      const float* bp = ds + (oh * 16 + li) * TS + lk;
#pragma unroll 4
      for (int k0 = 0; k0 < WG_TV; k0 += 4) {
        const float a = ap[k0];
#pragma unroll
        for (int t = 0; t < KT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, bp[t * 32 * TS + k0], acc[t], 0, 0, 0);
      }
      __syncthreads();
    }
  }
  // D[i = c][j = o]: col = lane & 15 -> o, row = (lane >> 4) * 4 + reg -> c
  float* sp = slab + (long long)chunk * Cin * Cout * KT;
  const int o = ob * 32 + oh * 16 + (lane & 15);
#pragma unroll
  for (int t = 0; t < KT; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int c = cbase + cbl * 32 + ch * 16 + (lane >> 4) * 4 + r;
      if (c < Cin && o < Cout) sp[((long long)c * Cout + o) * KT + t] = acc[t][r];
    }
}

// ---- weight gradient, split operands (kw == 2, even W): the v2 pipeline on the bf16 / fp16 matrix pipe, fp32-exact operands ----
// v2 is bound by its fp32 MFMAs (128 x 32 cycles per 64-voxel tile and wave, two waves per SIMD: 0.125 ms of a 0.25 ms
// launch at 64 -> 32 @64^3).  Both operands are split into three bf16 pieces when they are staged ([piece][row][64 voxels]
// bf16, row stride 144 B); the reduction dimension (voxels) is contiguous in both images, so an A / B fragment is one
// ds_read_b128; 96 v_mfma_f32_16x16x32_bf16 x 16 cycles per tile and wave.  The forward and the data gradient of the same
// scheme follow below.
//
// Round 6: the same three GEMMs with fp16 TWO-piece operands (NP = 2: three products per fp32 product instead of six, through
// v_mfma_f32_16x16x32_f16; NP = 3 keeps the bf16 three-piece form).  Both forms and the operand scales: e2e_split.h.  The range
// words: the activations' from the bound e2e_conv133_input_ranges derives from the producer's InstanceNorm parameters, the weights'
// from their measured maximum, dy's from max |dy of the consuming conv| x the L1 norm of that conv's weights over this tensor's
// channels.  Without the words a launch stays on the bf16 form.
// the NP packed words (two values each: `a` in the low half) of a value pair, piece p at dst + p * pstride
template <int NP>
__device__ __forceinline__ void store_pair(unsigned char* dst, int pstride, float a, float b) {
  if constexpr (NP == 2) {
    unsigned hw, lw;
    split_f16x2_fma_mix(a, b, hw, lw);
    *reinterpret_cast<unsigned*>(dst) = hw;
    *reinterpret_cast<unsigned*>(dst + pstride) = lw;
  } else {
    unsigned ha, ma, la, hb, mb, lb;
    split_bf3(a, ha, ma, la);
    split_bf3(b, hb, mb, lb);
    *reinterpret_cast<unsigned*>(dst) = pack_hi16(ha, hb);
    *reinterpret_cast<unsigned*>(dst + pstride) = pack_hi16(ma, mb);
    *reinterpret_cast<unsigned*>(dst + 2 * pstride) = pack_hi16(la, lb);
  }
}
// a fragment of eight values held in registers (weights): piece p -> out[p]
template <int NP>
__device__ __forceinline__ void split_frag(const float (&v)[8], bf16x8_t (&out)[NP]) {
  if constexpr (NP == 2) {
    unsigned hw[4], lw[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) split_f16x2_fma_mix(v[2 * j], v[2 * j + 1], hw[j], lw[j]);
    out[0] = __builtin_bit_cast(bf16x8_t, u32x4_t{hw[0], hw[1], hw[2], hw[3]});
    out[1] = __builtin_bit_cast(bf16x8_t, u32x4_t{lw[0], lw[1], lw[2], lw[3]});
  } else {
    unsigned h[8], m[8], l[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) split_bf3(v[j], h[j], m[j], l[j]);
    out[0] = __builtin_bit_cast(bf16x8_t, u32x4_t{pack_hi16(h[0], h[1]), pack_hi16(h[2], h[3]), pack_hi16(h[4], h[5]), pack_hi16(h[6], h[7])});
    out[1] = __builtin_bit_cast(bf16x8_t, u32x4_t{pack_hi16(m[0], m[1]), pack_hi16(m[2], m[3]), pack_hi16(m[4], m[5]), pack_hi16(m[6], m[7])});
    out[2] = __builtin_bit_cast(bf16x8_t, u32x4_t{pack_hi16(l[0], l[1]), pack_hi16(l[2], l[3]), pack_hi16(l[4], l[5]), pack_hi16(l[6], l[7])});
  }
}
// acc += A B rebuilt from the pieces: small terms first
template <int NP>
__device__ __forceinline__ f32x4_t mma_pieces(const bf16x8_t (&a)[NP], const bf16x8_t (&b)[NP], f32x4_t c) {
  if constexpr (NP == 2) {
    const f16x8_t a0 = __builtin_bit_cast(f16x8_t, a[0]), a1 = __builtin_bit_cast(f16x8_t, a[1]);
    const f16x8_t b0 = __builtin_bit_cast(f16x8_t, b[0]), b1 = __builtin_bit_cast(f16x8_t, b[1]);
    c = __builtin_amdgcn_mfma_f32_16x16x32_f16(a1, b0, c, 0, 0, 0);      // lo * hi
    c = __builtin_amdgcn_mfma_f32_16x16x32_f16(a0, b1, c, 0, 0, 0);      // hi * lo
    c = __builtin_amdgcn_mfma_f32_16x16x32_f16(a0, b0, c, 0, 0, 0);      // hi * hi
  } else {
    // lo*hi, mid*mid, hi*lo, then mid*hi, hi*mid, then hi*hi
    c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[2], b[0], c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[1], b[1], c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[0], b[2], c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[1], b[0], c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[0], b[1], c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[0], b[0], c, 0, 0, 0);
  }
  return c;
}
// scale exponent of a tensor bounded by the product of the floats whose bit patterns are *wa and *wb (either may be null = 1)
__device__ __forceinline__ int ct_scale_exp(const unsigned* wa, const unsigned* wb) {
  float b = 1.f;
  if (wa != nullptr) b *= __builtin_bit_cast(float, __builtin_nontemporal_load(wa));
  if (wb != nullptr) b *= __builtin_bit_cast(float, __builtin_nontemporal_load(wb));
  return scale_exp<LIM_CT>(__builtin_bit_cast(unsigned, b));
}

// A tile = WG_TV = 64 input voxels: one workgroup per CU (up to 138 KB of LDS), its phases serial (commit, barrier, matrix phase,
// barrier, with a single LDS image).
template <int KDH, int NCB, int NP>     // KDH = kd * kh (output rows per input voxel row), KT = 2 * KDH; NP pieces per operand
__global__ __launch_bounds__(256 * NCB, 1) void convT_wgrad_bf3_kernel(const float* __restrict__ x, const float* __restrict__ scale,
                                                                   const float* __restrict__ shift, float slope,
                                                                   const float* __restrict__ dy, float* __restrict__ slab,
                                                                   int B, int Cin, int Cout, int D, int H, int W, int kd, int kh,
                                                                   int tiles_per_chunk, int cgroups, const unsigned* __restrict__ x_word,
                                                                   const unsigned* __restrict__ dy_word_a, const unsigned* __restrict__ dy_word_b) {
  constexpr int KT = 2 * KDH;
  using Tile = DyTile<KDH, WG_TV>;
  constexpr int RS = WG_TV * 2 + 16;                   // 144 bytes per staged row (64 voxels bf16 + 16: odd multiple of 16, conflict-free b128)
  constexpr int ZG = WG_TV / 4;                        // 16 float4 groups per input channel row
  constexpr int ZIT = 8 * ZG / 64;                     // 2 wave iterations over its 8 input channels
  constexpr int ZP = NCB * 32 * RS, YP = KT * 32 * RS;  // bytes per piece
  constexpr int YCW = 32 / (4 * NCB);                  // dy channels staged per wave
  constexpr int YIT = Tile::UPC / 64;                  // wave iterations per dy channel
  static_assert(KDH == 2 || KDH == 4, "kd*kh in {2,4}");
  static_assert(NP * (NCB * 32 + 2 * KDH * 32) * RS <= 163840, "LDS budget");
  __shared__ __attribute__((aligned(16))) unsigned char zs[NP * ZP];     // [piece][channel][voxel] bf16 / fp16
  __shared__ __attribute__((aligned(16))) unsigned char ds[NP * YP];     // [piece][tap][out channel][voxel]
  // fp16 two-piece form: operand scales 2^kx (activations) and 2^ky (dy), the slab un-scaled by the two exact factors
  const int kx = NP == 2 ? ct_scale_exp(x_word, nullptr) : 0, ky = NP == 2 ? ct_scale_exp(dy_word_a, dy_word_b) : 0;
  const float xsc = pow2f(kx), ysc = pow2f(ky), unx = pow2f(-kx), uny = pow2f(-ky);

  const int chunk = blockIdx.x;
  const int cg = blockIdx.y % cgroups, ob = blockIdx.y / cgroups;
  const long long spatial = (long long)D * H * W;
  const long long tiles_per_n = e2e::cdivll(spatial, WG_TV);
  const long long total_tiles = tiles_per_n * B;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int cbl = wave >> 2, ch = wave & 1, oh = (wave >> 1) & 1;
  const Tile yt(Cout, D, H, W, kd, kh);
  const int cbase = cg * NCB * 32;

  f32x4_t acc[KT];
#pragma unroll
  for (int t = 0; t < KT; ++t) acc[t] = f32x4_t{0.f, 0.f, 0.f, 0.f};

  const long long tile_lo = (long long)chunk * tiles_per_chunk;
  long long tile_hi = tile_lo + tiles_per_chunk;
  if (tile_hi > total_tiles) tile_hi = total_tiles;

  // z: each wave stages 8 channels x 64 voxels = 128 float4 -> 2 iterations; lane -> (channel k = g / 16, group g % 16)
  f32x4_t vz[ZIT], vy[YCW][YIT];
  float za[ZIT], zb[ZIT];
  const bool row_tiles = yt.row_tiles() && yt.byte_offsets_fit_32();
  long long yoff[YIT];
#pragma unroll
  for (int it = 0; it < YIT; ++it) yoff[it] = yt.row_off(Tile::unit(lane + 64 * it));
  // row tiles: a tile's addresses are a wave-uniform base (scalar arithmetic) plus per-lane byte offsets that never change;
  // the normalise-on-load coefficients change only with the batch item.  (Clock stamps: issuing the ten float4 loads of a
  // tile with per-lane 64-bit index arithmetic, two integer divisions and four coefficient loads took ~2500 cycles, as long
  // as the tile's matrix phase.)
  unsigned zoffb[ZIT], yoffb[YCW][YIT];
  bool zcok[ZIT];
#pragma unroll
  for (int it = 0; it < ZIT; ++it) {
    const int g = lane + 64 * it;
    zcok[it] = cbase + wave * 8 + g / ZG < Cin;
    zoffb[it] = zcok[it] ? (unsigned)(((long long)(wave * 8 + g / ZG) * spatial + (g % ZG) * 4) * 4) : 0u;
  }
#pragma unroll
  for (int k = 0; k < YCW; ++k)
#pragma unroll
    for (int it = 0; it < YIT; ++it)
      yoffb[k][it] = yt.chan_ok(ob * 32 + wave * YCW + k) ? (unsigned)((yt.chan_off(k) + yoff[it]) * 4) : 0u;
  int cur_n = -1;
  auto prefetch = [&](long long tile) {
    const int n = (int)((unsigned)tile / (unsigned)tiles_per_n);
    const long long vbase = (tile - (long long)n * tiles_per_n) * WG_TV;
    if (row_tiles) {
      if (n != cur_n) {
        cur_n = n;
#pragma unroll
        for (int it = 0; it < ZIT; ++it) {
          const int c = cbase + wave * 8 + (lane + 64 * it) / ZG;
          za[it] = 1.f; zb[it] = 0.f;
          if (scale != nullptr && c < Cin) { za[it] = scale[(long long)n * Cin + c]; zb[it] = shift[(long long)n * Cin + c]; }
        }
      }
      const int ych = ob * 32 + wave * YCW < Cout ? ob * 32 + wave * YCW : 0;      // (waves past the last channel read channel 0 and drop it)
      const long long ybase = yt.row_base(n, ych, 0, vbase);
      const char* zb8 = reinterpret_cast<const char*>(x + ((long long)n * Cin + cbase) * spatial + vbase);
      const char* yb8 = reinterpret_cast<const char*>(dy + ybase);
#pragma unroll
      for (int it = 0; it < ZIT; ++it) vz[it] = *reinterpret_cast<gf4_p>((gfloat_p)(zb8 + zoffb[it]));
#pragma unroll
      for (int k = 0; k < YCW; ++k)
#pragma unroll
        for (int it = 0; it < YIT; ++it) vy[k][it] = *reinterpret_cast<gf4_p>((gfloat_p)(yb8 + yoffb[k][it]));
      return;
    }
#pragma unroll
    for (int it = 0; it < ZIT; ++it) {
      const int g = lane + 64 * it;
      const int c = cbase + wave * 8 + g / ZG;
      const long long vi = vbase + (g % ZG) * 4;
      const bool ok = c < Cin && vi + 3 < spatial;
      const long long off = ok ? ((long long)n * Cin + c) * spatial + vi : 0;
      vz[it] = *reinterpret_cast<gf4_p>((gfloat_p)x + off);
      za[it] = 1.f; zb[it] = 0.f;
      if (scale != nullptr && c < Cin) { za[it] = scale[(long long)n * Cin + c]; zb[it] = shift[(long long)n * Cin + c]; }
    }
#pragma unroll
    for (int k = 0; k < YCW; ++k) {
      const int o = ob * 32 + wave * YCW + k;
#pragma unroll
      for (int it = 0; it < YIT; ++it) vy[k][it] = *reinterpret_cast<gf4_p>((gfloat_p)dy + yt.offset(n, o, vbase, Tile::unit(lane + 64 * it)));
    }
  };
  auto commit = [&](long long tile) {
    const int n = (int)((unsigned)tile / (unsigned)tiles_per_n);
    const long long vbase = (tile - (long long)n * tiles_per_n) * WG_TV;
#pragma unroll
    for (int it = 0; it < ZIT; ++it) {
      const int g = lane + 64 * it;
      const int cl = wave * 8 + g / ZG;
      const long long vi = vbase + (g % ZG) * 4;
      const bool ok = cbase + cl < Cin && vi + 3 < spatial;
      unsigned char* dst = zs + cl * RS + (g % ZG) * 8;
      float tz[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float t = vz[it][j];
        if (scale != nullptr) t = e2e::in_act(t, za[it], zb[it], slope);
        tz[j] = ok ? (NP == 2 ? t * xsc : t) : 0.f;
      }
      store_pair<NP>(dst, ZP, tz[0], tz[1]);
      store_pair<NP>(dst + 4, ZP, tz[2], tz[3]);
    }
#pragma unroll
    for (int k = 0; k < YCW; ++k) {
      const int ol = wave * YCW + k;
#pragma unroll
      for (int it = 0; it < YIT; ++it) {
        const typename Tile::Unit u = Tile::unit(lane + 64 * it);
        const bool ok = yt.valid(ob * 32 + ol, vbase, u);
        f32x4_t q = vy[k][it];
        if (!ok) q = f32x4_t{0.f, 0.f, 0.f, 0.f};
        if (NP == 2) q *= ysc;
        unsigned char* d0 = ds + Tile::template tap_major<0, RS, 2>(ol, u);
        unsigned char* d1 = ds + Tile::template tap_major<1, RS, 2>(ol, u);
        store_pair<NP>(d0, YP, q[0], q[2]);
        store_pair<NP>(d1, YP, q[1], q[3]);
      }
    }
  };

  if (tile_lo < tile_hi) {
    prefetch(tile_lo);
    for (long long tile = tile_lo; tile < tile_hi; ++tile) {
      commit(tile);
      __syncthreads();
      if (tile + 1 < tile_hi) prefetch(tile + 1);
      const int li = lane & 15, lk = lane >> 4;
      // A: channel row, 8 consecutive voxels 32 kb + 8 lk ..; B: out channel row of tap t, the same voxels
      const unsigned char* ap = zs + (cbl * 32 + ch * 16 + li) * RS + lk * 16;
      const unsigned char* bp = ds + (oh * 16 + li) * RS + lk * 16;
#pragma unroll
      for (int kb = 0; kb < WG_TV / 32; ++kb) {
        bf16x8_t af[NP];
#pragma unroll
        for (int sp = 0; sp < NP; ++sp) af[sp] = *reinterpret_cast<const bf16x8_t*>(ap + sp * ZP + kb * 64);
#pragma unroll
        for (int t = 0; t < KT; ++t) {
          bf16x8_t bf[NP];
#pragma unroll
          for (int sp = 0; sp < NP; ++sp) bf[sp] = *reinterpret_cast<const bf16x8_t*>(bp + sp * YP + t * 32 * RS + kb * 64);
          acc[t] = mma_pieces<NP>(af, bf, acc[t]);
        }
      }
      __syncthreads();
    }
  }
  // D[i = c][j = o]: col = lane & 15 -> o, row = (lane >> 4) * 4 + reg -> c
  float* sp = slab + (long long)chunk * Cin * Cout * KT;
  const int o = ob * 32 + oh * 16 + (lane & 15);
#pragma unroll
  for (int t = 0; t < KT; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int c = cbase + cbl * 32 + ch * 16 + (lane >> 4) * 4 + r;
      if (c < Cin && o < Cout) sp[((long long)c * Cout + o) * KT + t] = NP == 2 ? acc[t][r] * unx * uny : acc[t][r];
    }
}


// DSFF liveness of the (in channel c, out channel o) kernel from the bit tables of e2e_dsff_expand (null = all alive).  The
// GEMM kernels below multiply whole tiles, so a pruned kernel is dropped where the weight enters a fragment -- the result
// does not depend on pruned weights being exact zeros in memory.
__device__ __forceinline__ bool ct_alive_rows(const unsigned* live_t, int Cout, int c, int o) {   // live_t: [Cin][ceil(Cout/32)]
  return live_t == nullptr || ((live_t[(long long)c * ((Cout + 31) >> 5) + (o >> 5)] >> (o & 31)) & 1u);
}
__device__ __forceinline__ bool ct_alive_cols(const unsigned* live, int Cin, int c, int o) {      // live: [Cout][ceil(Cin/32)]
  return live == nullptr || ((live[(long long)o * ((Cin + 31) >> 5) + (c >> 5)] >> (c & 31)) & 1u);
}

// ---- data gradient v3 (kw == 2): dense GEMM on the fp32 matrix cores ----------------------------------------------------
// dx[c, v] = sum_{(t, o)} W[c, o, t] * dy[o, out(v, t)]:  M = 64 input channels per workgroup (16 per wave), N = 32
// consecutive input voxels per tile, K = 32 output channels x KT taps per chunk.  At DSFF density 0.2 the dense GEMM does
// 5x the useful FLOPs, but a walk over the live (c, o) pairs issues one scalar weight load and KT dependent reads per pair
// -- latency bound at ~4x the HBM time of this op -- while the matrix pipe runs the dense product in less time than that
// (dead kernels enter the fragments as zeros, so the result is the same sum).  E2E_CT_BF3=0, or a W that is no multiple
// of 32, selects this kernel; the split-operand form below serves the rest.
//   * a wave keeps its 16 x K slice of W in registers (K/4 A fragments) for the whole run of tiles;
//   * the dy tile [K][32 voxels] is staged through LDS (row stride 48: the two k-rows of a 32-lane read group land on
//     disjoint banks), software pipelined: the float4 loads of the next tile are issued before the MFMA phase.
template <int KDH>
__global__ __launch_bounds__(256) void convT_dgrad_v3_kernel(const float* __restrict__ dy, const float* __restrict__ w,
                                                             const unsigned* __restrict__ live_t,
                                                             float* __restrict__ dx, int accumulate, int B, int Cin, int Cout,
                                                             int D, int H, int W, int kd, int kh, int tiles_per_wg) {
  constexpr int KT = 2 * KDH;
  constexpr int OC = 32, TV = 32, TS = 48;
  using Tile = DyTile<KDH, TV>;
  constexpr int K = OC * KT, KS = K / 4;               // k-steps per chunk
  constexpr int NUY = OC * Tile::UPC / 256;            // float4 loads per thread per tile: unit tid + 256 i -> channel / UPC, unit % UPC
  __shared__ __attribute__((aligned(16))) float ds[K * TS];

  const long long spatial = (long long)D * H * W;
  const long long tiles_per_n = e2e::cdivll(spatial, TV);
  const long long total_tiles = tiles_per_n * B;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 15, lk = lane >> 4;
  const Tile yt(Cout, D, H, W, kd, kh);
  const int cbase = blockIdx.y * 64 + wave * 16;
  const long long tile_lo = (long long)blockIdx.x * tiles_per_wg;
  long long tile_hi = tile_lo + tiles_per_wg;
  if (tile_hi > total_tiles) tile_hi = total_tiles;
  if (tile_lo >= tile_hi) return;

  f32x4_t v[NUY];
  // row tiles: the per-thread part of the dy offsets is constant over the tiles.  (The general path re-derives (d, h, w)
  // per unit with 64-bit divisions: ~1000 vector instructions per tile and thread, more than the MFMA phase.)
  const bool row_tiles = yt.row_tiles();
  long long uoff[NUY];
#pragma unroll
  for (int i = 0; i < NUY; ++i) {
    const int u = tid + i * 256;
    const int ol = u / Tile::UPC;
    uoff[i] = yt.chan_off(ol) + yt.row_off(Tile::unit(u - ol * Tile::UPC));
  }
  auto prefetch = [&](long long tile, int o0) {
    const int n = (int)((unsigned)tile / (unsigned)tiles_per_n);
    const long long vbase = (tile - (long long)n * tiles_per_n) * TV;
    if (row_tiles) {
      const long long tbase = yt.row_base(n, o0, 0, vbase);
#pragma unroll
      for (int i = 0; i < NUY; ++i) {
        const int ol = (tid + i * 256) / Tile::UPC;
        v[i] = *reinterpret_cast<gf4_p>((gfloat_p)dy + (yt.chan_ok(o0 + ol) ? tbase + uoff[i] : 0));
      }
      return;
    }
#pragma unroll
    for (int i = 0; i < NUY; ++i) {
      const int u = tid + i * 256;
      const int ol = u / Tile::UPC;
      v[i] = *reinterpret_cast<gf4_p>((gfloat_p)dy + yt.offset(n, o0 + ol, vbase, Tile::unit(u - ol * Tile::UPC)));
    }
  };
  auto commit = [&](long long tile, int o0) {
    const int n = (int)((unsigned)tile / (unsigned)tiles_per_n);
    const long long vbase = (tile - (long long)n * tiles_per_n) * TV;
#pragma unroll
    for (int i = 0; i < NUY; ++i) {
      const int u = tid + i * 256;
      const int ol = u / Tile::UPC;
      const typename Tile::Unit un = Tile::unit(u - ol * Tile::UPC);
      const bool ok = yt.valid(o0 + ol, vbase, un);
      float2* d0 = reinterpret_cast<float2*>(ds + Tile::template tap_major<0, TS, 1>(ol, un));
      float2* d1 = reinterpret_cast<float2*>(ds + Tile::template tap_major<1, TS, 1>(ol, un));
      *d0 = ok ? make_float2(v[i][0], v[i][2]) : make_float2(0.f, 0.f);
      *d1 = ok ? make_float2(v[i][1], v[i][3]) : make_float2(0.f, 0.f);
    }
  };

  for (int o0 = 0; o0 < Cout; o0 += OC) {
    // A fragments of this wave: row c = cbase + li, k = 4 s + lk = t * 32 + ol
    float afrag[KS];
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      const int k = 4 * s + lk;
      const int t = k / OC, ol = k - t * OC;
      const int c = cbase + li, o = o0 + ol;
      afrag[s] = (c < Cin && o < Cout && ct_alive_rows(live_t, Cout, c, o)) ? w[((long long)c * Cout + o) * KT + t] : 0.f;
    }
    prefetch(tile_lo, o0);
    for (long long tile = tile_lo; tile < tile_hi; ++tile) {
      commit(tile, o0);
      __syncthreads();
      if (tile + 1 < tile_hi) prefetch(tile + 1, o0);    // in flight during the MFMA phase
      f32x4_t acc[TV / 16];
#pragma unroll
      for (int b = 0; b < TV / 16; ++b) acc[b] = f32x4_t{0.f, 0.f, 0.f, 0.f};
      const float* bp = ds + lk * TS + li;
      // B fragments in groups of G k-steps, two register sets: the LDS reads of group g + 1 are in flight while the
      // MFMAs of group g issue (left to the compiler this loop was read -> wait -> 2 MFMAs, one LDS round trip per k-step)
      constexpr int G = 8, NB = TV / 16;
      float bfr[2][G][NB];
#pragma unroll
      for (int i = 0; i < G; ++i)
#pragma unroll
        for (int b = 0; b < NB; ++b) bfr[0][i][b] = bp[4 * i * TS + b * 16];
#pragma unroll
      for (int g = 0; g < KS / G; ++g) {
        if (g + 1 < KS / G) {
#pragma unroll
          for (int i = 0; i < G; ++i)
#pragma unroll
            for (int b = 0; b < NB; ++b) bfr[(g + 1) & 1][i][b] = bp[4 * ((g + 1) * G + i) * TS + b * 16];
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int i = 0; i < G; ++i)
#pragma unroll
          for (int b = 0; b < NB; ++b)
            acc[b] = __builtin_amdgcn_mfma_f32_16x16x4f32(afrag[g * G + i], bfr[g & 1][i][b], acc[b], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
      }
      // D[i = c][j = v]: col = lane & 15 -> v, row = (lane >> 4) * 4 + reg -> c
      const int n = (int)((unsigned)tile / (unsigned)tiles_per_n);
      const long long vbase = (tile - (long long)n * tiles_per_n) * TV;
#pragma unroll
      for (int b = 0; b < TV / 16; ++b) {
        const long long vi = vbase + b * 16 + li;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int c = cbase + lk * 4 + r;
          if (c < Cin && vi < spatial) {
            float* dst = dx + ((long long)n * Cin + c) * spatial + vi;
            if (accumulate || o0 > 0) *dst += acc[b][r];
            else *dst = acc[b][r];
          }
        }
      }
      __syncthreads();
    }
  }
}

// ---- forward GEMM (kw == 2, W % 32 == 0, Cin <= 256): dense GEMM on the bf16 / fp16 matrix pipe with fp32-exact operands ----
// y[v, (o, t)] = sum_c z[v, c] W[c, (o, t)]:  M = 32 consecutive input voxels of a row per tile, K = Cin (NKB blocks of 32),
// N = Cout x KT output columns.  The gather kernel above re-reads the input once per output channel (through L2) and is
// bound by scalar weight loads and the per-voxel FMA chains (2.9 TB/s at 64 -> 32 @64^3); here
//   * a wave keeps the three-piece B fragments of its 8 / NKB column tiles (16 columns = 16 / KT output channels x KT taps)
//     in registers for its whole run of tiles (96 VGPRs);
//   * the z tile (normalise-on-load applied) is split and staged voxel-major, [piece][32 voxels][K bf16 + 16 B], once per
//     tile for all columns of the workgroup (4 waves x 8 / NKB x 16 columns); the next tile's loads fly during the matrix phase;
//   * D[voxel][column]: a lane holds 4 consecutive voxels of one (o, i, j, k) column; the k = 0 / 1 columns are neighbouring
//     lanes, so one DPP pair swap turns them into two aligned float4 stores of the interleaved output row.
template <int KDH, int NKB, int NP>
__global__ __launch_bounds__(256, 2) void convT_fwd_bf3_kernel(const float* __restrict__ x, const float* __restrict__ scale,
                                                               const float* __restrict__ shift, float slope,
                                                               const float* __restrict__ w, const unsigned* __restrict__ live,
                                                               float* __restrict__ y, int B, int Cin,
                                                               int Cout, int D, int H, int W, int kd, int kh, int tiles_per_wg,
                                                               const unsigned* __restrict__ x_word, const unsigned* __restrict__ w_word) {
  constexpr int KT = 2 * KDH;
  constexpr int TV = 32;
  constexpr int K = NKB * 32;
  constexpr int NTW = 8 / NKB;                          // 16-column tiles per wave
  constexpr int RS = K * 2 + 16;                        // bytes per staged voxel and piece (odd multiple of 16)
  constexpr int PSZ = TV * RS;
  constexpr int NRD = K / 64;                           // staging rounds: 256 threads x (2 channels x 4 voxels)
  __shared__ __attribute__((aligned(16))) unsigned char zs[NP * PSZ];
  const int kx = NP == 2 ? ct_scale_exp(x_word, nullptr) : 0, kwt = NP == 2 ? ct_scale_exp(w_word, nullptr) : 0;
  const float xsc = pow2f(kx), wsc = pow2f(kwt), unx = pow2f(-kx), unw = pow2f(-kwt);

  const long long spatial = (long long)D * H * W;
  const long long tiles_per_n = spatial / TV;
  const long long total_tiles = tiles_per_n * B;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 15, lk = lane >> 4;
  const int Ho = H * kh, Wo = W * 2;
  const long long ospatial = spatial * KT;
  const int ncols = Cout * KT;
  const int col0 = (blockIdx.y * 4 + wave) * NTW * 16;   // first column of this wave
  const long long tile_lo = (long long)blockIdx.x * tiles_per_wg;
  long long tile_hi = tile_lo + tiles_per_wg;
  if (tile_hi > total_tiles) tile_hi = total_tiles;
  if (tile_lo >= tile_hi) return;

  // B fragments: column n = col0 + 16 nt + li = (o, t), k = 32 kb + 8 lk + j = input channel
  bf16x8_t bfr[NTW][NKB][NP];
  long long coff[NTW];                                   // offset of the column's output row origin inside a sample
  bool cok[NTW];
#pragma unroll
  for (int nt = 0; nt < NTW; ++nt) {
    const int col = col0 + nt * 16 + li;
    cok[nt] = col < ncols;
    const int o = cok[nt] ? col / KT : 0, t = cok[nt] ? col - o * KT : 0;
    const int rr = t >> 1, kk = t & 1;
    const int ii = rr / kh, jj = rr - ii * kh;
    coff[nt] = (long long)o * ospatial + ((long long)ii * Ho + jj) * Wo + 4 * kk;   // + 4 kk: the second float4 of the pair
#pragma unroll
    for (int kb = 0; kb < NKB; ++kb) {
      float wv[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int c = kb * 32 + lk * 8 + j;
        wv[j] = (cok[nt] && c < Cin && ct_alive_cols(live, Cin, c, o)) ? w[((long long)c * Cout + o) * KT + t] : 0.f;
        if (NP == 2) wv[j] *= wsc;
      }
      split_frag<NP>(wv, bfr[nt][kb]);
    }
  }

  // staging: thread -> channel pair cp = tid / 8 (+ 32 per round), voxel group vq = tid % 8 (4 voxels)
  const int cp = tid >> 3, vq = tid & 7;
  f32x4_t vx[NRD][2];
  float za[NRD][2], zb[NRD][2];
  auto prefetch = [&](long long tile) {
    const int n = (int)((unsigned)tile / (unsigned)tiles_per_n);
    const long long vbase = (tile - (long long)n * tiles_per_n) * TV;
#pragma unroll
    for (int r = 0; r < NRD; ++r)
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        const int c = r * 64 + cp * 2 + e;
        const bool ok = c < Cin;
        vx[r][e] = *reinterpret_cast<gf4_p>((gfloat_p)x + (((long long)n * Cin + (ok ? c : 0)) * spatial + vbase + vq * 4));
        za[r][e] = 1.f; zb[r][e] = 0.f;
        if (scale != nullptr && ok) { za[r][e] = scale[(long long)n * Cin + c]; zb[r][e] = shift[(long long)n * Cin + c]; }
      }
  };
  auto commit = [&]() {
#pragma unroll
    for (int r = 0; r < NRD; ++r) {
      float tz[2][4];
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        const bool ok = r * 64 + cp * 2 + e < Cin;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          float t = vx[r][e][q];
          if (scale != nullptr) t = e2e::in_act(t, za[r][e], zb[r][e], slope);
          tz[e][q] = ok ? (NP == 2 ? t * xsc : t) : 0.f;
        }
      }
      unsigned char* dst = zs + (vq * 4) * RS + (r * 64 + cp * 2) * 2;
#pragma unroll
      for (int q = 0; q < 4; ++q) store_pair<NP>(dst + q * RS, PSZ, tz[0][q], tz[1][q]);
    }
  };

  prefetch(tile_lo);
  for (long long tile = tile_lo; tile < tile_hi; ++tile) {
    commit();
    __syncthreads();
    if (tile + 1 < tile_hi) prefetch(tile + 1);          // in flight during the matrix phase
    f32x4_t acc[2][NTW];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
      for (int nt = 0; nt < NTW; ++nt) acc[mt][nt] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    // A fragment: voxel 16 mt + li, channels 32 kb + 8 lk .. + 7
    const unsigned char* ap = zs + li * RS + lk * 16;
#pragma unroll
    for (int kb = 0; kb < NKB; ++kb)
#pragma unroll
      for (int mt = 0; mt < 2; ++mt) {
        bf16x8_t af[NP];
#pragma unroll
        for (int sp = 0; sp < NP; ++sp) af[sp] = *reinterpret_cast<const bf16x8_t*>(ap + sp * PSZ + mt * 16 * RS + kb * 64);
#pragma unroll
        for (int nt = 0; nt < NTW; ++nt) acc[mt][nt] = mma_pieces<NP>(af, bfr[nt][kb], acc[mt][nt]);
      }
    // (The store side is not DyTile's unit map: a lane owns four consecutive voxels of one result column (o, t), not a voxel pair.)
    // D: row (voxel) = 16 mt + 4 lk + i, column = lane & 15.  Lanes 2p, 2p + 1 hold taps k = 0, 1 of one (o, i, j): after the
    // pair swap lane k = 0 owns output floats [2 v .. 2 v + 3] and lane k = 1 the next four of the interleaved row.
    const int n = (int)((unsigned)tile / (unsigned)tiles_per_n);
    const long long vbase = (tile - (long long)n * tiles_per_n) * TV;
    int dv, hv, w0;
    decode_dhw(vbase, W, H, dv, hv, w0);
    float* yb = y + (long long)n * Cout * ospatial + ((long long)dv * kd * Ho + (long long)hv * kh) * Wo + 2 * w0;
    const bool odd = (lane & 1) != 0;
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
      for (int nt = 0; nt < NTW; ++nt) {
        f32x4_t a = acc[mt][nt];
        if (NP == 2) a = a * unx * unw;
        const float s0 = odd ? a[0] : a[2], s1 = odd ? a[1] : a[3];
        // quad_perm [1, 0, 3, 2]: swap with the neighbouring lane
        const float r0 = __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, s0), 0xb1, 0xf, 0xf, true));
        const float r1 = __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, s1), 0xb1, 0xf, 0xf, true));
        const f32x4_t o4 = odd ? f32x4_t{r0, a[2], r1, a[3]} : f32x4_t{a[0], r0, a[1], r1};
        if (cok[nt]) *reinterpret_cast<f32x4_t*>(yb + coff[nt] + 2 * (mt * 16 + lk * 4)) = o4;
      }
    __syncthreads();
  }
}

// ---- data gradient, split operands (kw == 2, W % 32 == 0): the v3 GEMM on the bf16 / fp16 matrix pipe, fp32-exact operands ----
// v3 is bound by its fp32 MFMAs (128 x 32 cycles per 32-voxel tile and wave: ~0.15 ms of a 0.31 ms launch at 64 -> 32 @64^3,
// the staging and the HBM stream not overlapped with them).  Every fp32 value is split without error into three bf16
// pieces (hi, mid, lo) and a product is rebuilt from the six leading cross terms, as in conv133_wgrad_bf3.hip / conv133_dense.hip
// (error class of an fp32 FMA chain): 96 v_mfma_f32_16x16x32_bf16 x 16 cycles per tile and wave.
//   * K order k = o * KT + t (the memory order of W[c][o][t]): a lane's A fragment (8 consecutive k of row c) is 32
//     contiguous bytes of W; a wave keeps the split fragments of its 16 x K slice in registers (K/32 x 3 x 4 VGPRs);
//   * the dy tile is staged voxel-major, [piece][32 voxels][K bf16 + 16 B] (row stride an odd multiple of 16 B:
//     conflict-free ds_read_b128 B fragments); a float4 of dy (two voxels x taps (2 rr, 2 rr + 1) of one output channel)
//     becomes one packed word per voxel and piece; the loads of the next tile are in flight during the matrix phase.
template <int KDH, int NP>
__global__ __launch_bounds__(256, 2) void convT_dgrad_bf3_kernel(const float* __restrict__ dy, const float* __restrict__ w,
                                                                 const unsigned* __restrict__ live_t, float* __restrict__ dx, int accumulate, int B, int Cin, int Cout,
                                                                 int D, int H, int W, int kd, int kh, int tiles_per_wg,
                                                                 const unsigned* __restrict__ w_word, const unsigned* __restrict__ dy_word_a,
                                                                 const unsigned* __restrict__ dy_word_b) {
  constexpr int KT = 2 * KDH;
  constexpr int OC = 32, TV = 32;
  using Tile = DyTile<KDH, TV>;
  constexpr int K = OC * KT, NKB = K / 32;             // 16x16x32 k-blocks per chunk
  constexpr int S = K * 2 + 16;                        // bytes per staged voxel and piece (528 / 272: odd multiples of 16)
  constexpr int PSZ = TV * S;
  constexpr int NUY = OC * Tile::UPC / 256;            // float4 loads per thread per tile: unit tid + 256 i -> channel / UPC, unit % UPC
  __shared__ __attribute__((aligned(16))) unsigned char ds[NP * PSZ];
  const int kwt = NP == 2 ? ct_scale_exp(w_word, nullptr) : 0, ky = NP == 2 ? ct_scale_exp(dy_word_a, dy_word_b) : 0;
  const float wsc = pow2f(kwt), ysc = pow2f(ky), unw = pow2f(-kwt), uny = pow2f(-ky);

  const long long spatial = (long long)D * H * W;
  const long long tiles_per_n = spatial / TV;          // (launched on row tiles only)
  const long long total_tiles = tiles_per_n * B;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 15, lk = lane >> 4;
  const Tile yt(Cout, D, H, W, kd, kh);
  const int cbase = blockIdx.y * 64 + wave * 16;
  const long long tile_lo = (long long)blockIdx.x * tiles_per_wg;
  long long tile_hi = tile_lo + tiles_per_wg;
  if (tile_hi > total_tiles) tile_hi = total_tiles;
  if (tile_lo >= tile_hi) return;

  f32x4_t v[NUY];
  long long uoff[NUY];
  int ulds[NUY];                                       // where the unit goes in the LDS image
#pragma unroll
  for (int i = 0; i < NUY; ++i) {
    const int u = tid + i * 256;
    const int ol = u / Tile::UPC;
    const typename Tile::Unit un = Tile::unit(u - ol * Tile::UPC);
    uoff[i] = yt.chan_off(ol) + yt.row_off(un);
    ulds[i] = Tile::template voxel_major<S, 2>(ol, un);
  }
  auto prefetch = [&](long long tile, int o0) {
    const int n = (int)((unsigned)tile / (unsigned)tiles_per_n);
    const long long vbase = (tile - (long long)n * tiles_per_n) * TV;
    const long long tbase = yt.row_base(n, o0, 0, vbase);
#pragma unroll
    for (int i = 0; i < NUY; ++i) {
      const int ol = (tid + i * 256) / Tile::UPC;
      v[i] = *reinterpret_cast<gf4_p>((gfloat_p)dy + (yt.chan_ok(o0 + ol) ? tbase + uoff[i] : 0));
    }
  };
  auto commit = [&](int o0) {
#pragma unroll
    for (int i = 0; i < NUY; ++i) {
      const int ol = (tid + i * 256) / Tile::UPC;
      const bool ok = yt.chan_ok(o0 + ol);
      f32x4_t q = ok ? v[i] : f32x4_t{0.f, 0.f, 0.f, 0.f};
      if (NP == 2) q *= ysc;
      unsigned char* d0 = ds + ulds[i];
      store_pair<NP>(d0, PSZ, q[0], q[1]);
      store_pair<NP>(d0 + S, PSZ, q[2], q[3]);
    }
  };

  for (int o0 = 0; o0 < Cout; o0 += OC) {
    // A fragments of this wave: row c = cbase + li, k-block kb, k = 32 kb + 8 lk + j  <->  W[c][o0 + k / KT][k % KT]
    bf16x8_t af[NKB][NP];
    {
      const int c = cbase + li;
#pragma unroll
      for (int kb = 0; kb < NKB; ++kb) {
        const int k0 = kb * 32 + lk * 8;
        float wv[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int o = o0 + (k0 + j) / KT;
          wv[j] = (c < Cin && o < Cout && ct_alive_rows(live_t, Cout, c, o)) ? w[((long long)c * Cout + o0) * KT + k0 + j] : 0.f;
          if (NP == 2) wv[j] *= wsc;
        }
        split_frag<NP>(wv, af[kb]);
      }
    }
    prefetch(tile_lo, o0);
    for (long long tile = tile_lo; tile < tile_hi; ++tile) {
      commit(o0);
      __syncthreads();
      if (tile + 1 < tile_hi) prefetch(tile + 1, o0);    // in flight during the matrix phase
      // accumulate mode / later channel chunks: the old dx values are requested now, not behind the matrix phase (a dependent
      // load -> add -> store per tile there cost 0.08 ms of a 0.26 ms launch at 64 -> 32 @64^3)
      const int n = (int)((unsigned)tile / (unsigned)tiles_per_n);
      const long long vbase = (tile - (long long)n * tiles_per_n) * TV;
      const bool rmw = accumulate || o0 > 0;
      float* dstp[TV / 16][4];
      float old[TV / 16][4];
#pragma unroll
      for (int b = 0; b < TV / 16; ++b)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int c = cbase + lk * 4 + r;
          dstp[b][r] = dx + ((long long)n * Cin + (c < Cin ? c : 0)) * spatial + vbase + b * 16 + li;
          old[b][r] = rmw ? *dstp[b][r] : 0.f;
        }
      f32x4_t acc[TV / 16];
#pragma unroll
      for (int b = 0; b < TV / 16; ++b) acc[b] = f32x4_t{0.f, 0.f, 0.f, 0.f};
      // B fragment: voxel 16 b + li, k = 32 kb + 8 lk .. + 7
      const unsigned char* bp = ds + li * S + lk * 16;
      bf16x8_t bf[2][TV / 16][NP];
#pragma unroll
      for (int b = 0; b < TV / 16; ++b)
#pragma unroll
        for (int sp = 0; sp < NP; ++sp) bf[0][b][sp] = *reinterpret_cast<const bf16x8_t*>(bp + sp * PSZ + b * 16 * S);
#pragma unroll
      for (int kb = 0; kb < NKB; ++kb) {
        if (kb + 1 < NKB) {
#pragma unroll
          for (int b = 0; b < TV / 16; ++b)
#pragma unroll
            for (int sp = 0; sp < NP; ++sp)
              bf[(kb + 1) & 1][b][sp] = *reinterpret_cast<const bf16x8_t*>(bp + sp * PSZ + b * 16 * S + (kb + 1) * 64);
        }
#pragma unroll
        for (int b = 0; b < TV / 16; ++b) acc[b] = mma_pieces<NP>(af[kb], bf[kb & 1][b], acc[b]);
      }
      // D[i = c][j = v]: col = lane & 15 -> v, row = (lane >> 4) * 4 + reg -> c
#pragma unroll
      for (int b = 0; b < TV / 16; ++b)
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (cbase + lk * 4 + r < Cin) *dstp[b][r] = (NP == 2 ? acc[b][r] * unw * uny : acc[b][r]) + old[b][r];
      __syncthreads();
    }
  }
}

}  // namespace

// calls f(std::integral_constant<int, V>{}) for the V among Vs that equals v: the one place a run-time plan value becomes a
// template argument.  The entry points and plans only produce listed values (check_k; nkb, ncb, np below).
template <int... Vs, class F>
static void with_const(int v, F&& f) {
  (void)((v == Vs ? (f(std::integral_constant<int, Vs>{}), true) : false) || ...);
}

static int check_k(int kd, int kh, int kw) {
  return (kd == 1 || kd == 2) && (kh == 1 || kh == 2) && (kw == 1 || kw == 2);
}

// fp16 two-piece operands (round 6) where the caller hands over the range words; E2E_CT_H2=0 keeps the bf16 three-piece form
static int ct_h2_env() { static const int v = getenv("E2E_CT_H2") ? atoi(getenv("E2E_CT_H2")) : 1; return v; }
// E2E_CT_BF3=0 keeps the round-2 kernels (gather forward, fp32-MFMA gradients) instead of the split-operand matrix-pipe ones
static int ct_bf3_env() { static const int v = getenv("E2E_CT_BF3") ? atoi(getenv("E2E_CT_BF3")) : 1; return v; }

// ---- plans: which kernel serves a shape, on what grid ---------------------------------------------------------------------
enum CtPath {
  CT_PLAIN,      // gather forward / data gradient, v1 weight gradient: any kernel in {1,2}^3
  CT_FP32,       // fp32 matrix instructions: data gradient v3, weight gradient v2
  CT_SPLIT       // split operands on the bf16 / fp16 matrix pipe: *_bf3_kernel, np pieces per operand
};

// A GEMM kernel can serve the shape: kw == 2 and an even W make the taps (k = 0, 1) of a voxel pair one aligned float4 of an
// output row (the unit of DyTile, and what the forward stores), KDH = kd * kh such rows per input row are instantiated for
// 2 and 4, and the input is read as float4 (spatial % 4 == 0).
static bool ct_gemm_shape(long long spatial, int W, int kd, int kh, int kw) {
  return kw == 2 && (kd * kh == 2 || kd * kh == 4) && (W % 2) == 0 && spatial % 4 == 0;
}
// pieces per operand: 2 (fp16) where the caller handed over both range words, else 3 (bf16)
static int ct_pieces(bool words) { return (ct_h2_env() && words) ? 2 : 3; }

// forward / data gradient on a run of 32-voxel tiles per workgroup
struct CtTilePlan {
  CtPath path;
  int np;                // CT_SPLIT: pieces per operand
  int nkb;               // forward, CT_SPLIT: 32-channel k-blocks (template argument)
  int vpl;               // forward, CT_PLAIN: voxels per thread (template argument)
  int cgroups;           // launch grid y
  int tiles_per_wg;
  unsigned wgs;          // launch grid x
};
// about `target` workgroups over all channel groups, at least 4 tiles each
static void ct_tile_grid(CtTilePlan& pl, long long total_tiles, int target) {
  long long wgs = target / pl.cgroups;
  if (wgs < 1) wgs = 1;
  pl.tiles_per_wg = (int)e2e::cdivll(total_tiles, wgs);
  if (pl.tiles_per_wg < 4) pl.tiles_per_wg = 4;
  pl.wgs = (unsigned)e2e::cdivll(total_tiles, pl.tiles_per_wg);
}

static CtTilePlan plan_convT_fwd(int B, int Cin, int Cout, int D, int H, int W, int kd, int kh, int kw, bool words) {
  CtTilePlan pl{};
  const long long spatial = (long long)D * H * W;
  const int kt = kd * kh * kw;
  const long long total_tiles = (spatial / 32) * B;
  // the forward GEMM has the row-tile path only (W % 32 == 0) and keeps all of Cin in a wave's registers
  if (!(ct_bf3_env() && ct_gemm_shape(spatial, W, kd, kh, kw) && W % 32 == 0 && Cin <= 256 && total_tiles >= 256)) {
    pl.path = CT_PLAIN;
    pl.vpl = spatial >= 4096 ? (kt <= 4 ? 4 : 2) : 1;
    return pl;
  }
  pl.path = CT_SPLIT;
  pl.np = ct_pieces(words);
  pl.nkb = Cin <= 64 ? 2 : (Cin <= 128 ? 4 : 8);
  const int cols_per_wg = 4 * (8 / pl.nkb) * 16;
  pl.cgroups = e2e::cdiv(Cout * kt, cols_per_wg);
  // two 4-wave workgroups per CU, one round; the fp16 two-piece form with <= 64 input channels needs 164 registers: THREE
  // workgroups per CU, i.e. half again as many requests in flight on a kernel bound by the CU's request path (64 -> 32 @64^3 x 2:
  // 0.189 -> 0.165 ms; 1024 workgroups 0.193; the 128-channel form does not move: profiles/r06_kbench_convt.txt)
  ct_tile_grid(pl, total_tiles, (pl.np == 2 && pl.nkb == 2) ? 768 : 512);
  return pl;
}

static CtTilePlan plan_convT_dgrad(int B, int Cin, int Cout, int D, int H, int W, int kd, int kh, int kw, bool words) {
  CtTilePlan pl{};
  const long long spatial = (long long)D * H * W;
  const long long total_tiles = e2e::cdivll(spatial, 32) * B;
  const int min_tiles = 256;                                // 256 tiles (16^3 x 2) still win over the gather kernel, 64 do not
  if (!(ct_gemm_shape(spatial, W, kd, kh, kw) && total_tiles >= min_tiles)) {
    pl.path = CT_PLAIN;
    return pl;
  }
  // dense GEMM on the matrix cores for the large planes; the split-operand kernel has the row-tile path only, and
  // E2E_CT_BF3=0 keeps the fp32 matrix instructions
  pl.path = (ct_bf3_env() && W % 32 == 0) ? CT_SPLIT : CT_FP32;
  pl.np = ct_pieces(words);
  pl.cgroups = e2e::cdiv(Cin, 64);
  ct_tile_grid(pl, total_tiles, 512);   // two 4-wave workgroups fit a CU (218 VGPRs): exactly one round (768: 0.174 -> 0.203 ms)
  return pl;
}

// What e2e_convT_wgrad_ws_bytes and e2e_convT_wgrad share: the launch writes `slabs` slabs of Cin x Cout x kt floats into a
// workspace that carries no size, so the size query is this plan's slab count and nothing else.
struct CtWgPlan {
  CtPath path;
  int ncb;               // 32-channel input blocks per workgroup
  int cgroups, pairs;    // input-channel groups; launch grid y
  int tiles_per_chunk;
  int slabs;             // launch grid x = slabs the main kernel writes = slabs the reduction reads
};
static CtWgPlan plan_convT_wgrad(int B, int Cin, int Cout, int D, int H, int W, int kd, int kh, int kw) {
  CtWgPlan pl{};
  const long long spatial = (long long)D * H * W;
  const bool mfma = ct_gemm_shape(spatial, W, kd, kh, kw);
  pl.path = !mfma ? CT_PLAIN : (ct_bf3_env() ? CT_SPLIT : CT_FP32);
  pl.ncb = (mfma && Cin > 32) ? 2 : 1;
  pl.cgroups = e2e::cdiv(Cin, 32 * pl.ncb);
  pl.pairs = pl.cgroups * e2e::cdiv(Cout, 32);
  // aim at ~256 workgroups (one 84 KB workgroup per CU, equal work each) and keep the slabs few: every chunk is a slab the
  // reduction has to read (1024 chunks cost 14 % more on the 64 -> 32 @64^3 layer); at least 8 tiles per chunk.  Tiles are
  // WG_TV = 64 voxels on every path: 32-voxel tiles of the bf16x3 weight gradient, two workgroups per CU, were measured
  // SLOWER than one workgroup per CU with 64-voxel tiles on every level but the 8^3 one (0.215 -> 0.27 ms at 64 -> 32 @64^3,
  // profiles/r04_convt_wgrad_tiles.txt).
  pl.slabs = e2e::split_tiles(e2e::cdivll(spatial, WG_TV) * B, pl.pairs, 256, 8, &pl.tiles_per_chunk);
  return pl;
}

// ---- entry points: validate, plan, note, launch ---------------------------------------------------------------------------
extern "C" int e2e_convT_fwd(const float* x, const float* scale, const float* shift, float slope, const float* w,
                             const unsigned* live, float* y, int B, int Cin, int Cout, int D, int H, int W, int kd,
                             int kh, int kw, const unsigned* x_absmax, const unsigned* w_absmax, void* stream) {
  E2E_REQUIRE(x && w && y, "convT_fwd: null pointer");
  E2E_REQUIRE(check_k(kd, kh, kw), "convT_fwd: kernel must be in {1,2}^3");
  E2E_REQUIRE((long long)D * H * W * kd * kh * kw < (1ll << 31), "convT_fwd: a sample must have fewer than 2^31 output voxels");
  E2E_REQUIRE((scale == nullptr) == (shift == nullptr), "convT_fwd: scale/shift must both be given");
  hipStream_t st = (hipStream_t)stream;
  const CtTilePlan pl = plan_convT_fwd(B, Cin, Cout, D, H, W, kd, kh, kw, x_absmax != nullptr && w_absmax != nullptr);
  const int kt = kd * kh * kw, kdh = kd * kh, tpw = pl.tiles_per_wg;
  if (pl.path == CT_SPLIT) {
    const dim3 grid(pl.wgs, pl.cgroups);
    e2e::note_kernel("convT_fwd_%s<%d,%d> wgs=%u cgroups=%d tiles_per_wg=%d", pl.np == 2 ? "h2" : "bf3", kdh, pl.nkb, grid.x, pl.cgroups, tpw);
    with_const<2, 4>(kdh, [&](auto KDH) { with_const<2, 4, 8>(pl.nkb, [&](auto NKB) { with_const<2, 3>(pl.np, [&](auto NP) {
      hipLaunchKernelGGL((convT_fwd_bf3_kernel<KDH(), NKB(), NP()>), grid, dim3(256), 0, st, x, scale, shift, slope, w, live, y,
                         B, Cin, Cout, D, H, W, kd, kh, tpw, x_absmax, w_absmax);
    }); }); });
    return e2e::check_launch("convT_fwd_bf3_kernel");
  }
  const dim3 grid((unsigned)e2e::cdivll((long long)D * H * W, 256 * pl.vpl), Cout, B);
  e2e::note_kernel("convT_fwd_gather<%d,%d>", kt, pl.vpl);
  with_const<1, 2, 4, 8>(kt, [&](auto KT) { with_const<1, 2, 4>(pl.vpl, [&](auto VPL) {
    hipLaunchKernelGGL((convT_fwd_kernel<KT(), VPL()>), grid, dim3(256), 0, st, x, scale, shift, slope, w, live, y,
                       Cin, Cout, D, H, W, kd, kh, kw);
  }); });
  return e2e::check_launch("convT_fwd_kernel");
}

extern "C" int e2e_convT_dgrad(const float* dy, const float* w, const unsigned* live_t, float* dx, int accumulate,
                               int B, int Cin, int Cout, int D, int H, int W, int kd, int kh, int kw, const unsigned* w_absmax,
                               const unsigned* dy_bound_a, const unsigned* dy_bound_b, void* stream) {
  E2E_REQUIRE(dy && w && dx, "convT_dgrad: null pointer");
  E2E_REQUIRE(check_k(kd, kh, kw), "convT_dgrad: kernel must be in {1,2}^3");
  E2E_REQUIRE((long long)D * H * W * kd * kh * kw < (1ll << 31), "convT_dgrad: a sample must have fewer than 2^31 output voxels");
  hipStream_t st = (hipStream_t)stream;
  const CtTilePlan pl = plan_convT_dgrad(B, Cin, Cout, D, H, W, kd, kh, kw, w_absmax != nullptr && dy_bound_a != nullptr);
  const int kdh = kd * kh, tpw = pl.tiles_per_wg;
  const dim3 grid(pl.wgs, pl.cgroups);
  switch (pl.path) {
    case CT_SPLIT:
      e2e::note_kernel("convT_dgrad_%s<%d> wgs=%u cgroups=%d tiles_per_wg=%d", pl.np == 2 ? "h2" : "bf3", kdh, grid.x, pl.cgroups, tpw);
      with_const<2, 4>(kdh, [&](auto KDH) { with_const<2, 3>(pl.np, [&](auto NP) {
        hipLaunchKernelGGL((convT_dgrad_bf3_kernel<KDH(), NP()>), grid, dim3(256), 0, st, dy, w, live_t, dx, accumulate, B, Cin, Cout,
                           D, H, W, kd, kh, tpw, w_absmax, dy_bound_a, dy_bound_b);
      }); });
      return e2e::check_launch("convT_dgrad_bf3_kernel");
    case CT_FP32:
      e2e::note_kernel("convT_dgrad_v3<%d> wgs=%u cgroups=%d tiles_per_wg=%d", kdh, grid.x, pl.cgroups, tpw);
      with_const<2, 4>(kdh, [&](auto KDH) {
        hipLaunchKernelGGL((convT_dgrad_v3_kernel<KDH()>), grid, dim3(256), 0, st, dy, w, live_t, dx, accumulate, B, Cin, Cout, D, H, W, kd, kh, tpw);
      });
      return e2e::check_launch("convT_dgrad_v3_kernel");
    case CT_PLAIN:
      break;
  }
  e2e::note_kernel("convT_dgrad_gather<%d>", kdh * kw);
  with_const<1, 2, 4, 8>(kdh * kw, [&](auto KT) {
    hipLaunchKernelGGL((convT_dgrad_kernel<KT()>), dim3((unsigned)e2e::cdivll((long long)D * H * W, 256), Cin, B), dim3(256), 0, st, dy, w, live_t,
                       dx, accumulate, Cin, Cout, D, H, W, kd, kh, kw);
  });
  return e2e::check_launch("convT_dgrad_kernel");
}

extern "C" long long e2e_convT_wgrad_ws_bytes(int B, int Cin, int Cout, int D, int H, int W, int kd, int kh, int kw) {
  return (long long)plan_convT_wgrad(B, Cin, Cout, D, H, W, kd, kh, kw).slabs * Cin * Cout * kd * kh * kw * (long long)sizeof(float);
}

extern "C" int e2e_convT_wgrad(const float* x, const float* scale, const float* shift, float slope, const float* dy,
                               float* dw, void* ws, int B, int Cin, int Cout, int D, int H, int W, int kd, int kh,
                               int kw, const unsigned* x_absmax, const unsigned* dy_bound_a, const unsigned* dy_bound_b, void* stream) {
  E2E_REQUIRE(x && dy && dw && ws, "convT_wgrad: null pointer");
  E2E_REQUIRE(check_k(kd, kh, kw), "convT_wgrad: kernel must be in {1,2}^3");
  E2E_REQUIRE((long long)D * H * W * kd * kh * kw < (1ll << 31), "convT_wgrad: a sample must have fewer than 2^31 output voxels");
  hipStream_t st = (hipStream_t)stream;
  const CtWgPlan pl = plan_convT_wgrad(B, Cin, Cout, D, H, W, kd, kh, kw);
  const int kt = kd * kh * kw, kdh = kd * kh, tpc = pl.tiles_per_chunk, cgroups = pl.cgroups;
  const int np = ct_pieces(x_absmax != nullptr && dy_bound_a != nullptr);
  float* slab = reinterpret_cast<float*>(ws);
  const dim3 grid(pl.slabs, pl.pairs);
  switch (pl.path) {
    case CT_SPLIT:
      e2e::note_kernel("convT_wgrad_%s<%d,%d> chunks=%d pairs=%d", np == 2 ? "h2" : "bf3", kdh, pl.ncb, pl.slabs, pl.pairs);
      with_const<2, 4>(kdh, [&](auto KDH) { with_const<1, 2>(pl.ncb, [&](auto NCB) { with_const<2, 3>(np, [&](auto NP) {
        hipLaunchKernelGGL((convT_wgrad_bf3_kernel<KDH(), NCB(), NP()>), grid, dim3(256 * NCB()), 0, st, x, scale, shift, slope, dy, slab,
                           B, Cin, Cout, D, H, W, kd, kh, tpc, cgroups, x_absmax, dy_bound_a, dy_bound_b);
      }); }); });
      break;
    case CT_FP32:
      e2e::note_kernel("convT_wgrad_v2<%d,%d> chunks=%d pairs=%d", kdh, pl.ncb, pl.slabs, pl.pairs);
      with_const<2, 4>(kdh, [&](auto KDH) { with_const<1, 2>(pl.ncb, [&](auto NCB) {
        hipLaunchKernelGGL((convT_wgrad_v2_kernel<KDH(), NCB()>), grid, dim3(256 * NCB()), 0, st, x, scale, shift, slope, dy, slab,
                           B, Cin, Cout, D, H, W, kd, kh, tpc, cgroups);
      }); });
      break;
    case CT_PLAIN:
      e2e::note_kernel("convT_wgrad_v1<%d> chunks=%d pairs=%d", kt, pl.slabs, pl.pairs);
      with_const<1, 2, 4, 8>(kt, [&](auto KT) {
        hipLaunchKernelGGL((convT_wgrad_kernel<KT()>), grid, dim3(256), 0, st, x, scale, shift, slope, dy, slab, B,
                           Cin, Cout, D, H, W, kd, kh, kw, tpc, pl.slabs);
      });
      break;
  }
  const int rc = e2e::check_launch("convT_wgrad");
  if (rc != E2E_OK) return rc;
  return e2e::reduce_slabs(slab, dw, (long long)Cin * Cout * kt, pl.slabs, st);
}
