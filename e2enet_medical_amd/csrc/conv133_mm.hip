// K1m (round 5): the 1x3x3 convolution, forward and stride-1 data gradient, as a GEMM on the fp16 matrix pipe with fp32-exact
// two-piece operands -- for EVERY stride-1 layer of the 16 x 32 tile class, DSFF-masked or not (gfx950).
//
// Reference semantics: as conv133.hip (unetpp_d.py:45-59 depth shift, :453-478 concat, :93/:108 Conv3d k(1,3,3) of a weight whose
// DSFF-pruned kernels are zero, core_channel.py:427-434; autograd of the same for the data gradient).
//
// Why (tools/scratch/h2_numerics.hip, profiles/r05_*): an fp32 product rebuilt from fp16 two-piece operands costs THREE matrix
// instructions per 16 k-steps (bf16 three-piece: six), with an error at or below an fp32 FMA chain's.  At that price the dense
// product of a 64 -> 32 layer at 128^3 x 2 is 0.22 ms of matrix-pipe time against 0.78 ms for the sparse vector walk of the same
// layer at density 0.2 (conv133_sparse.hip; the walk is VALU + LDS bound at 0.2 of the HBM roofline): the mask
// stops paying on the vector pipe long before it stops paying in FLOPs.  The mask stays structural: pruned kernels are packed as
// zeros whatever the weight tensor holds.
//
// GEMM per tap: D[out channel][pixel] += W[out channel][16 in] x X[16 in][pixel] -- the WEIGHTS are the A operand, 32 pixels of a
// tile row the B operand (v_mfma_f32_32x32x16_f16): an accumulator register of a lane is one out channel at 32 consecutive pixels
// across the lanes, so the epilogue stores whole 128-byte lines without a transposition and the InstanceNorm sums of an out channel
// are DPP row reductions (row_bcast:15 + v_readlane).  Operands in the fp16 two-piece form of e2e_split.h, scaled before the split:
// the weights by max |w| of the tensor (recorded by the packing launch), the activations by a BOUND of |x| over all input planes of
// the launch (e2e_conv133_input_ranges: |gamma| sqrt(N - 1) + |beta| for a normalised source); product = hi_w lo_x + lo_w hi_x +
// hi_w hi_x in that order, accumulated in fp32, un-scaled on store.  The data gradient runs the same kernel on dy (scaled by max
// |dy|, recorded by e2e_in_lrelu_bwd) with transposed, tap-reversed weights; its destinations (un-shift on store, accumulate or
// overwrite) are resolved per item into LDS records by the staging waves.
//
// Workgroup = 8 waves = 4 matrix waves + 4 staging waves (two per SIMD; the streams of different waves of a SIMD overlap,
// tools/scratch/mfma_overlap.hip), PERSISTENT: one workgroup per CU walks the items (a 512-pixel tile of one depth slice x 32 out
// channels; tile geometries below) l, l + G, l + 2G, ... as ONE pipeline over (item, 16-channel chunk): while the matrix waves
// multiply chunk s out of LDS image s & 1, the staging waves convert chunk s + 1 (registers -> normalise-on-load -> split -> image
// (s + 1) & 1, channel-fastest 32-byte pixel records whose two 16-byte halves are swapped for pixels with bit 3 set: every shifted
// ds_read_b128 fragment is conflict-free), have the loads of chunk s + 2 in flight and fetch the packed weights of chunk s + 1 by
// LDS-DMA (global_load_lds_dwordx4).  One barrier per chunk.  A matrix wave owns a quarter of the tile's rows (4 x 16 accumulator
// registers, 108 matrix instructions per chunk in six half-phases with register double-buffered fragments); its epilogue (bias,
// store, InstanceNorm partial record) runs while the staging waves are already a chunk into the next item.
//
// What bounds it (profiles/r05_mm_stamps.txt, r05_mm_pmc.txt): the CU's memory path -- the staging waves' plane
// requests return at ~10 B/clk/CU (TCP pending-stall 77 % of the cycles), 8.4 k cycles per chunk against 3.5 k of matrix
// instructions; the matrix pipe is busy a third of the time.
//
// Shapes: stride (1,1,1), W % 32 == 0, H % 16 == 0, more than 16 channels on the reduction side, at most CT_MAX.
#include "e2e_common.h"
#include "e2e_split.h"
#include "e2e_concat.h"
#include <cstdlib>
#include <type_traits>

// phase stamps (diagnostic build: make DEFS=-DMM_STAMPS, E2E_MM_STAMPS=1): cycles per workgroup pipeline, staging wave 4 and matrix wave 0
#ifndef MM_DIAG
#define MM_DIAG 0      // timing-only diagnostic builds (results wrong): 1 no matrix instructions, 2 every plane request reads offset 0 of its plane (cache hits), 4 no conversion arithmetic, 8 no forward stores, 16 no forward statistics
#endif
__device__ unsigned long long g_mm_clock[2];     // [0] shader-clock cycles, [1] 100 MHz ticks of workgroup 0, summed over launches (e2e_diag_kernel_clock)
#ifdef MM_STAMPS
__device__ unsigned long long g_mm_stamps[16];   // staging: [0] dma [1] ctab [2] request [3] commit [4] vmcnt wait [5] barrier; matrix: [8] mma [9] lgkm wait [10] barrier [11] epilogue; [15] chunks
#define MMT(v) const unsigned long long v = __builtin_readcyclecounter()
#define MMA(i, a, b) st_acc[i] += (b) - (a)
#else
#define MMT(v)
#define MMA(i, a, b)
#endif

namespace {

using namespace e2e;

// Tile geometries (all 512 output pixels per item, so the items of a depth slice and the InstanceNorm partial records of
// conv133_kernel's 16 x 32 tile class are the same in number):
//   GEOM 0: 16 x 32 tiles of planes whose width is a multiple of 32; halo columns are loaded (aligned float4 groups w0 - 4 .. w0 + 35)
//   GEOM 1:  8 x 64 tiles of planes 64 wide       } FULL-WIDTH tiles: the halo columns are the zero padding of the convolution
//   GEOM 2:  4 x 128 tiles of planes 128 wide     } (written to LDS once), every plane request is whole 128-byte lines.
//   GEOM 3: 16 x 32 tiles of planes 32 wide       } The memory path of a CU moves ~10 B/clk, in LINES: with 16 x 32 tiles of a 128-wide
// plane a chunk touches (16 + 2) rows x 3 lines per channel = 54 lines for 16 lines of payload, with 4 x 128 tiles 6 x 4 = 24, and the
// phase stamps of the first form (profiles/r05_mm_stamps.txt) put the staging waves' request issue -- blocked on that path -- at
// twice the matrix phase.
template <int GEOM> struct Geo {
  static constexpr int TH = GEOM == 1 ? 8 : (GEOM == 2 ? 4 : 16), TW = GEOM == 1 ? 64 : (GEOM == 2 ? 128 : 32);
  static constexpr bool FULLW = GEOM != 0;
  static constexpr int XR = TH + 2, XC = TW + 2, NPIX = XR * XC;
  static constexpr int PSZ = NPIX * 32;            // bytes per piece: 16 channels fp16 per pixel
  static constexpr int IMG = 2 * PSZ;              // one image (hi, lo)
  static constexpr int RPW = TH / 4, CB = TW / 32; // tile rows per matrix wave, 32-pixel column blocks: RPW * CB = 4 accumulators
  static constexpr int NG = FULLW ? TW / 4 : 10;   // 16-byte column groups per staged row
  static constexpr int SROWS = XR / 2;             // halo'd rows per staging-wave pair
  static constexpr int SITEMS = SROWS * NG;        // (row, group) items per staging wave: at most two rounds of 64 lanes
  static constexpr int NF = (RPW + 2) * CB / 2;    // A fragments (row, column block) per half-phase
  static constexpr int CT_MAX = GEOM == 2 ? 256 : 320;      // reduction-side channels with an entry in the LDS channel table
  static constexpr int LREC_MAX = GEOM == 2 ? 384 : (GEOM == 1 ? 768 : 1024);   // forward: batch items x padded input channels held in LDS
  static_assert(RPW * CB == 4 && SITEMS <= 128 && XR % 2 == 0, "geometry");
  // fragment j of half-phase `half`: halo'd row (relative to the wave's first) and column block
  static constexpr int frag_ir(int half, int j) { return GEOM == 2 ? j >> 1 : ((RPW + 2) / 2) * half + j / CB; }
  static constexpr int frag_cb(int half, int j) { return GEOM == 2 ? 2 * half + (j & 1) : j % CB; }
};
constexpr int PXB = 32;                          // bytes per pixel and piece
constexpr int WTAP = 32 * 32;                    // one (tap, piece) block: 32 out channels x 16 ch fp16
constexpr int WCH = 9 * 2 * WTAP;                // one chunk of packed weights: 18 432 B
constexpr int WUNITS = WCH / 16;                 // 1152 16-byte units
constexpr int WSH = 8;                           // weights are packed as w 2^WSH when no max |w| word is given (|w| < 256)
template <int GEOM> constexpr int lds_bytes() {
  return 2 * Geo<GEOM>::IMG + 2 * WCH + 2 * Geo<GEOM>::CT_MAX * 20 + Geo<GEOM>::LREC_MAX * 24 + 2 * 4 * 32 * 2 * 4 + (Geo<GEOM>::CT_MAX + 32) * 4;
}
static_assert(lds_bytes<0>() <= 160 * 1024 && lds_bytes<1>() <= 160 * 1024 && lds_bytes<2>() <= 160 * 1024 && lds_bytes<3>() <= 160 * 1024, "LDS budget");

struct MmParams {
  const e2e_in_chan_t* chans;     // MODE 0: P input planes
  const float* xin;               // MODE 1: dy [B, P, D, H, W]
  const unsigned* x_absmax;       // bit pattern of (a bound of) max |x| over the reduction-side planes: MODE 0 the activations after
                                  // normalise-on-load (nullptr: the fixed 2^XSH), MODE 1 dy (nullptr: unscaled)
  const unsigned* w_absmax;       // bit pattern of max |w| the packing launch recorded (nullptr: packed with the fixed 2^WSH)
  const unsigned char* wpk;       // packed weights [qblock][chunk][tap][piece][32 q][16 ch] fp16, pre-scaled, swizzled
  const float* bias;
  float* y;
  double* part;
  const e2e_out_chan_t* outs;     // MODE 1: Q destination planes
  int P, Q, B, D, H, W;
  int nchunks, qblocks, tiles_x, tiles_y, tiles_per_n, total, grid;
  int pairq;                      // two chunks x two out-channel blocks: a workgroup walks BOTH blocks of a tile back to back and
                                  // stages the tile's planes once (they stay in the two LDS images): `total` counts tiles then
};

struct ChanRec {                   // 24 bytes: one input plane of one batch item, resolved once per launch
  unsigned long long ptr;          // plane of depth 0 of (batch item, channel)
  float a, b, slope;               // normalise-on-load (a = b = 0: channel absent)
  int dshift;
};

struct CtEntry {                   // 16 bytes
  unsigned long long ptr;          // plane of (batch item, shifted depth); always dereferenceable
  float a, b;                      // normalise-on-load (0, 0: channel absent or depth out of range)
};

// ---- weights: fp32 [Q][P][9] (strides wq, wp; reversed taps for the data gradient) -> packed two-piece fp16 -----------------------
// One launch for ALL layers and both directions (round 6; until round 5 one launch in front of every conv launch): job j of the device
// table is one (layer, direction).  `quads` (null = dense layer): DSFF liveness quad words of this direction, word [q / 4][p / 8],
// bit (p % 8) * 4 + q % 4 (e2e_dsff_expand_quads); a pruned (q, p) kernel is packed as zeros (the mask is structural).
// First launch: max |w| per tensor (one workgroup per job that owns its word; plain stores, no atomics, no zeroing launch).
__global__ __launch_bounds__(1024) void weights_absmax_kernel(const e2e_mm_pack_job_t* __restrict__ jobs) {
  const e2e_mm_pack_job_t jb = jobs[blockIdx.x];
  if (jb.w_absmax == nullptr || !jb.owns_absmax) return;
  const long long n = (long long)jb.P * jb.Q * 9;
  float m = 0.f;
  const bool vec = (reinterpret_cast<unsigned long long>(jb.w) & 15ull) == 0;
  const long long n4 = vec ? n >> 2 : 0;
  const float4* w4 = reinterpret_cast<const float4*>(jb.w);
  for (long long i = threadIdx.x; i < n4; i += 1024) {
    const float4 v = w4[i];
    m = fmaxf(m, fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fmaxf(fabsf(v.z), fabsf(v.w))));
    if (!(v.x == v.x && v.y == v.y && v.z == v.z && v.w == v.w)) m = __builtin_inff();      // NaN: fmaxf would drop it
  }
  for (long long i = (n4 << 2) + threadIdx.x; i < n; i += 1024) {
    const float v = jb.w[i];
    m = fmaxf(m, fabsf(v));
    if (!(v == v)) m = __builtin_inff();
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, 64));
  __shared__ float sh[16];
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    float t = sh[0];
    for (int i = 1; i < 16; ++i) t = fmaxf(t, sh[i]);
    *jb.w_absmax = __builtin_bit_cast(unsigned, t);
  }
}

__global__ __launch_bounds__(256) void pack_weights_h2_kernel(const e2e_mm_pack_job_t* __restrict__ jobs) {
  const e2e_mm_pack_job_t jb = jobs[blockIdx.y];
  const int P = jb.P, Q = jb.Q;
  const int nchunks = e2e::cdiv(P, 16), qblocks = e2e::cdiv(Q, 32);
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long n = (long long)qblocks * nchunks * 9 * 32 * 16;
  if (idx >= n) return;
  const int k = (int)(idx % 16), ql = (int)((idx / 16) % 32), tap = (int)((idx / 512) % 9);
  const int ch = (int)((idx / (512 * 9)) % nchunks), qb = (int)(idx / ((long long)512 * 9 * nchunks));
  const int q = qb * 32 + ql, pp = ch * 16 + k;
  float v = 0.f;
  if (q < Q && pp < P) {
    const bool alive = jb.quads == nullptr || ((jb.quads[(long long)(q >> 2) * ((P + 7) >> 3) + (pp >> 3)] >> (((pp & 7) << 2) + (q & 3))) & 1u);
    if (alive) v = jb.w[(long long)q * jb.wq_stride + (long long)pp * jb.wp_stride + (jb.reverse ? 8 - tap : tap)];
  }
  v *= pow2f(jb.w_absmax != nullptr ? scale_exp<LIM_W>(*jb.w_absmax) : WSH);
  _Float16 h, l;
  split_f16_cvt_sub(v, h, l);
  // 32-byte rows; the two 16-byte halves of rows with bit 3 set are swapped (conflict-free ds_read_b128 fragments)
  unsigned short* wpk = reinterpret_cast<unsigned short*>(jb.wpk);
  const long long base = ((((long long)qb * nchunks + ch) * 9 + tap) * 2) * 512 + ql * 16 + (k ^ (((ql >> 3) & 1) << 3));
  wpk[base] = __builtin_bit_cast(unsigned short, h);
  wpk[base + 512] = __builtin_bit_cast(unsigned short, l);
}

template <int MODE, int GEOM>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(2, 2))) void conv133_mm_kernel(MmParams p) {
  using GE = Geo<GEOM>;
  constexpr int TH = GE::TH, TW = GE::TW, XC = GE::XC, PSZ = GE::PSZ, IMG = GE::IMG, RPW = GE::RPW, CB = GE::CB, NF = GE::NF;
  constexpr int NG = GE::NG, SROWS = GE::SROWS, SITEMS = GE::SITEMS, CT_MAX = GE::CT_MAX, LREC_MAX = GE::LREC_MAX;
  constexpr bool FULLW = GE::FULLW;
  __shared__ __attribute__((aligned(16))) unsigned char lds_x[2 * IMG];
  __shared__ __attribute__((aligned(16))) unsigned char lds_w[2 * WCH];
  __shared__ __attribute__((aligned(16))) CtEntry ctab[2][CT_MAX];
  __shared__ float cslope[2][CT_MAX];
  __shared__ __attribute__((aligned(8))) ChanRec lrec[MODE == 0 ? LREC_MAX : CT_MAX]; // forward: the launch's resolved input planes, all batch items;
  static_assert(sizeof(ChanRec) == sizeof(e2e_out_chan_t), "the data gradient keeps its destination table in the same array");
  const e2e_out_chan_t* const lout = reinterpret_cast<const e2e_out_chan_t*>(lrec);   // data gradient: the Q destination descriptors
  __shared__ float red[2][4][32][2];                       // (mean, M2) of 128 values per (item parity, matrix wave, out channel)
  struct ODesc { float* dst; float usc; int flags; };      // data gradient: destination of one out channel for one item (flags: 1 store, 2 accumulate)
  __shared__ __attribute__((aligned(16))) float lbias[MODE == 0 ? CT_MAX + 32 : 4];    // forward: the bias vector (zero padded to whole blocks)
  __shared__ __attribute__((aligned(16))) ODesc odesc[MODE == 1 ? 3 : 1][32];   // by item % 3: the records of item k + 1 are written while the epilogue of item k - 1 may still read its own

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
#ifdef MM_STAMPS
  unsigned long long st_acc[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#endif
  const int G = p.grid;
  const int l0 = e2e::xcd_remap(blockIdx.x, G);
  if (l0 >= p.total) return;
  const unsigned long long clk_c0 = __builtin_readcyclecounter(), clk_r0 = __builtin_amdgcn_s_memrealtime();
  const bool pairq = p.pairq != 0;                           // (wave-uniform)
  const int qrun = pairq ? p.qblocks : 1;                    // out-channel blocks a workgroup walks per tile
  const int nitems = ((p.total - l0 + G - 1) / G) * qrun;
  const int S = nitems * p.nchunks;                          // chunks of this workgroup's pipeline
  const int plane = p.H * p.W;                               // (host: H * W < 2^31 / 4)

  struct Item { int n, d, h0, w0, qb, tile_in_n; };
  auto decode = [&](int k) __attribute__((always_inline)) {
    Item it;
    int id;
    if (pairq) {                                             // items Q j .. Q j + Q - 1 of a workgroup: the Q out-channel blocks of its j-th tile
      const int j = k / qrun;
      id = l0 + j * G;
      it.qb = k - j * qrun;
    } else {
      id = l0 + k * G;
      it.qb = id % p.qblocks;
      id /= p.qblocks;
    }
    it.n = id / p.tiles_per_n;
    it.tile_in_n = id - it.n * p.tiles_per_n;
    const int tx = it.tile_in_n % p.tiles_x, t2 = it.tile_in_n / p.tiles_x;
    const int ty = t2 % p.tiles_y;
    it.d = t2 / p.tiles_y;
    it.h0 = ty * TH;
    it.w0 = tx * TW;
    return it;
  };

  // operand scales: xsc = 2^kx moves the reduction-side planes (forward: the activations after normalise-on-load, bound by
  // *x_absmax; data gradient: dy, max |dy| recorded by e2e_in_lrelu_bwd) into the fp16 range, the weights were packed as w 2^kw;
  // the accumulators are un-scaled by the two exact factors 2^-kw and 2^-kx (two: the sum of the exponents may leave the fp32 range)
  const int kx = p.x_absmax != nullptr ? scale_exp<LIM_X>(__builtin_nontemporal_load(p.x_absmax)) : (MODE == 0 ? XSH : 0);
  const int kw = p.w_absmax != nullptr ? scale_exp<LIM_W>(__builtin_nontemporal_load(p.w_absmax)) : WSH;
  const float xsc = pow2f(kx), unsc_w = pow2f(-kw), unsc = pow2f(-kx);

  // channel table of an item: plane pointer (batch item, shifted depth) and normalise-on-load coefficients per reduction-side
  // channel, from the records the packing launch resolved (one independent 24-byte load per channel); built by `nthreads`
  // threads starting at `t0`; NR entries per thread cover up to NR * nthreads channels
  // forward: the resolved input planes of the whole launch (plane pointer of depth 0, normalise-on-load coefficients, depth shift
  // per batch item and channel; written by the packing launch) are copied to LDS once per workgroup; the channel table of an item
  // (plane pointer at the shifted depth, coefficients zeroed where that depth is outside) is then LDS-to-LDS work: no global load
  // and no wait inside the staging loop
  if (MODE == 0) {
    // plane pointers and normalise-on-load coefficients of every (batch item, input channel): resolved once per workgroup
    // (descriptor -> scale / shift: a dependent chain, paid once per persistent workgroup instead of once per item; until round 5 a
    // separate launch in front of every conv wrote these records)
    const int np16 = p.nchunks * 16, nrec = p.B * np16;
    for (int i = tid; i < nrec; i += 512) {
      const int ch = i % np16, nb = i / np16;
      const bool have = ch < p.P;                              // (absent: channel 0's planes, read and multiplied by 0)
      const ConcatChan cc = concat_chan(p.chans[have ? ch : 0], nb);
      ChanRec r;
      r.ptr = (unsigned long long)cc.base;
      r.a = have ? cc.a : 0.f; r.b = have ? cc.b : 0.f; r.slope = have ? cc.slope : 1.f;
      r.dshift = have ? cc.dshift : 0;
      lrec[i] = r;
    }
    for (int i = tid; i < p.qblocks * 32; i += 512) lbias[i] = (p.bias != nullptr && i < p.Q) ? p.bias[i] : 0.f;
  } else {
    for (int i = tid; i < p.Q; i += 512) reinterpret_cast<e2e_out_chan_t*>(lrec)[i] = p.outs[i];
  }
  if (FULLW)                                                  // full-width tiles: the halo columns are zero padding, never written again
    for (int i = tid; i < 2 * IMG / 16; i += 512) reinterpret_cast<u32x4_t*>(lds_x)[i] = u32x4_t{0u, 0u, 0u, 0u};
  __syncthreads();
  auto build_ctab = [&](const Item& it, int par, int t0, int nthreads) __attribute__((always_inline)) {
    CtEntry* tab = ctab[par];
    float* sl = cslope[par];
    const int np16 = p.nchunks * 16;
    for (int ch = t0; ch < np16; ch += nthreads) {
      CtEntry e;
      float sv = 1.f;
      if (MODE == 0) {
        const ChanRec r = lrec[it.n * np16 + ch];
        const ConcatDepth sl = concat_depth(it.d, 1, r.dshift, p.D);
        e.a = sl.valid ? r.a * xsc : 0.f;                      // (LeakyReLU commutes with the positive pre-scale)
        e.b = sl.valid ? r.b * xsc : 0.f;
        sv = r.slope;
        e.ptr = r.ptr + (unsigned long long)(sl.valid ? sl.din : 0) * (unsigned long long)plane * 4ull;
      } else {
        const bool valid = ch < p.P;
        e.a = valid ? xsc : 0.f;
        e.b = 0.f;
        e.ptr = (unsigned long long)(p.xin + (((long long)it.n * p.P + (valid ? ch : 0)) * p.D + it.d) * plane);
      }
      tab[ch] = e;
      sl[ch] = sv;
    }
  };

  // data gradient: where the 32 out channels of an item go (concat_store_slice), resolved once per item into LDS by the staging
  // waves (LDS-to-LDS, like the channel table)
  auto build_odesc = [&](const Item& it, int slot, int t) __attribute__((always_inline)) {
    if (MODE != 1 || t < 0 || t >= 32) return;
    const int q = it.qb * 32 + t;
    ODesc od;
    od.dst = nullptr; od.usc = 0.f; od.flags = 0;
    if (q < p.Q) {
      const e2e_out_chan_t oc = lout[q];
      if (oc.ptr != nullptr) {
        const ConcatSlice sl = concat_store_slice(it.d, oc.dshift, p.D, oc.accumulate);
        if (sl.action != CONCAT_SKIP) {
          od.dst = oc.ptr + (long long)it.n * oc.nstride + (long long)sl.dd * plane + (long long)it.h0 * p.W + it.w0;
          od.usc = sl.action == CONCAT_ZERO_FILL ? 0.f : unsc;
          od.flags = 1 | (sl.action == CONCAT_ADD ? 2 : 0);
        }
      }
    }
    odesc[MODE == 1 ? slot : 0][t] = od;
  };

  build_ctab(decode(0), 0, tid, 512);
  build_odesc(decode(0), 0, tid);
  __syncthreads();                                            // barrier #0

  if (wave >= 4) {
    // ================================================= staging waves =========================================================
    // Iteration s runs beside the matrix phase of chunk s: the packed weights of chunk s + 1 are requested (LDS-DMA), the planes
    // of chunk s + 2 are requested into the register set chunk s left, chunk s + 1 is converted out of the other set into image
    // (s + 1) & 1.  Straight-line code (no branch around a load: exact vmcnt distances); past the end the last chunk is requested
    // and staged again into the image nobody reads.
    const int sw = wave - 4;
    const int shalf = sw & 1, srh = sw >> 1;                  // channel half of the chunk, row half of the halo'd tile
    int s_row[2], s_g[2], s_pix0[2], s_loff[2];
    bool s_act[2];
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      const int it = r * 64 + lane;
      s_act[r] = it < SITEMS;
      const int itc = s_act[r] ? it : 0;
      s_row[r] = srh * SROWS + itc / NG;
      s_g[r] = itc % NG;
      // halo'd pixel index of the group's first column, element offset from the tile origin (h0, w0): general tiles load the aligned
      // groups w0 - 4 .. w0 + 35 (three columns beyond either halo column are dropped), full-width tiles exactly the plane's rows
      s_pix0[r] = s_row[r] * XC + (FULLW ? 4 * s_g[r] + 1 : 4 * s_g[r] - 3);
      s_loff[r] = (s_row[r] - 1) * p.W + (FULLW ? 4 * s_g[r] : 4 * s_g[r] - 4);
    }
    struct Cur { int k, c; Item it; };                        // a position in the (item, chunk) sequence; past the end: the last item again
    auto advance = [&](Cur& q) __attribute__((always_inline)) {
      if (++q.c == p.nchunks) {                               // (wave-uniform; scalar work only)
        asm volatile("" ::: "memory");                        // a real branch: the divisions of decode() are not to be speculated into every iteration
        q.c = 0;
        ++q.k;
        q.it = decode(q.k < nitems ? q.k : nitems - 1);
      }
    };
    f32x4_t xv[2][2][8];                                      // [register set][round][channel]
    bool inside[2][2];

    // plane loads of chunk q -> register set SET: addresses first (channel table entries from LDS), then `issue(i)` requests load
    // i = 8 round + channel.  The sixteen requests of a chunk are dealt between the conversion steps of the previous chunk
    // (stage below): all four staging waves of a CU run in step behind the barrier, and sixteen back-to-back requests per wave
    // saturate the CU's memory path for ~6 k cycles (10 B/clk/CU) and leave it idle while everybody converts (phase stamps,
    // profiles/r05_mm_stamps.txt): spread out, the path is busy all the time.
    struct Req { unsigned long long base[8]; unsigned off[2]; };
    auto prepare = [&](auto SETC, const Cur& q) __attribute__((always_inline)) {
      constexpr int SET = decltype(SETC)::value;
      Req rq;
      const int par = (q.k < nitems ? q.k : nitems - 1) & 1;
      const CtEntry* tab = ctab[par] + q.c * 16 + shalf * 8;
#pragma unroll
      for (int j = 0; j < 8; ++j) rq.base[j] = tab[j].ptr;
      const int torg = q.it.h0 * p.W + q.it.w0;
#pragma unroll
      for (int r = 0; r < 2; ++r) {
        const int hi = q.it.h0 - 1 + s_row[r], wi = FULLW ? 0 : q.it.w0 - 4 + 4 * s_g[r];
        inside[SET][r] = s_act[r] & ((unsigned)hi < (unsigned)p.H) & ((unsigned)wi < (unsigned)p.W);
        rq.off[r] = (inside[SET][r] && !(MM_DIAG & 2)) ? (unsigned)(torg + s_loff[r]) : 0u;
      }
      return rq;
    };
    auto issue = [&](auto SETC, const Req& rq, int i) __attribute__((always_inline)) {     // i: compile-time after unrolling
      constexpr int SET = decltype(SETC)::value;
      xv[SET][i >> 3][i & 7] = *(gf4_p)(rq.base[i & 7] + (unsigned long long)rq.off[i >> 3] * 4ull);
    };
    auto request_w = [&](const Cur& q, int buf) __attribute__((always_inline)) {      // packed weights of chunk q -> lds_w[buf] by LDS-DMA
      const unsigned char* src = p.wpk + ((long long)q.it.qb * p.nchunks + q.c) * WCH;
      unsigned char* dst = lds_w + buf * WCH;
#pragma unroll
      for (int rd = 0; rd < (WUNITS + 255) / 256; ++rd) {
        const int u0 = rd * 256 + sw * 64;                    // (wave-uniform)
        if (u0 < WUNITS) {
          // (inline asm: the compiler waits vmcnt(0) in front of every LDS-DMA builtin and again at the first LDS access that might
          //  alias it -- that would drain the plane loads in flight; M0 = wave-uniform LDS byte address, written in the same statement)
          unsigned keep;
          const unsigned lds_dst = (unsigned)(unsigned long long)(__attribute__((address_space(3))) unsigned char*)(dst + u0 * 16);
          const unsigned char* gsrc = src + (long long)(u0 + lane) * 16;
          asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                       : "=&s"(keep) : "v"(gsrc), "s"(__builtin_amdgcn_readfirstlane(lds_dst)) : "memory");
        }
      }
    };
    // register set CUR (chunk qc) -> image buf, with the sixteen plane requests of chunk qn into set NEW dealt two per pixel step
    // pairq: the second out-channel block of a tile finds the tile's two chunks in the two images (nchunks == 2: image = chunk):
    // nothing is requested and nothing converted for it.  The (convert, request) combination of the common case stays ONE
    // straight-line block (the conversion steps hide the requests dealt between them; a branch around a load inside it would
    // make the compiler drain vmcnt); the three other combinations are blocks of their own.
    auto request_only = [&](auto NEWC, const Cur& qn) __attribute__((always_inline)) {
      const Req rq = prepare(NEWC, qn);
#pragma unroll
      for (int i = 0; i < 16; ++i) issue(NEWC, rq, i);
    };
    auto stage = [&](auto CURC, auto NEWC, const Cur& qc, const Cur& qn, int buf, auto REQC) __attribute__((always_inline)) {
      constexpr int CUR = decltype(CURC)::value;
      constexpr bool REQ = decltype(REQC)::value;            // false: convert only (no request dealt between the steps)
      MMT(u0);
      Req rq{};
      if constexpr (REQ) rq = prepare(NEWC, qn);
      unsigned char* img = lds_x + buf * IMG;
      const int parc = (qc.k < nitems ? qc.k : nitems - 1) & 1;
      const CtEntry* tab = ctab[parc] + qc.c * 16 + shalf * 8;
      const float* sl = cslope[parc] + qc.c * 16 + shalf * 8;
      float ca[8], cb[8], csl[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) { const CtEntry e = tab[j]; ca[j] = e.a; cb[j] = e.b; csl[j] = sl[j]; }
      MMT(u1);
      MMA(6, u0, u1);
#pragma unroll
      for (int r = 0; r < 2; ++r) {
        MMT(u2);
        float ae[8], be[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) { ae[j] = inside[CUR][r] ? ca[j] : 0.f; be[j] = inside[CUR][r] ? cb[j] : 0.f; }
#pragma unroll
        for (int kx = 0; kx < 4; ++kx) {
          if constexpr (REQ) {
            issue(NEWC, rq, (r * 4 + kx) * 2);
            issue(NEWC, rq, (r * 4 + kx) * 2 + 1);
          }
          const int hc = FULLW ? 1 : 4 * s_g[r] - 3 + kx;     // halo column of this pixel (general tiles: may fall outside the halo'd row)
          float t[8];
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            if (MM_DIAG & 4) {
              t[j] = xv[CUR][r][j][kx];
            } else if (MODE == 0) {
              const float u = fmaf(xv[CUR][r][j][kx], ae[j], be[j]);
              t[j] = fmaxf(u, u * csl[j]);                    // LeakyReLU, 0 <= slope <= 1 (the engine's contract); slope 1 = identity
            } else {
              t[j] = xv[CUR][r][j][kx] * ae[j];
            }
          }
          u32x4_t hv, lv;
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            if (MM_DIAG & 4) { hv[j] = __builtin_bit_cast(unsigned, t[2 * j]); lv[j] = __builtin_bit_cast(unsigned, t[2 * j + 1]); continue; }
            unsigned hw, lw;
            split_f16x2_fma_mix(t[2 * j], t[2 * j + 1], hw, lw);       // 3 instructions per pair
            hv[j] = hw;
            lv[j] = lw;
          }
          if (s_act[r] && hc >= 0 && hc < XC) {
            const int px = s_pix0[r] + kx;
            unsigned char* dst = img + px * PXB + ((shalf ^ ((px >> 3) & 1)) << 4);
            *reinterpret_cast<u32x4_t*>(dst) = hv;
            *reinterpret_cast<u32x4_t*>(dst + PSZ) = lv;
          }
          __builtin_amdgcn_sched_barrier(0);                  // the next two requests stay behind this step
        }
        MMT(u3);
        MMA(7, u2, u3);
        if (r == 0) MMA(2, u2, u3);
      }
    };

    using R0 = std::integral_constant<int, 0>; using R1 = std::integral_constant<int, 1>;
    const bool w_resident = p.nchunks == 2 && p.qblocks == 1;         // (wave-uniform)
    // prologue: chunk 0 requested and staged, chunk 1 in flight
    Cur q1{0, 0, decode(0)};                                  // the chunk being converted (s + 1 inside the loop)
    Cur q2 = q1;                                              // the chunk being requested (s + 2)
    request_w(q1, 0);
    {
      const Req rq = prepare(R0{}, q1);
#pragma unroll
      for (int i = 0; i < 16; ++i) issue(R0{}, rq, i);
    }
    advance(q2);                                              // chunk 1 (item 0: nchunks >= 2)
    if (nitems > 1) { build_ctab(decode(1), 1, tid - 256, 256); build_odesc(decode(1), 1, tid - 256); }
    stage(R0{}, R1{}, q1, q2, 0, std::true_type{});           // chunk 0 -> image 0, chunk 1 -> set 1
    asm volatile("s_waitcnt vmcnt(16)" ::: "memory");
    __syncthreads();                                          // barrier #1: image 0 and weights 0 are in LDS
    auto iteration = [&](auto PARC, int s) __attribute__((always_inline)) {            // PAR = s & 1
      constexpr int PAR = decltype(PARC)::value;
      q1 = q2;                                                // chunk s + 1 (requested last iteration into set PAR ^ 1)
      advance(q2);                                            // chunk s + 2 -> set PAR
      MMT(t0);
      // layers of two chunks and one out-channel block (32 -> 32 at full resolution, both directions): the two weight buffers hold
      // the layer's whole packed tensor from the second chunk on -- no weight request at all after that (18 KB of the ~67 KB a
      // chunk moves through the CU's memory path: the path is what bounds this kernel)
      if (!(w_resident && s >= 1)) request_w(q1, PAR ^ 1);
      MMT(t1);
      // table of the item after q1's, written while q1's first chunk is converted: a barrier before its first reader (nchunks >= 2);
      // LDS-to-LDS (no global load: a branch around a load would cost the exact vmcnt distances of this loop)
      if (q1.c == 0 && q1.k + 1 < nitems) {
        const Item itn = decode(q1.k + 1);
        build_ctab(itn, (q1.k + 1) & 1, tid - 256, 256);
        build_odesc(itn, (q1.k + 1) % 3, tid - 256);
      }
      MMT(t2);
      // (past the end the position is clamped to the last item -- in pairq mode a second block: nothing to do, as it should be)
      const bool conv = !(pairq && ((q1.k < nitems ? q1.k : nitems - 1) % qrun));
      const bool req = !(pairq && ((q2.k < nitems ? q2.k : nitems - 1) % qrun));
      using CURC = std::integral_constant<int, PAR ^ 1>; using NEWC = std::integral_constant<int, PAR>;
      if (conv && req) stage(CURC{}, NEWC{}, q1, q2, PAR ^ 1, std::true_type{});
      else if (conv) stage(CURC{}, NEWC{}, q1, q2, PAR ^ 1, std::false_type{});
      else if (req) request_only(NEWC{}, q2);
      MMT(t4);
      if (req) asm volatile("s_waitcnt vmcnt(16)" ::: "memory");      // the weight DMA has landed; the 16 plane loads stay in flight
      else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");           // (no plane loads behind the DMA: wait for everything)
      MMT(t5);
      __syncthreads();                                        // barrier #(s + 2)
      MMT(t6);
      MMA(0, t0, t1); MMA(1, t1, t2); MMA(3, t2, t4); MMA(4, t4, t5); MMA(5, t5, t6);
    };
    for (int s = 0; s < S; s += 2) {
      iteration(R0{}, s);
      if (s + 1 < S) iteration(R1{}, s + 1);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();                                          // the last item's statistics records
#ifdef MM_STAMPS
    if (sw == 0 && lane == 0) { for (int i = 0; i < 8; ++i) atomicAdd(&g_mm_stamps[i], st_acc[i]); atomicAdd(&g_mm_stamps[15], (unsigned long long)S); }
#endif
    return;
  }

  // =================================================== matrix waves ===========================================================
  const int wr = wave;                                        // tile rows RPW wr .. RPW wr + RPW - 1, all CB column blocks
  const int fq = lane & 31, fh8 = lane >> 5;
  const int wfo = fq * 32 + ((fh8 ^ ((fq >> 3) & 1)) << 4);   // weight fragment: out channel fq, channels 8 fh8 .. + 7
  // A fragment of halo'd row RPW wr + ir, column block cb, tap column kw: pixel (RPW wr + ir) XC + 32 cb + fq + kw; the column block
  // is an immediate offset (32 pixels leave bit 3 of the pixel index, the half swap, unchanged)
  int aoff[RPW + 2][3];
#pragma unroll
  for (int ir = 0; ir < RPW + 2; ++ir)
#pragma unroll
    for (int kw = 0; kw < 3; ++kw) {
      const int px = (RPW * wr + ir) * XC + kw + fq;
      aoff[ir][kw] = px * PXB + ((fh8 ^ ((px >> 3) & 1)) << 4);
    }
  f32x16_t acc[4];
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[r][i] = 0.f;

  auto combine = [&](int k) __attribute__((always_inline)) {                                  // tile record of item k from the four waves' (mean, M2) of 128 values
    if (MODE != 0 || p.part == nullptr || wr != 0 || lane >= 32) return;
    const Item it = decode(k);
    const int q = it.qb * 32 + lane;
    if (q >= p.Q) return;
    // Chan combination of four records of 128 values, fp64; the counts are known: bn / tot and cn bn / tot are constants
    double cm = (double)red[k & 1][0][lane][0], c2 = (double)red[k & 1][0][lane][1];
    constexpr double wgt[4] = {0.0, 0.5, 1.0 / 3.0, 0.25}, cross[4] = {0.0, 64.0, 256.0 / 3.0, 96.0};
#pragma unroll
    for (int w = 1; w < 4; ++w) {
      const double bm = (double)red[k & 1][w][lane][0], b2 = (double)red[k & 1][w][lane][1];
      const double dl = bm - cm;
      cm += dl * wgt[w];
      c2 += b2 + dl * dl * cross[w];
    }
    double* pp = p.part + (((long long)it.n * p.Q + q) * p.tiles_per_n + it.tile_in_n) * 3;
    pp[0] = 512.0; pp[1] = cm; pp[2] = c2;
  };

  // A chunk is six HALF-PHASES of 18 matrix instructions: kernel column kw = hp / 2 and one half of the wave's (halo'd row, column
  // block) fragments (Geo::frag_ir / frag_cb).
  // A fragments (hi and lo piece) are double-buffered in registers by half-phase, B fragments (the three taps of a
  // kernel column, hi and lo) by kernel column: the ds_read_b128 of the next half-phase are issued in front of the matrix
  // instructions of the current one.  The workgroup barrier of a chunk sits in front of its LAST half-phase: by then every read of
  // the chunk's image has been issued and has landed, the staging waves have finished the next image, and the first fragments of
  // the next chunk are requested right behind it.
  f16x8_t fa[2][NF][2], fb[2][3][2];
  auto load_a = [&](auto HPC, int s) __attribute__((always_inline)) {                        // A fragments of half-phase HP of chunk s -> set HP & 1
    constexpr int HP = decltype(HPC)::value, SET = HP & 1, KW = HP >> 1, HALF = HP & 1;
    const unsigned char* img = lds_x + (s & 1) * IMG;
#pragma unroll
    for (int j = 0; j < NF; ++j) {
      const unsigned char* ap = img + aoff[GE::frag_ir(HALF, j)][KW] + GE::frag_cb(HALF, j) * 32 * PXB;
      fa[SET][j][0] = *reinterpret_cast<const f16x8_t*>(ap);
      fa[SET][j][1] = *reinterpret_cast<const f16x8_t*>(ap + PSZ);
    }
  };
  auto load_b = [&](auto SETC, auto KWC, int s) __attribute__((always_inline)) {             // B fragments of kernel column KW of chunk s -> set SET
    constexpr int SET = decltype(SETC)::value, KW = decltype(KWC)::value;
    const unsigned char* wl = lds_w + (s & 1) * WCH + wfo;
#pragma unroll
    for (int kh = 0; kh < 3; ++kh) {
      fb[SET][kh][0] = *reinterpret_cast<const f16x8_t*>(wl + ((kh * 3 + KW) * 2) * WTAP);
      fb[SET][kh][1] = *reinterpret_cast<const f16x8_t*>(wl + ((kh * 3 + KW) * 2 + 1) * WTAP);
    }
  };
  auto mma = [&](auto HPC, auto BSETC) __attribute__((always_inline)) {
    constexpr int HP = decltype(HPC)::value, SET = HP & 1, HALF = HP & 1, BS = decltype(BSETC)::value;
#pragma unroll
    for (int j = 0; j < NF; ++j)
#pragma unroll
      for (int kh = 0; kh < 3; ++kh) {
        const int rr = GE::frag_ir(HALF, j) - kh;             // tile row (of this wave) the fragment feeds through kernel row kh
        if (rr < 0 || rr >= RPW) continue;
        const int ai = rr * CB + GE::frag_cb(HALF, j);
        if (MM_DIAG & 1) { acc[ai][0] += (float)fa[SET][j][0][0] + (float)fb[BS][kh][1][0] + (float)fa[SET][j][1][0] + (float)fb[BS][kh][0][0]; continue; }
        f32x16_t a = acc[ai];                                 // small terms first: lo*hi, hi*lo, then hi*hi
        // D[out channel][pixel]: the weight fragment is the A operand (row = out channel fq), the pixel fragment the B operand
        // (column = pixel fq): a lane then owns ONE pixel column and 16 out channels, so a store of one accumulator register is two
        // whole 128-byte lines (lanes 0-31 / 32-63: channels 4 apart) -- with D[pixel][channel] it was 32 partial lines
        a = __builtin_amdgcn_mfma_f32_32x32x16_f16(fb[BS][kh][0], fa[SET][j][1], a, 0, 0, 0);
        a = __builtin_amdgcn_mfma_f32_32x32x16_f16(fb[BS][kh][1], fa[SET][j][0], a, 0, 0, 0);
        a = __builtin_amdgcn_mfma_f32_32x32x16_f16(fb[BS][kh][0], fa[SET][j][0], a, 0, 0, 0);
        acc[ai] = a;
      }
  };
  int pending = -1;                                           // item whose statistics records wait for the next barrier
  Item itm = decode(0);                                       // the item of the chunk being multiplied
  int mk = 0, mc = 0;
  // sum over the 32 lanes of a half wave (the pixels of a tile row): four DPP steps inside the 16-lane rows, then row_bcast:15 adds
  // the sum of rows 0 / 2 to rows 1 / 3 -- the total is valid in lanes 16-31 and 48-63; no LDS crossbar round trip (32 dependent
  // ds_bpermute per item were the bulk of the first version of this epilogue)
  auto half_sum_hi = [&](float v) __attribute__((always_inline)) {
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xB1, 0xF, 0xF, true));
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x4E, 0xF, 0xF, true));
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x141, 0xF, 0xF, true));
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x140, 0xF, 0xF, true));
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x142, 0xA, 0xF, false));
    return v;
  };
  // 4 x 4 transpose across the lanes of a quad: before, register r of lane l holds (channel c0 + r, pixel 4 q + l); after, register r
  // holds (channel c0 + l, pixel 4 q + r) -- four consecutive pixels of one channel per lane, i.e. ONE 16-byte store per lane and
  // block instead of four 4-byte ones, and ONE destination record per lane and block instead of four (data gradient).  Measured
  // on one box against 4-byte stores (profiles/r05_store_ab.txt): data gradient -3 ... -4 %, forward +2 ... +3 % (kept there as it
  // was): the width of the stores is not what the ~9 k cycles per item of the epilogue wait for.
  const bool q_hi2 = (lane & 2) != 0, q_hi1 = (lane & 1) != 0;
  auto quad_transpose = [&](float r0, float r1, float r2, float r3) __attribute__((always_inline)) {
    auto x2 = [](float v) __attribute__((always_inline)) { return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x4E, 0xf, 0xf, false)); };   // quad_perm [2,3,0,1]
    auto x1 = [](float v) __attribute__((always_inline)) { return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xB1, 0xf, 0xf, false)); };   // quad_perm [1,0,3,2]
    const float t0 = x2(r0), t1 = x2(r1), t2 = x2(r2), t3 = x2(r3);
    const float a0 = q_hi2 ? t2 : r0, a1 = q_hi2 ? t3 : r1, a2 = q_hi2 ? r2 : t0, a3 = q_hi2 ? r3 : t1;
    const float u0 = x1(a0), u1 = x1(a1), u2 = x1(a2), u3 = x1(a3);
    return f32x4_t{q_hi1 ? u1 : a0, q_hi1 ? a1 : u0, q_hi1 ? u3 : a2, q_hi1 ? a3 : u2};
  };
  auto epilogue = [&](int k) __attribute__((always_inline)) {
    // ---- epilogue of item k.  D layout of v_mfma_f32_32x32x16 with the weights as the A operand: column (pixel of the tile row) =
    // lane & 31, row (out channel of the block) = (i & 3) + 8 (i >> 2) + 4 (lane >> 5): register i of accumulator a is one pixel of
    // channel ch(i) in tile row a / CB, column block a % CB -- a store of it is two whole lines
    const Item it = itm;
    const long long cs = (long long)p.D * plane;              // channel stride of y
    if (MODE == 0) {
      float bi[16];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const f32x4_t b4 = *reinterpret_cast<const f32x4_t*>(lbias + it.qb * 32 + 8 * j + 4 * fh8);
        bi[4 * j] = b4[0]; bi[4 * j + 1] = b4[1]; bi[4 * j + 2] = b4[2]; bi[4 * j + 3] = b4[3];
      }
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[a][i] = fmaf(acc[a][i] * unsc_w, unsc, bi[i]);
      if (p.part != nullptr && !(MM_DIAG & 16)) {
        // (count 128, mean, M2) of this wave's 4 x 32 pixels per out channel: per-lane sums over the four accumulators, then over
        // the 32 lanes of the half; two passes (mean first) like every other kernel of the family
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const float tot = half_sum_hi((acc[0][i] + acc[1][i]) + (acc[2][i] + acc[3][i]));
          const float t0 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, tot), 31));
          const float t1 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, tot), 63));
          const float mean = (fh8 ? t1 : t0) * (1.f / 128.f);
          float m2 = 0.f;
#pragma unroll
          for (int a = 0; a < 4; ++a) {
            const float dl = acc[a][i] - mean;
            m2 = fmaf(dl, dl, m2);
          }
          m2 = half_sum_hi(m2);
          if (fq == 31) {
            const int ch = (i & 3) + 8 * (i >> 2) + 4 * fh8;
            red[k & 1][wr][ch][0] = mean; red[k & 1][wr][ch][1] = m2;
          }
        }
        pending = k;
      }
      if (!(MM_DIAG & 8)) {
        // (4-byte stores, two whole lines per instruction; the quad-transposed 16-byte form of the data gradient below was measured
        //  2-3 % SLOWER here on one box, profiles/r05_store_ab.txt: the transposition costs more than the narrower stores)
        float* yb = p.y + ((long long)it.n * p.Q + it.qb * 32 + 4 * fh8) * cs + (long long)it.d * plane + (long long)(it.h0 + RPW * wr) * p.W + it.w0 + fq;
        const int qlim = p.Q - it.qb * 32 - 4 * fh8;          // channels of this lane's half that exist
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const int chl = (i & 3) + 8 * (i >> 2);
          if (chl < qlim) {
#pragma unroll
            for (int a = 0; a < 4; ++a) yb[chl * cs + (a / CB) * p.W + (a % CB) * 32] = acc[a][i];
          }
        }
      }
    } else {
      // data gradient: destinations from the item's records (odesc).  After the quad transpose a lane owns ONE out channel per
      // block j -- 8 j + 4 fh8 + (lane & 3) -- and four consecutive pixels of it: one 16-byte store, or four no-return
      // global_atomic_add_f32 where the destination accumulates (one lane of one workgroup per element and launch, launches
      // stream-ordered: RN(old + acc * usc), the same number as a load / add / store, deterministic; the adder sits in L2)
      const int rowoff = RPW * wr * p.W + (fq & ~3);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const ODesc od = odesc[k % 3][8 * j + 4 * fh8 + (lane & 3)];
#pragma unroll
        for (int a = 0; a < 4; ++a) {
          const f32x4_t v = quad_transpose(acc[a][4 * j], acc[a][4 * j + 1], acc[a][4 * j + 2], acc[a][4 * j + 3]) * unsc_w * od.usc;
          if (od.flags & 1) {
            float* q = od.dst + rowoff + (a / CB) * p.W + (a % CB) * 32;
            if (od.flags & 2) {
#pragma unroll
              for (int e = 0; e < 4; ++e) asm volatile("global_atomic_add_f32 %0, %1, off" :: "v"(q + e), "v"(v[e]) : "memory");
            } else {
              *(__attribute__((address_space(1))) f32x4_t*)(q) = v;      // (a global store: the pointer came out of LDS as a generic one)
            }
          }
        }
      }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[r][i] = 0.f;
  };
  __syncthreads();                                            // barrier #1
  using I0 = std::integral_constant<int, 0>; using I1 = std::integral_constant<int, 1>; using I2 = std::integral_constant<int, 2>;
  using I3 = std::integral_constant<int, 3>; using I4 = std::integral_constant<int, 4>; using I5 = std::integral_constant<int, 5>;
  load_a(I0{}, 0);
  load_b(I0{}, I0{}, 0);
  auto chunk = [&](auto PARC, int s) __attribute__((always_inline)) {                        // PAR: the B register set that holds kernel column 0 of chunk s
    constexpr int PAR = decltype(PARC)::value;
    using B0 = std::integral_constant<int, PAR>;
    using B1 = std::integral_constant<int, PAR ^ 1>;
    MMT(m0);
    __builtin_amdgcn_sched_barrier(0);
    load_a(I1{}, s); load_b(B1{}, I1{}, s);
    __builtin_amdgcn_sched_barrier(0);
    mma(I0{}, B0{});
    __builtin_amdgcn_sched_barrier(0);
    load_a(I2{}, s);
    __builtin_amdgcn_sched_barrier(0);
    mma(I1{}, B0{});
    __builtin_amdgcn_sched_barrier(0);
    load_a(I3{}, s); load_b(B0{}, I2{}, s);
    __builtin_amdgcn_sched_barrier(0);
    mma(I2{}, B1{});
    __builtin_amdgcn_sched_barrier(0);
    load_a(I4{}, s);
    __builtin_amdgcn_sched_barrier(0);
    mma(I3{}, B1{});
    __builtin_amdgcn_sched_barrier(0);
    load_a(I5{}, s);
    __builtin_amdgcn_sched_barrier(0);
    mma(I4{}, B0{});
    __builtin_amdgcn_sched_barrier(0);
    MMT(m1);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    MMT(m2);
    __syncthreads();                                          // barrier #(s + 2): image s & 1 is free, image (s + 1) & 1 is complete
    MMT(m3);
    const bool item_end = mc + 1 == p.nchunks;                // (wave-uniform)
    if (!item_end && s + 1 < S) { load_a(I0{}, s + 1); load_b(B1{}, I0{}, s + 1); }
    __builtin_amdgcn_sched_barrier(0);
    mma(I5{}, B0{});
    __builtin_amdgcn_sched_barrier(0);
    MMT(m4);
    if (pending >= 0) { combine(pending); pending = -1; }
    if (++mc == p.nchunks) {
      asm volatile("" ::: "memory");                          // (a real branch: no speculated divisions)
      epilogue(mk);
      mc = 0;
      ++mk;
      itm = decode(mk < nitems ? mk : nitems - 1);
      if (s + 1 < S) { load_a(I0{}, s + 1); load_b(B1{}, I0{}, s + 1); }      // (behind the epilogue: its registers are the fragments')
    }
    MMT(m5);
    MMA(8, m0, m1); MMA(8, m3, m4); MMA(9, m1, m2); MMA(10, m2, m3); MMA(11, m4, m5);
  };
  for (int s = 0; s < S; s += 2) {
    chunk(std::integral_constant<int, 0>{}, s);
    if (s + 1 < S) chunk(std::integral_constant<int, 1>{}, s + 1);
  }
  __syncthreads();                                            // the last item's statistics records
  if (pending >= 0) combine(pending);
  if (blockIdx.x == 0 && tid == 0) {
    atomicAdd(&g_mm_clock[0], __builtin_readcyclecounter() - clk_c0);
    atomicAdd(&g_mm_clock[1], __builtin_amdgcn_s_memrealtime() - clk_r0);
  }
#ifdef MM_STAMPS
  if (wr == 0 && lane == 0) for (int i = 8; i < 15; ++i) atomicAdd(&g_mm_stamps[i], st_acc[i]);
#endif
}

inline bool mm_knob() {
  static const int v = getenv("E2E_CONV_MM") ? atoi(getenv("E2E_CONV_MM")) : 1;
  return v != 0;
}

}  // namespace

void e2e::mm_clock_read(unsigned long long out[2], bool reset) {
  const unsigned long long z[2] = {0, 0};
  (void)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_mm_clock), sizeof(z));
  if (reset) (void)hipMemcpyToSymbol(HIP_SYMBOL(g_mm_clock), z, sizeof(z));
}

// tile geometry of a plane width (Geo<>): full-width tiles where the plane is 32, 64 or 128 wide; E2E_MM_GEOM=0 keeps 16 x 32 tiles
static int mm_geom(int Wi) {
  static const int knob = getenv("E2E_MM_GEOM") ? atoi(getenv("E2E_MM_GEOM")) : 1;
  if (!knob) return 0;
  return Wi == 128 ? 2 : (Wi == 64 ? 1 : (Wi == 32 ? 3 : 0));
}
static bool mm_fits(int geom, int B, int Cin, int Cout) {
  const int ct = geom == 2 ? Geo<2>::CT_MAX : Geo<0>::CT_MAX;
  const int lr = geom == 2 ? Geo<2>::LREC_MAX : (geom == 1 ? Geo<1>::LREC_MAX : Geo<0>::LREC_MAX);
  return Cin <= ct && Cout <= ct && (long long)B * e2e::cdiv(Cin, 16) * 16 <= lr;   // LDS channel table; the forward's LDS copy of the resolved input planes
}

// ---- operand ranges of the split-operand kernels (round 6: closes the fixed-2^3 hole) ----------------------------------------------
// One workgroup per conv: a rigorous bound of |x| over ALL input planes of that conv after normalise-on-load, from the parameters
// alone -- no pass over the activations, no change to any producer:
//   kind 1  normalised source (a conv block's output, or its max-pool): x = lrelu(gamma xhat + beta), |xhat| <= sqrt(N - 1) over the N
//           voxels of an instance (biased variance, rstd <= 1 / sigma)  =>  |x| <= |gamma_c| sqrt(N - 1) + |beta_c|
//   kind 2  transposed conv (k = stride, no bias) of a normalised source: |z[o, 2v + k]| <= sum_c bound_c |W[c, o, k]|, max over (o, k)
//   kind 3  a tensor whose max |x| somebody measured (the network input: e2e_absmax_word)
//   kind 4  max |w| of a weight tensor (the transposed convs split their weights inside the kernels)
//   kind 5  max_c sum_{o, tap} |w[o, c, tap]| over a channel range of a conv: x max |dy| (recorded at run time) it bounds the conv's
//           data gradient w.r.t. those channels -- the dy of the transposed conv that produced them
// The result (bit pattern of a float, 2^-10 relative head room for the fp32 rounding of fma(y, a, b)) is what e2e_conv133_fwd_mm and
// e2e_conv133_wgrad take as x_absmax.  How tight: sqrt(N - 1) is 2^10.5 above a typical |xhat| ~ 1 at 128^3, which leaves typical
// values at 2^4 after scaling -- lo pieces normal down to 2^-7 of typical, an absolute error of 2^-25 / 2^4 below that (fp32 eps of
// typical: 2^-24); at the benchmarked configuration the derived exponent is the 3 that rounds 5 hard-coded.
// Two launches: (job, part) workgroups leave partial maxima in the workspace (plain stores), one workgroup per job folds them.
// RANGE_PARTS workgroups share the long reductions (a 320 x 320 x 8 transposed-conv weight is 3.3 MB: one workgroup needs 250 us).
constexpr int RANGE_PARTS = 16;
__global__ __launch_bounds__(256) void input_ranges_kernel(const e2e_range_job_t* __restrict__ jobs, float* __restrict__ ws) {
  const e2e_range_job_t jb = jobs[blockIdx.x];
  const int part = blockIdx.y;
  __shared__ float red[4];
  __shared__ float cb[1024];                                  // per-channel bounds of a kind-2 source (C <= 1024)
  for (int si = 0; si < 3; ++si) {
    const e2e_range_src_t s = jb.src[si];
    float m = 0.f;
    if (s.kind == 1 || s.kind == 2) {
      const float root = sqrtf((float)(s.N > 1 ? s.N - 1 : 1));
      if (s.kind == 1) {
        if (part == 0)
          for (int c = threadIdx.x; c < s.C; c += 256) {
            const float b = fmaf(fabsf(s.gamma[c]), root, fabsf(s.beta[c]));
            m = (b == b) ? fmaxf(m, b) : __builtin_inff();
          }
      } else {
        for (int c = threadIdx.x; c < s.C; c += 256) cb[c] = fmaf(fabsf(s.gamma[c]), root, fabsf(s.beta[c]));
        __syncthreads();
        const int cols = s.wCout * s.wks;                     // W [C][wCout][wks]
        for (int col = part * 256 + threadIdx.x; col < cols; col += RANGE_PARTS * 256) {
          float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;       // (independent chains: the loads of four channels in flight)
          int c = 0;
          for (; c + 3 < s.C; c += 4) {
            a0 = fmaf(cb[c], fabsf(s.w[(long long)c * cols + col]), a0);
            a1 = fmaf(cb[c + 1], fabsf(s.w[(long long)(c + 1) * cols + col]), a1);
            a2 = fmaf(cb[c + 2], fabsf(s.w[(long long)(c + 2) * cols + col]), a2);
            a3 = fmaf(cb[c + 3], fabsf(s.w[(long long)(c + 3) * cols + col]), a3);
          }
          for (; c < s.C; ++c) a0 = fmaf(cb[c], fabsf(s.w[(long long)c * cols + col]), a0);
          const float acc = (a0 + a1) + (a2 + a3);
          m = (acc == acc) ? fmaxf(m, acc) : __builtin_inff();
        }
        __syncthreads();
      }
    } else if (s.kind == 3) {
      if (part == 0 && threadIdx.x == 0) m = __builtin_bit_cast(float, *s.word);
      if (!(m == m)) m = __builtin_inff();
    } else if (s.kind == 4) {                                 // max |w| over N floats (transposed-conv weights)
      for (long long i = (long long)part * 256 + threadIdx.x; i < s.N; i += RANGE_PARTS * 256) {
        const float v = s.w[i];
        m = (v == v) ? fmaxf(m, fabsf(v)) : __builtin_inff();
      }
    } else if (s.kind == 5) {
      // what a conv's data gradient can reach per unit of max |dy|: max over the input channels c in [C, C + wks) of
      // sum_{o, tap} |w[o][c][tap]| (w [wCout][Cin = (int)N][9]); the gradient buffer of those channels is bounded by this x max |dy|
      const int Cin = (int)s.N;
      for (int c = s.C + part * 256 + threadIdx.x; c < s.C + s.wks; c += RANGE_PARTS * 256) {
        float acc = 0.f;
        for (int o = 0; o < s.wCout; ++o) {
          const float* wp = s.w + ((long long)o * Cin + c) * 9;
#pragma unroll
          for (int t = 0; t < 9; ++t) acc += fabsf(wp[t]);
        }
        m = (acc == acc) ? fmaxf(m, acc) : __builtin_inff();
      }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, 64));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) ws[((long long)blockIdx.x * 3 + si) * RANGE_PARTS + part] = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    __syncthreads();
  }
}
__global__ __launch_bounds__(64) void input_ranges_fold_kernel(const e2e_range_job_t* __restrict__ jobs, const float* __restrict__ ws) {
  float m = threadIdx.x < 3 * RANGE_PARTS ? ws[(long long)blockIdx.x * 3 * RANGE_PARTS + threadIdx.x] : 0.f;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, 64));
  if (threadIdx.x == 0) *jobs[blockIdx.x].out = __builtin_bit_cast(unsigned, m * (1.f + 0x1p-10f));
}

__global__ __launch_bounds__(256) void absmax_word_kernel(const float* __restrict__ x, long long n, unsigned* __restrict__ word) {
  float m = 0.f;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    const float v = x[i];
    m = (v == v) ? fmaxf(m, fabsf(v)) : __builtin_inff();
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, 64));
  if ((threadIdx.x & 63) == 0 && m > 0.f) atomicMax(word, __builtin_bit_cast(unsigned, m));   // non-negative floats order like their bit patterns
}

extern "C" long long e2e_conv133_input_ranges_ws_bytes(int njobs) { return (long long)njobs * 3 * RANGE_PARTS * (long long)sizeof(float); }

extern "C" int e2e_conv133_input_ranges(const e2e_range_job_t* jobs, int njobs, void* ws, void* stream) {
  E2E_REQUIRE(jobs != nullptr && njobs > 0 && ws != nullptr, "conv133_input_ranges: bad arguments");
  hipLaunchKernelGGL(input_ranges_kernel, dim3(njobs, RANGE_PARTS), dim3(256), 0, (hipStream_t)stream, jobs, reinterpret_cast<float*>(ws));
  hipLaunchKernelGGL(input_ranges_fold_kernel, dim3(njobs), dim3(64), 0, (hipStream_t)stream, jobs, reinterpret_cast<const float*>(ws));
  return e2e::check_launch("input_ranges_kernel");
}

extern "C" int e2e_absmax_word(const float* x, long long n, unsigned* word, void* stream) {
  E2E_REQUIRE(x != nullptr && word != nullptr && n > 0, "absmax_word: bad arguments");
  hipStream_t st = (hipStream_t)stream;
  e2e::zero_async(word, 4, st);
  long long blocks = e2e::cdivll(n, 256 * 16);
  if (blocks > 2048) blocks = 2048;
  hipLaunchKernelGGL(absmax_word_kernel, dim3((unsigned)blocks), dim3(256), 0, st, x, n, word);
  return e2e::check_launch("absmax_word_kernel");
}

// shapes the kernel serves; 0 bytes = not eligible.  The bytes are those of ONE direction's packed weights (an upper bound that
// holds for either direction): the caller keeps one such buffer per layer and direction and has e2e_conv133_mm_pack fill them
extern "C" long long e2e_conv133_mm_ws_bytes(int B, int Cin, int Cout, int Di, int Hi, int Wi, int sd, int sh, int sw) {
  if (!mm_knob()) return 0;
  if (sd != 1 || sh != 1 || sw != 1) return 0;
  if (Wi % 32 != 0 || Hi % 16 != 0 || Hi <= 16 || Di < 1) return 0;   // the 16 x 32 tile class of conv133_kernel (the partial records line up)
  if (Cin <= 16 || Cout <= 16) return 0;                    // at least two 16-channel chunks in both directions (the 4-modal input layer: conv133_kernel)
  if ((long long)Hi * Wi >= (1ll << 29)) return 0;
  if (!mm_fits(mm_geom(Wi), B, Cin, Cout) && !mm_fits(0, B, Cin, Cout)) return 0;
  const long long cmax = Cin > Cout ? Cin : Cout;
  const long long blocks = e2e::cdiv((int)cmax, 32) * (long long)e2e::cdiv((int)cmax, 16);
  return (blocks * WCH + 63) & ~63ll;
}

// (re)build the packed weights of every (layer, direction) of the device job table: two launches, whatever the number of layers
extern "C" int e2e_conv133_mm_pack(const e2e_mm_pack_job_t* jobs, int njobs, long long max_elems, void* stream) {
  E2E_REQUIRE(jobs != nullptr && njobs > 0 && max_elems > 0, "conv133_mm_pack: bad arguments");
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(weights_absmax_kernel, dim3(njobs), dim3(1024), 0, st, jobs);
  hipLaunchKernelGGL(pack_weights_h2_kernel, dim3((unsigned)e2e::cdivll(max_elems, 256), njobs), dim3(256), 0, st, jobs);
  return e2e::check_launch("pack_weights_h2_kernel");
}

// compute units of the CURRENT device, rounded down to a multiple of 8 (one persistent workgroup per CU, XCD-aware remap);
// cached per device id: a process may drive GPUs with different CU counts
static int mm_num_cus() {
  static int cache[64] = {0};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = 0;
  if (cache[dev] == 0) {
    hipDeviceProp_t prop;
    int n = 0;
    if (hipGetDeviceProperties(&prop, dev) == hipSuccess) n = prop.multiProcessorCount;
    if (n <= 0) n = 256;
    n &= ~7;
    cache[dev] = n < 8 ? 8 : n;
  }
  return cache[dev];
}

static int mm_launch(int mode, const e2e_in_chan_t* chans, const float* xin, const unsigned* x_absmax, const void* wpk, const unsigned* w_absmax,
                     const float* bias, float* y, double* part, const e2e_out_chan_t* outs, int B, int P, int Q, int D, int H, int W,
                     hipStream_t st) {
  MmParams p{};
  p.chans = chans; p.xin = xin; p.x_absmax = x_absmax; p.w_absmax = w_absmax; p.bias = bias; p.y = y; p.part = part; p.outs = outs;
  p.P = P; p.Q = Q; p.B = B; p.D = D; p.H = H; p.W = W;
  p.nchunks = e2e::cdiv(P, 16);
  p.qblocks = e2e::cdiv(Q, 32);
  p.wpk = reinterpret_cast<const unsigned char*>(wpk);
  int geom = mm_geom(W);
  const int fwd_cin = mode == 0 ? P : Q, fwd_cout = mode == 0 ? Q : P;
  if (!mm_fits(geom, B, fwd_cin, fwd_cout)) geom = 0;
  const int th = geom == 1 ? 8 : (geom == 2 ? 4 : 16), tw = geom == 1 ? 64 : (geom == 2 ? 128 : 32);
  p.tiles_x = W / tw; p.tiles_y = H / th;
  p.tiles_per_n = D * p.tiles_y * p.tiles_x;
  // data gradient of a 64 -> 32 layer (two chunks of dy, two blocks of 32 destinations): a workgroup takes both blocks of a tile
  // back to back and stages dy once -- the second block's planes are still in the two LDS images (E2E_MM_PAIRQ=0: off, A/B)
  static const int pairq_knob = getenv("E2E_MM_PAIRQ") ? atoi(getenv("E2E_MM_PAIRQ")) : 1;
  p.pairq = (pairq_knob && p.nchunks == 2 && p.qblocks >= 2) ? 1 : 0;
  p.total = B * p.tiles_per_n * (p.pairq ? 1 : p.qblocks);
  const int ncu = mm_num_cus();
  static const int grid_knob = getenv("E2E_MM_GRID") ? atoi(getenv("E2E_MM_GRID")) : 0;
  int grid = grid_knob > 0 ? (grid_knob & ~7) : ncu;
  if (grid < 8) grid = 8;                                   // (E2E_MM_GRID = 1..7: the XCD remap works on multiples of 8)
  const int padded = (p.total + 7) & ~7;
  if (grid > padded) grid = padded;
  p.grid = grid;
  e2e::note_kernel("conv133_mm_h2<mode=%d,tile=%dx%d> wgs=%d items=%d chunks=%d%s", mode, th, tw, grid, p.total * (p.pairq ? p.qblocks : 1), p.nchunks,
                   p.pairq ? " pairq" : "");
#define MM_LAUNCH(M, G_) hipLaunchKernelGGL((conv133_mm_kernel<M, G_>), dim3(grid), dim3(512), 0, st, p)
  if (mode == 0) { if (geom == 0) MM_LAUNCH(0, 0); else if (geom == 1) MM_LAUNCH(0, 1); else if (geom == 2) MM_LAUNCH(0, 2); else MM_LAUNCH(0, 3); }
  else { if (geom == 0) MM_LAUNCH(1, 0); else if (geom == 1) MM_LAUNCH(1, 1); else if (geom == 2) MM_LAUNCH(1, 2); else MM_LAUNCH(1, 3); }
#undef MM_LAUNCH
#ifdef MM_STAMPS
  if (getenv("E2E_MM_STAMPS")) {
    (void)hipStreamSynchronize(st);
    unsigned long long h[16], z[16] = {0};
    (void)hipMemcpyFromSymbol(h, HIP_SYMBOL(g_mm_stamps), sizeof(h));
    const double c = h[15] ? (double)h[15] : 1.0;
    fprintf(stderr, "[conv133_mm mode %d P %d Q %d] cycles per chunk: staging wave: dma %.0f ctab %.0f stage %.0f (prepare %.0f rounds %.0f, round 0: %.0f) vmcnt %.0f barrier %.0f | matrix wave: mma %.0f lgkm %.0f barrier %.0f epilogue %.0f\n",
            mode, P, Q, h[0] / c, h[1] / c, h[3] / c, h[6] / c, h[7] / c, h[2] / c, h[4] / c, h[5] / c, h[8] / c, h[9] / c, h[10] / c, h[11] / c);
    (void)hipMemcpyToSymbol(HIP_SYMBOL(g_mm_stamps), z, sizeof(z));
  }
#endif
  return e2e::check_launch("conv133_mm_kernel");
}

extern "C" int e2e_conv133_fwd_mm(const e2e_in_chan_t* chans, int Cin, const void* wpk, const unsigned* w_absmax, const float* bias,
                                  const unsigned* x_absmax, float* y, double* part, int B, int Cout, int Di, int Hi, int Wi, void* stream) {
  E2E_REQUIRE(chans && wpk && y, "conv133_fwd_mm: null pointer");
  E2E_REQUIRE(e2e_conv133_mm_ws_bytes(B, Cin, Cout, Di, Hi, Wi, 1, 1, 1) > 0, "conv133_fwd_mm: shape not served (stride 1, W %% 32 == 0, H %% 16 == 0, 17..320 channels)");
  return mm_launch(0, chans, nullptr, x_absmax, wpk, w_absmax, bias, y, part, nullptr, B, Cin, Cout, Di, Hi, Wi, (hipStream_t)stream);
}

extern "C" int e2e_conv133_dgrad_mm(const float* dy, const unsigned* dy_absmax, const void* wpk_t, const unsigned* w_absmax,
                                    const e2e_out_chan_t* outs, int B, int Cin, int Cout, int Di, int Hi, int Wi, void* stream) {
  E2E_REQUIRE(dy && wpk_t && outs, "conv133_dgrad_mm: null pointer");
  E2E_REQUIRE(e2e_conv133_mm_ws_bytes(B, Cin, Cout, Di, Hi, Wi, 1, 1, 1) > 0, "conv133_dgrad_mm: shape not served");
  // the forward kernel with transposed, tap-reversed weights (packed that way: job.reverse): its "input planes" are dy's Cout
  // channels, its output planes the Cin virtual-concat channels (weight element [q = c][p = o][tap] = w[o][c][8 - tap])
  return mm_launch(1, nullptr, dy, dy_absmax, wpk_t, w_absmax, nullptr, nullptr, nullptr, outs, B, Cout, Cin, Di, Hi, Wi, (hipStream_t)stream);
}
