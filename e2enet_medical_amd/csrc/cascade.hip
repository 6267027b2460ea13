// The two-stage cascade on the device (gfx950): the hand-over of the 3d_lowres stage and the augmentation of its segmentation as an
// input of the full-resolution stage.
// Reference: e2enet/training/cascade_stuff/predict_next_stage.py:31-43 (resample_and_save: resample_data_or_seg(order 1) + argmax(0)),
// e2enet/training/data_augmentation/pyramid_augmentations.py:23-136 (MoveSegAsOneHotToData, ApplyRandomBinaryOperatorTransform with
// skimage's binary_dilation / erosion / closing / opening and ball(), RemoveRandomConnectedComponentFromOneHotEncodingTransform with
// skimage's label()).
//
//   e2e_resample_argmax_u8    per output voxel the K order-1 values of e2e_resample_linear (e2e_resample.h: the same expression) and
//                             their first maximum as one byte: the K x full-resolution fp32 tensor is never written
//   e2e_seg_onehot            seg channel -> len(labels) 0 / 1 channels behind the data channels of the network input
//   e2e_morph_pack / pass / unpack
//                             binary morphology on bit-packed rows.  A channel [D, H, W] is packed once (x != 0) into 64-bit words,
//                             ceil(W / 64) per row; a pass ORs, for every (z, y) row of the footprint, the source row shifted over the
//                             row's one x-run; unpack writes 0.0 / 1.0 and clears the other channels where a voxel "was added".
//                             dilation: out[p] = OR_s in[p - o_s], 0 outside the volume.  erosion (border value 1) is the
//                             complement of the dilation of the complement by the reflected footprint: out[p] = AND_s in[p + o_s].
//   e2e_rcc_remove            26-connected components of one channel (e2e_unionfind.h: merge_back26), their sizes, the components
//                             with size < threshold ranked by the raster index of their root (e2e_rank.h) -- the id order of
//                             skimage's and scipy's label -- and the floor(u * count)-th of them cleared (and set in another channel)
//
// Every result is an integer or a bit; the atomics are integer min / or / add: the same bits on every run.
#include "e2e_common.h"
#include "e2e_rank.h"
#include "e2e_resample.h"
#include "e2e_unionfind.h"
#include <cmath>

namespace {

namespace rk = e2e::rank;
using e2e::uf::NONE;
using e2e::uf::MAX_VOXELS;
using e2e::uf::find_root;
typedef unsigned long long u64;
typedef unsigned __int128 u128;

// ---- hand-over: fused order-1 resample + argmax ----------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void resample_argmax_kernel(const float* __restrict__ src, unsigned char* __restrict__ seg, int K,
                                                              long long kstride, int A, int B, int C, long long sa, long long sb,
                                                              long long sc, int OA, int OB, int OC) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long long)OA * OB * OC) return;
  const int oc = (int)(idx % OC);
  const int ob = (int)((idx / OC) % OB);
  const int oa = (int)(idx / ((long long)OC * OB));
  const int n_in[3] = {A, B, C}, n_out[3] = {OA, OB, OC}, o[3] = {oa, ob, oc};
  const long long st[3] = {sa, sb, sc};
  e2e::rs::Lin3 L;
  e2e::rs::lin3_setup(L, o, n_in, n_out, -1);
  float best = -INFINITY;
  int lab = 0;
  for (int k = 0; k < K; ++k) {                                 // the first maximum; a NaN counts as one (export_argmax_kernel)
    const float p = e2e::rs::lin3_eval(L, src + (long long)k * kstride, st);
    if (p > best || (p != p && best == best)) { best = p; lab = k; }
  }
  seg[idx] = (unsigned char)lab;
}

// ---- one-hot of a seg channel ------------------------------------------------------------------------------------------------------
constexpr int ONEHOT_MAX_LABELS = 64;
struct Labels { float v[ONEHOT_MAX_LABELS]; };

// out[b, c0 + l, i] = seg[b, ch, i] == labels[l]
__global__ __launch_bounds__(256) void seg_onehot_kernel(const float* __restrict__ seg, float* __restrict__ out, Labels labels, int n_labels,
                                                         int CS, int ch, int CO, int c0, long long vol) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= vol) return;
  const long long b = blockIdx.y;
  const float s = seg[(b * CS + ch) * vol + i];
  float* o = out + (b * CO + c0) * vol + i;
  for (int l = 0; l < n_labels; ++l) o[(long long)l * vol] = s == labels.v[l] ? 1.f : 0.f;
}

// ---- binary morphology on bit-packed rows -------------------------------------------------------------------------------------------
constexpr int MORPH_MAX_N = 17, MORPH_MAX_ROWS = MORPH_MAX_N * MORPH_MAX_N;
constexpr int MORPH_MARGIN = 16;                                // bits of the neighbouring words in a window: >= MORPH_MAX_N / 2 + run
struct RunTable { signed char r[MORPH_MAX_ROWS][4]; };          // (oz, oy, x_lo, x_hi), offsets from the footprint's origin
constexpr int UNPACK_MAX_OTHERS = 64;
struct Others { int c[UNPACK_MAX_OTHERS]; };

__device__ __forceinline__ int words_per_row(int W) { return (W + 63) >> 6; }
// the bits of word w that lie inside the row
__device__ __forceinline__ u64 valid_bits(int w, int W) {
  const int left = W - (w << 6);
  return left >= 64 ? ~0ull : (1ull << left) - 1ull;
}

// wave g of the grid owns word g of the packed volume: 64 consecutive voxels of one row
__global__ __launch_bounds__(256) void morph_pack_kernel(const float* __restrict__ x, u64* __restrict__ bits, int rows, int W) {
  const int Ww = words_per_row(W);
  const long long g = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  const bool live = g < (long long)rows * Ww;                  // (the same for the whole wave)
  const long long row = live ? g / Ww : 0;
  const int col = (int)(live ? g % Ww : 0) * 64 + lane;
  const u64 b = __ballot(live && col < W && x[row * W + col] != 0.f);
  if (live && lane == 0) bits[g] = b;
}

// thread t owns word t of dst.  The window of a source row holds MARGIN bits of the word before, the word, MARGIN bits of the word
// behind: bit j is voxel x = 64 w - MARGIN + j.  in[x - ox] lands on x by a shift left by ox.
__global__ __launch_bounds__(256) void morph_pass_kernel(const u64* __restrict__ src, u64* __restrict__ dst, RunTable table, int n_rows,
                                                         int reflect, int complement, int D, int H, int W) {
  const int Ww = words_per_row(W);
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= (long long)D * H * Ww) return;
  const int w = (int)(t % Ww);
  const int y = (int)((t / Ww) % H), z = (int)(t / ((long long)Ww * H));
  const u64 inv = complement ? ~0ull : 0ull;
  u128 acc = 0;
  for (int r = 0; r < n_rows; ++r) {
    int oz = table.r[r][0], oy = table.r[r][1], lo = table.r[r][2], hi = table.r[r][3];
    if (reflect) {
      oz = -oz; oy = -oy;
      const int l2 = -hi;
      hi = -lo; lo = l2;
    }
    const int zz = z - oz, yy = y - oy;
    if (zz < 0 || zz >= D || yy < 0 || yy >= H) continue;      // outside the volume: 0 (the complement of erosion's border 1)
    const u64* row = src + ((long long)zz * H + yy) * Ww;
    const u64 cur = (row[w] ^ inv) & valid_bits(w, W);
    const u64 prev = w > 0 ? (row[w - 1] ^ inv) : 0ull;         // (a word that is not the last of its row is all valid bits)
    const u64 next = w + 1 < Ww ? (row[w + 1] ^ inv) & valid_bits(w + 1, W) : 0ull;
    const u128 win = (u128)(prev >> (64 - MORPH_MARGIN)) | ((u128)cur << MORPH_MARGIN) |
                     ((u128)(next & ((1ull << MORPH_MARGIN) - 1ull)) << (64 + MORPH_MARGIN));
    // OR of the window shifted left by 0 .. len - 1, by doubling; then the run's first offset
    const int len = hi - lo + 1;
    u128 run = win;
    int k = 1;
    while (2 * k <= len) {
      run |= run << k;
      k <<= 1;
    }
    if (k < len) run |= run << (len - k);
    acc |= lo >= 0 ? run << lo : run >> (-lo);
  }
  u64 out = (u64)(acc >> MORPH_MARGIN);
  dst[t] = (out ^ inv) & valid_bits(w, W);
}

// chan[i] = bit i as 0.0 / 1.0; where the bit is 1 and chan[i] was 0 the voxel "was added": the other listed channels become 0
__global__ __launch_bounds__(256) void morph_unpack_kernel(const u64* __restrict__ bits, float* __restrict__ sample, long long vol, int chan,
                                                           Others others, int n_others, int rows, int W) {
  const int Ww = words_per_row(W);
  const long long g = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (g >= (long long)rows * Ww) return;
  const long long row = g / Ww;
  const int col = (int)(g % Ww) * 64 + lane;
  if (col >= W) return;
  const bool on = (bits[g] >> lane) & 1ull;
  const long long i = row * W + col;
  float* p = sample + (long long)chan * vol + i;
  const bool was = *p != 0.f;
  *p = on ? 1.f : 0.f;
  if (on && !was)
    for (int k = 0; k < n_others; ++k) sample[(long long)others.c[k] * vol + i] = 0.f;
}

// ---- removal of one random connected component ----------------------------------------------------------------------------------------
constexpr int WS_WORDS = 16;
enum { W_ROOTS = 0, W_CHOSEN = 1, W_GIVEUP = 3 };               // words[W_CHOSEN]: root of the chosen component + 1, 0 = none

__global__ __launch_bounds__(256) void rcc_init_kernel(const float* __restrict__ x, unsigned* __restrict__ parent, unsigned* __restrict__ size,
                                                       unsigned* __restrict__ words, unsigned V, unsigned W) {
  if (blockIdx.x == 0 && threadIdx.x < WS_WORDS) words[threadIdx.x] = 0u;
  e2e::uf::init_runs([&](unsigned j) { return x[j] != 0.f; }, parent, V, W);
  const u64 i64 = (u64)blockIdx.x * 256ull + threadIdx.x;
  if (i64 < V) size[i64] = 0u;
}

__global__ __launch_bounds__(256) void rcc_merge_kernel(unsigned* parent, unsigned* words, unsigned V, unsigned W, unsigned H) {
  e2e::uf::merge_back26(parent, &words[W_GIVEUP], V, W, H);
}

// parent[i] = root(i); size[root] += 1, one atomicAdd per run of equal roots in a wave; roots are counted
__global__ __launch_bounds__(256) void rcc_flatten_count_kernel(unsigned* parent, unsigned* size, unsigned* words, unsigned V) {
  const unsigned lane = threadIdx.x & 63u;
  const u64 i64 = (u64)blockIdx.x * 256ull + threadIdx.x;
  const unsigned i = (unsigned)i64;
  unsigned root = NONE;
  if (i64 < V && parent[i] != NONE) {
    unsigned budget = V + 64u;
    root = find_root(parent, i, budget, &words[W_GIVEUP]);
    if (root != NONE) parent[i] = root;                          // (roots keep parent[r] == r; a racing reader sees an ancestor)
  }
  const bool m = root != NONE;
  const unsigned prev = __shfl_up(root, 1, 64);
  const bool brk = lane == 0u || !m || prev != root;
  const u64 brks = __ballot(brk);
  if (m && brk) {
    const u64 rest = lane == 63u ? 0ull : brks >> (lane + 1u);
    const unsigned len = rest ? (unsigned)__builtin_ctzll(rest) + 1u : 64u - lane;
    atomicAdd(&size[root], len);
  }
  const u64 roots = __ballot(m && root == i);
  if (lane == 0u && roots) atomicAdd(&words[W_ROOTS], (unsigned)__popcll(roots));
}

struct IsSet {
  __device__ __forceinline__ bool operator()(float v) const { return v > 0.f; }
};

// v[it] = 1 where voxel base + it * THREADS + thread is the root of a component with size < threshold (the layout of rank::load_chunk)
__device__ __forceinline__ void load_eligible(const unsigned* __restrict__ parent, const unsigned* __restrict__ size, unsigned V,
                                              double threshold, long long base, float v[rk::ITERS]) {
#pragma unroll
  for (int it = 0; it < rk::ITERS; ++it) {
    const long long i = base + (long long)(it * rk::THREADS + (int)threadIdx.x);
    v[it] = (i < (long long)V && parent[i] == (unsigned)i && (double)size[i] < threshold) ? 1.f : 0.f;
  }
}

__global__ __launch_bounds__(rk::THREADS) void rcc_count_kernel(const unsigned* __restrict__ parent, const unsigned* __restrict__ size, unsigned V,
                                                               double threshold, unsigned* __restrict__ counts) {
  const long long blk = blockIdx.x;
  float v[rk::ITERS];
  load_eligible(parent, size, V, threshold, blk * rk::CHUNK, v);
  const unsigned tot = rk::wave_matches(v, IsSet{});
  __shared__ unsigned sh[rk::WAVES];
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = tot;
  __syncthreads();
  if (threadIdx.x == 0) counts[blk] = sh[0] + sh[1] + sh[2] + sh[3];
}

// the eligible root of raster rank floor(u * count) writes itself (+ 1) into words[W_CHOSEN]: one writer
__global__ __launch_bounds__(rk::THREADS) void rcc_choose_kernel(const unsigned* __restrict__ parent, const unsigned* __restrict__ size, unsigned V,
                                                                double threshold, double u, const unsigned* __restrict__ counts,
                                                                const u64* __restrict__ offsets, const long long* __restrict__ total,
                                                                unsigned* __restrict__ words) {
  const long long blk = blockIdx.x;
  const long long count = *total;
  if (count <= 0 || words[W_GIVEUP] != 0u) return;              // (a given-up labelling removes nothing)
  long long n = (long long)floor(u * (double)count);
  n = n < 0 ? 0 : (n > count - 1 ? count - 1 : n);
  const long long lo = (long long)offsets[blk];
  if (n < lo || n >= lo + (long long)counts[blk]) return;       // (the same for the whole workgroup)
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  float v[rk::ITERS];
  load_eligible(parent, size, V, threshold, blk * rk::CHUNK, v);
  __shared__ unsigned wtot[rk::ITERS * rk::WAVES];
  const unsigned ex = rk::matches_before(v, IsSet{}, wtot, lane, wave);
#pragma unroll
  for (int it = 0; it < rk::ITERS; ++it) {
    const bool m = IsSet{}(v[it]);
    const u64 bits = __ballot(m);
    const unsigned local = rk::rank_in_chunk(ex, it, wave, bits, lane);
    if (m && lo + (long long)local == n) words[W_CHOSEN] = (unsigned)(blk * rk::CHUNK + (long long)(it * rk::THREADS + t)) + 1u;
  }
}

__global__ __launch_bounds__(256) void rcc_clear_kernel(float* __restrict__ x, float* __restrict__ fill, const unsigned* __restrict__ parent,
                                                        const unsigned* __restrict__ words, unsigned V) {
  const u64 i64 = (u64)blockIdx.x * 256ull + threadIdx.x;
  const unsigned chosen = words[W_CHOSEN];
  if (i64 >= V || chosen == 0u) return;
  if (parent[i64] == chosen - 1u) {                              // (parent[i] is i's root after the flatten pass)
    x[i64] = 0.f;
    if (fill) fill[i64] = 1.f;
  }
}

// result: components, eligible components, size of the removed one (0 = none), give-up word
__global__ void rcc_result_kernel(const unsigned* words, const unsigned* size, const long long* total, u64* result) {
  if (threadIdx.x == 0) {
    result[0] = words[W_ROOTS];
    result[1] = (u64)*total;
    result[2] = words[W_CHOSEN] ? size[words[W_CHOSEN] - 1u] : 0u;
    result[3] = words[W_GIVEUP];
  }
}

struct RccWs {
  unsigned *parent, *size, *words;
  long long* total;
  void* rank;
};
RccWs rcc_ws(void* ws, long long V) {
  unsigned* p = (unsigned*)ws;
  RccWs a;
  a.parent = p;
  a.size = p + V;
  a.words = p + 2 * V;
  char* q = (char*)(a.words + WS_WORDS);
  q += (16 - ((size_t)q & 15)) & 15;
  a.total = (long long*)q;
  a.rank = q + 16;
  return a;
}

bool dims_ok(const char* what, int D, int H, int W, int* rc) {
  if (D < 1 || H < 1 || W < 1) {
    e2e::set_error("%s: every axis needs at least one voxel (got %d x %d x %d)", what, D, H, W);
    *rc = E2E_ERR_ARG;
    return false;
  }
  if ((long long)D * H * W > MAX_VOXELS) {
    e2e::set_error("%s: %d x %d x %d is more than the 2^31 - 2 voxels a 32-bit index reaches", what, D, H, W);
    *rc = E2E_ERR_UNSUPPORTED;
    return false;
  }
  return true;
}

}  // namespace

extern "C" int e2e_resample_argmax_u8(const float* src, unsigned char* seg, int K, long long kstride, int A, int B, int C, long long sa,
                                      long long sb, long long sc, int OA, int OB, int OC, void* stream) {
  E2E_REQUIRE(src && seg && K > 0 && K <= 256 && A > 0 && B > 0 && C > 0 && OA > 0 && OB > 0 && OC > 0,
              "resample_argmax_u8: bad arguments (1 .. 256 classes fit a byte)");
  hipLaunchKernelGGL(resample_argmax_kernel, dim3((unsigned)e2e::cdivll((long long)OA * OB * OC, 256)), dim3(256), 0, (hipStream_t)stream,
                     src, seg, K, kstride, A, B, C, sa, sb, sc, OA, OB, OC);
  return e2e::check_launch("resample_argmax_kernel");
}

extern "C" int e2e_seg_onehot(const float* seg, float* out, const int* labels, int n_labels, int B, int CS, int channel, int CO, int c0,
                              long long vol, void* stream) {
  E2E_REQUIRE(seg && out && labels && B > 0 && B <= 65535 && vol > 0, "seg_onehot: bad arguments");
  E2E_REQUIRE(n_labels > 0 && n_labels <= ONEHOT_MAX_LABELS, "seg_onehot: 1 .. %d labels (got %d)", ONEHOT_MAX_LABELS, n_labels);
  E2E_REQUIRE(channel >= 0 && channel < CS, "seg_onehot: seg channel %d of %d", channel, CS);
  E2E_REQUIRE(c0 >= 0 && c0 + n_labels <= CO, "seg_onehot: channels %d .. %d do not fit the %d of the output", c0, c0 + n_labels - 1, CO);
  Labels l;
  for (int k = 0; k < n_labels; ++k) l.v[k] = (float)labels[k];
  hipLaunchKernelGGL(seg_onehot_kernel, dim3((unsigned)e2e::cdivll(vol, 256), (unsigned)B), dim3(256), 0, (hipStream_t)stream, seg, out, l,
                     n_labels, CS, channel, CO, c0, vol);
  return e2e::check_launch("seg_onehot_kernel");
}

extern "C" int e2e_morph_max_footprint(void) { return MORPH_MAX_N; }

extern "C" long long e2e_morph_bits_words(int D, int H, int W) {
  if (D < 1 || H < 1 || W < 1) return 0;
  return (long long)D * H * ((W + 63) / 64);
}

extern "C" int e2e_morph_pack(const float* x, unsigned long long* bits, int D, int H, int W, void* stream) {
  int rc;
  if (!dims_ok("morph_pack", D, H, W, &rc)) return rc;
  E2E_REQUIRE(x && bits, "morph_pack: null pointer");
  const long long words = e2e_morph_bits_words(D, H, W);
  hipLaunchKernelGGL(morph_pack_kernel, dim3((unsigned)e2e::cdivll(words, 4)), dim3(256), 0, (hipStream_t)stream, x, bits, D * H, W);
  return e2e::check_launch("morph_pack_kernel");
}

extern "C" int e2e_morph_pass(const unsigned long long* src, unsigned long long* dst, int D, int H, int W, const int* table, int n_rows,
                              int N, int reflect, int complement, void* stream) {
  int rc;
  if (!dims_ok("morph_pass", D, H, W, &rc)) return rc;
  E2E_REQUIRE(src && dst && src != dst && (table || n_rows == 0) && n_rows >= 0 && N >= 1, "morph_pass: bad arguments");
  if (N > MORPH_MAX_N) {
    e2e::set_error("morph_pass: a footprint of %d^3 is more than the %d^3 the row window holds", N, MORPH_MAX_N);
    return E2E_ERR_UNSUPPORTED;
  }
  const int c = N / 2;
  RunTable t;
  bool seen[MORPH_MAX_N][MORPH_MAX_N] = {};
  for (int r = 0; r < n_rows; ++r) {
    const int oz = table[4 * r], oy = table[4 * r + 1], lo = table[4 * r + 2], hi = table[4 * r + 3];
    E2E_REQUIRE(oz >= -c && oz < N - c && oy >= -c && oy < N - c && lo >= -c && hi < N - c && lo <= hi,
                "morph_pass: run %d (%d, %d, %d .. %d) lies outside a footprint of %d^3 with origin %d", r, oz, oy, lo, hi, N, c);
    if (seen[oz + c][oy + c]) {                                 // (also the only way n_rows could pass N * N)
      e2e::set_error("morph_pass: footprint row (%d, %d) has a gap: one contiguous x-run per row is served", oz, oy);
      return E2E_ERR_UNSUPPORTED;
    }
    seen[oz + c][oy + c] = true;
    t.r[r][0] = (signed char)oz; t.r[r][1] = (signed char)oy; t.r[r][2] = (signed char)lo; t.r[r][3] = (signed char)hi;
  }
  const long long words = e2e_morph_bits_words(D, H, W);
  hipLaunchKernelGGL(morph_pass_kernel, dim3((unsigned)e2e::cdivll(words, 256)), dim3(256), 0, (hipStream_t)stream, src, dst, t, n_rows,
                     reflect != 0, complement != 0, D, H, W);
  return e2e::check_launch("morph_pass_kernel");
}

extern "C" int e2e_morph_unpack(const unsigned long long* bits, float* sample, int n_channels, int channel, const int* others, int n_others,
                                int D, int H, int W, void* stream) {
  int rc;
  if (!dims_ok("morph_unpack", D, H, W, &rc)) return rc;
  E2E_REQUIRE(bits && sample && channel >= 0 && channel < n_channels, "morph_unpack: bad arguments");
  E2E_REQUIRE(n_others >= 0 && n_others <= UNPACK_MAX_OTHERS && (others || n_others == 0), "morph_unpack: 0 .. %d other channels", UNPACK_MAX_OTHERS);
  Others o;
  for (int k = 0; k < n_others; ++k) {
    E2E_REQUIRE(others[k] >= 0 && others[k] < n_channels && others[k] != channel, "morph_unpack: other channel %d of %d (own: %d)", others[k],
                n_channels, channel);
    o.c[k] = others[k];
  }
  const long long words = e2e_morph_bits_words(D, H, W);
  hipLaunchKernelGGL(morph_unpack_kernel, dim3((unsigned)e2e::cdivll(words, 4)), dim3(256), 0, (hipStream_t)stream, bits, sample,
                     (long long)D * H * W, channel, o, n_others, D * H, W);
  return e2e::check_launch("morph_unpack_kernel");
}

extern "C" long long e2e_rcc_ws_bytes(int D, int H, int W) {
  int rc;
  if (!dims_ok("rcc_ws_bytes", D, H, W, &rc)) return 0;
  const long long V = (long long)D * H * W;
  return 8ll * V + 4ll * WS_WORDS + 48 + rk::ws_bytes(rk::chunks(V), 1);
}

extern "C" int e2e_rcc_remove(float* x, float* fill, int D, int H, int W, double threshold, double u, void* ws, unsigned long long* result,
                              void* stream) {
  int rc;
  if (!dims_ok("rcc_remove", D, H, W, &rc)) return rc;
  E2E_REQUIRE(x && ws && result && x != fill, "rcc_remove: bad pointers");
  E2E_REQUIRE(threshold == threshold && u >= 0. && u < 1., "rcc_remove: the threshold is NaN or u = %g is outside [0, 1)", u);
  hipStream_t st = (hipStream_t)stream;
  const long long Vl = (long long)D * H * W, nb = rk::chunks(Vl);
  const unsigned V = (unsigned)Vl;
  const RccWs a = rcc_ws(ws, Vl);
  unsigned* counts = (unsigned*)a.rank;
  const dim3 grid((unsigned)e2e::cdivll(Vl, 256)), block(256);
  hipLaunchKernelGGL(rcc_init_kernel, grid, block, 0, st, x, a.parent, a.size, a.words, V, (unsigned)W);
  if (int e = e2e::check_launch("rcc_init_kernel")) return e;
  hipLaunchKernelGGL(rcc_merge_kernel, grid, block, 0, st, a.parent, a.words, V, (unsigned)W, (unsigned)H);
  hipLaunchKernelGGL(rcc_flatten_count_kernel, grid, block, 0, st, a.parent, a.size, a.words, V);
  hipLaunchKernelGGL(rcc_count_kernel, dim3((unsigned)nb), dim3(rk::THREADS), 0, st, a.parent, a.size, V, threshold, counts);
  if (int e = rk::launch_scan(a.rank, nb, 1, a.total, st)) return e;
  hipLaunchKernelGGL(rcc_choose_kernel, dim3((unsigned)nb), dim3(rk::THREADS), 0, st, a.parent, a.size, V, threshold, u, counts,
                     rk::ws_offsets(a.rank, nb, 1), a.total, a.words);
  hipLaunchKernelGGL(rcc_clear_kernel, grid, block, 0, st, x, fill, a.parent, a.words, V);
  hipLaunchKernelGGL(rcc_result_kernel, dim3(1), dim3(64), 0, st, a.words, a.size, a.total, result);
  return e2e::check_launch("rcc kernels");
}
