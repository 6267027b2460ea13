// N5: raw DEFLATE (RFC 1951) of a device buffer, and zlib's CRC-32 of it.  The format is the one include/e2e_hip.h states and
// tests/test_gpu_deflate.py restates in Python (reference_stream): chunks of CHUNK bytes, one workgroup each, a chunk one
// fixed-Huffman block whose only matches say "the same element again" (distance elem), or one stored block where that is shorter.
// No workgroup waits for another: every chunk goes to its own worst-case slot with its byte count, the host side forms the prefix
// sum of the counts and a second kernel gathers the slots.  Every loop is bounded by CHUNK.
//
// One chunk, 512 lanes, lane t owns the bytes [64 t, 64 t + 64):
//   1. the lane loads its bytes (and the 8 in front of them), leaves them in LDS for the literals, and forms a 64-bit mask:
//      bit j says byte j equals byte j - elem.  A run of set bits is a run of matches.
//   2. two scans over the lanes (9 steps each) tell a lane how far the run it starts in reaches back, and how far the run it ends
//      in goes on: with both ends known a position knows whether a token begins there (every 258 bytes, then the rest).
//   3. the lane walks its runs and literals twice: once for the number of bits, and after a prefix sum over the lanes once to put
//      the bits into the chunk's LDS image with ds_or (two lanes may share a word).  The image is stored with vector stores.
#include "e2e_common.h"

#include <cstdint>

namespace {

constexpr int CHUNK = 32768;                       // bytes per chunk (<= 65535: a stored block's LEN is 16 bits).  32768 = 127 * 258 + 2:
                                                   // a chunk of one value is 127 matches and a match or two literals
constexpr int THREADS = 512;
constexpr int PER = CHUNK / THREADS;               // 64: one mask bit per byte in one 64-bit word
constexpr int STORED_EXTRA = 5;                    // header byte, LEN, NLEN
constexpr int SLOT = (CHUNK + STORED_EXTRA + 15) / 16 * 16;
constexpr int OUT_WORDS = SLOT / 4 + 2;            // the fixed form is written only when it is no longer than the stored one,
                                                   // so every token (and the word its last bits spill into) lands inside
constexpr unsigned POLY = 0xEDB88320u;             // zlib's CRC-32, reflected

static_assert(PER == 64 && THREADS == 512 && CHUNK % 16 == 0 && CHUNK <= 65535, "one 64-bit mask per lane");

// ---- CRC-32 arithmetic: polynomials over GF(2) modulo POLY, reflected (bit 31 is x^0), as zlib's crc32_combine has them ---------
__host__ __device__ constexpr unsigned mulmod(unsigned a, unsigned b) {
  unsigned p = 0;
  for (int i = 0; i < 32; ++i) {
    if (a & (0x80000000u >> i)) p ^= b;
    b = (b & 1u) ? (b >> 1) ^ POLY : b >> 1;
  }
  return p;
}
// x^nbits
__host__ __device__ constexpr unsigned xpow(unsigned long long nbits) {
  unsigned p = 0x80000000u, sq = 0x40000000u;      // 1, x
  for (int i = 0; i < 64; ++i) {                   // (bounded: 64 squarings)
    if ((nbits >> i) & 1ull) p = mulmod(sq, p);
    sq = mulmod(sq, sq);
  }
  return p;
}
constexpr unsigned X_CHUNK = xpow(8ull * CHUNK);   // the shift operator of one whole chunk

// the shift operator of 64 * 2^s bytes, s = 0 .. 8: the levels of a chunk's tree
template <int S> struct LevelShift { static constexpr unsigned value = xpow(8ull * PER << S); };
__device__ __forceinline__ unsigned level_shift(int s) {
  switch (s) {
    case 0: return LevelShift<0>::value;
    case 1: return LevelShift<1>::value;
    case 2: return LevelShift<2>::value;
    case 3: return LevelShift<3>::value;
    case 4: return LevelShift<4>::value;
    case 5: return LevelShift<5>::value;
    case 6: return LevelShift<6>::value;
    case 7: return LevelShift<7>::value;
    default: return LevelShift<8>::value;
  }
}

__device__ __forceinline__ unsigned crc_table_entry(unsigned i) {
  unsigned c = i;
#pragma unroll
  for (int k = 0; k < 8; ++k) c = (c & 1u) ? (c >> 1) ^ POLY : c >> 1;
  return c;
}

// The CRC register after the bytes of one chunk, started at 0 and not inverted ("raw"): linear in the data, and blind to zero bytes
// in front.  The lanes therefore take 64-byte pieces counted from the END of the chunk -- the piece that is short or empty in a
// partial chunk is the first, where the missing bytes count as zeros in front -- and piece t is shifted by the 64 (511 - t) bytes
// behind it in a tree whose shifts are constants.
__global__ __launch_bounds__(THREADS) void deflate_crc_kernel(const unsigned char* __restrict__ src, long long nbytes,
                                                              unsigned* __restrict__ chunk_crcs) {
  __shared__ unsigned table[256];
  __shared__ unsigned part[THREADS];
  const int t = threadIdx.x;
  const long long c0 = (long long)blockIdx.x * CHUNK;
  const int n = (int)(nbytes - c0 < CHUNK ? nbytes - c0 : CHUNK);
  if (t < 256) table[t] = crc_table_entry((unsigned)t);
  __syncthreads();
  const int end = n - (THREADS - 1 - t) * PER;      // this lane: [end - 64, end) of the chunk, cut at 0
  unsigned r = 0;
  if (end >= PER) {
    typedef unsigned uvec __attribute__((ext_vector_type(4)));
#pragma unroll
    for (int v = 0; v < PER / 16; ++v) {
      uvec w;
      __builtin_memcpy(&w, src + c0 + (end - PER) + 16 * v, 16);      // (any alignment: a partial chunk shifts the pieces)
#pragma unroll
      for (int k = 0; k < 4; ++k) {
#pragma unroll
        for (int b = 0; b < 4; ++b) r = table[(r ^ (w[k] >> (8 * b))) & 0xFFu] ^ (r >> 8);
      }
    }
  } else {
    for (int i = 0; i < end; ++i) r = table[(r ^ src[c0 + i]) & 0xFFu] ^ (r >> 8);
  }
  part[t] = r;
  __syncthreads();
#pragma unroll
  for (int s = 0; s < 9; ++s) {                     // 2^9 = THREADS
    const int stride = 1 << s, group = 2 << s;
    const unsigned shift = level_shift(s);                          // (a constant after unrolling)
    if ((t & (group - 1)) == group - 1) r = mulmod(part[t - stride], shift) ^ r;
    __syncthreads();
    part[t] = r;
    __syncthreads();
  }
  if (t == THREADS - 1) chunk_crcs[blockIdx.x] = r;
}

// raw CRCs of the chunks -> zlib.crc32 of the input.  raw(A || B) = raw(A) x^(8 |B|) + raw(B): every chunk but the last shifts what
// came before it by X_CHUNK, the last by its own length.  512 lanes fold 512 stretches of chunks (again counted from the end, so
// that an empty or short stretch is the first), lane 0 folds the 512 results; then the effect of the start value and the final
// inversion, which is the CRC of nbytes zero bytes.
__global__ __launch_bounds__(THREADS) void deflate_crc_combine_kernel(const unsigned* __restrict__ chunk_crcs, long long nchunks,
                                                                      long long nbytes, unsigned* __restrict__ crc) {
  __shared__ unsigned part[THREADS];
  const int t = threadIdx.x;
  const long long nfull = nchunks > 0 ? nchunks - 1 : 0;           // chunks that are followed by another (all of them whole)
  const long long per = e2e::cdivll(nfull, THREADS);
  long long hi = nfull - (long long)(THREADS - 1 - t) * per, lo = hi - per;
  lo = lo < 0 ? 0 : lo;
  unsigned r = 0;
  for (long long c = lo; c < hi; ++c) r = mulmod(r, X_CHUNK) ^ chunk_crcs[c];
  part[t] = r;
  __syncthreads();
  if (t != 0) return;
  const unsigned x_per = xpow(8ull * CHUNK * (unsigned long long)per);
  unsigned acc = 0;
  for (int i = 0; i < THREADS; ++i) acc = mulmod(acc, x_per) ^ part[i];
  if (nchunks > 0) {
    const long long last = nbytes - nfull * CHUNK;
    acc = mulmod(acc, xpow(8ull * (unsigned long long)last)) ^ chunk_crcs[nchunks - 1];
  }
  *crc = acc ^ ~mulmod(xpow(8ull * (unsigned long long)nbytes), 0xFFFFFFFFu);
}

// ---- the fixed Huffman code (RFC 1951, 3.2.6); Huffman codes go most significant bit first, extra bits least -----------------
struct Token {
  unsigned bits;
  int n;
};

__device__ __forceinline__ unsigned rev(unsigned code, int n) { return __brev(code) >> (32 - n); }

__device__ __forceinline__ Token literal(unsigned v) {
  return v < 144u ? Token{rev(0x30u + v, 8), 8} : Token{rev(0x190u + (v - 144u), 9), 9};
}

// distance ELEM: code 0, 1, 3, or 5 with one extra bit set (7..8)
template <int ELEM> struct Dist;
template <> struct Dist<1> { static constexpr unsigned bits = 0x00u; static constexpr int n = 5; };      // rev5(0)
template <> struct Dist<2> { static constexpr unsigned bits = 0x10u; static constexpr int n = 5; };      // rev5(1)
template <> struct Dist<4> { static constexpr unsigned bits = 0x18u; static constexpr int n = 5; };      // rev5(3)
template <> struct Dist<8> { static constexpr unsigned bits = 0x14u | (1u << 5); static constexpr int n = 6; };   // rev5(5), extra 1

template <int ELEM>
__device__ __forceinline__ Token match(int len) {                  // 3 <= len <= 258
  int sym, eb = 0;
  unsigned extra = 0;
  if (len == 258) {
    sym = 285;
  } else {
    const int l = len - 3;
    if (l < 8) {
      sym = 257 + l;
    } else {
      eb = (31 - __builtin_clz((unsigned)l)) - 2;
      sym = 261 + 4 * eb + ((l >> eb) & 3);
      extra = (unsigned)l & ((1u << eb) - 1u);
    }
  }
  const int cn = sym < 280 ? 7 : 8;
  const unsigned code = sym < 280 ? rev((unsigned)(sym - 256), 7) : rev(0xC0u + (unsigned)(sym - 280), 8);
  return Token{code | (extra << cn) | (Dist<ELEM>::bits << (cn + eb)), cn + eb + Dist<ELEM>::n};
}

// The tokens that begin in this lane's bytes, in order.  mask: bit j set = byte j repeats byte j - ELEM (bits at and behind the
// lane's valid bytes are clear).  back: set bits immediately in front of the lane inside the chunk; fwd: set bits immediately behind
// it.  A maximal run [s, e) of the chunk is cut into 258s from s, then one match of the rest, or one or two literals.
template <int ELEM, typename F>
__device__ __forceinline__ void walk(unsigned long long mask, int valid, int base, int back, int fwd, const unsigned char* in,
                                     F&& put) {
  int pos = 0;
  while (pos < valid) {                            // (at most 64 rounds: every round advances pos)
    if (!((mask >> pos) & 1ull)) {
      put(literal(in[base + pos]));
      ++pos;
      continue;
    }
    const unsigned long long rest = ~mask >> pos;
    const int q = rest ? pos + __builtin_ctzll(rest) : PER;        // the run leaves the lane's bytes at q
    const int s = pos == 0 ? base - back : base + pos;
    const int e = q == PER ? base + PER + fwd : base + q;
    const int len = e - s, tail0 = s + len / 258 * 258, r = e - tail0;
    const int a = base + pos, b = base + q;
    for (int p = s + (a - s + 257) / 258 * 258; p < b && p < tail0; p += 258) put(match<ELEM>(258));      // (at most once: 258 > 64)
    if (r >= 3) {
      if (tail0 >= a && tail0 < b) put(match<ELEM>(r));
    } else {
      for (int p = tail0 > a ? tail0 : a; p < b && p < e; ++p) put(literal(in[p]));                       // (at most twice)
    }
    pos = q;
  }
}

// inclusive scan step operator on (whole lane set: bit 31, count): the count of set bits that end at the right edge
__device__ __forceinline__ unsigned join(unsigned left, unsigned right) {
  return (right & 0x80000000u) ? ((left & 0x80000000u) | ((left & 0x7FFFFFFFu) + (right & 0x7FFFFFFFu))) : right;
}

template <int ELEM>
__global__ __launch_bounds__(THREADS) void deflate_encode_kernel(const unsigned char* __restrict__ src, long long nbytes,
                                                                 unsigned char* __restrict__ slots,
                                                                 unsigned* __restrict__ counts) {
  __shared__ __attribute__((aligned(16))) unsigned in_w[CHUNK / 4];
  __shared__ unsigned out_w[OUT_WORDS];
  __shared__ unsigned sc_back[2][THREADS], sc_fwd[2][THREADS], sc_bits[2][THREADS];
  const unsigned char* in = (const unsigned char*)in_w;
  const int t = threadIdx.x, base = t * PER;
  const long long c0 = (long long)blockIdx.x * CHUNK;
  const int n = (int)(nbytes - c0 < CHUNK ? nbytes - c0 : CHUNK);  // 1 .. CHUNK
  const int valid = n - base < 0 ? 0 : (n - base > PER ? PER : n - base);

  for (int i = t; i < OUT_WORDS; i += THREADS) out_w[i] = 0u;

  // 1. the lane's 64 bytes as 16 words, the 8 bytes in front of them as 2; what does not exist reads as zero
  unsigned w[PER / 4 + 2];
#pragma unroll
  for (int k = 0; k < PER / 4 + 2; ++k) w[k] = 0u;
  const long long g0 = c0 + base;                                 // the lane's first byte in the input
  if (valid == PER && g0 >= 8) {
    typedef unsigned uvec __attribute__((ext_vector_type(4)));
    unsigned long long prev;
    __builtin_memcpy(&prev, src + g0 - 8, 8);
    w[0] = (unsigned)prev, w[1] = (unsigned)(prev >> 32);
#pragma unroll
    for (int v = 0; v < PER / 16; ++v) {
      uvec x;
      __builtin_memcpy(&x, src + g0 + 16 * v, 16);
      w[2 + 4 * v] = x[0], w[3 + 4 * v] = x[1], w[4 + 4 * v] = x[2], w[5 + 4 * v] = x[3];
    }
  } else if (valid > 0) {
    // the first lane of the input and the lanes of a partial chunk's end: byte by byte, nothing read outside [0, nbytes)
#pragma unroll
    for (int j = -8; j < PER; ++j) {
      if (j < valid && g0 + j >= 0) w[(j + 8) >> 2] |= (unsigned)src[g0 + j] << (8 * ((j + 8) & 3));
    }
  }
#pragma unroll
  for (int v = 0; v < PER / 16; ++v) {
    typedef unsigned uvec __attribute__((ext_vector_type(4)));
    uvec x = {w[2 + 4 * v], w[3 + 4 * v], w[4 + 4 * v], w[5 + 4 * v]};
    *(uvec*)(in_w + base / 4 + 4 * v) = x;
  }

  unsigned long long mask = 0;
#pragma unroll
  for (int k = 0; k < PER / 4; ++k) {
    const unsigned cur = w[k + 2];
    unsigned old;                                   // the word ELEM bytes earlier
    if (ELEM == 8) old = w[k];
    else if (ELEM == 4) old = w[k + 1];
    else old = (cur << (8 * ELEM)) | (w[k + 1] >> (32 - 8 * ELEM));
    const unsigned x = cur ^ old;
    const unsigned eq = ((x & 0xFFu) == 0u ? 1u : 0u) | ((x & 0xFF00u) == 0u ? 2u : 0u) | ((x & 0xFF0000u) == 0u ? 4u : 0u) |
                        ((x & 0xFF000000u) == 0u ? 8u : 0u);
    mask |= (unsigned long long)eq << (4 * k);
  }
  if (valid < PER) mask &= (1ull << valid) - 1ull;                 // (valid = 0: nothing)
  if (g0 < ELEM) mask &= ~((1ull << (ELEM - g0)) - 1ull);          // the first ELEM bytes of the input repeat nothing

  // 2. how far set bits reach in front of the lane and behind it
  const bool whole = mask == ~0ull;
  const unsigned lead = whole ? PER : (unsigned)__builtin_ctzll(~mask);
  const unsigned trail = whole ? PER : (unsigned)__builtin_clzll(~mask);            // (a lane with valid < 64 has bit 63 clear: 0)
  unsigned vb = (whole ? 0x80000000u : 0u) | trail, vf = (whole ? 0x80000000u : 0u) | lead;
  int cur = 0;
  sc_back[0][t] = vb, sc_fwd[0][t] = vf;
  __syncthreads();
#pragma unroll
  for (int off = 1; off < THREADS; off <<= 1) {
    if (t >= off) vb = join(sc_back[cur][t - off], vb);
    if (t + off < THREADS) vf = join(sc_fwd[cur][t + off], vf);    // (mirrored: the count of set bits that begin at the left edge)
    cur ^= 1;
    sc_back[cur][t] = vb, sc_fwd[cur][t] = vf;
    __syncthreads();
  }
  const int back = t > 0 ? (int)(sc_back[cur][t - 1] & 0x7FFFFFFFu) : 0;
  const int fwd = t + 1 < THREADS ? (int)(sc_fwd[cur][t + 1] & 0x7FFFFFFFu) : 0;

  // 3. bits of the lane's tokens, their prefix sum, the bits themselves
  unsigned my_bits = 0;
  walk<ELEM>(mask, valid, base, back, fwd, in, [&](Token k) { my_bits += (unsigned)k.n; });
  unsigned incl = my_bits;
  cur = 0;
  sc_bits[0][t] = incl;
  __syncthreads();
#pragma unroll
  for (int off = 1; off < THREADS; off <<= 1) {
    if (t >= off) incl += sc_bits[cur][t - off];
    cur ^= 1;
    sc_bits[cur][t] = incl;
    __syncthreads();
  }
  const unsigned token_bits = sc_bits[cur][THREADS - 1];
  // block header (3) + tokens + end of block (7) + header of the empty stored block (3), padded, then 00 00 FF FF
  const unsigned fixed_bytes = (3u + token_bits + 7u + 3u + 7u) / 8u + 4u;
  const unsigned stored_bytes = (unsigned)n + STORED_EXTRA;
  unsigned* slot_w = (unsigned*)(slots + (long long)blockIdx.x * SLOT);             // (16-byte aligned: SLOT is, and slots)
  if (fixed_bytes <= stored_bytes) {
    unsigned at = 3u + incl - my_bits;
    walk<ELEM>(mask, valid, base, back, fwd, in, [&](Token k) {
      const unsigned word = at >> 5, sh = at & 31u;
      atomicOr(&out_w[word], k.bits << sh);
      if (sh + (unsigned)k.n > 32u) atomicOr(&out_w[word + 1], k.bits >> (32u - sh));
      at += (unsigned)k.n;
    });
    if (t == 0) {
      atomicOr(&out_w[0], 2u);                                     // BFINAL 0, BTYPE 01
      // (end of block and the stored header are ten zero bits; LEN = 0000, NLEN = FFFF)
      const unsigned p = fixed_bytes - 2u;
      atomicOr(&out_w[p >> 2], 0xFFu << (8u * (p & 3u)));
      atomicOr(&out_w[(p + 1u) >> 2], 0xFFu << (8u * ((p + 1u) & 3u)));
    }
    __syncthreads();
    for (unsigned i = t; i < (fixed_bytes + 3u) / 4u; i += THREADS) slot_w[i] = out_w[i];
    if (t == 0) counts[blockIdx.x] = fixed_bytes;
  } else {
    // one stored block: 00, LEN, NLEN, the bytes (in_w behind the chunk's end is zero)
    const unsigned len = (unsigned)n, nlen = ~len & 0xFFFFu;
    for (unsigned i = t; i < (stored_bytes + 3u) / 4u; i += THREADS) {
      unsigned v;
      if (i == 0) v = (len << 8) | ((nlen & 0xFFu) << 24);
      else if (i == 1) v = (nlen >> 8) | (in_w[0] << 8);
      else v = (in_w[i - 2] >> 24) | ((i - 1 < CHUNK / 4 ? in_w[i - 1] : 0u) << 8);
      slot_w[i] = v;
    }
    if (t == 0) counts[blockIdx.x] = stored_bytes;
  }
}

__global__ void deflate_crc_zero_kernel(unsigned* crc) { *crc = 0u; }

// slot c -> out[offsets[c] ...): 16 bytes per lane and step from the 16-byte aligned slot to wherever the chunk lands
constexpr int GATHER_MAX_BLOCKS = 4096;

__global__ __launch_bounds__(THREADS) void deflate_gather_kernel(const unsigned char* __restrict__ slots,
                                                                 const unsigned* __restrict__ counts,
                                                                 const long long* __restrict__ offsets, long long nchunks,
                                                                 unsigned char* __restrict__ out, long long out_bytes) {
  typedef unsigned uvec __attribute__((ext_vector_type(4)));
  for (long long c = blockIdx.x; c < nchunks; c += gridDim.x) {
    const long long off = offsets[c];
    const int cnt = (int)counts[c];
    if (cnt < 0 || cnt > SLOT || off < 0 || off + cnt > out_bytes) continue;       // never behind the buffer
    const unsigned char* s = slots + c * SLOT;
    unsigned char* d = out + off;
    const int vecs = cnt / 16;
    for (int i = threadIdx.x; i < vecs; i += THREADS) {
      const uvec v = *(const uvec*)(s + 16 * i);
      __builtin_memcpy(d + 16 * i, &v, 16);
    }
    const int i = vecs * 16 + (int)threadIdx.x;
    if (i < cnt) d[i] = s[i];
  }
}

}  // namespace

extern "C" int e2e_deflate_chunk_bytes(void) { return CHUNK; }
extern "C" int e2e_deflate_slot_bytes(void) { return SLOT; }

extern "C" int e2e_deflate_encode(const void* src, long long nbytes, int elem, unsigned char* slots, unsigned* counts,
                                  unsigned* chunk_crcs, unsigned* crc, void* stream) {
  const char* what = "deflate_encode";
  const hipStream_t st = (hipStream_t)stream;
  E2E_REQUIRE(elem == 1 || elem == 2 || elem == 4 || elem == 8, "%s: elem %d is not 1, 2, 4 or 8", what, elem);
  E2E_REQUIRE(nbytes >= 0 && nbytes <= (1ll << 37), "%s: %lld bytes, at most 2^37", what, nbytes);
  E2E_REQUIRE(nbytes % elem == 0, "%s: %lld bytes are no whole number of %d-byte elements", what, nbytes, elem);
  E2E_REQUIRE(crc != nullptr, "%s: null pointer", what);
  if (nbytes == 0) {
    hipLaunchKernelGGL(deflate_crc_zero_kernel, dim3(1), dim3(1), 0, st, crc);
    return e2e::check_launch("deflate_crc_zero_kernel");
  }
  E2E_REQUIRE(src && slots && counts && chunk_crcs, "%s: null pointer", what);
  E2E_REQUIRE((uintptr_t)slots % 16 == 0, "%s: slots at %p is not aligned to 16 bytes", what, (const void*)slots);
  const long long nchunks = e2e::cdivll(nbytes, CHUNK);            // (at most 2^22: the grid fits)
  const dim3 grid((unsigned)nchunks), block(THREADS);
  const unsigned char* p = (const unsigned char*)src;
  switch (elem) {
    case 1: hipLaunchKernelGGL(deflate_encode_kernel<1>, grid, block, 0, st, p, nbytes, slots, counts); break;
    case 2: hipLaunchKernelGGL(deflate_encode_kernel<2>, grid, block, 0, st, p, nbytes, slots, counts); break;
    case 4: hipLaunchKernelGGL(deflate_encode_kernel<4>, grid, block, 0, st, p, nbytes, slots, counts); break;
    default: hipLaunchKernelGGL(deflate_encode_kernel<8>, grid, block, 0, st, p, nbytes, slots, counts); break;
  }
  int rc = e2e::check_launch("deflate_encode_kernel");
  if (rc != E2E_OK) return rc;
  hipLaunchKernelGGL(deflate_crc_kernel, grid, block, 0, st, p, nbytes, chunk_crcs);
  rc = e2e::check_launch("deflate_crc_kernel");
  if (rc != E2E_OK) return rc;
  hipLaunchKernelGGL(deflate_crc_combine_kernel, dim3(1), block, 0, st, chunk_crcs, nchunks, nbytes, crc);
  return e2e::check_launch("deflate_crc_combine_kernel");
}

extern "C" int e2e_deflate_gather(const unsigned char* slots, const unsigned* counts, const long long* offsets, long long nchunks,
                                  unsigned char* out, long long out_bytes, void* stream) {
  const char* what = "deflate_gather";
  E2E_REQUIRE(nchunks >= 0 && nchunks <= (1ll << 22), "%s: %lld chunks", what, nchunks);
  E2E_REQUIRE(out_bytes >= 0, "%s: %lld bytes", what, out_bytes);
  if (nchunks == 0) return E2E_OK;
  E2E_REQUIRE(slots && counts && offsets && out, "%s: null pointer", what);
  E2E_REQUIRE((uintptr_t)slots % 16 == 0, "%s: slots at %p is not aligned to 16 bytes", what, (const void*)slots);
  E2E_REQUIRE((uintptr_t)offsets % 8 == 0, "%s: offsets at %p is not aligned to 8 bytes", what, (const void*)offsets);
  const long long blocks = nchunks < GATHER_MAX_BLOCKS ? nchunks : GATHER_MAX_BLOCKS;
  hipLaunchKernelGGL(deflate_gather_kernel, dim3((unsigned)blocks), dim3(THREADS), 0, (hipStream_t)stream, slots, counts, offsets,
                     nchunks, out, out_bytes);
  return e2e::check_launch("deflate_gather_kernel");
}
