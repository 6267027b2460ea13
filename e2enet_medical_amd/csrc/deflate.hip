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
//
// N5b, e2e_deflate_encode_dynamic: the same chunks, slots, tokens and steps 1 and 2, with a third form of the chunk, a dynamic
// block whose literal/length code comes from the chunk's own token counts (tests/deflate_dynamic_oracle.py restates it).  The
// first walk also counts the tokens into an LDS histogram (ds_add); the code is built between two walks (a rank per lane, the
// tree and the header's run codes in lane 0: at most 286 symbols); a walk with the new lengths and a second prefix sum size the
// dynamic form, and the chunk is written in the shortest of the three forms.  What both kernels do is one set of functions below.
//
// e2e_crc32 is the two CRC kernels on their own (launch_crc), for a buffer that inflate.hip wrote; the way back is that file.
#include "e2e_common.h"
#include "e2e_deflate.h"

#include <cstdint>

namespace {

using e2e::deflate::CHUNK;                         // (the format's constants: e2e_deflate.h, shared with inflate.hip)
using e2e::deflate::STORED_EXTRA;
constexpr int THREADS = 512;
constexpr int PER = CHUNK / THREADS;               // 64: one mask bit per byte in one 64-bit word
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

// the length symbol (257 .. 285) of a match of 3 <= len <= 258 bytes, the number of its extra bits and their value
struct LengthSymbol {
  int sym, eb;
  unsigned extra;
};

__device__ __forceinline__ LengthSymbol length_symbol(int len) {
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
  return LengthSymbol{sym, eb, extra};
}

template <int ELEM>
__device__ __forceinline__ Token match(int len) {                  // 3 <= len <= 258
  const LengthSymbol ls = length_symbol(len);
  const int sym = ls.sym, eb = ls.eb;
  const unsigned extra = ls.extra;
  const int cn = sym < 280 ? 7 : 8;
  const unsigned code = sym < 280 ? rev((unsigned)(sym - 256), 7) : rev(0xC0u + (unsigned)(sym - 280), 8);
  return Token{code | (extra << cn) | (Dist<ELEM>::bits << (cn + eb)), cn + eb + Dist<ELEM>::n};
}

// The tokens that begin in this lane's bytes, in order.  mask: bit j set = byte j repeats byte j - ELEM (bits at and behind the
// lane's valid bytes are clear).  back: set bits immediately in front of the lane inside the chunk; fwd: set bits immediately behind
// it.  A maximal run [s, e) of the chunk is cut into 258s from s, then one match of the rest, or one or two literals.  lit(v) takes
// a literal byte, mat(len) a match length: the fixed and the dynamic kernel see the same tokens and give them their own codes.
template <typename L, typename M>
__device__ __forceinline__ void walk(unsigned long long mask, int valid, int base, int back, int fwd, const unsigned char* in,
                                     L&& lit, M&& mat) {
  int pos = 0;
  while (pos < valid) {                            // (at most 64 rounds: every round advances pos)
    if (!((mask >> pos) & 1ull)) {
      lit((unsigned)in[base + pos]);
      ++pos;
      continue;
    }
    const unsigned long long rest = ~mask >> pos;
    const int q = rest ? pos + __builtin_ctzll(rest) : PER;        // the run leaves the lane's bytes at q
    const int s = pos == 0 ? base - back : base + pos;
    const int e = q == PER ? base + PER + fwd : base + q;
    const int len = e - s, tail0 = s + len / 258 * 258, r = e - tail0;
    const int a = base + pos, b = base + q;
    for (int p = s + (a - s + 257) / 258 * 258; p < b && p < tail0; p += 258) mat(258);                   // (at most once: 258 > 64)
    if (r >= 3) {
      if (tail0 >= a && tail0 < b) mat(r);
    } else {
      for (int p = tail0 > a ? tail0 : a; p < b && p < e; ++p) lit((unsigned)in[p]);                      // (at most twice)
    }
    pos = q;
  }
}

// inclusive scan step operator on (whole lane set: bit 31, count): the count of set bits that end at the right edge
__device__ __forceinline__ unsigned join(unsigned left, unsigned right) {
  return (right & 0x80000000u) ? ((left & 0x80000000u) | ((left & 0x7FFFFFFFu) + (right & 0x7FFFFFFFu))) : right;
}

// ---- what the fixed and the dynamic kernel share: the steps 1 and 2, the prefix sum of 3, the fixed and the stored form -------
// The lane's place in its chunk
struct Lane {
  int n;                                           // bytes of the chunk, 1 .. CHUNK
  int base, valid;                                 // the lane's bytes: [base, base + valid) of the chunk
  unsigned long long mask;                         // bit j: byte base + j repeats the byte ELEM in front of it
  int back, fwd;                                   // set bits immediately in front of the lane's bytes and behind them
};

// 1. the lane's 64 bytes as 16 words, the 8 bytes in front of them as 2; what does not exist reads as zero.  Leaves the bytes in
// in_w and clears out_w (no barrier: run_scans has the next one).
template <int ELEM>
__device__ __forceinline__ Lane load_chunk(const unsigned char* __restrict__ src, long long nbytes, unsigned* in_w,
                                           unsigned* out_w) {
  const int t = threadIdx.x, base = t * PER;
  const long long c0 = (long long)blockIdx.x * CHUNK;
  const int n = (int)(nbytes - c0 < CHUNK ? nbytes - c0 : CHUNK);  // 1 .. CHUNK
  const int valid = n - base < 0 ? 0 : (n - base > PER ? PER : n - base);

  for (int i = t; i < OUT_WORDS; i += THREADS) out_w[i] = 0u;

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
  return Lane{n, base, valid, mask, 0, 0};
}

// 2. how far set bits reach in front of the lane and behind it (two double buffers of THREADS words each)
__device__ __forceinline__ void run_scans(Lane& lane, unsigned (*sc_back)[THREADS], unsigned (*sc_fwd)[THREADS]) {
  const int t = threadIdx.x;
  const unsigned long long mask = lane.mask;
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
  lane.back = t > 0 ? (int)(sc_back[cur][t - 1] & 0x7FFFFFFFu) : 0;
  lane.fwd = t + 1 < THREADS ? (int)(sc_fwd[cur][t + 1] & 0x7FFFFFFFu) : 0;
}

// inclusive prefix sum of one count per lane (a double buffer of THREADS words); returns the sum over all lanes
__device__ __forceinline__ unsigned scan_bits(unsigned& incl, unsigned (*sc_bits)[THREADS]) {
  const int t = threadIdx.x;
  int cur = 0;
  sc_bits[0][t] = incl;
  __syncthreads();
#pragma unroll
  for (int off = 1; off < THREADS; off <<= 1) {
    if (t >= off) incl += sc_bits[cur][t - off];
    cur ^= 1;
    sc_bits[cur][t] = incl;
    __syncthreads();
  }
  return sc_bits[cur][THREADS - 1];
}

// n <= 32 bits into the chunk's image at bit `at` (two lanes may share a word)
__device__ __forceinline__ void put_bits(unsigned* out_w, unsigned& at, unsigned bits, int n) {
  const unsigned word = at >> 5, sh = at & 31u;
  atomicOr(&out_w[word], bits << sh);
  if (sh + (unsigned)n > 32u) atomicOr(&out_w[word + 1], bits >> (32u - sh));
  at += (unsigned)n;
}

template <int ELEM>
__device__ __forceinline__ unsigned fixed_bits_of(const Lane& lane, const unsigned char* in) {
  unsigned my_bits = 0;
  walk(lane.mask, lane.valid, lane.base, lane.back, lane.fwd, in, [&](unsigned v) { my_bits += (unsigned)literal(v).n; },
       [&](int len) { my_bits += (unsigned)match<ELEM>(len).n; });
  return my_bits;
}

// block header (3) + tokens + end of block (7) + header of the empty stored block (3), padded, then 00 00 FF FF
__device__ __forceinline__ unsigned fixed_bytes_of(unsigned token_bits) { return (3u + token_bits + 7u + 3u + 7u) / 8u + 4u; }

// the ending of a Huffman block of `bytes` bytes whose bits up to the empty stored block's header are in place: LEN = 0000 is
// there, NLEN = FFFF; then the image goes to the slot with vector stores
__device__ __forceinline__ void close_and_store(unsigned* out_w, unsigned* slot_w, unsigned* counts, unsigned bytes) {
  const int t = threadIdx.x;
  if (t == 0) {
    const unsigned p = bytes - 2u;
    atomicOr(&out_w[p >> 2], 0xFFu << (8u * (p & 3u)));
    atomicOr(&out_w[(p + 1u) >> 2], 0xFFu << (8u * ((p + 1u) & 3u)));
  }
  __syncthreads();
  for (unsigned i = t; i < (bytes + 3u) / 4u; i += THREADS) slot_w[i] = out_w[i];
  if (t == 0) counts[blockIdx.x] = bytes;
}

// the fixed form: the lane's tokens begin `before` bits behind the block header
template <int ELEM>
__device__ __forceinline__ void write_fixed(const Lane& lane, const unsigned char* in, unsigned before, unsigned fixed_bytes,
                                            unsigned* out_w, unsigned* slot_w, unsigned* counts) {
  unsigned at = 3u + before;
  walk(lane.mask, lane.valid, lane.base, lane.back, lane.fwd, in,
       [&](unsigned v) { const Token k = literal(v); put_bits(out_w, at, k.bits, k.n); },
       [&](int len) { const Token k = match<ELEM>(len); put_bits(out_w, at, k.bits, k.n); });
  if (threadIdx.x == 0) atomicOr(&out_w[0], 2u);                   // BFINAL 0, BTYPE 01
  // (end of block and the stored header are ten zero bits)
  close_and_store(out_w, slot_w, counts, fixed_bytes);
}

// one stored block: 00, LEN, NLEN, the bytes (in_w behind the chunk's end is zero)
__device__ __forceinline__ void write_stored(int n, const unsigned* in_w, unsigned* slot_w, unsigned* counts) {
  const int t = threadIdx.x;
  const unsigned stored_bytes = (unsigned)n + STORED_EXTRA;
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

template <int ELEM>
__global__ __launch_bounds__(THREADS) void deflate_encode_kernel(const unsigned char* __restrict__ src, long long nbytes,
                                                                 unsigned char* __restrict__ slots,
                                                                 unsigned* __restrict__ counts) {
  __shared__ __attribute__((aligned(16))) unsigned in_w[CHUNK / 4];
  __shared__ unsigned out_w[OUT_WORDS];
  __shared__ unsigned sc_back[2][THREADS], sc_fwd[2][THREADS], sc_bits[2][THREADS];
  const unsigned char* in = (const unsigned char*)in_w;
  Lane lane = load_chunk<ELEM>(src, nbytes, in_w, out_w);
  run_scans(lane, sc_back, sc_fwd);

  // 3. bits of the lane's tokens, their prefix sum, the bits themselves
  const unsigned my_bits = fixed_bits_of<ELEM>(lane, in);
  unsigned incl = my_bits;
  const unsigned token_bits = scan_bits(incl, sc_bits);
  const unsigned fixed_bytes = fixed_bytes_of(token_bits);
  unsigned* slot_w = (unsigned*)(slots + (long long)blockIdx.x * SLOT);             // (16-byte aligned: SLOT is, and slots)
  if (fixed_bytes <= (unsigned)lane.n + STORED_EXTRA) write_fixed<ELEM>(lane, in, incl - my_bits, fixed_bytes, out_w, slot_w, counts);
  else write_stored(lane.n, in_w, slot_w, counts);
}

// ---- the dynamic form: one Huffman code per chunk from the chunk's own token counts (RFC 1951, 3.2.7) -------------------------
// Code lengths, for the literal/length code (286 symbols, 15 bits) and the code-length code (19 symbols, 7 bits) alike:
//   1. the used symbols are ordered by count descending, equal counts by symbol number ascending (a rank per lane);
//   2. lane 0 puts the counts in ascending order through the two-queue Huffman construction in Moffat and Katajainen's in-place
//      form (a leaf before an internal node of the same weight) and keeps only the number of leaves per depth;
//   3. leaves deeper than the limit count at the limit, which leaves the Kraft sum above 1 by a whole number of 2^-limit.  Once
//      per such unit (the step of zlib's gen_bitlen): the deepest level below the limit that has a leaf gives one up, it becomes an
//      internal node with two leaves one level down, one of them taken from the limit's level.  A step lowers the sum by exactly
//      2^-limit: the code ends complete;
//   4. the lengths are dealt out along the order of 1, shortest first: of two symbols with equal counts the one with the smaller
//      number never has the longer code.  Then the canonical codes of 3.2.2, bit-reversed for the image.
// All loops are bounded by the number of symbols.
constexpr int LL_SYMS = 286, CL_SYMS = 19, SYM_PAD = 288;
constexpr int CL_TOKENS = 320;                     // (at most one token per length of the two sequences: 286 + 6)

struct CodeTables {
  unsigned freq[SYM_PAD];                          // token counts of the literal/length symbols
  unsigned work[SYM_PAD];                          // step 2: weights, parents, depths
  unsigned short order[SYM_PAD];                   // step 1
  unsigned short code[SYM_PAD];                    // bit-reversed
  unsigned char len[SYM_PAD];
  unsigned short cl_tok[CL_TOKENS];                // the two length sequences in run codes: symbol | extra value << 5
  unsigned cl_freq[CL_SYMS];
  unsigned short cl_code[CL_SYMS];
  unsigned char cl_len[CL_SYMS];
  unsigned bl[16];                                 // symbols per length
  int used, hlit, hdist, hclen, ntok;
  unsigned header_bits;
};

// steps 2 and 3, one lane: bl[1 .. LIMIT] from the n >= 1 used symbols, order[0 .. n) as step 1 left them
template <int LIMIT>
__device__ void leaves_per_length(const unsigned* freq, const unsigned short* order, int n, unsigned* a, unsigned* bl) {
  for (int d = 0; d <= LIMIT; ++d) bl[d] = 0u;
  if (n == 1) {
    bl[1] = 1u;
    return;
  }
  for (int i = 0; i < n; ++i) a[i] = freq[order[n - 1 - i]];       // ascending
  a[0] += a[1];
  int root = 0, leaf = 2;
  for (int next = 1; next < n - 1; ++next) {
    if (leaf >= n || a[root] < a[leaf]) {
      a[next] = a[root];
      a[root++] = (unsigned)next;
    } else {
      a[next] = a[leaf++];
    }
    if (leaf >= n || (root < next && a[root] < a[leaf])) {
      a[next] += a[root];
      a[root++] = (unsigned)next;
    } else {
      a[next] += a[leaf++];
    }
  }
  a[n - 2] = 0u;
  for (int next = n - 3; next >= 0; --next) a[next] = a[a[next]] + 1u;             // depths of the internal nodes
  int avbl = 1, r = n - 2;
  for (unsigned depth = 0; avbl > 0 && depth < (unsigned)n; ++depth) {             // (a tree of n leaves is less than n deep)
    int used = 0;
    while (r >= 0 && a[r] == depth) ++used, --r;
    bl[depth < (unsigned)LIMIT ? depth : (unsigned)LIMIT] += (unsigned)(avbl - used);
    avbl = 2 * used;
  }
  int excess = -(1 << LIMIT);                      // of the Kraft sum, in units of 2^-LIMIT
  for (int d = 1; d <= LIMIT; ++d) excess += (int)(bl[d] << (LIMIT - d));
  for (; excess > 0; --excess) {                   // (fewer than n steps: every one takes a leaf from the limit's level)
    int bits = LIMIT - 1;
    while (bits > 0 && bl[bits] == 0u) --bits;
    if (bits == 0) break;                          // (never: a code over-subscribed at the limit has a shorter leaf)
    --bl[bits];
    bl[bits + 1] += 2u;
    --bl[LIMIT];
  }
}

// steps 1 to 4 for N symbols, all lanes; the tables are complete behind the last barrier
template <int N, int LIMIT>
__device__ void build_code(const unsigned* freq, unsigned char* len, unsigned short* code, CodeTables& tb) {
  const int t = threadIdx.x;
  const unsigned c = t < N ? freq[t] : 0u;
  int rank = 0, used = 0;
  for (int s = 0; s < N; ++s) {
    const unsigned cs = freq[s];
    used += cs != 0u;
    rank += cs > c || (cs == c && s < t);
  }
  if (c) tb.order[rank] = (unsigned short)t;
  __syncthreads();
  if (t == 0) leaves_per_length<LIMIT>(freq, tb.order, used, tb.work, tb.bl);
  __syncthreads();
  int mine = 0;
  if (c) {
    int upto = 0;
    for (int d = 1; d <= LIMIT && mine == 0; ++d) {
      upto += (int)tb.bl[d];
      if (rank < upto) mine = d;
    }
  }
  if (t < N) len[t] = (unsigned char)mine;
  __syncthreads();
  if (mine) {
    unsigned first = 0;                            // the first code of this length (3.2.2)
    for (int d = 1; d < mine; ++d) first = (first + tb.bl[d]) << 1;
    for (int s = 0; s < t; ++s) first += len[s] == (unsigned char)mine;
    code[t] = (unsigned short)rev(first, mine);
  }
  __syncthreads();
}

// one length sequence in the run codes 16, 17, 18, as zlib's scan_tree cuts it; one lane
template <typename F>
__device__ void run_code(F&& length_at, int count_of, CodeTables& tb) {
  int prev = -1, count = 0, nextlen = length_at(0);
  int max_count = nextlen == 0 ? 138 : 7, min_count = nextlen == 0 ? 3 : 4;
  auto emit = [&](int sym, int extra) {
    if (tb.ntok < CL_TOKENS) tb.cl_tok[tb.ntok++] = (unsigned short)(sym | (extra << 5));
    ++tb.cl_freq[sym];
  };
  for (int k = 0; k < count_of; ++k) {
    const int cur = nextlen;
    nextlen = k + 1 < count_of ? length_at(k + 1) : -1;
    if (++count < max_count && cur == nextlen) continue;
    if (count < min_count) {
      for (int i = 0; i < count; ++i) emit(cur, 0);                // (at most three times)
    } else if (cur != 0) {
      if (cur != prev) emit(cur, 0), --count;
      emit(16, count - 3);
    } else if (count <= 10) {
      emit(17, count - 3);
    } else {
      emit(18, count - 11);
    }
    count = 0, prev = cur;
    if (nextlen == 0) max_count = 138, min_count = 3;
    else if (cur == nextlen) max_count = 6, min_count = 3;
    else max_count = 7, min_count = 4;
  }
}

__device__ __forceinline__ int cl_extra_bits(int sym) { return sym == 16 ? 2 : sym == 17 ? 3 : sym == 18 ? 7 : 0; }
__device__ __forceinline__ int cl_permuted(int k) {                // 16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15
  return k < 3 ? 16 + k : k == 3 ? 0 : (k & 1) ? 8 - (k - 3) / 2 : 8 + (k - 4) / 2;
}

// the distance code: the one symbol of distance ELEM (0, 1, 3, 5) with length 1, code 0; distance 8 has an extra bit, set
template <int ELEM> struct DistSymbol { static constexpr int value = ELEM == 1 ? 0 : ELEM == 2 ? 1 : ELEM == 4 ? 3 : 5; };

template <int ELEM>
__device__ __forceinline__ Token dynamic_match(int len, const CodeTables& tb) {
  const LengthSymbol ls = length_symbol(len);
  const int cn = tb.len[ls.sym];
  unsigned bits = (unsigned)tb.code[ls.sym] | (ls.extra << cn);
  int n = cn + ls.eb + 1;
  if (ELEM == 8) bits |= 1u << n++;
  return Token{bits, n};
}

template <int ELEM>
__global__ __launch_bounds__(THREADS) void deflate_encode_dynamic_kernel(const unsigned char* __restrict__ src, long long nbytes,
                                                                         unsigned char* __restrict__ slots,
                                                                         unsigned* __restrict__ counts,
                                                                         unsigned char* __restrict__ kinds) {
  __shared__ __attribute__((aligned(16))) unsigned in_w[CHUNK / 4];
  __shared__ unsigned out_w[OUT_WORDS];
  __shared__ unsigned sc[4][THREADS];              // the two run scans, then the two bit counts
  __shared__ CodeTables tb;
  const unsigned char* in = (const unsigned char*)in_w;
  const int t = threadIdx.x;
  if (t < SYM_PAD) tb.freq[t] = t == 256 ? 1u : 0u;                // (end of block counts once)
  if (t < CL_SYMS) tb.cl_freq[t] = 0u;
  Lane lane = load_chunk<ELEM>(src, nbytes, in_w, out_w);
  run_scans(lane, sc, sc + 2);

  // 3. the fixed route's bits and the token counts in one walk
  unsigned my_bits = 0;
  walk(lane.mask, lane.valid, lane.base, lane.back, lane.fwd, in,
       [&](unsigned v) { my_bits += (unsigned)literal(v).n; atomicAdd(&tb.freq[v], 1u); },
       [&](int len) { my_bits += (unsigned)match<ELEM>(len).n; atomicAdd(&tb.freq[length_symbol(len).sym], 1u); });
  unsigned incl = my_bits;
  const unsigned token_bits = scan_bits(incl, sc);                 // (its first barrier is also the one behind the counts)
  const unsigned fixed_bytes = fixed_bytes_of(token_bits);
  const unsigned stored_bytes = (unsigned)lane.n + STORED_EXTRA;

  // 4. the literal/length code, the header's two length sequences in run codes, the code-length code
  build_code<LL_SYMS, 15>(tb.freq, tb.len, tb.code, tb);
  if (t == 0) {
    int hlit = LL_SYMS;
    while (hlit > 257 && tb.len[hlit - 1] == 0) --hlit;
    const bool has_match = hlit > 257;             // (a length symbol is in use)
    tb.hlit = hlit, tb.hdist = has_match ? DistSymbol<ELEM>::value + 1 : 1, tb.ntok = 0;
    run_code([&](int k) { return (int)tb.len[k]; }, hlit, tb);
    run_code([&](int k) { return has_match && k == DistSymbol<ELEM>::value ? 1 : 0; }, tb.hdist, tb);
  }
  __syncthreads();
  build_code<CL_SYMS, 7>(tb.cl_freq, tb.cl_len, tb.cl_code, tb);
  if (t == 0) {
    int hclen = CL_SYMS;
    while (hclen > 4 && tb.cl_len[cl_permuted(hclen - 1)] == 0) --hclen;
    unsigned bits = 3u + 5u + 5u + 4u + 3u * (unsigned)hclen;
    for (int s = 0; s < CL_SYMS; ++s) bits += tb.cl_freq[s] * (unsigned)(tb.cl_len[s] + cl_extra_bits(s));
    tb.hclen = hclen, tb.header_bits = bits;
  }
  __syncthreads();

  // 5. the dynamic form's bits per lane, and the choice: dynamic only where it is strictly shorter than both other forms
  unsigned my_dyn = 0;
  walk(lane.mask, lane.valid, lane.base, lane.back, lane.fwd, in, [&](unsigned v) { my_dyn += (unsigned)tb.len[v]; },
       [&](int len) { my_dyn += (unsigned)dynamic_match<ELEM>(len, tb).n; });
  unsigned incl_dyn = my_dyn;
  const unsigned dyn_token_bits = scan_bits(incl_dyn, sc + 2);
  // header + tokens + end of block + header of the empty stored block (3), padded, then 00 00 FF FF
  const unsigned dyn_bytes = (tb.header_bits + dyn_token_bits + (unsigned)tb.len[256] + 3u + 7u) / 8u + 4u;
  unsigned* slot_w = (unsigned*)(slots + (long long)blockIdx.x * SLOT);             // (16-byte aligned: SLOT is, and slots)
  if (dyn_bytes < fixed_bytes && dyn_bytes < stored_bytes) {
    unsigned at = tb.header_bits + incl_dyn - my_dyn;
    walk(lane.mask, lane.valid, lane.base, lane.back, lane.fwd, in,
         [&](unsigned v) { put_bits(out_w, at, tb.code[v], tb.len[v]); },
         [&](int len) { const Token k = dynamic_match<ELEM>(len, tb); put_bits(out_w, at, k.bits, k.n); });
    if (t == 0) {
      unsigned h = 0;
      put_bits(out_w, h, 4u, 3);                                   // BFINAL 0, BTYPE 10
      put_bits(out_w, h, (unsigned)(tb.hlit - 257), 5);
      put_bits(out_w, h, (unsigned)(tb.hdist - 1), 5);
      put_bits(out_w, h, (unsigned)(tb.hclen - 4), 4);
      for (int k = 0; k < tb.hclen; ++k) put_bits(out_w, h, tb.cl_len[cl_permuted(k)], 3);
      for (int k = 0; k < tb.ntok; ++k) {
        const int sym = tb.cl_tok[k] & 31, extra = tb.cl_tok[k] >> 5;
        put_bits(out_w, h, tb.cl_code[sym], tb.cl_len[sym]);
        if (cl_extra_bits(sym)) put_bits(out_w, h, (unsigned)extra, cl_extra_bits(sym));
      }
      unsigned e = tb.header_bits + dyn_token_bits;
      put_bits(out_w, e, tb.code[256], tb.len[256]);               // end of block; the stored header is three zero bits
    }
    close_and_store(out_w, slot_w, counts, dyn_bytes);
    if (t == 0) kinds[blockIdx.x] = 2;
  } else if (fixed_bytes <= stored_bytes) {
    write_fixed<ELEM>(lane, in, incl - my_bits, fixed_bytes, out_w, slot_w, counts);
    if (t == 0) kinds[blockIdx.x] = 1;
  } else {
    write_stored(lane.n, in_w, slot_w, counts);
    if (t == 0) kinds[blockIdx.x] = 0;
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

// zlib.crc32 of nbytes > 0 bytes: one raw CRC per chunk, then the fold (the encoders and e2e_crc32)
int launch_crc(const unsigned char* p, long long nbytes, unsigned* chunk_crcs, unsigned* crc, hipStream_t st) {
  const long long nchunks = e2e::cdivll(nbytes, CHUNK);
  hipLaunchKernelGGL(deflate_crc_kernel, dim3((unsigned)nchunks), dim3(THREADS), 0, st, p, nbytes, chunk_crcs);
  const int rc = e2e::check_launch("deflate_crc_kernel");
  if (rc != E2E_OK) return rc;
  hipLaunchKernelGGL(deflate_crc_combine_kernel, dim3(1), dim3(THREADS), 0, st, chunk_crcs, nchunks, nbytes, crc);
  return e2e::check_launch("deflate_crc_combine_kernel");
}

// both encoder entries: the same refusals, the same CRC kernels; only the dynamic one writes kinds
int encode(const char* what, bool dynamic, const void* src, long long nbytes, int elem, unsigned char* slots, unsigned* counts,
           unsigned char* kinds, unsigned* chunk_crcs, unsigned* crc, void* stream) {
  const hipStream_t st = (hipStream_t)stream;
  E2E_REQUIRE(elem == 1 || elem == 2 || elem == 4 || elem == 8, "%s: elem %d is not 1, 2, 4 or 8", what, elem);
  E2E_REQUIRE(nbytes >= 0 && nbytes <= (1ll << 37), "%s: %lld bytes, at most 2^37", what, nbytes);
  E2E_REQUIRE(nbytes % elem == 0, "%s: %lld bytes are no whole number of %d-byte elements", what, nbytes, elem);
  E2E_REQUIRE(crc != nullptr, "%s: null pointer", what);
  if (nbytes == 0) {
    hipLaunchKernelGGL(deflate_crc_zero_kernel, dim3(1), dim3(1), 0, st, crc);
    return e2e::check_launch("deflate_crc_zero_kernel");
  }
  E2E_REQUIRE(src && slots && counts && chunk_crcs && (kinds || !dynamic), "%s: null pointer", what);
  E2E_REQUIRE((uintptr_t)slots % 16 == 0, "%s: slots at %p is not aligned to 16 bytes", what, (const void*)slots);
  const long long nchunks = e2e::cdivll(nbytes, CHUNK);            // (at most 2^22: the grid fits)
  const dim3 grid((unsigned)nchunks), block(THREADS);
  const unsigned char* p = (const unsigned char*)src;
  int rc;
  if (dynamic) {
    switch (elem) {
      case 1: hipLaunchKernelGGL(deflate_encode_dynamic_kernel<1>, grid, block, 0, st, p, nbytes, slots, counts, kinds); break;
      case 2: hipLaunchKernelGGL(deflate_encode_dynamic_kernel<2>, grid, block, 0, st, p, nbytes, slots, counts, kinds); break;
      case 4: hipLaunchKernelGGL(deflate_encode_dynamic_kernel<4>, grid, block, 0, st, p, nbytes, slots, counts, kinds); break;
      default: hipLaunchKernelGGL(deflate_encode_dynamic_kernel<8>, grid, block, 0, st, p, nbytes, slots, counts, kinds); break;
    }
    rc = e2e::check_launch("deflate_encode_dynamic_kernel");
  } else {
    switch (elem) {
      case 1: hipLaunchKernelGGL(deflate_encode_kernel<1>, grid, block, 0, st, p, nbytes, slots, counts); break;
      case 2: hipLaunchKernelGGL(deflate_encode_kernel<2>, grid, block, 0, st, p, nbytes, slots, counts); break;
      case 4: hipLaunchKernelGGL(deflate_encode_kernel<4>, grid, block, 0, st, p, nbytes, slots, counts); break;
      default: hipLaunchKernelGGL(deflate_encode_kernel<8>, grid, block, 0, st, p, nbytes, slots, counts); break;
    }
    rc = e2e::check_launch("deflate_encode_kernel");
  }
  if (rc != E2E_OK) return rc;
  return launch_crc(p, nbytes, chunk_crcs, crc, st);
}

}  // namespace

extern "C" int e2e_crc32(const void* buf, long long nbytes, unsigned* chunk_crcs, unsigned* crc, void* stream) {
  const char* what = "crc32";
  const hipStream_t st = (hipStream_t)stream;
  E2E_REQUIRE(nbytes >= 0 && nbytes <= (1ll << 37), "%s: %lld bytes, at most 2^37", what, nbytes);
  E2E_REQUIRE(crc != nullptr, "%s: null pointer", what);
  if (nbytes == 0) {
    hipLaunchKernelGGL(deflate_crc_zero_kernel, dim3(1), dim3(1), 0, st, crc);
    return e2e::check_launch("deflate_crc_zero_kernel");
  }
  E2E_REQUIRE(buf && chunk_crcs, "%s: null pointer", what);
  return launch_crc((const unsigned char*)buf, nbytes, chunk_crcs, crc, st);
}

extern "C" int e2e_deflate_chunk_bytes(void) { return CHUNK; }
extern "C" int e2e_deflate_slot_bytes(void) { return SLOT; }

extern "C" int e2e_deflate_encode(const void* src, long long nbytes, int elem, unsigned char* slots, unsigned* counts,
                                  unsigned* chunk_crcs, unsigned* crc, void* stream) {
  return encode("deflate_encode", false, src, nbytes, elem, slots, counts, nullptr, chunk_crcs, crc, stream);
}

extern "C" int e2e_deflate_encode_dynamic(const void* src, long long nbytes, int elem, unsigned char* slots, unsigned* counts,
                                          unsigned char* kinds, unsigned* chunk_crcs, unsigned* crc, void* stream) {
  return encode("deflate_encode_dynamic", true, src, nbytes, elem, slots, counts, kinds, chunk_crcs, crc, stream);
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
