// What the two device inflaters share (inflate.hip: the chunk records of the device encoder; inflate_any.hip: any DEFLATE stream):
// the bit reader, the canonical-code tables and the helpers that build and read them.  One wave per parser: all 64 lanes run the
// helpers on the same values, so control flow is uniform and every lane writes the same value to the same LDS address.
#pragma once
#include <hip/hip_runtime.h>

namespace e2e {
namespace inflate_bits {

constexpr int WAVE = 64;
constexpr int MAX_BITS = 15;
constexpr int FAST_BITS = 10, FAST = 1 << FAST_BITS;          // first-level lookup of the literal/length code
constexpr int LL_MAX = 288, LL_VALID = 286, D_MAX = 32, D_VALID = 30, CL_SYMS = 19, CL_BITS = 7;

// order between what one lane wrote to LDS and what another reads (one wave: the LDS unit keeps the order of the instructions)
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// ---- bits, least significant first, from comp[next...) with zeros behind ncomp ------------------------------------------------
struct Bits {
  const unsigned char* comp;
  long long ncomp, next;                           // next: the first byte not yet in buf
  unsigned long long buf;
  int cnt;

  __device__ __forceinline__ unsigned load32() const {
    unsigned v = 0;
    if (next + 4 <= ncomp) {
      __builtin_memcpy(&v, comp + next, 4);
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if (next + i < ncomp) v |= (unsigned)comp[next + i] << (8 * i);
      }
    }
    return v;
  }
  // at least 32 bits behind it
  __device__ __forceinline__ void refill() {
    if (cnt <= 32) {
      buf |= (unsigned long long)load32() << cnt;
      next += 4;
      cnt += 32;
    }
  }
  __device__ __forceinline__ void drop(int n) { buf >>= n, cnt -= n; }
  __device__ __forceinline__ unsigned take(int n) {                // n <= 16
    const unsigned v = (unsigned)buf & ((1u << n) - 1u);
    drop(n);
    return v;
  }
  __device__ __forceinline__ void align() { drop(cnt & 7); }       // (whole bytes were loaded: cnt mod 8 bits are left of this byte)
  __device__ __forceinline__ long long byte_pos() const { return next - (cnt >> 3); }
  __device__ __forceinline__ long long bit_pos() const { return 8 * next - cnt; }
};

// a reader whose next bit is bit `pos` of the stream (bit 0 = the least significant bit of comp[0]); pos >= 0
__device__ __forceinline__ Bits bits_at(const unsigned char* comp, long long ncomp, long long pos) {
  Bits b{comp, ncomp, pos >> 3, 0ull, 0};
  b.refill();
  b.drop((int)(pos & 7));
  return b;
}

struct Tables {
  unsigned short fast[FAST];                       // symbol | length << 9; 0: longer than FAST_BITS (or no such code)
  unsigned short ll_sym[LL_MAX], d_sym[D_MAX], cl_sym[CL_SYMS + 1];       // symbols in the order of (length, symbol)
  unsigned short ll_count[MAX_BITS + 1], d_count[MAX_BITS + 1], cl_count[MAX_BITS + 1], offs[MAX_BITS + 1];
  unsigned char lens[LL_MAX + D_MAX];
};

// canonical code of n lengths: count per length and the symbols in order (every lane, the same values).  Returns what is left of
// the code space: < 0 over-subscribed (nothing else is built then), 0 complete, > 0 incomplete.
static __device__ int build_code(const unsigned char* lens, int n, unsigned short* count, unsigned short* sym, unsigned short* offs) {
  for (int l = 0; l <= MAX_BITS; ++l) count[l] = 0;
  wave_sync();
  for (int s = 0; s < n; ++s) {
    const int l = lens[s] & MAX_BITS;
    count[l] = (unsigned short)(count[l] + 1);
    wave_sync();
  }
  int left = 1;
  for (int l = 1; l <= MAX_BITS; ++l) {
    left = (left << 1) - (int)count[l];
    if (left < 0) return -1;
  }
  offs[1] = 0;
  for (int l = 1; l < MAX_BITS; ++l) offs[l + 1] = (unsigned short)(offs[l] + count[l]);
  wave_sync();
  for (int s = 0; s < n; ++s) {
    const int l = lens[s] & MAX_BITS;
    if (l) {
      sym[offs[l]] = (unsigned short)s;            // (offs[l] < n: the counts sum to at most n)
      offs[l] = (unsigned short)(offs[l] + 1);
      wave_sync();
    }
  }
  return left;
}

// one symbol, bit by bit along the canonical code (at most maxbits rounds); -1: no such code
__device__ __forceinline__ int decode_slow(Bits& b, const unsigned short* count, const unsigned short* sym, int maxbits) {
  unsigned bits = (unsigned)b.buf;
  int code = 0, first = 0, index = 0;
  for (int len = 1; len <= maxbits; ++len) {
    code |= (int)(bits & 1u);
    bits >>= 1;
    const int c = count[len];
    if (code - c < first) {
      b.drop(len);
      return sym[index + (code - first)];
    }
    index += c, first = (first + c) << 1, code <<= 1;
  }
  return -1;
}

// the first-level table of the literal/length code, lanes over the symbols in code order
static __device__ void fill_fast(Tables& tb) {
  const int lane = threadIdx.x;
  for (int i = lane; i < FAST; i += WAVE) tb.fast[i] = 0;
  wave_sync();
  int total = 0;
  for (int l = 1; l <= MAX_BITS; ++l) total += tb.ll_count[l];
  for (int idx = lane; idx < total && idx < LL_MAX; idx += WAVE) {
    int len = 1, first = 0, index = 0;
    while (len <= MAX_BITS && idx >= index + (int)tb.ll_count[len]) {
      index += tb.ll_count[len];
      first = (first + tb.ll_count[len]) << 1;
      ++len;
    }
    if (len <= FAST_BITS) {
      const unsigned code = (unsigned)(first + idx - index);       // < 2^len: the code is not over-subscribed
      const unsigned r = (__brev(code) >> (32 - len)) & (FAST - 1);
      const unsigned short entry = (unsigned short)(tb.ll_sym[idx] | (len << 9));
      for (unsigned j = r; j < (unsigned)FAST; j += 1u << len) tb.fast[j] = entry;
    }
  }
  wave_sync();
}

// The tables of one Huffman block whose three header bits have been read (btype 1: the fixed code; 2: the code lengths follow in
// the stream).  false: HLIT > 286 or HDIST > 30 symbols; a code-length or literal/length code that is over-subscribed or incomplete;
// a repeat of nothing or lengths running over HLIT + HDIST; no end-of-block code; a distance code that is over-subscribed, or
// incomplete other than by having one code of length 1 or none (zlib's rules).
static __device__ bool block_tables(Bits& b, unsigned btype, Tables& tb) {
  if (btype == 1u) {
    for (int s = threadIdx.x; s < LL_MAX + D_MAX; s += WAVE) {
      tb.lens[s] = (unsigned char)(s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : s < LL_MAX ? 8 : s < LL_MAX + D_VALID ? 5 : 0);
    }
    wave_sync();
  } else {
    const int hlit = (int)b.take(5) + 257, hdist = (int)b.take(5) + 1, hclen = (int)b.take(4) + 4;
    if (hlit > LL_VALID || hdist > D_VALID) return false;
    for (int s = threadIdx.x; s < LL_MAX + D_MAX; s += WAVE) tb.lens[s] = 0;
    wave_sync();
    for (int k = 0; k < hclen; ++k) {
      // 16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15
      const int s = k < 3 ? 16 + k : k == 3 ? 0 : (k & 1) ? 8 - (k - 3) / 2 : 8 + (k - 4) / 2;
      b.refill();
      tb.lens[s] = (unsigned char)b.take(3);
    }
    wave_sync();
    if (build_code(tb.lens, CL_SYMS, tb.cl_count, tb.cl_sym, tb.offs) != 0) return false;       // (zlib: this code is complete)
    // the hlit + hdist lengths are one sequence (a repeat may cross from one code into the other): staged in the words of the
    // first-level table, which is filled later, because lens still holds the code-length code while they are read
    const int total = hlit + hdist;
    int at = 0, prev = -1;
    for (int guard = 0; at < total && guard < LL_MAX + D_MAX; ++guard) {
      b.refill();
      const int s = decode_slow(b, tb.cl_count, tb.cl_sym, CL_BITS);
      if (s < 0) return false;
      int rep = 1, val = s;
      if (s == 16) {
        if (prev < 0) return false;
        rep = 3 + (int)b.take(2), val = prev;
      } else if (s == 17) {
        rep = 3 + (int)b.take(3), val = 0;
      } else if (s == 18) {
        rep = 11 + (int)b.take(7), val = 0;
      }
      if (at + rep > total) return false;
      for (int i = 0; i < rep; ++i, ++at) tb.fast[at] = (unsigned short)val;             // (at < total <= 316 < FAST)
      prev = val;
      wave_sync();
    }
    if (at != total) return false;
    // the literal/length lengths go to lens[0, hlit), the distance lengths to lens[LL_MAX, LL_MAX + hdist)
    for (int s = threadIdx.x; s < LL_MAX + D_MAX; s += WAVE) {
      const int from = s < LL_MAX ? (s < hlit ? s : -1) : (s - LL_MAX < hdist ? hlit + (s - LL_MAX) : -1);
      tb.lens[s] = (unsigned char)(from >= 0 ? tb.fast[from] : 0);
    }
    wave_sync();
    if (tb.lens[256] == 0) return false;           // no end-of-block code
  }

  // the two codes: literal/length complete, distance complete or a single code of length 1 or none at all (zlib's rule)
  if (build_code(tb.lens, LL_MAX, tb.ll_count, tb.ll_sym, tb.offs) != 0) return false;
  const int dleft = build_code(tb.lens + LL_MAX, D_MAX, tb.d_count, tb.d_sym, tb.offs);
  if (dleft < 0) return false;
  if (dleft > 0) {
    int codes = 0;
    for (int l = 1; l <= MAX_BITS; ++l) codes += tb.d_count[l];
    if (!(codes == 0 || (codes == 1 && tb.d_count[1] == 1) || btype == 1u)) return false;        // (the fixed code has 30 of 32)
  }
  fill_fast(tb);
  return true;
}

}  // namespace inflate_bits
}  // namespace e2e
