// N8: inflate on the device what deflate.hip wrote.  The stream is a sequence of byte-aligned chunk records (e2e_hip.h, N5 / N5b):
// one stored block, or one fixed / dynamic Huffman block closed by an empty stored block, every match of a record at one distance
// d of 1, 2, 4 or 8, and nothing needed from outside the record but the 8 bytes in front of it.  Records are therefore parsed
// independently, one wave each; no wave waits for another.
//
//   e2e_inflate_scan    parses one record at every candidate offset and writes a fixed-size entry: status, kind, d, how far the
//                       record reads in front of itself, output length, end offset, and a descriptor of its last 8 output bytes
//                       (a value, or "byte j of the 8 bytes in front of the record").  No output byte is written.
//   e2e_inflate_chunks  parses record k of the resolved chain again, trusting nothing of the scan, into an LDS image of the chunk
//                       that begins with the 8 bytes the host resolved for it, and stores the image with 16-byte vectors.
//
// One parser (parse_record) serves both; they differ in the sink the tokens go to.  All 64 lanes of the wave run the parser on the
// same values (the stream's bytes and the LDS tables read as broadcasts), so control flow is uniform and the serial parts need no
// lane 0: every lane writes the same value to the same LDS address.  The lanes split only the work that has a width: clearing
// and filling the first-level table, the bytes of a match (out[p + i] = out[p - d + i mod d], 64 at a time), the stored payload
// and the final stores.
//
// Every loop is bounded by CHUNK output bytes or by the sizes of the code tables; bytes behind ncomp read as zero and a record that
// ends behind ncomp is invalid, so nothing is read or written outside the buffers whatever the input holds.  A corrupt stream is
// a status word.
#include "e2e_common.h"
#include "e2e_deflate.h"

#include <cstdint>

namespace {

using e2e::deflate::CHUNK;
using e2e::deflate::MAX_DISTANCE;
using e2e::deflate::STORED_EXTRA;

constexpr int WAVE = 64;
constexpr int MAX_BITS = 15;
constexpr int FAST_BITS = 10, FAST = 1 << FAST_BITS;          // first-level lookup of the literal/length code
constexpr int LL_MAX = 288, LL_VALID = 286, D_MAX = 32, D_VALID = 30, CL_SYMS = 19, CL_BITS = 7;
constexpr int RECORD_WORDS = 8;
constexpr int FRONT = 16;                          // the chunk's image begins 16 bytes into its LDS buffer: the 8 bytes in front of
                                                   // the record sit right before it and the image stays aligned for 16-byte reads
constexpr unsigned DEP_VALUE = 0xFu;               // a nibble of the tail descriptor: 0..7 = that byte of the previous tail

static_assert(MAX_DISTANCE == 8 && FRONT >= MAX_DISTANCE && FRONT % 16 == 0, "the tail is 8 bytes");

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
};

struct Tables {
  unsigned short fast[FAST];                       // symbol | length << 9; 0: longer than FAST_BITS (or no such code)
  unsigned short ll_sym[LL_MAX], d_sym[D_MAX], cl_sym[CL_SYMS + 1];       // symbols in the order of (length, symbol)
  unsigned short ll_count[MAX_BITS + 1], d_count[MAX_BITS + 1], cl_count[MAX_BITS + 1], offs[MAX_BITS + 1];
  unsigned char lens[LL_MAX + D_MAX];
};

// canonical code of n lengths: count per length and the symbols in order (every lane, the same values).  Returns what is left of
// the code space: < 0 over-subscribed (nothing else is built then), 0 complete, > 0 incomplete.
__device__ int build_code(const unsigned char* lens, int n, unsigned short* count, unsigned short* sym, unsigned short* offs) {
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
__device__ void fill_fast(Tables& tb) {
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

// ---- the two sinks ----------------------------------------------------------------------------------------------------------------
// scan: a window over the last 8 output bytes, each a value or a byte of the previous tail
struct TailSink {
  unsigned long long vals;                         // byte i: the value of window entry i (0 where it depends)
  unsigned deps;                                   // nibble i: DEP_VALUE, or j = "byte j of the 8 bytes in front of the record"

  __device__ __forceinline__ void push(unsigned v, unsigned dep) {
    vals = (vals >> 8) | ((unsigned long long)v << 56);
    deps = (deps >> 4) | (dep << 28);
  }
  __device__ __forceinline__ void literal(int, unsigned v) { push(v, DEP_VALUE); }
  // every byte of a match copies the entry d back; after 8 of them the window has the period d and d more change nothing
  __device__ __forceinline__ void match(int, int len, int d) {
    const int shifts = len < 8 ? len : 8 + ((len - 8) & (d - 1));
    for (int i = 0; i < shifts; ++i) push((unsigned)(vals >> (8 * (8 - d))) & 0xFFu, (deps >> (4 * (8 - d))) & 0xFu);
  }
  __device__ __forceinline__ void stored(const unsigned char* payload, int len) {
    const int m = len < 8 ? len : 8;
    for (int i = 0; i < m; ++i) push(payload[len - m + i], DEP_VALUE);
  }
};

// chunks: the LDS image of the chunk
struct ImageSink {
  unsigned char* img;                              // img[-8 .. 0) are the bytes in front of the record

  __device__ __forceinline__ void literal(int pos, unsigned v) {
    img[pos] = (unsigned char)v;
    wave_sync();
  }
  __device__ __forceinline__ void match(int pos, int len, int d) {
    for (int i = threadIdx.x; i < len; i += WAVE) img[pos + i] = img[pos - d + (i & (d - 1))];      // (reads only in front of pos)
    wave_sync();
  }
  __device__ __forceinline__ void stored(const unsigned char* payload, int len) {
    for (int i = 4 * (int)threadIdx.x; i < len; i += 4 * WAVE) {
      unsigned v = 0;
      if (i + 4 <= len) {
        __builtin_memcpy(&v, payload + i, 4);
      } else {
        for (int k = 0; i + k < len; ++k) v |= (unsigned)payload[i + k] << (8 * k);
      }
      *(unsigned*)(img + i) = v;                   // (the image has CHUNK bytes, a multiple of 4)
    }
    wave_sync();
  }
};

struct Parsed {
  int kind, d, reach, outlen;
  long long end;
};

// One chunk record at comp[start...).  false: invalid (e2e_hip.h lists the reasons).
template <typename Sink>
__device__ bool parse_record(const unsigned char* __restrict__ comp, long long ncomp, long long start, Tables& tb, Sink& sink,
                             Parsed& out) {
  out = Parsed{0, 0, 0, 0, 0};
  if (start < 0 || start >= ncomp) return false;
  Bits b{comp, ncomp, start, 0ull, 0};
  b.refill();
  if (b.take(1) != 0u) return false;               // BFINAL
  const unsigned btype = b.take(2);
  if (btype == 3u) return false;
  out.kind = (int)btype;

  if (btype == 0u) {
    b.align();
    b.refill();
    const unsigned len = b.take(16), nlen = b.take(16);
    if (len != (~nlen & 0xFFFFu) || len == 0u || len > (unsigned)CHUNK) return false;
    const long long payload = start + STORED_EXTRA;
    if (payload + (long long)len > ncomp) return false;
    sink.stored(comp + payload, (int)len);
    out.outlen = (int)len, out.end = payload + len;
    return true;
  }

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

  int pos = 0;
  for (int guard = 0; guard <= CHUNK; ++guard) {   // (every round but the last adds a byte)
    b.refill();
    const unsigned e = tb.fast[(unsigned)b.buf & (FAST - 1)];
    int sym;
    if (e) {
      sym = (int)(e & 0x1FFu);
      b.drop((int)(e >> 9));
    } else {
      sym = decode_slow(b, tb.ll_count, tb.ll_sym, MAX_BITS);
      if (sym < 0) return false;
    }
    if (sym < 256) {
      if (pos >= CHUNK) return false;
      sink.literal(pos, (unsigned)sym);
      ++pos;
      continue;
    }
    if (sym == 256) {
      // the closing block: BFINAL 0, BTYPE 00, padding, LEN 0000, NLEN FFFF
      b.refill();
      if (b.take(3) != 0u) return false;
      b.align();
      b.refill();
      const unsigned len = b.take(16), nlen = b.take(16);
      if (len != 0u || nlen != 0xFFFFu) return false;
      out.end = b.byte_pos();
      out.outlen = pos;
      return pos > 0 && out.end <= ncomp;
    }
    if (sym >= LL_VALID) return false;
    int len;
    if (sym < 265) {
      len = sym - 254;
    } else if (sym == 285) {
      len = 258;
    } else {
      const int eb = (sym - 261) >> 2;
      len = 3 + ((4 + ((sym - 261) & 3)) << eb) + (int)b.take(eb);
    }
    b.refill();
    const int dc = decode_slow(b, tb.d_count, tb.d_sym, MAX_BITS);
    if (dc < 0 || dc >= D_VALID) return false;
    int d;
    if (dc == 0) d = 1;
    else if (dc == 1) d = 2;
    else if (dc == 3) d = 4;
    else if (dc == 5 && b.take(1) == 1u) d = 8;
    else return false;
    if (out.d != 0 && out.d != d) return false;
    out.d = d;
    if (pos + len > CHUNK) return false;
    if (pos < d && d - pos > out.reach) out.reach = d - pos;
    sink.match(pos, len, d);
    pos += len;
  }
  return false;
}

__global__ __launch_bounds__(WAVE) void inflate_scan_kernel(const unsigned char* __restrict__ comp, long long ncomp,
                                                            const long long* __restrict__ starts, long long nstarts,
                                                            unsigned* __restrict__ records) {
  __shared__ Tables tb;
  const long long c = blockIdx.x;
  if (c >= nstarts) return;
  TailSink sink{0ull, 0x76543210u};                // nothing written yet: entry i is byte i in front of the record
  Parsed p;
  const bool ok = parse_record(comp, ncomp, starts[c], tb, sink, p);
  if (threadIdx.x == 0) {
    unsigned* r = records + c * RECORD_WORDS;
    r[0] = ok ? 0u : 1u;
    r[1] = ok ? (unsigned)p.kind | ((unsigned)p.d << 8) | ((unsigned)p.reach << 16) : 0u;
    r[2] = ok ? (unsigned)p.outlen : 0u;
    r[3] = ok ? (unsigned)((unsigned long long)p.end & 0xFFFFFFFFull) : 0u;
    r[4] = ok ? (unsigned)((unsigned long long)p.end >> 32) : 0u;
    r[5] = ok ? (unsigned)(sink.vals & 0xFFFFFFFFull) : 0u;
    r[6] = ok ? (unsigned)(sink.vals >> 32) : 0u;
    r[7] = ok ? sink.deps : 0u;
  }
}

__global__ __launch_bounds__(WAVE) void inflate_chunks_kernel(const unsigned char* __restrict__ comp, long long ncomp,
                                                              const long long* __restrict__ starts,
                                                              const unsigned char* __restrict__ prev_tails, long long nchunks,
                                                              unsigned char* __restrict__ out, long long nbytes,
                                                              unsigned* __restrict__ status) {
  __shared__ Tables tb;
  __shared__ __attribute__((aligned(16))) unsigned char buf[FRONT + CHUNK];
  typedef unsigned uvec __attribute__((ext_vector_type(4)));
  const long long k = blockIdx.x;
  if (k >= nchunks) return;
  const int lane = threadIdx.x;
  const long long o0 = k * CHUNK;
  const int expect = (int)(nbytes - o0 < CHUNK ? nbytes - o0 : CHUNK);
  if (lane < MAX_DISTANCE) buf[FRONT - MAX_DISTANCE + lane] = prev_tails[k * MAX_DISTANCE + lane];
  wave_sync();
  ImageSink sink{buf + FRONT};
  Parsed p;
  const bool ok = parse_record(comp, ncomp, starts[k], tb, sink, p);
  if (!ok || p.outlen != expect || expect <= 0 || (k == 0 && p.reach > 0)) {
    if (lane == 0) atomicAdd(status, 1u);
    return;
  }
  wave_sync();
  const int vecs = expect / 16;
  for (int i = lane; i < vecs; i += WAVE) *(uvec*)(out + o0 + 16 * i) = *(const uvec*)(buf + FRONT + 16 * i);
  const int i = vecs * 16 + lane;
  if (i < expect) out[o0 + i] = buf[FRONT + i];
}

__global__ void inflate_status_zero_kernel(unsigned* status) { *status = 0u; }

}  // namespace

extern "C" int e2e_inflate_record_words(void) { return RECORD_WORDS; }

extern "C" int e2e_inflate_scan(const unsigned char* comp, long long ncomp, const long long* starts, long long nstarts,
                                unsigned* records, void* stream) {
  const char* what = "inflate_scan";
  E2E_REQUIRE(ncomp >= 0 && ncomp <= (1ll << 38), "%s: %lld compressed bytes, at most 2^38", what, ncomp);
  E2E_REQUIRE(nstarts >= 0 && nstarts <= (1ll << 26), "%s: %lld candidates, at most 2^26", what, nstarts);
  if (nstarts == 0) return E2E_OK;
  E2E_REQUIRE(starts && records && (comp || ncomp == 0), "%s: null pointer", what);
  E2E_REQUIRE((uintptr_t)starts % 8 == 0 && (uintptr_t)records % 4 == 0, "%s: starts or records is not aligned", what);
  hipLaunchKernelGGL(inflate_scan_kernel, dim3((unsigned)nstarts), dim3(WAVE), 0, (hipStream_t)stream, comp, ncomp, starts, nstarts,
                     records);
  return e2e::check_launch("inflate_scan_kernel");
}

extern "C" int e2e_inflate_chunks(const unsigned char* comp, long long ncomp, const long long* starts,
                                  const unsigned char* prev_tails, long long nchunks, unsigned char* out, long long nbytes,
                                  unsigned* status, void* stream) {
  const char* what = "inflate_chunks";
  const hipStream_t st = (hipStream_t)stream;
  E2E_REQUIRE(ncomp >= 0 && ncomp <= (1ll << 38), "%s: %lld compressed bytes, at most 2^38", what, ncomp);
  E2E_REQUIRE(nbytes >= 0 && nbytes <= (1ll << 37), "%s: %lld bytes, at most 2^37", what, nbytes);
  E2E_REQUIRE(nchunks == e2e::cdivll(nbytes, CHUNK), "%s: %lld records for %lld bytes, not %lld", what, nchunks, nbytes,
              e2e::cdivll(nbytes, CHUNK));
  E2E_REQUIRE(status != nullptr, "%s: null pointer", what);
  hipLaunchKernelGGL(inflate_status_zero_kernel, dim3(1), dim3(1), 0, st, status);
  int rc = e2e::check_launch("inflate_status_zero_kernel");
  if (rc != E2E_OK || nchunks == 0) return rc;
  E2E_REQUIRE(comp && starts && prev_tails && out, "%s: null pointer", what);
  E2E_REQUIRE((uintptr_t)out % 16 == 0, "%s: out at %p is not aligned to 16 bytes", what, (const void*)out);
  E2E_REQUIRE((uintptr_t)starts % 8 == 0, "%s: starts at %p is not aligned to 8 bytes", what, (const void*)starts);
  hipLaunchKernelGGL(inflate_chunks_kernel, dim3((unsigned)nchunks), dim3(WAVE), 0, st, comp, ncomp, starts, prev_tails, nchunks, out,
                     nbytes, status);
  return e2e::check_launch("inflate_chunks_kernel");
}
