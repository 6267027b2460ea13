// N9: inflate any raw DEFLATE stream (RFC 1951) on the device.  One stream is serial only for whoever insists on knowing the 32 KiB
// window before starting.  Here the stream is cut where dynamic blocks start, every span is decoded at once into 16-bit symbols -- a
// byte, or "byte j of the 32 KiB in front of this span" --, the windows are handed down the chain of spans, and the markers are
// replaced (the scheme of pugz and rapidgzip).
//
//   e2e_inflate_find         one wave per segment of S compressed bytes: the first bit position in the segment at which a non-final
//                            dynamic block header is valid, 64 positions at a time, one per lane, the lowest accepted lane wins.
//   e2e_inflate_spans_count  one wave per start: parses whole blocks until the next start (or the final block at the stream's end)
//                            and writes a record: status, end bit, output length.  No output, no window.
//   e2e_inflate_spans_write  the same parse into 16-bit symbols; the span's last 32 Ki symbols stay in an LDS ring for its matches.
//   e2e_inflate_windows      one workgroup walks the spans in order: win_k = the 32 KiB in front of span k, two LDS buffers.
//   e2e_inflate_resolve      out[i] = sym[i] or win_k(i)[marker], 16 bytes per thread.
//
// One parser (parse_span) serves count and write; they differ in the sink.  Every loop is bounded by a launch argument or a table
// size: the symbol loop by 8 max_span_bytes + 64 rounds (a symbol takes a bit at least), the find loop by S / 8 rounds.  Bytes behind
// n read as zero, every output index is checked against the span's own range before the store: a bad stream is a status.
#include "e2e_common.h"
#include "e2e_inflate_bits.h"

#include <cstdint>

namespace {

using namespace e2e::inflate_bits;

constexpr int W = 32768;                           // DEFLATE's window
constexpr int RECORD_WORDS = 8;
constexpr unsigned MARKER = 0x8000u;
constexpr int WIN_THREADS = 1024, WIN_PER_THREAD = W / WIN_THREADS;
constexpr int RESOLVE_THREADS = 256;

// word 0 of a span record (include/e2e_hip.h lists them)
enum Status {
  ST_OK = 0, ST_BTYPE = 1, ST_HEADER = 2, ST_NO_SYMBOL = 3, ST_SYMBOL = 4, ST_DISTANCE = 5, ST_STORED = 6, ST_FINAL = 7, ST_BEHIND = 8,
  ST_OVERSHOOT = 9, ST_CAP = 10, ST_LENGTH = 11, ST_REACH = 12, ST_START = 13
};

// ---- find: the header check, one lane per bit position, no table but 19 bytes of LDS per lane ---------------------------------------
// pos: a non-final dynamic block header is valid there (the rules of block_tables, zlib's own)
__device__ bool header_valid(const unsigned char* __restrict__ comp, long long n, long long pos, unsigned char* cl_sym) {
  Bits b = bits_at(comp, n, pos);                  // 25 bits at least
  const unsigned head = (unsigned)b.buf;
  if ((head & 7u) != 4u) return false;             // BFINAL 0, BTYPE 10
  const int hlit = (int)((head >> 3) & 31u) + 257, hdist = (int)((head >> 8) & 31u) + 1, hclen = (int)((head >> 13) & 15u) + 4;
  if (hlit > LL_VALID || hdist > D_VALID) return false;
  b.drop(17);
  // the code-length code: 3 bits per symbol in one register, the count per length in another, Kraft's sum in units of 2^-7
  unsigned long long cl = 0ull, counts = 0ull;
  int kraft = 0;
  for (int k = 0; k < hclen; ++k) {
    const int s = k < 3 ? 16 + k : k == 3 ? 0 : (k & 1) ? 8 - (k - 3) / 2 : 8 + (k - 4) / 2;
    b.refill();
    const unsigned l = b.take(3);
    cl |= (unsigned long long)l << (3 * s);
    if (l) {
      counts += 1ull << (8 * l);
      kraft += 128 >> l;
    }
  }
  if (kraft != 128) return false;
  int idx = 0;
  for (int l = 1; l <= CL_BITS; ++l) {
    for (int s = 0; s < CL_SYMS; ++s) {
      if ((int)((cl >> (3 * s)) & 7ull) == l) cl_sym[idx++] = (unsigned char)s;      // (idx <= 19)
    }
  }
  // the hlit + hdist lengths: only Kraft's sums of the two codes (units of 2^-15) and whether 256 has a code
  const int total = hlit + hdist;
  int at = 0, prev = 0, ll_sum = 0, d_sum = 0, d_codes = 0, d_ones = 0;
  bool has_end = false;
  for (int guard = 0; at < total && guard < LL_MAX + D_MAX; ++guard) {
    b.refill();
    unsigned bits = (unsigned)b.buf;
    int code = 0, first = 0, index = 0, s = -1;
    for (int len = 1; len <= CL_BITS; ++len) {
      code |= (int)(bits & 1u);
      bits >>= 1;
      const int c = (int)((counts >> (8 * len)) & 0xFFull);
      if (code - c < first) {
        b.drop(len);
        s = cl_sym[index + (code - first)];
        break;
      }
      index += c, first = (first + c) << 1, code <<= 1;
    }
    if (s < 0) return false;
    int rep = 1, val = s;
    if (s == 16) {
      if (at == 0) return false;
      rep = 3 + (int)b.take(2), val = prev;
    } else if (s == 17) {
      rep = 3 + (int)b.take(3), val = 0;
    } else if (s == 18) {
      rep = 11 + (int)b.take(7), val = 0;
    }
    if (at + rep > total) return false;
    if (val) {
      const int in_ll = at >= hlit ? 0 : (at + rep <= hlit ? rep : hlit - at), in_d = rep - in_ll;
      ll_sum += in_ll * (32768 >> val);
      d_sum += in_d * (32768 >> val);
      d_codes += in_d;
      if (val == 1) d_ones += in_d;
      if (at <= 256 && 256 < at + in_ll) has_end = true;
    }
    at += rep;
    prev = val;
  }
  if (at != total || !has_end || ll_sum != 32768 || d_sum > 32768) return false;
  if (d_sum < 32768 && !(d_codes == 0 || (d_codes == 1 && d_ones == 1))) return false;
  return b.bit_pos() <= 8 * n;
}

__global__ __launch_bounds__(WAVE) void inflate_find_kernel(const unsigned char* __restrict__ comp, long long n, long long seg_bytes,
                                                            long long nseg, long long* __restrict__ starts) {
  __shared__ unsigned char cl_sym[WAVE][CL_SYMS + 1];
  const long long s = (long long)blockIdx.x + 1;
  if (s >= nseg) return;
  const int lane = threadIdx.x;
  const long long lo = 8 * s * seg_bytes;
  const long long hi = 8 * (s + 1) * seg_bytes < 8 * n ? 8 * (s + 1) * seg_bytes : 8 * n;
  const long long rounds = e2e::cdivll(8 * seg_bytes, WAVE);
  long long found = -1;
  for (long long r = 0; r < rounds; ++r) {
    const long long p = lo + r * WAVE + lane;
    const bool ok = p < hi && header_valid(comp, n, p, cl_sym[lane]);
    const unsigned long long mask = __ballot(ok);
    if (mask) {                                    // positions are accepted in ascending order: the lowest lane of the first round
      found = lo + r * WAVE + (__ffsll((long long)mask) - 1);
      break;
    }
  }
  if (lane == 0) starts[s] = found;
}

// ---- spans: one parser, two sinks -------------------------------------------------------------------------------------------------
struct CountSink {
  __device__ __forceinline__ void literal(long long, unsigned) {}
  __device__ __forceinline__ bool match(long long, int, int) { return true; }
  __device__ __forceinline__ void stored(const unsigned char*, int, long long) {}
};

// symbols to sym[0, len) (the span's own part of the buffer), the last W of them also in the LDS ring
struct SymbolSink {
  unsigned short* ring;                            // W entries: symbol q of the span lies at q mod W while p - W <= q < p
  unsigned short* __restrict__ sym;
  long long off;                                   // the span's absolute output position

  __device__ __forceinline__ void literal(long long p, unsigned v) {
    ring[p & (W - 1)] = (unsigned short)v;
    if (threadIdx.x == 0) sym[p] = (unsigned short)v;
    wave_sync();
  }
  // out[p + i] = out[p - d + i mod d]; a source in front of the span is the marker of that byte of the window.  Every source lies in
  // front of p, and its ring slot is rewritten by the lane that reads it (d = W) or by a later lane or round, never by an earlier one.
  __device__ __forceinline__ bool match(long long p, int len, int d) {
    if (off + p - d < 0) return false;             // in front of the first byte of the output
    for (int base = 0; base < len; base += WAVE) {
      const int i = base + (int)threadIdx.x;
      if (i < len) {
        const long long q = p - d + (d >= len ? i : i % d);
        const unsigned short v = q < 0 ? (unsigned short)(MARKER | (unsigned)(W + q)) : ring[q & (W - 1)];
        ring[(p + i) & (W - 1)] = v;
        sym[p + i] = v;
      }
      wave_sync();
    }
    return true;
  }
  __device__ __forceinline__ void stored(const unsigned char* payload, int len, long long p) {
    for (int i = threadIdx.x; i < len; i += WAVE) {
      const unsigned short v = payload[i];
      ring[(p + i) & (W - 1)] = v;
      sym[p + i] = v;
    }
    wave_sync();
  }
};

struct Span {
  int status, final;
  long long end, outlen;                           // end: the bit behind the last block parsed
};

// Whole blocks from bit `start` until a block ends at `next` (next < 0: until the final block, which must end in the stream's last
// byte).  At most max_out symbols go to the sink.
template <typename Sink>
__device__ void parse_span(const unsigned char* __restrict__ comp, long long n, long long start, long long next, long long max_span,
                           long long max_out, Tables& tb, Sink& sink, Span& r) {
  r = Span{ST_START, 0, 0, 0};
  if (start < 0 || start >= 8 * n) return;
  Bits b = bits_at(comp, n, start);
  const long long limit = 8 * max_span + 64;       // rounds of the two loops together: a block or a symbol each, a bit at least
  long long rounds = 0, p = 0;
#define SPAN_FAIL(code)        \
  do {                         \
    r = Span{(code), 0, 0, 0}; \
    return;                    \
  } while (0)
  while (true) {
    if (++rounds > limit) SPAN_FAIL(ST_CAP);
    b.refill();
    const unsigned final = b.take(1), btype = b.take(2);
    if (btype == 3u) SPAN_FAIL(ST_BTYPE);
    if (final && next >= 0) SPAN_FAIL(ST_FINAL);
    if (btype == 0u) {
      b.align();
      b.refill();
      const unsigned len = b.take(16), nlen = b.take(16);
      if (len != (~nlen & 0xFFFFu)) SPAN_FAIL(ST_STORED);
      const long long payload = b.byte_pos();
      if (payload + (long long)len > n) SPAN_FAIL(ST_BEHIND);
      if (p + (long long)len > max_out) SPAN_FAIL(ST_LENGTH);
      sink.stored(comp + payload, (int)len, p);
      p += len;
      b = bits_at(comp, n, 8 * (payload + (long long)len));
    } else {
      if (!block_tables(b, btype, tb)) SPAN_FAIL(ST_HEADER);
      while (true) {
        if (++rounds > limit) SPAN_FAIL(ST_CAP);
        b.refill();
        const unsigned e = tb.fast[(unsigned)b.buf & (FAST - 1)];
        int sym;
        if (e) {
          sym = (int)(e & 0x1FFu);
          b.drop((int)(e >> 9));
        } else {
          sym = decode_slow(b, tb.ll_count, tb.ll_sym, MAX_BITS);
          if (sym < 0) SPAN_FAIL(ST_NO_SYMBOL);
        }
        if (sym < 256) {
          if (p >= max_out) SPAN_FAIL(ST_LENGTH);
          sink.literal(p, (unsigned)sym);
          ++p;
          continue;
        }
        if (sym == 256) break;
        if (sym >= LL_VALID) SPAN_FAIL(ST_SYMBOL);
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
        if (dc < 0) SPAN_FAIL(ST_NO_SYMBOL);
        if (dc >= D_VALID) SPAN_FAIL(ST_DISTANCE);
        int d = dc + 1;
        if (dc >= 4) {
          const int eb = (dc >> 1) - 1;            // <= 13
          d = 1 + ((2 + (dc & 1)) << eb) + (int)b.take(eb);
        }
        if (p + len > max_out) SPAN_FAIL(ST_LENGTH);
        if (!sink.match(p, len, d)) SPAN_FAIL(ST_REACH);
        p += len;
      }
    }
    const long long at = b.bit_pos();
    if (at > 8 * n) SPAN_FAIL(ST_BEHIND);
    if (at - start > 8 * max_span) SPAN_FAIL(ST_CAP);
    if (final) {
      if ((at + 7) / 8 != n) SPAN_FAIL(ST_FINAL);
      r = Span{ST_OK, 1, at, p};
      return;
    }
    if (next >= 0 && at == next) {
      r = Span{ST_OK, 0, at, p};
      return;
    }
    if (next >= 0 && at > next) SPAN_FAIL(ST_OVERSHOOT);
  }
#undef SPAN_FAIL
}

__global__ __launch_bounds__(WAVE) void inflate_spans_count_kernel(const unsigned char* __restrict__ comp, long long n,
                                                                   const long long* __restrict__ starts, long long m,
                                                                   long long max_span, unsigned* __restrict__ records) {
  __shared__ Tables tb;
  const long long k = blockIdx.x;
  if (k >= m) return;
  CountSink sink;
  Span r;
  parse_span(comp, n, starts[k], k + 1 < m ? starts[k + 1] : -1ll, max_span, 0x7FFFFFFFFFFFFFFFll, tb, sink, r);
  if (threadIdx.x == 0) {
    unsigned* w = records + k * RECORD_WORDS;
    w[0] = (unsigned)r.status, w[1] = (unsigned)r.final;
    w[2] = (unsigned)((unsigned long long)r.end & 0xFFFFFFFFull), w[3] = (unsigned)((unsigned long long)r.end >> 32);
    w[4] = (unsigned)((unsigned long long)r.outlen & 0xFFFFFFFFull), w[5] = (unsigned)((unsigned long long)r.outlen >> 32);
    w[6] = 0u, w[7] = 0u;
  }
}

__global__ __launch_bounds__(WAVE) void inflate_spans_write_kernel(const unsigned char* __restrict__ comp, long long n,
                                                                   const long long* __restrict__ starts,
                                                                   const long long* __restrict__ offs, long long m, long long max_span,
                                                                   unsigned short* __restrict__ sym, long long nbytes,
                                                                   unsigned* __restrict__ status) {
  __shared__ Tables tb;
  extern __shared__ __attribute__((aligned(16))) unsigned short ring[];           // W entries
  const long long k = blockIdx.x;
  if (k >= m) return;
  const long long off = offs[k], len = offs[k + 1] - off;
  bool ok = off >= 0 && len >= 0 && off + len <= nbytes;                          // (nothing of the host's is trusted to be in range)
  if (ok) {
    SymbolSink sink{ring, sym + off, off};
    Span r;
    parse_span(comp, n, starts[k], k + 1 < m ? starts[k + 1] : -1ll, max_span, len, tb, sink, r);
    ok = r.status == ST_OK && r.outlen == len;
  }
  if (!ok && threadIdx.x == 0) atomicAdd(status, 1u);
}

// ---- windows: win_k[j] = the byte at off_k - W + j, from win_{k-1} and the symbols of span k - 1 --------------------------------------
__global__ __launch_bounds__(WIN_THREADS) void inflate_windows_kernel(const unsigned short* __restrict__ sym,
                                                                      const long long* __restrict__ offs, long long m, long long nbytes,
                                                                      unsigned char* __restrict__ wins, unsigned* __restrict__ status) {
  __shared__ unsigned char win[2][W];
  const int t = threadIdx.x;
  for (int j = t; j < W; j += WIN_THREADS) win[0][j] = 0;                         // win_0: in front of the output, never referenced
  __syncthreads();
  unsigned bad = 0u;
  for (long long k = 1; k < m; ++k) {
    const unsigned char* before = win[(k & 1) ^ 1];
    unsigned char* cur = win[k & 1];
    const long long off = offs[k], from = offs[k - 1];
    const bool sane = from >= 0 && from <= off && off <= nbytes;
    const long long plen = sane ? off - from : 0;
    if (!sane) bad = 1u;
    unsigned short s[WIN_PER_THREAD];
#pragma unroll
    for (int i = 0; i < WIN_PER_THREAD; ++i) {     // the loads of a lane are independent: all in flight together
      const int j = t + i * WIN_THREADS;
      s[i] = (sane && (long long)j >= W - plen) ? sym[off - W + j] : (unsigned short)0;
    }
#pragma unroll
    for (int i = 0; i < WIN_PER_THREAD; ++i) {
      const int j = t + i * WIN_THREADS;
      unsigned v;
      if ((long long)j < W - plen) {
        v = before[j + plen];
      } else if (s[i] & MARKER) {
        if (k == 1) bad = 1u;                      // span 0 has nothing in front of it
        v = before[s[i] & (W - 1)];
      } else {
        v = s[i] & 0xFFu;
      }
      cur[j] = (unsigned char)v;
      wins[k * W + j] = (unsigned char)v;
    }
    __syncthreads();
  }
  if (bad) atomicAdd(status, 1u);
}

// ---- resolve: 16 output bytes per thread -----------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned resolve_one(unsigned s, long long i, const long long* __restrict__ offs, long long m,
                                                const unsigned char* __restrict__ wins, unsigned& bad) {
  if (!(s & MARKER)) return s & 0xFFu;
  long long lo = 0, hi = m;                        // the last span k with offs[k] <= i (offs[0] = 0)
  for (int round = 0; round < 40 && hi - lo > 1; ++round) {
    const long long mid = (lo + hi) >> 1;
    if (offs[mid] <= i) lo = mid;
    else hi = mid;
  }
  if (lo == 0) {
    bad = 1u;
    return 0u;
  }
  return wins[lo * W + (s & (W - 1))];
}

__global__ __launch_bounds__(RESOLVE_THREADS) void inflate_resolve_kernel(const unsigned short* __restrict__ sym,
                                                                          const long long* __restrict__ offs, long long m,
                                                                          const unsigned char* __restrict__ wins,
                                                                          unsigned char* __restrict__ out, long long nbytes,
                                                                          unsigned* __restrict__ status) {
  typedef unsigned uvec __attribute__((ext_vector_type(4)));
  const long long i0 = 16 * ((long long)blockIdx.x * RESOLVE_THREADS + threadIdx.x);
  if (i0 >= nbytes) return;
  unsigned bad = 0u;
  if (i0 + 16 <= nbytes) {
    const uvec a = *(const uvec*)(sym + i0), b = *(const uvec*)(sym + i0 + 8);
    const unsigned w[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    unsigned o[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const unsigned w0 = w[2 * q], w1 = w[2 * q + 1];
      if (((w0 | w1) & 0x80008000u) == 0u) {
        o[q] = (w0 & 0xFFu) | ((w0 >> 8) & 0xFF00u) | ((w1 & 0xFFu) << 16) | ((w1 >> 16) << 24);
      } else {
        o[q] = resolve_one(w0 & 0xFFFFu, i0 + 4 * q, offs, m, wins, bad) | (resolve_one(w0 >> 16, i0 + 4 * q + 1, offs, m, wins, bad) << 8) |
               (resolve_one(w1 & 0xFFFFu, i0 + 4 * q + 2, offs, m, wins, bad) << 16) |
               (resolve_one(w1 >> 16, i0 + 4 * q + 3, offs, m, wins, bad) << 24);
      }
    }
    *(uvec*)(out + i0) = uvec{o[0], o[1], o[2], o[3]};
  } else {
    for (long long i = i0; i < nbytes; ++i) out[i] = (unsigned char)resolve_one(sym[i], i, offs, m, wins, bad);
  }
  if (bad) atomicAdd(status, 1u);
}

__global__ void inflate_any_status_zero_kernel(unsigned* status) { *status = 0u; }

int zero_status(unsigned* status, hipStream_t st) {
  hipLaunchKernelGGL(inflate_any_status_zero_kernel, dim3(1), dim3(1), 0, st, status);
  return e2e::check_launch("inflate_any_status_zero_kernel");
}

}  // namespace

#define INFLATE_ANY_COMMON(what, n, m)                                                                          \
  E2E_REQUIRE((n) >= 0 && (n) <= (1ll << 38), "%s: %lld compressed bytes, at most 2^38", what, (long long)(n)); \
  E2E_REQUIRE((m) >= 0 && (m) <= (1ll << 26), "%s: %lld spans, at most 2^26", what, (long long)(m))

extern "C" int e2e_inflate_any_record_words(void) { return RECORD_WORDS; }
extern "C" int e2e_inflate_any_window_bytes(void) { return W; }

extern "C" int e2e_inflate_find(const unsigned char* comp, long long n, long long segment_bytes, long long nseg, long long* starts,
                                void* stream) {
  const char* what = "inflate_find";
  E2E_REQUIRE(n >= 0 && n <= (1ll << 38), "%s: %lld compressed bytes, at most 2^38", what, n);
  E2E_REQUIRE(segment_bytes >= 16 && segment_bytes <= (1ll << 24), "%s: segments of %lld bytes, 16 .. 2^24", what, segment_bytes);
  E2E_REQUIRE(nseg == e2e::cdivll(n, segment_bytes), "%s: %lld segments for %lld bytes, not %lld", what, nseg, n,
              e2e::cdivll(n, segment_bytes));
  E2E_REQUIRE(nseg <= (1ll << 30), "%s: %lld segments, at most 2^30", what, nseg);
  if (nseg <= 1) return E2E_OK;
  E2E_REQUIRE(comp && starts, "%s: null pointer", what);
  E2E_REQUIRE((uintptr_t)starts % 8 == 0, "%s: starts at %p is not aligned to 8 bytes", what, (const void*)starts);
  hipLaunchKernelGGL(inflate_find_kernel, dim3((unsigned)(nseg - 1)), dim3(WAVE), 0, (hipStream_t)stream, comp, n, segment_bytes, nseg,
                     starts);
  return e2e::check_launch("inflate_find_kernel");
}

extern "C" int e2e_inflate_spans_count(const unsigned char* comp, long long n, const long long* starts, long long m,
                                       long long max_span_bytes, unsigned* records, void* stream) {
  const char* what = "inflate_spans_count";
  INFLATE_ANY_COMMON(what, n, m);
  E2E_REQUIRE(max_span_bytes >= 1 && max_span_bytes <= (1ll << 31), "%s: a span cap of %lld bytes, 1 .. 2^31", what, max_span_bytes);
  if (m == 0) return E2E_OK;
  E2E_REQUIRE(starts && records && (comp || n == 0), "%s: null pointer", what);
  E2E_REQUIRE((uintptr_t)starts % 8 == 0 && (uintptr_t)records % 4 == 0, "%s: starts or records is not aligned", what);
  hipLaunchKernelGGL(inflate_spans_count_kernel, dim3((unsigned)m), dim3(WAVE), 0, (hipStream_t)stream, comp, n, starts, m,
                     max_span_bytes, records);
  return e2e::check_launch("inflate_spans_count_kernel");
}

extern "C" int e2e_inflate_spans_write(const unsigned char* comp, long long n, const long long* starts, const long long* offs,
                                       long long m, long long max_span_bytes, unsigned short* sym, long long nbytes, unsigned* status,
                                       void* stream) {
  const char* what = "inflate_spans_write";
  const hipStream_t st = (hipStream_t)stream;
  INFLATE_ANY_COMMON(what, n, m);
  E2E_REQUIRE(nbytes >= 0 && nbytes <= (1ll << 37), "%s: %lld bytes, at most 2^37", what, nbytes);
  E2E_REQUIRE(max_span_bytes >= 1 && max_span_bytes <= (1ll << 31), "%s: a span cap of %lld bytes, 1 .. 2^31", what, max_span_bytes);
  E2E_REQUIRE(status != nullptr, "%s: null pointer", what);
  int rc = zero_status(status, st);
  if (rc != E2E_OK || m == 0) return rc;
  E2E_REQUIRE(starts && offs && (comp || n == 0) && (sym || nbytes == 0), "%s: null pointer", what);
  E2E_REQUIRE((uintptr_t)starts % 8 == 0 && (uintptr_t)offs % 8 == 0, "%s: starts or offs is not aligned to 8 bytes", what);
  E2E_REQUIRE((uintptr_t)sym % 16 == 0, "%s: sym at %p is not aligned to 16 bytes", what, (const void*)sym);
  // static tables + the ring: beyond the default 64 KiB (set before every launch; a process-wide flag would race)
  E2E_REQUIRE(hipFuncSetAttribute((const void*)inflate_spans_write_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                  W * (int)sizeof(unsigned short)) == hipSuccess,
              "%s: cannot raise the dynamic LDS limit", what);
  hipLaunchKernelGGL(inflate_spans_write_kernel, dim3((unsigned)m), dim3(WAVE), W * sizeof(unsigned short), st, comp, n, starts, offs, m,
                     max_span_bytes, sym, nbytes, status);
  return e2e::check_launch("inflate_spans_write_kernel");
}

extern "C" int e2e_inflate_windows(const unsigned short* sym, const long long* offs, long long m, long long nbytes, unsigned char* wins,
                                   unsigned* status, void* stream) {
  const char* what = "inflate_windows";
  const hipStream_t st = (hipStream_t)stream;
  INFLATE_ANY_COMMON(what, 0, m);
  E2E_REQUIRE(nbytes >= 0 && nbytes <= (1ll << 37), "%s: %lld bytes, at most 2^37", what, nbytes);
  E2E_REQUIRE(status != nullptr, "%s: null pointer", what);
  int rc = zero_status(status, st);
  if (rc != E2E_OK || m <= 1) return rc;
  E2E_REQUIRE(sym && offs && wins, "%s: null pointer", what);
  E2E_REQUIRE((uintptr_t)offs % 8 == 0 && (uintptr_t)sym % 16 == 0, "%s: offs or sym is not aligned", what);
  hipLaunchKernelGGL(inflate_windows_kernel, dim3(1), dim3(WIN_THREADS), 0, st, sym, offs, m, nbytes, wins, status);
  return e2e::check_launch("inflate_windows_kernel");
}

extern "C" int e2e_inflate_resolve(const unsigned short* sym, const long long* offs, long long m, const unsigned char* wins,
                                   unsigned char* out, long long nbytes, unsigned* status, void* stream) {
  const char* what = "inflate_resolve";
  const hipStream_t st = (hipStream_t)stream;
  INFLATE_ANY_COMMON(what, 0, m);
  E2E_REQUIRE(nbytes >= 0 && nbytes <= (1ll << 37), "%s: %lld bytes, at most 2^37", what, nbytes);
  E2E_REQUIRE(status != nullptr, "%s: null pointer", what);
  int rc = zero_status(status, st);
  if (rc != E2E_OK || nbytes == 0) return rc;
  E2E_REQUIRE(m >= 1 && sym && offs && out && (wins || m == 1), "%s: null pointer", what);
  E2E_REQUIRE((uintptr_t)offs % 8 == 0, "%s: offs at %p is not aligned to 8 bytes", what, (const void*)offs);
  E2E_REQUIRE((uintptr_t)sym % 16 == 0 && (uintptr_t)out % 16 == 0, "%s: sym or out is not aligned to 16 bytes", what);
  const long long groups = e2e::cdivll(nbytes, 16);
  hipLaunchKernelGGL(inflate_resolve_kernel, dim3((unsigned)e2e::cdivll(groups, RESOLVE_THREADS)), dim3(RESOLVE_THREADS), 0, st, sym, offs,
                     m, wins, out, nbytes, status);
  return e2e::check_launch("inflate_resolve_kernel");
}
