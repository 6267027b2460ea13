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
#include "e2e_inflate_bits.h"

#include <cstdint>

namespace {

using e2e::deflate::CHUNK;
using e2e::deflate::MAX_DISTANCE;
using e2e::deflate::STORED_EXTRA;

using namespace e2e::inflate_bits;             // the bit reader and the canonical-code helpers (shared with inflate_any.hip)

constexpr int RECORD_WORDS = 8;
constexpr int FRONT = 16;                          // the chunk's image begins 16 bytes into its LDS buffer: the 8 bytes in front of
                                                   // the record sit right before it and the image stays aligned for 16-byte reads
constexpr unsigned DEP_VALUE = 0xFu;               // a nibble of the tail descriptor: 0..7 = that byte of the previous tail

static_assert(MAX_DISTANCE == 8 && FRONT >= MAX_DISTANCE && FRONT % 16 == 0, "the tail is 8 bytes");

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

  if (!block_tables(b, btype, tb)) return false;

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
