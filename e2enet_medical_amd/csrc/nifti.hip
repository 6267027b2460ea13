// N4: decoding of NIfTI-1 voxel payloads.  The host inflates a file and parses its 348-byte header (e2enet_medical_amd/nifti.py); the
// payload is uploaded as the file stores it and turned here into what the other kernels take: fp32 in a channel of a case's
// [C, Z, Y, X] tensor, or the uint8 label volume of the census and component kernels.  A pure stream: elsize bytes read per voxel,
// 4 or 1 written, 16 bytes of payload per lane and load.  Built with -ffp-contract=off: the scaling is numpy's, a fp64 multiply and
// a fp64 add, each rounded, then one rounding to fp32.
// The integrity scan (e2e_nifti_scan, below the decode) reads the same bytes through the same decode1 and writes 260 words: NaN and
// non-label counts with their first raster indices, and the 256 label counts.
#include "e2e_common.h"

#include <cstdint>

namespace {

constexpr int VEC_BYTES = 16;              // payload per lane and load
constexpr int MAX_BLOCKS = 2048;           // 256 CUs x 8 workgroups; the rest of the volume is walked with a grid stride

template <int S> struct Bits;
template <> struct Bits<1> { typedef unsigned char type; };
template <> struct Bits<2> { typedef unsigned short type; };
template <> struct Bits<4> { typedef unsigned int type; };
template <> struct Bits<8> { typedef unsigned long long type; };

__device__ __forceinline__ unsigned char bswap(unsigned char v) { return v; }
__device__ __forceinline__ unsigned short bswap(unsigned short v) { return __builtin_bswap16(v); }
__device__ __forceinline__ unsigned int bswap(unsigned int v) { return __builtin_bswap32(v); }
__device__ __forceinline__ unsigned long long bswap(unsigned long long v) { return __builtin_bswap64(v); }

// a 64-bit magnitude to fp32 with one rounding to nearest even (ndarray.astype(np.float32) of int64 / uint64), written out so that
// it does not go through fp64: the top 24 bits, the rest as the rounding remainder, an exact scaling by a power of two
__device__ __forceinline__ float u64_to_f32(unsigned long long x) {
  if (x == 0) return 0.f;
  const int lz = __builtin_clzll(x);
  const unsigned long long y = x << lz;                          // leading one at bit 63
  unsigned m = (unsigned)(y >> 40);                              // 24 bits
  const unsigned long long rem = y & ((1ull << 40) - 1), half = 1ull << 39;
  if (rem > half || (rem == half && (m & 1u))) ++m;              // (m may become 2^24: still exact as a float)
  const int e = 63 - lz - 23;                                    // the value is m * 2^e, -23 <= e <= 40
  return __fmul_rn((float)m, __builtin_bit_cast(float, (unsigned)(e + 127) << 23));
}

// one element to fp32 with one rounding (no scaling)
__device__ __forceinline__ float cvt1(unsigned char v) { return (float)v; }
__device__ __forceinline__ float cvt1(signed char v) { return (float)v; }
__device__ __forceinline__ float cvt1(short v) { return (float)v; }
__device__ __forceinline__ float cvt1(unsigned short v) { return (float)v; }
__device__ __forceinline__ float cvt1(int v) { return (float)v; }                      // v_cvt_f32_i32: nearest even
__device__ __forceinline__ float cvt1(unsigned int v) { return (float)v; }             // v_cvt_f32_u32
__device__ __forceinline__ float cvt1(float v) { return v; }                           // the bits as they are, a NaN's included
__device__ __forceinline__ float cvt1(double v) { return (float)v; }                   // v_cvt_f32_f64: nearest even
__device__ __forceinline__ float cvt1(unsigned long long v) { return u64_to_f32(v); }
__device__ __forceinline__ float cvt1(long long v) {
  const float m = u64_to_f32(v < 0 ? 0ull - (unsigned long long)v : (unsigned long long)v);
  return v < 0 ? -m : m;
}

template <typename T, bool SWAP, bool SCALE>
__device__ __forceinline__ float decode1(typename Bits<sizeof(T)>::type bits, double slope, double inter) {
  if (SWAP) bits = bswap(bits);
  const T v = __builtin_bit_cast(T, bits);
  if (SCALE) return (float)__dadd_rn(__dmul_rn((double)v, slope), inter);
  return cvt1(v);
}

// fp32 -> label byte: a whole number in [0, 255], anything else (a NaN too) is 0 and counted
__device__ __forceinline__ unsigned char label_of(float r, unsigned& bad) {
  if (r >= 0.f && r <= 255.f && r == truncf(r)) return (unsigned char)(int)r;
  ++bad;
  return 0;
}

__device__ __forceinline__ void put(float* o, float r, unsigned&) { *o = r; }
__device__ __forceinline__ void put(unsigned char* o, float r, unsigned& bad) { *o = label_of(r, bad); }

// O = float: out[i] = fp32 of element i.  O = unsigned char: the label byte, and *rejected += the elements that are none
template <typename T, bool SWAP, bool SCALE, typename O>
__global__ __launch_bounds__(256) void nifti_decode_kernel(const unsigned char* __restrict__ raw, long long nvox, double slope,
                                                           double inter, O* __restrict__ out,
                                                           unsigned long long* __restrict__ rejected) {
  typedef typename Bits<sizeof(T)>::type U;
  constexpr int PER = VEC_BYTES / (int)sizeof(T);
  typedef U uvec __attribute__((ext_vector_type(PER)));
  typedef O ovec __attribute__((ext_vector_type(PER)));
  const long long chunks = e2e::cdivll(nvox, PER);
  unsigned bad = 0;
  for (long long t = (long long)blockIdx.x * 256 + threadIdx.x; t < chunks; t += (long long)gridDim.x * 256) {
    const long long i0 = t * PER;
    if (nvox - i0 >= PER) {
      // the payload is aligned to its element size only, the output to its own: the copies state no more (gfx950 global loads
      // and stores take any alignment)
      uvec v;
      __builtin_memcpy(&v, raw + i0 * (long long)sizeof(T), sizeof(v));
      ovec o;
#pragma unroll
      for (int j = 0; j < PER; ++j) {
        O r;
        put(&r, decode1<T, SWAP, SCALE>(v[j], slope, inter), bad);
        o[j] = r;
      }
      __builtin_memcpy(out + i0, &o, sizeof(o));
    } else {
      // the last, partial vector: element by element, nothing read or written past the end
      for (long long i = i0; i < nvox; ++i) {
        U b;
        __builtin_memcpy(&b, raw + i * (long long)sizeof(T), sizeof(b));
        put(out + i, decode1<T, SWAP, SCALE>(b, slope, inter), bad);
      }
    }
  }
  if (sizeof(O) == 1) {
    // one atomic per workgroup, and only from one that rejected something: an integer sum, the same on every run.  (These four
    // words are the only LDS of the file; the fp32 kernels have none.)
    __shared__ unsigned wave_bad[4];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) bad += __shfl_xor(bad, off, 64);
    if ((threadIdx.x & 63) == 0) wave_bad[threadIdx.x >> 6] = bad;
    __syncthreads();
    if (threadIdx.x == 0) {
      const unsigned total = wave_bad[0] + wave_bad[1] + wave_bad[2] + wave_bad[3];
      if (total) atomicAdd(rejected, (unsigned long long)total);
    }
  }
}

unsigned grid_for(long long nvox, int elsize) {
  const long long blocks = e2e::cdivll(e2e::cdivll(nvox, VEC_BYTES / elsize), 256);
  return (unsigned)(blocks < MAX_BLOCKS ? blocks : MAX_BLOCKS);
}

template <typename T, typename O>
void launch(const void* raw, long long nvox, bool swap, bool scale, double slope, double inter, O* out, unsigned long long* rejected,
            hipStream_t st) {
  const dim3 grid(grid_for(nvox, (int)sizeof(T))), block(256);
  const unsigned char* p = (const unsigned char*)raw;
  swap = swap && sizeof(T) > 1;
#define E2E_NIFTI_LAUNCH(SW, SC) \
  hipLaunchKernelGGL((nifti_decode_kernel<T, SW, SC, O>), grid, block, 0, st, p, nvox, slope, inter, out, rejected)
  if (swap && scale) E2E_NIFTI_LAUNCH(true, true);
  else if (swap) E2E_NIFTI_LAUNCH(true, false);
  else if (scale) E2E_NIFTI_LAUNCH(false, true);
  else E2E_NIFTI_LAUNCH(false, false);
#undef E2E_NIFTI_LAUNCH
}

// bytes per element of a NIfTI-1 datatype code, 0 for a code that is not decoded
int elsize_of(int datatype) {
  switch (datatype) {
    case 2: case 256: return 1;                    // uint8, int8
    case 4: case 512: return 2;                    // int16, uint16
    case 8: case 768: case 16: return 4;           // int32, uint32, float32
    case 64: case 1024: case 1280: return 8;       // float64, int64, uint64
  }
  return 0;
}

template <typename O>
int decode(const char* what, const void* raw, long long nvox, int datatype, int swap, int scale, double slope, double inter, O* out,
           unsigned long long* rejected, hipStream_t st) {
  const int elsize = elsize_of(datatype);
  E2E_REQUIRE(elsize != 0, "%s: datatype %d is not one of 2, 4, 8, 16, 64, 256, 512, 768, 1024, 1280", what, datatype);
  E2E_REQUIRE(nvox >= 0, "%s: %lld voxels", what, nvox);
  E2E_REQUIRE(nvox <= (1ll << 40), "%s: %lld voxels, at most 2^40", what, nvox);
  if (nvox == 0) return E2E_OK;
  E2E_REQUIRE(raw && out, "%s: null pointer", what);
  E2E_REQUIRE((uintptr_t)raw % (uintptr_t)elsize == 0, "%s: the payload at %p is not aligned to its %d-byte elements", what, raw,
              elsize);
  const bool sw = swap != 0, sc = scale != 0;
  switch (datatype) {
    case 2: launch<unsigned char, O>(raw, nvox, sw, sc, slope, inter, out, rejected, st); break;
    case 256: launch<signed char, O>(raw, nvox, sw, sc, slope, inter, out, rejected, st); break;
    case 4: launch<short, O>(raw, nvox, sw, sc, slope, inter, out, rejected, st); break;
    case 512: launch<unsigned short, O>(raw, nvox, sw, sc, slope, inter, out, rejected, st); break;
    case 8: launch<int, O>(raw, nvox, sw, sc, slope, inter, out, rejected, st); break;
    case 768: launch<unsigned int, O>(raw, nvox, sw, sc, slope, inter, out, rejected, st); break;
    case 16: launch<float, O>(raw, nvox, sw, sc, slope, inter, out, rejected, st); break;
    case 64: launch<double, O>(raw, nvox, sw, sc, slope, inter, out, rejected, st); break;
    case 1024: launch<long long, O>(raw, nvox, sw, sc, slope, inter, out, rejected, st); break;
    case 1280: launch<unsigned long long, O>(raw, nvox, sw, sc, slope, inter, out, rejected, st); break;
  }
  return e2e::check_launch("nifti_decode_kernel");
}

// ---- the integrity scan: one pass over the stored bytes, 260 words written -------------------------------------------------------
constexpr int SCAN_WORDS = 4 + 256;        // NaN count, first NaN, non-label count, first non-label, 256 label counts
constexpr int SCAN_COPIES = 16;            // sub-histograms of a workgroup: lane l adds into copy l % 16
constexpr int SCAN_UNROLL = 4;             // vectors a lane requests before it looks at the first: the loads in flight per lane
constexpr int SCAN_MAX_BLOCKS = 1024;      // 256 CUs x 4 workgroups, each lane with SCAN_UNROLL loads in flight

__global__ void nifti_scan_init_kernel(unsigned long long* __restrict__ out) {
  for (int i = threadIdx.x; i < SCAN_WORDS; i += blockDim.x) out[i] = (i == 1 || i == 3) ? ~0ull : 0ull;
}

// What one lane has seen.  The label counts go to the workgroup's LDS histogram, run by run: a lane that keeps meeting the value
// it met last only counts, and adds the run when the value changes (and once at the end), so a volume of one value -- background --
// costs a lane one LDS atomic, not one per voxel.  Everything is an integer sum or a minimum: no order of arrival shows.
struct ScanLane {
  unsigned nan = 0, bad = 0, run = 0;
  int cur = 0;
  unsigned long long first_nan = ~0ull, first_bad = ~0ull;
  unsigned* hist;                          // this lane's copy: bin v at hist[v * SCAN_COPIES]

  __device__ __forceinline__ void flush() {
    if (run) atomicAdd(hist + cur * SCAN_COPIES, run);
    run = 0;
  }
  __device__ __forceinline__ void take(float r, long long i) {
    unsigned rejected = 0;
    const int v = label_of(r, rejected);   // the rule of decode_u8
    if (!rejected) {
      if (v != cur) {
        flush();
        cur = v;
      }
      ++run;
    } else if (r != r) {
      ++nan;
      if ((unsigned long long)i < first_nan) first_nan = (unsigned long long)i;
    } else {
      ++bad;
      if ((unsigned long long)i < first_bad) first_bad = (unsigned long long)i;
    }
  }
};

__device__ __forceinline__ unsigned long long wave_min_u64(unsigned long long v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const unsigned long long o = __shfl_xor(v, off, 64);
    v = o < v ? o : v;
  }
  return v;
}

// head: the elements in front of the first 16-byte boundary of the payload (fewer than 16 / sizeof(T), or all of a short volume);
// then `chunks` aligned 16-byte vectors, a grid stride apart, SCAN_UNROLL of them requested at a time (the kernel waits on memory,
// not on arithmetic: what counts is the loads in flight), the last fewer than SCAN_UNROLL steps of a lane one by one; then the tail.  Head and tail go element by element to the first lanes
// of workgroup 0.
template <typename T, bool SWAP, bool SCALE>
__global__ __launch_bounds__(256) void nifti_scan_kernel(const unsigned char* __restrict__ raw, long long nvox, long long head,
                                                         double slope, double inter, unsigned long long* __restrict__ out) {
  typedef typename Bits<sizeof(T)>::type U;
  constexpr int PER = VEC_BYTES / (int)sizeof(T);
  typedef U uvec __attribute__((ext_vector_type(PER)));
  __shared__ unsigned hist[256 * SCAN_COPIES];
  __shared__ unsigned long long wave_part[4][4];
  for (int i = threadIdx.x; i < 256 * SCAN_COPIES; i += 256) hist[i] = 0u;
  __syncthreads();

  ScanLane lane;
  lane.hist = hist + (threadIdx.x % SCAN_COPIES);
  const long long chunks = (nvox - head) / PER, tail0 = head + chunks * PER;
  const uvec* body = (const uvec*)(raw + head * (long long)sizeof(T));          // 16-byte aligned by the choice of head
  const long long stride = (long long)gridDim.x * 256;
  long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  for (; t + (SCAN_UNROLL - 1) * stride < chunks; t += SCAN_UNROLL * stride) {
    uvec v[SCAN_UNROLL];
#pragma unroll
    for (int k = 0; k < SCAN_UNROLL; ++k) v[k] = body[t + k * stride];
#pragma unroll
    for (int k = 0; k < SCAN_UNROLL; ++k) {
      const long long i0 = head + (t + k * stride) * PER;
#pragma unroll
      for (int j = 0; j < PER; ++j) lane.take(decode1<T, SWAP, SCALE>(v[k][j], slope, inter), i0 + j);
    }
  }
  for (; t < chunks; t += stride) {
    const uvec v = body[t];
    const long long i0 = head + t * PER;
#pragma unroll
    for (int j = 0; j < PER; ++j) lane.take(decode1<T, SWAP, SCALE>(v[j], slope, inter), i0 + j);
  }
  if (blockIdx.x == 0) {
    // (at most PER - 1 elements on either side, PER <= 16: one element per lane)
    const long long edge[2] = {threadIdx.x < head ? (long long)threadIdx.x : -1ll,
                               tail0 + threadIdx.x < nvox ? tail0 + threadIdx.x : -1ll};
    for (int k = 0; k < 2; ++k) {
      if (edge[k] < 0) continue;
      U b;
      __builtin_memcpy(&b, raw + edge[k] * (long long)sizeof(T), sizeof(b));
      lane.take(decode1<T, SWAP, SCALE>(b, slope, inter), edge[k]);
    }
  }
  lane.flush();

  // the two counts and the two first indices: wave, then workgroup, then one atomic each and only where there is something to say
  unsigned long long nan = lane.nan, bad = lane.bad;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    nan += __shfl_xor(nan, off, 64);
    bad += __shfl_xor(bad, off, 64);
  }
  const unsigned long long first_nan = wave_min_u64(lane.first_nan), first_bad = wave_min_u64(lane.first_bad);
  if ((threadIdx.x & 63) == 0) {
    unsigned long long* w = wave_part[threadIdx.x >> 6];
    w[0] = nan, w[1] = first_nan, w[2] = bad, w[3] = first_bad;
  }
  __syncthreads();                         // (also: every lane's histogram adds are done)
  if (threadIdx.x == 0) {
    unsigned long long n = 0, b = 0, fn = ~0ull, fb = ~0ull;
    for (int w = 0; w < 4; ++w) {
      n += wave_part[w][0];
      b += wave_part[w][2];
      fn = wave_part[w][1] < fn ? wave_part[w][1] : fn;
      fb = wave_part[w][3] < fb ? wave_part[w][3] : fb;
    }
    if (n) {
      atomicAdd(out + 0, n);
      atomicMin(out + 1, fn);
    }
    if (b) {
      atomicAdd(out + 2, b);
      atomicMin(out + 3, fb);
    }
  }
  // the workgroup's one flush of the histogram: lane v owns bin v (the copies read in a rotated order: 16 banks, not one)
  unsigned long long total = 0;
#pragma unroll
  for (int c = 0; c < SCAN_COPIES; ++c) total += hist[threadIdx.x * SCAN_COPIES + ((c + threadIdx.x) % SCAN_COPIES)];
  if (total) atomicAdd(out + 4 + threadIdx.x, total);
}

template <typename T>
void launch_scan(const void* raw, long long nvox, bool swap, bool scale, double slope, double inter, unsigned long long* out,
                 hipStream_t st) {
  constexpr long long PER = VEC_BYTES / (long long)sizeof(T);
  long long head = (long long)((0 - (uintptr_t)raw) % VEC_BYTES) / (long long)sizeof(T);
  if (head > nvox) head = nvox;
  // a lane takes SCAN_UNROLL vectors per step also where one workgroup is enough (workgroup 0 always runs: head and tail are its)
  long long blocks = e2e::cdivll((nvox - head) / PER, 256 * SCAN_UNROLL);
  blocks = blocks < 1 ? 1 : (blocks < SCAN_MAX_BLOCKS ? blocks : SCAN_MAX_BLOCKS);
  const dim3 grid((unsigned)blocks), block(256);
  const unsigned char* p = (const unsigned char*)raw;
  swap = swap && sizeof(T) > 1;
#define E2E_NIFTI_SCAN(SW, SC) hipLaunchKernelGGL((nifti_scan_kernel<T, SW, SC>), grid, block, 0, st, p, nvox, head, slope, inter, out)
  if (swap && scale) E2E_NIFTI_SCAN(true, true);
  else if (swap) E2E_NIFTI_SCAN(true, false);
  else if (scale) E2E_NIFTI_SCAN(false, true);
  else E2E_NIFTI_SCAN(false, false);
#undef E2E_NIFTI_SCAN
}

}  // namespace

extern "C" long long e2e_nifti_scan_grid_voxels(int datatype) {
  const int elsize = elsize_of(datatype);
  return elsize ? (long long)SCAN_MAX_BLOCKS * 256 * SCAN_UNROLL * (VEC_BYTES / elsize) : 0;
}

extern "C" int e2e_nifti_scan(const void* raw, long long nvox, int datatype, int swap, int scale, double slope, double inter,
                              unsigned long long* out, void* stream) {
  const char* what = "nifti_scan";
  const hipStream_t st = (hipStream_t)stream;
  const int elsize = elsize_of(datatype);
  E2E_REQUIRE(elsize != 0, "%s: datatype %d is not one of 2, 4, 8, 16, 64, 256, 512, 768, 1024, 1280", what, datatype);
  E2E_REQUIRE(nvox >= 0, "%s: %lld voxels", what, nvox);
  E2E_REQUIRE(nvox <= (1ll << 40), "%s: %lld voxels, at most 2^40", what, nvox);
  E2E_REQUIRE(out != nullptr, "%s: null pointer", what);
  E2E_REQUIRE((uintptr_t)out % 8 == 0, "%s: out at %p is not aligned to its 64-bit words", what, (const void*)out);
  E2E_REQUIRE(nvox == 0 || raw != nullptr, "%s: null pointer", what);
  E2E_REQUIRE((uintptr_t)raw % (uintptr_t)elsize == 0, "%s: the payload at %p is not aligned to its %d-byte elements", what, raw,
              elsize);
  hipLaunchKernelGGL(nifti_scan_init_kernel, dim3(1), dim3(SCAN_WORDS), 0, st, out);
  if (nvox == 0) return e2e::check_launch("nifti_scan_init_kernel");
  const bool sw = swap != 0, sc = scale != 0;
  switch (datatype) {
    case 2: launch_scan<unsigned char>(raw, nvox, sw, sc, slope, inter, out, st); break;
    case 256: launch_scan<signed char>(raw, nvox, sw, sc, slope, inter, out, st); break;
    case 4: launch_scan<short>(raw, nvox, sw, sc, slope, inter, out, st); break;
    case 512: launch_scan<unsigned short>(raw, nvox, sw, sc, slope, inter, out, st); break;
    case 8: launch_scan<int>(raw, nvox, sw, sc, slope, inter, out, st); break;
    case 768: launch_scan<unsigned int>(raw, nvox, sw, sc, slope, inter, out, st); break;
    case 16: launch_scan<float>(raw, nvox, sw, sc, slope, inter, out, st); break;
    case 64: launch_scan<double>(raw, nvox, sw, sc, slope, inter, out, st); break;
    case 1024: launch_scan<long long>(raw, nvox, sw, sc, slope, inter, out, st); break;
    case 1280: launch_scan<unsigned long long>(raw, nvox, sw, sc, slope, inter, out, st); break;
  }
  return e2e::check_launch("nifti_scan_kernel");
}

extern "C" int e2e_nifti_decode_f32(const void* raw, long long nvox, int datatype, int swap, int scale, double slope, double inter,
                                    float* out, void* stream) {
  return decode<float>("nifti_decode_f32", raw, nvox, datatype, swap, scale, slope, inter, out, nullptr, (hipStream_t)stream);
}

extern "C" int e2e_nifti_decode_u8(const void* raw, long long nvox, int datatype, int swap, int scale, double slope, double inter,
                                   unsigned char* out, unsigned long long* rejected, void* stream) {
  E2E_REQUIRE(rejected != nullptr, "nifti_decode_u8: no counter for the rejected voxels");
  return decode<unsigned char>("nifti_decode_u8", raw, nvox, datatype, swap, scale, slope, inter, out, rejected, (hipStream_t)stream);
}
