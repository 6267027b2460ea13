// N2: ensembling of saved class probabilities.  The `-z` export of the device softmax as fp16 and the merge of N such volumes
// (reference e2enet/inference/segmentation_export.py:117-140, e2enet/inference/ensemble_predictions.py:28-30) in one streaming pass:
// mean, argmax / region thresholds and crop-box placement, 2*N*K bytes read per voxel, the label byte (and, on request, the fp16
// mean) written.  Built with -ffp-contract=off: the arithmetic is numpy's, add by add.
#include "e2e_common.h"

namespace {

typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef float float8 __attribute__((ext_vector_type(8)));

constexpr int VEC = 8;                     // halves per lane and load: 16 bytes
constexpr int MAX_BLOCKS = 2048;           // 256 CUs x 8 workgroups; the rest of the volume is walked with a grid stride

// 16 bytes from / to an address that is only 2-byte aligned: class planes k >= 1 start at k * A*B*C halves, which is a multiple of
// 8 only when A*B*C is.  gfx950 global loads and stores take any alignment; the copy states no more than the type's own.
__device__ __forceinline__ half8 load8(const _Float16* p) {
  half8 v;
  __builtin_memcpy(&v, p, sizeof(v));
  return v;
}
__device__ __forceinline__ void store8(_Float16* p, half8 v) { __builtin_memcpy(p, &v, sizeof(v)); }

struct MergeSrcs {
  const _Float16* p[E2E_MERGE_MAX_SOURCES];
};

// the mean of one class at one voxel: fp32 adds in source order, one fp32 division, one rounding to fp16
template <int N>
__device__ __forceinline__ _Float16 mean1(const MergeSrcs& srcs, long long off) {
  float acc = (float)srcs.p[0][off];
#pragma unroll
  for (int s = 1; s < N; ++s) acc = __fadd_rn(acc, (float)srcs.p[s][off]);
  return (_Float16)__fdiv_rn(acc, (float)N);
}

// first maximum over k, a NaN counting as one (np.argmax); or the last region above 0.5 (segmentation_export.py:124-130).
// `p` is the fp16 mean widened: the comparison is the one numpy makes on the fp16 array
__device__ __forceinline__ void decide(float p, int k, float& best, int& lab, const int* __restrict__ regions, int n_regions) {
  if (regions == nullptr) {
    if (p > best || (p != p && best == best)) { best = p; lab = k; }
  } else if (k < n_regions && p > 0.5f) {
    lab = regions[k];
  }
}

template <int N>
__global__ __launch_bounds__(256) void merge_softmax_f16_kernel(const MergeSrcs srcs, int K, int A, int B, int C,
                                                                unsigned char* __restrict__ seg, int OA, int OB, int OC, int a0,
                                                                int b0, int c0, const int* __restrict__ regions, int n_regions,
                                                                _Float16* __restrict__ mean) {
  const long long n = (long long)A * B * C;
  const long long chunks = e2e::cdivll(n, VEC);
  for (long long t = (long long)blockIdx.x * 256 + threadIdx.x; t < chunks; t += (long long)gridDim.x * 256) {
    const long long i0 = t * VEC;
    const int cnt = (n - i0 >= VEC) ? VEC : (int)(n - i0);
    float best[VEC];
    int lab[VEC];
#pragma unroll
    for (int j = 0; j < VEC; ++j) { best[j] = -INFINITY; lab[j] = 0; }
    if (cnt == VEC) {
      for (int k = 0; k < K; ++k) {
        const long long off = (long long)k * n + i0;
        half8 v[N];
#pragma unroll
        for (int s = 0; s < N; ++s) v[s] = load8(srcs.p[s] + off);
        float8 acc = __builtin_convertvector(v[0], float8);
#pragma unroll
        for (int s = 1; s < N; ++s) {
          const float8 x = __builtin_convertvector(v[s], float8);
#pragma unroll
          for (int j = 0; j < VEC; ++j) acc[j] = __fadd_rn(acc[j], x[j]);
        }
        half8 m;
#pragma unroll
        for (int j = 0; j < VEC; ++j) m[j] = (_Float16)__fdiv_rn(acc[j], (float)N);
        if (mean != nullptr) store8(mean + off, m);
        if (seg != nullptr) {
#pragma unroll
          for (int j = 0; j < VEC; ++j) decide((float)m[j], k, best[j], lab[j], regions, n_regions);
        }
      }
    } else {
      // the last, partial vector of the volume: element by element, nothing read or written past a plane's end
      for (int k = 0; k < K; ++k) {
        const long long off = (long long)k * n + i0;
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
          if (j >= cnt) continue;
          const _Float16 m = mean1<N>(srcs, off + j);
          if (mean != nullptr) mean[off + j] = m;
          if (seg != nullptr) decide((float)m, k, best[j], lab[j], regions, n_regions);
        }
      }
    }
    if (seg == nullptr) continue;
    int c = (int)(i0 % C);
    const long long r = i0 / C;
    int b = (int)(r % B), a = (int)(r / B);
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
      // bbox clipped to the original size (segmentation_export.py:137)
      if (j < cnt && a0 + a < OA && b0 + b < OB && c0 + c < OC)
        seg[((long long)(a0 + a) * OB + (b0 + b)) * OC + (c0 + c)] = (unsigned char)lab[j];
      if (++c == C) {
        c = 0;
        if (++b == B) { b = 0; ++a; }
      }
    }
  }
}

// out[k, i] = fp16(probs[k * kstride + a*sa + b*sb + c*sc]) for the voxel i = (a, b, c) of the transposed frame; eight voxels per
// lane.  `contig`: the transposed frame is the source's own raster order (sa = B*C, sb = C, sc = 1), eight floats are one run
template <bool CONTIG>
__global__ __launch_bounds__(256) void softmax_to_f16_kernel(const float* __restrict__ probs, _Float16* __restrict__ out, int K,
                                                             long long kstride, int A, int B, int C, long long sa, long long sb,
                                                             long long sc) {
  const long long n = (long long)A * B * C;
  const long long chunks = e2e::cdivll(n, VEC);
  for (long long t = (long long)blockIdx.x * 256 + threadIdx.x; t < chunks; t += (long long)gridDim.x * 256) {
    const long long i0 = t * VEC;
    const int cnt = (n - i0 >= VEC) ? VEC : (int)(n - i0);
    long long o[VEC];
    if (CONTIG) {
#pragma unroll
      for (int j = 0; j < VEC; ++j) o[j] = i0 + j;
    } else {
      int c = (int)(i0 % C);
      const long long r = i0 / C;
      int b = (int)(r % B), a = (int)(r / B);
#pragma unroll
      for (int j = 0; j < VEC; ++j) {
        o[j] = (j < cnt) ? a * sa + b * sb + c * sc : 0;
        if (++c == C) {
          c = 0;
          if (++b == B) { b = 0; ++a; }
        }
      }
    }
    for (int k = 0; k < K; ++k) {
      const float* sp = probs + (long long)k * kstride;
      _Float16* dp = out + (long long)k * n + i0;
      if (cnt == VEC) {
        float8 x;
        if (CONTIG) {
          __builtin_memcpy(&x, sp + i0, sizeof(x));
        } else {
#pragma unroll
          for (int j = 0; j < VEC; ++j) x[j] = sp[o[j]];
        }
        store8(dp, __builtin_convertvector(x, half8));             // v_cvt_f16_f32: round to nearest even, fp16 denormals kept
      } else {
#pragma unroll
        for (int j = 0; j < VEC; ++j)
          if (j < cnt) dp[j] = (_Float16)sp[o[j]];
      }
    }
  }
}

unsigned grid_for(long long n) {
  const long long blocks = e2e::cdivll(e2e::cdivll(n, VEC), 256);
  return (unsigned)(blocks < MAX_BLOCKS ? blocks : MAX_BLOCKS);
}

template <int N>
void launch_merge(const MergeSrcs& srcs, int K, int A, int B, int C, unsigned char* seg, int OA, int OB, int OC, int a0, int b0,
                  int c0, const int* regions, int n_regions, _Float16* mean, hipStream_t st) {
  hipLaunchKernelGGL(merge_softmax_f16_kernel<N>, dim3(grid_for((long long)A * B * C)), dim3(256), 0, st, srcs, K, A, B, C, seg, OA,
                     OB, OC, a0, b0, c0, regions, n_regions, mean);
}

}  // namespace

extern "C" int e2e_softmax_to_f16(const float* probs, void* out, int K, long long kstride, int A, int B, int C, long long sa,
                                  long long sb, long long sc, void* stream) {
  E2E_REQUIRE(probs && out && K > 0 && A > 0 && B > 0 && C > 0, "softmax_to_f16: bad arguments");
  E2E_REQUIRE(kstride >= 0 && sa >= 0 && sb >= 0 && sc >= 0, "softmax_to_f16: negative stride");
  const long long n = (long long)A * B * C;
  const bool contig = sc == 1 && sb == C && sa == (long long)B * C;
  if (contig)
    hipLaunchKernelGGL(softmax_to_f16_kernel<true>, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, probs, (_Float16*)out, K,
                       kstride, A, B, C, sa, sb, sc);
  else
    hipLaunchKernelGGL(softmax_to_f16_kernel<false>, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, probs, (_Float16*)out, K,
                       kstride, A, B, C, sa, sb, sc);
  return e2e::check_launch("softmax_to_f16_kernel");
}

extern "C" int e2e_merge_softmax_f16(const void* const* srcs, int n_src, int K, int A, int B, int C, unsigned char* seg, int OA,
                                     int OB, int OC, int a0, int b0, int c0, const int* regions, int n_regions, void* mean,
                                     void* stream) {
  E2E_REQUIRE(srcs && n_src >= 1, "merge_softmax_f16: no sources");
  E2E_REQUIRE(n_src <= E2E_MERGE_MAX_SOURCES, "merge_softmax_f16: %d sources, at most %d are merged in one call", n_src,
              E2E_MERGE_MAX_SOURCES);
  E2E_REQUIRE(K > 0 && A > 0 && B > 0 && C > 0, "merge_softmax_f16: bad arguments");
  E2E_REQUIRE(seg || mean, "merge_softmax_f16: neither a label volume nor a mean volume to write");
  E2E_REQUIRE(!seg || (a0 >= 0 && b0 >= 0 && c0 >= 0 && OA > 0 && OB > 0 && OC > 0), "merge_softmax_f16: bad placement");
  E2E_REQUIRE(regions == nullptr || (n_regions > 0 && n_regions <= K), "merge_softmax_f16: bad region list");
  MergeSrcs m;
  for (int s = 0; s < E2E_MERGE_MAX_SOURCES; ++s) {
    m.p[s] = (const _Float16*)srcs[s < n_src ? s : 0];
    E2E_REQUIRE(m.p[s] != nullptr && m.p[s] != mean, "merge_softmax_f16: source %d is null or is the mean volume", s);
  }
  hipStream_t st = (hipStream_t)stream;
  _Float16* mo = (_Float16*)mean;
#define E2E_MERGE_CASE(N) \
  case N: launch_merge<N>(m, K, A, B, C, seg, OA, OB, OC, a0, b0, c0, regions, n_regions, mo, st); break;
  switch (n_src) {
    E2E_MERGE_CASE(1) E2E_MERGE_CASE(2) E2E_MERGE_CASE(3) E2E_MERGE_CASE(4) E2E_MERGE_CASE(5) E2E_MERGE_CASE(6)
    E2E_MERGE_CASE(7) E2E_MERGE_CASE(8) E2E_MERGE_CASE(9) E2E_MERGE_CASE(10) E2E_MERGE_CASE(11) E2E_MERGE_CASE(12)
    E2E_MERGE_CASE(13) E2E_MERGE_CASE(14) E2E_MERGE_CASE(15) E2E_MERGE_CASE(16)
  }
#undef E2E_MERGE_CASE
  return e2e::check_launch("merge_softmax_f16_kernel");
}
