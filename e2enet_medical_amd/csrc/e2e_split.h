// The split-operand arithmetic of the matrix-pipe kernels (gfx950): how an fp32 operand becomes pieces the bf16 / fp16 matrix
// instructions multiply exactly, and the power of two that moves an fp16 operand into range.  K1m (conv133_mm.hip), the weight
// gradient K6b (conv133_wgrad_bf3.hip), the transposed convs (convt.hip) and the dense bf16 conv (conv133_dense.hip) take their
// pieces from here, and so does the numerics gate (e2e_diag_split_gemm, tests/test_gpu_ops.py::test_split_operand_products_vs_fp64),
// which holds every form below against fp64.  The product orders stay with the kernels.
//
// bf16 three-piece form (split_bf3): v = hi + mid + lo, 8 + 8 + 8 significant bits, truncating splits whose remainders are exact.
// A product is rebuilt from the six leading cross terms (lo*hi, mid*mid, hi*lo, mid*hi, hi*mid, hi*hi), each exact in the fp32
// accumulator; the dropped terms are <= 2^-23 |a b|, the class of the one rounding an fp32 FMA makes per term.  8 exponent bits:
// no range to manage.
//
// fp16 two-piece form: v = hi + lo + r, hi = rn16(v), lo = rn16(v - hi) (the subtraction is exact), 11 + 11 significant bits, three
// products (lo*hi, hi*lo, hi*hi) instead of six, |r| <= 2^-23 |v|.  The splits round to nearest: truncating ones are biased (4e-4
// of the result at K = 262144 with one-signed operands).  fp16 has 5 exponent bits, so every operand is first multiplied by the
// exact power of two 2^k that puts a bound of its max |v| in [2^14, 2^15); k comes from the bound's bit pattern, the "range word"
// (scale_exp), and results are un-scaled by one exact factor 2^-k per operand (the sum of two exponents may leave the fp32 range).
// lo is a normal fp16 down to 2^-3 in scaled units; the lo piece of values 2^11 below the bound's scale is subnormal, an absolute
// error of 2^-25 of the scaled range there instead of a relative 2^-23 (the negative half of a LeakyReLU output lives around 0.01).
// Against fp64 (K = 256 .. 262144; uniform, activation x heavy-tailed 1e-7 gradient and all-positive operands) the error is at or
// below the bf16 form's and an fp32 FMA chain's: profiles/r05_h2_numerics.txt.
//
// The fp16 split has two instruction forms.  Both round the same exact difference, so they give the same bits:
//   split_f16x2_fma_mix  v_cvt_pk_f16_f32, then lo as one v_fma_mix per value (fma(hi, -1, v) rounded to fp16): 3 instructions per
//                        value pair.  K1m's activation staging, the transposed convs.
//   split_f16x2_cvt_sub  hi converted, the exact difference v - hi formed in fp32 (widen and subtract, or v_fma_mix_f32, as the
//                        compiler picks), converted again: about 5 instructions per value pair.  K6b, K1m's weight packing
//                        (split_f16_cvt_sub, one value).
// K6b's sched_group_barrier fill counts (WG5H_FILL) were tuned to the longer form: moving K6b onto the short one is a performance
// change to be measured, not a rewrite of the same code.
#pragma once
#include <hip/hip_runtime.h>

namespace e2e {

typedef float f32x2_t __attribute__((ext_vector_type(2)));
typedef float f32x4_t __attribute__((ext_vector_type(4)));
typedef float f32x16_t __attribute__((ext_vector_type(16)));
typedef unsigned u32x2_t __attribute__((ext_vector_type(2)));
typedef unsigned u32x4_t __attribute__((ext_vector_type(4)));
typedef int i32x4_t __attribute__((ext_vector_type(4)));            // buffer resource
typedef short bf16x8_t __attribute__((ext_vector_type(8)));         // bf16 operand of a matrix instruction (raw bits)
typedef _Float16 f16x2_t __attribute__((ext_vector_type(2)));
typedef _Float16 f16x8_t __attribute__((ext_vector_type(8)));
typedef const f32x4_t __attribute__((address_space(1)))* gf4_p;     // 16-byte global load

// wave-uniform read-only operands (liveness words, bias, descriptors) go through the scalar cache: a vector load of them would
// sit in the same vmcnt queue as the staged planes and make the wave wait for those too
template <class T>
__device__ __forceinline__ T load_uniform(const T* ptr) {
#if defined(__HIP_DEVICE_COMPILE__)
  return *reinterpret_cast<const T __attribute__((address_space(4)))*>((unsigned long long)ptr);
#else
  return *ptr;
#endif
}

// ---- range words -------------------------------------------------------------------------------------------------------------
constexpr int XSH = 3;         // activations without a range word are staged as x 2^XSH (lo normal down to |x| = 2^-6; Inf beyond 8188)
// clamps of the scale exponent: |k| <= LIM keeps 2^k and 2^-k normal numbers; they bind only for zero, denormal or absurd bounds
constexpr int LIM_W = 60;      // weights: a max |w| below 2^-46 is an all-zero tensor in practice
constexpr int LIM_X = 110;     // activations (K1m's reduction side, dy in its data gradient; K6b's input side)
constexpr int LIM_DY = 120;    // K6b's dy: also keeps 2^-(k + XSH) normal
constexpr int LIM_CT = 100;    // the transposed convs: the bound is the product of two words

__device__ __forceinline__ float pow2f(int k) { return __builtin_bit_cast(float, (unsigned)(127 + k) << 23); }

// k = 141 - E (E the biased exponent of the bound whose bit pattern is `word`) puts the bound in [2^14, 2^15); a zero / denormal
// bound takes E = 1, Inf / NaN propagate; clamped to +-LIM
template <int LIM>
__host__ __device__ inline int scale_exp(unsigned word) {
  int E = (int)((word >> 23) & 0xffu);
  E = E < 1 ? 1 : E;
  const int k = 141 - E;
  return k > LIM ? LIM : (k < -LIM ? -LIM : k);
}

// ---- bf16 three-piece form ------------------------------------------------------------------------------------------------------
// the pieces are the high halves of h, m, l (pack_hi16 puts two of them in one word)
__device__ __forceinline__ void split_bf3(float v, unsigned& h, unsigned& m, unsigned& l) {
  h = __builtin_bit_cast(unsigned, v);
  const float r1 = v - __builtin_bit_cast(float, h & 0xffff0000u);            // exact
  m = __builtin_bit_cast(unsigned, r1);
  const float r2 = r1 - __builtin_bit_cast(float, m & 0xffff0000u);           // exact, <= 8 significant bits
  l = __builtin_bit_cast(unsigned, r2);
}
// v_perm_b32 0x07060302 = (S1 >> 16) | (S0 & 0xffff0000): the bf16 pieces of two values in one word, `lo` in the low half
__device__ __forceinline__ unsigned pack_hi16(unsigned lo, unsigned hi) { return __builtin_amdgcn_perm(hi, lo, 0x07060302u); }

// ---- fp16 two-piece form: the hi and lo words of value pairs (the first value in the low half) ---------------------------------
__device__ __forceinline__ void split_f16x2_fma_mix(float a, float b, unsigned& hw, unsigned& lw) {
  hw = __builtin_bit_cast(unsigned, __builtin_convertvector((f32x2_t{a, b}), f16x2_t));
  asm("v_fma_mixlo_f16 %0, %1, -1.0, %2 op_sel_hi:[1,0,0]\n\tv_fma_mixhi_f16 %0, %1, -1.0, %3 op_sel:[1,0,0] op_sel_hi:[1,0,0]"
      : "=&v"(lw) : "v"(hw), "v"(a), "v"(b));
}
// N value pairs (pair j: v[2j], v[2j + 1]); all hi words are converted before the lo words (the order K6b was scheduled with)
template <int N>
__device__ __forceinline__ void split_f16x2_cvt_sub(const float (&v)[2 * N], unsigned (&hw)[N], unsigned (&lw)[N]) {
  f16x2_t h[N];
#pragma unroll
  for (int j = 0; j < N; ++j) h[j] = __builtin_convertvector((f32x2_t{v[2 * j], v[2 * j + 1]}), f16x2_t);
#pragma unroll
  for (int j = 0; j < N; ++j) {
    hw[j] = __builtin_bit_cast(unsigned, h[j]);
    lw[j] = __builtin_bit_cast(unsigned, __builtin_convertvector((f32x2_t{v[2 * j] - (float)h[j][0], v[2 * j + 1] - (float)h[j][1]}), f16x2_t));
  }
}
// the same on one value
__device__ __forceinline__ void split_f16_cvt_sub(float v, _Float16& h, _Float16& l) {
  h = (_Float16)v;
  l = (_Float16)(v - (float)h);
}

}  // namespace e2e
