// K8 / K8r: the two fused deep-supervision losses, forward and gradient for one scale (gfx950).
//   K8 : softmax + soft-Dice + cross-entropy, DC_and_CE_loss (dice_loss.py:302-359) = RobustCrossEntropyLoss
//        (crossentropy.py:4-12, mean over voxels) + SoftDiceLoss(softmax, batch_dice, do_bg=False, smooth) (dice_loss.py:156-192)
//   K8r: sigmoid + soft-Dice + binary cross-entropy over overlapping label regions, DC_and_BCE_loss (dice_loss.py:362-387) =
//        BCEWithLogitsLoss() + SoftDiceLoss(sigmoid, batch_dice, do_bg=True, smooth), the loss of nnUNetTrainerV2BraTSRegions
// with tp/fp/fn of get_tp_fp_fn_tn (dice_loss.py:100-153); the per-scale weight of MultipleOutputLoss2
// (deep_supervision.py:31-43) is folded into the gradient.  What the two share is defined once, below: the Dice statistics
// and their gradient.  The two reduce kernels have the same accumulator scheme (fp32 partials tp/fp/fn[NB] flushed into fp64
// sums, wave sum, block sum through LDS, one fp64 atomic per block and slot) and each writes it out in place: they are bound by
// instruction issue, and any helper around the register arrays or their unrolled loops changes the schedule the compiler finds.
//   acc layout (fp64): [B][K][3] (tp, fp, fn) followed by one CE / BCE sum (K8r: K = R regions).
#include "e2e_common.h"

namespace {
constexpr int KMAX = 32;

// ---- soft Dice of one (sample, class): dice = N / Dn, N = 2tp + s, Dn = 2tp + fp + fn + s + 1e-8 (s = smooth) ----
// The classes from K0 on have a dice term: K0 = 1 for K8 (do_bg=False drops class 0), K0 = 0 for K8r (every region counts,
// there is no background to drop).
struct DiceStats {
  double tp, fp, fn;
  __device__ __forceinline__ double N(float smooth) const { return 2 * tp + smooth; }
  __device__ __forceinline__ double Dn(float smooth) const { return 2 * tp + fp + fn + smooth + 1e-8; }
};

// tp/fp/fn of class k: summed over the batch (batch_dice) or of sample n
__device__ __forceinline__ DiceStats dice_stats(const double* acc, int batch_dice, int n, int B, int K, int k) {
  DiceStats s = {0, 0, 0};
  if (batch_dice) {
    for (int b = 0; b < B; ++b) {
      s.tp += acc[((long long)b * K + k) * 3]; s.fp += acc[((long long)b * K + k) * 3 + 1]; s.fn += acc[((long long)b * K + k) * 3 + 2];
    }
  } else {
    s.tp = acc[((long long)n * K + k) * 3]; s.fp = acc[((long long)n * K + k) * 3 + 1]; s.fn = acc[((long long)n * K + k) * 3 + 2];
  }
  return s;
}

// M = number of (sample, class) dice terms the loss averages
__device__ __forceinline__ double dice_terms(int batch_dice, int B, int K, int K0) {
  return batch_dice ? (double)(K - K0) : (double)B * (K - K0);
}

// g = dDiceLoss/dp of a voxel of the class: g_hit where the target is the class, g_miss elsewhere.
// DiceLoss = -(1/M) sum N/Dn, so g_hit = -(2*Dn - N)/(Dn^2 M) and g_miss = N/(Dn^2 M).
// A class absent from a sample with smooth = 0 has N = 0: g_miss = 0 on all its voxels (none is a hit), all finite.
__device__ __forceinline__ void dice_grads(const DiceStats& s, float smooth, double M, float& g_hit, float& g_miss) {
  const double N = s.N(smooth), Dn = s.Dn(smooth);
  g_hit = (float)(-(2 * Dn - N) / (Dn * Dn) / M);
  g_miss = (float)(N / (Dn * Dn) / M);
}

// mean dice over the M terms, summed b-major over k = K0..K-1
__device__ __forceinline__ double dice_mean(const double* acc, int batch_dice, float smooth, int B, int K, int K0) {
  double dsum = 0.0;
  if (batch_dice) {
    for (int k = K0; k < K; ++k) {
      const DiceStats s = dice_stats(acc, 1, 0, B, K, k);
      dsum += s.N(smooth) / s.Dn(smooth);
    }
  } else {
    for (int b = 0; b < B; ++b)
      for (int k = K0; k < K; ++k) {
        const DiceStats s = dice_stats(acc, 0, b, B, K, k);
        dsum += s.N(smooth) / s.Dn(smooth);
      }
  }
  return dsum / dice_terms(batch_dice, B, K, K0);
}

// prologue of the gradient kernels: g_hit / g_miss of this block's sample into LDS, and from one thread of the grid the
// loss value weight * (mean CE - mean dice), mean CE = acc's last slot / ce_count
template <int KB>
__device__ __forceinline__ void dice_prologue(const double* acc, float weight, int batch_dice, float smooth,
                                              float* loss_out, int n, int B, int K, int K0, double ce_count,
                                              float* g_hit, float* g_miss) {
  if (threadIdx.x < KB) {
    const int k = threadIdx.x;
    float gh = 0.f, gm = 0.f;
    if (k >= K0 && k < K) dice_grads(dice_stats(acc, batch_dice, n, B, K, k), smooth, dice_terms(batch_dice, B, K, K0), gh, gm);
    g_hit[k] = gh;
    g_miss[k] = gm;
  }
  if (blockIdx.x == 0 && n == 0 && threadIdx.x == 0) {
    const double dsum = dice_mean(acc, batch_dice, smooth, B, K, K0);
    const double ce = acc[(long long)B * K * 3] / ce_count;
    *loss_out += (float)(weight * (ce - dsum));
  }
  __syncthreads();
}

// ---- K8 ----
// the KB logits of voxel v (-INF past class K); returns their maximum (dc_ce_reduce_kernel writes its own, see the top)
template <int KB>
__device__ __forceinline__ float load_logits(const float* lp, int K, long long spatial, long long v, float l[KB]) {
  float m = -INFINITY;
#pragma unroll
  for (int k = 0; k < KB; ++k) {
    l[k] = (k < K) ? lp[(long long)k * spatial + v] : -INFINITY;
    m = fmaxf(m, l[k]);
  }
  return m;
}

template <int KB>
__global__ __launch_bounds__(256) void dc_ce_reduce_kernel(const float* __restrict__ logits, const float* __restrict__ target,
                                                           double* __restrict__ acc, int K, long long spatial) {
  const int n = blockIdx.y;
  const float* lp = logits + (long long)n * K * spatial;
  const float* tp_ = target + (long long)n * spatial;
  float tp[KB], fp[KB], fn[KB];
#pragma unroll
  for (int k = 0; k < KB; ++k) { tp[k] = 0.f; fp[k] = 0.f; fn[k] = 0.f; }
  double dtp[KB], dfp[KB], dfn[KB];
#pragma unroll
  for (int k = 0; k < KB; ++k) { dtp[k] = 0.0; dfp[k] = 0.0; dfn[k] = 0.0; }
  double ce = 0.0;
  int it = 0;
  for (long long v = (long long)blockIdx.x * 256 + threadIdx.x; v < spatial; v += (long long)gridDim.x * 256) {
    float l[KB];
    float m = -INFINITY;
#pragma unroll
    for (int k = 0; k < KB; ++k) {
      l[k] = (k < K) ? lp[(long long)k * spatial + v] : -INFINITY;
      m = fmaxf(m, l[k]);
    }
    const int t = (int)tp_[v];
    // cross entropy as torch's log_softmax forms it: (l_t - max) - log(sum exp(l - max)); -log(p_t) would turn into +Inf where
    // p_t underflows (logits apart by more than ~100: large InstanceNorm weights) although the loss is finite
    // label outside [0, K): torch's CrossEntropyLoss raises; here the loss turns NaN.  Such a label matches no slot (tc = -1) and
    // lt keeps its NaN: a label in [K, KB) would otherwise pick up the -INF of a padded slot and turn the loss into +Inf
    const int tc = (unsigned)t < (unsigned)K ? t : -1;
    float lt = NAN;
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < KB; ++k) {
      if (k == tc) lt = l[k] - m;
      l[k] = (k < K) ? expf(l[k] - m) : 0.f;
      s += l[k];
    }
    const float inv = 1.f / s;
#pragma unroll
    for (int k = 0; k < KB; ++k) {
      const float pk = l[k] * inv;
      if (k == t) { tp[k] += pk; fn[k] += 1.f - pk; }
      else fp[k] += pk;
    }
    ce -= (double)(lt - logf(s));
    if ((++it & 31) == 0) {
#pragma unroll
      for (int k = 0; k < KB; ++k) {
        dtp[k] += tp[k]; dfp[k] += fp[k]; dfn[k] += fn[k];
        tp[k] = 0.f; fp[k] = 0.f; fn[k] = 0.f;
      }
    }
  }
  __shared__ double sh[4][3 * KB + 1];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
  for (int k = 0; k < KB; ++k) {
    const double a = e2e::wave_sum_d(dtp[k] + (double)tp[k]);
    const double b = e2e::wave_sum_d(dfp[k] + (double)fp[k]);
    const double c = e2e::wave_sum_d(dfn[k] + (double)fn[k]);
    if (lane == 0) { sh[wave][3 * k] = a; sh[wave][3 * k + 1] = b; sh[wave][3 * k + 2] = c; }
  }
  ce = e2e::wave_sum_d(ce);
  if (lane == 0) sh[wave][3 * KB] = ce;
  __syncthreads();
  if (threadIdx.x < 3 * K) {
    const int i = threadIdx.x;
    atomicAdd(&acc[(long long)n * K * 3 + i], sh[0][i] + sh[1][i] + sh[2][i] + sh[3][i]);
  }
  if (threadIdx.x == 255) atomicAdd(&acc[(long long)gridDim.y * K * 3], sh[0][3 * KB] + sh[1][3 * KB] + sh[2][3 * KB] + sh[3][3 * KB]);
}


// gradient: dlogit_j = weight * [ (p_j - [t == j]) / (B * spatial) + p_j * (g_j - sum_k g_k p_k) ], g_k of dice_grads (K0 = 1)
template <int KB>
__global__ __launch_bounds__(256) void dc_ce_grad_kernel(const float* __restrict__ logits, const float* __restrict__ target,
                                                         const double* __restrict__ acc, float weight, int batch_dice,
                                                         float smooth, float* __restrict__ dlogits, float* __restrict__ loss_out,
                                                         int B, int K, long long spatial) {
  const int n = blockIdx.y;
  __shared__ float g_hit[KB], g_miss[KB];
  dice_prologue<KB>(acc, weight, batch_dice, smooth, loss_out, n, B, K, 1, (double)B * (double)spatial, g_hit, g_miss);
  if (dlogits == nullptr) return;                      // value only (validation batches)
  const float inv_cnt = 1.f / ((float)B * (float)spatial);
  const float* lp = logits + (long long)n * K * spatial;
  float* dp = dlogits + (long long)n * K * spatial;
  const float* tg = target + (long long)n * spatial;
  for (long long v = (long long)blockIdx.x * 256 + threadIdx.x; v < spatial; v += (long long)gridDim.x * 256) {
    float l[KB];
    const float m = load_logits<KB>(lp, K, spatial, v, l);
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < KB; ++k) {
      l[k] = (k < K) ? expf(l[k] - m) : 0.f;
      s += l[k];
    }
    const float inv = 1.f / s;
    const int t = (int)tg[v];
    float dot = 0.f;
    float g[KB];
#pragma unroll
    for (int k = 0; k < KB; ++k) {
      l[k] *= inv;
      g[k] = (k == t) ? g_hit[k] : g_miss[k];
      dot = fmaf(g[k], l[k], dot);
    }
#pragma unroll
    for (int k = 0; k < KB; ++k)
      if (k < K) dp[(long long)k * spatial + v] = weight * ((l[k] - (k == t ? 1.f : 0.f)) * inv_cnt + l[k] * (g[k] - dot));
  }
}
// batch dice across data-parallel ranks (reference nnUNetTrainerV2_DDP.py:263-268 gathers the per-sample numerators and
// denominators and sums them): fold the [B][K][3] rows into row 0 (rows 1.. zeroed) so that ONE small all-reduce of
// row 0 gives every rank the global tp/fp/fn; dice_stats(batch_dice = 1) then sums the rows as before.
__global__ void dc_ce_fold_batch_kernel(double* __restrict__ acc, int B, int K) {
  const int i = threadIdx.x;
  if (i >= 3 * K) return;
  double s = 0.0;
  for (int b = 0; b < B; ++b) {
    s += acc[(long long)b * K * 3 + i];
    if (b > 0) acc[(long long)b * K * 3 + i] = 0.0;
  }
  acc[i] = s;
}

// online evaluation of a validation batch (reference nnUNetTrainer_simple.py:373-405): hard tp / fp / fn voxel counts per
// class of argmax(softmax(logits)) against the target, summed over the batch.  counts [K][3] (class 0 is filled too,
// the reference reports classes 1..K-1).
template <int KB>
__global__ __launch_bounds__(256) void online_eval_kernel(const float* __restrict__ logits, const float* __restrict__ target,
                                                          unsigned long long* __restrict__ counts, int K, long long spatial) {
  __shared__ unsigned int h[3][KB];
  for (int i = threadIdx.x; i < 3 * KB; i += 256) (&h[0][0])[i] = 0u;
  __syncthreads();
  const int n = blockIdx.y;
  const float* lp = logits + (long long)n * K * spatial;
  const float* tg = target + (long long)n * spatial;
  for (long long v = (long long)blockIdx.x * 256 + threadIdx.x; v < spatial; v += (long long)gridDim.x * 256) {
    float l[KB];
    const float m = load_logits<KB>(lp, K, spatial, v, l);
    // argmax of the softmax = first maximum of exp(l - m) (the common 1/sum factor keeps order and ties)
    int seg = 0;
    float best = -1.f;
#pragma unroll
    for (int k = 0; k < KB; ++k) {
      const float ek = (k < K) ? expf(l[k] - m) : -1.f;
      if (ek > best) { best = ek; seg = k; }
    }
    const int t = (int)tg[v];
    if (seg == t) atomicAdd(&h[0][seg], 1u);
    else {
      atomicAdd(&h[1][seg], 1u);
      if ((unsigned)t < (unsigned)K) atomicAdd(&h[2][t], 1u);
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 3 * K; i += 256) {
    const int k = i / 3, j = i - 3 * k;
    if (h[j][k]) atomicAdd(&counts[i], (unsigned long long)h[j][k]);
  }
}

// ---- K8r ----
// Every region r is a binary problem of its own: p = sigmoid(l_r), y_r in {0, 1}.  acc is [B][R][3] as for K8, so
// e2e_dc_ce_fold_batch serves it too.  Targets come in two forms (template LABELS):
//   true : a [B,1,spatial] label map and one word per region, bit t of words[r] = "label t belongs to region r"; y_r is
//          formed on load and no R-channel target exists in HBM (ConvertSegmentationToRegionsTransform, custom_transforms.py:96-123,
//          fused: labels outside [0, 32) or not whole numbers belong to no region, as in its `seg == l` loop)
//   false: a [B,R,spatial] multi-hot float tensor, y = (value >= 0.5)
// Both forms run the same arithmetic in the same order on the same y, so their results agree bit for bit.
// A thread owns groups of four consecutive voxels (one dwordx4 per plane where the planes are 16-byte aligned, four guarded
// dword loads otherwise -- the order of the sums does not depend on which) and flushes its accumulator every 8 groups = 32 voxels.
struct Quad { float v[4]; };

template <bool VEC>
__device__ __forceinline__ Quad load_quad(const float* __restrict__ row, long long v0, long long spatial, float fill) {
  Quad q;
  if (VEC) {                                 // spatial % 4 == 0: the whole group is inside the plane
    const float4 t = *reinterpret_cast<const float4*>(row + v0);
    q.v[0] = t.x; q.v[1] = t.y; q.v[2] = t.z; q.v[3] = t.w;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) q.v[j] = (v0 + j < spatial) ? row[v0 + j] : fill;
  }
  return q;
}

__device__ __forceinline__ unsigned label_bit(float f) {
  const int t = (int)f;
  return ((unsigned)t < 32u && (float)t == f) ? (1u << t) : 0u;
}

// prologue of a group of four voxels from v0 on, label form: lbits[j] = 1 << label of voxel j (0 in the multi-hot form)
template <bool LABELS, bool VEC>
__device__ __forceinline__ void group_label_bits(const float* __restrict__ tgt, long long v0, long long spatial, unsigned lbits[4]) {
#pragma unroll
  for (int j = 0; j < 4; ++j) lbits[j] = 0u;
  if (LABELS) {
    const Quad t = load_quad<VEC>(tgt, v0, spatial, -1.f);
#pragma unroll
    for (int j = 0; j < 4; ++j) lbits[j] = label_bit(t.v[j]);
  }
}

// bit j: voxel v0 + j is inside the plane (the gradient kernel guards its stores instead)
template <bool VEC>
__device__ __forceinline__ unsigned group_valid(long long v0, long long spatial) {
  if (VEC) return 15u;
  return (spatial - v0 >= 4) ? 15u : ((1u << (int)(spatial - v0)) - 1u);
}

// the region words in registers (label form; 0 otherwise)
template <int RB, bool LABELS>
__device__ __forceinline__ void load_words(const unsigned* __restrict__ words, int R, unsigned wd[RB]) {
#pragma unroll
  for (int r = 0; r < RB; ++r) wd[r] = (LABELS && r < R) ? words[r] : 0u;
}

// y of the four voxels of a group for region r: bit j of the result
template <bool LABELS, bool VEC>
__device__ __forceinline__ unsigned region_hits(const float* __restrict__ tgt, const unsigned lbits[4], unsigned word, int r,
                                                long long v0, long long spatial) {
  unsigned y = 0;
  if (LABELS) {
#pragma unroll
    for (int j = 0; j < 4; ++j) y |= (lbits[j] & word) ? (1u << j) : 0u;
  } else {
    const Quad t = load_quad<VEC>(tgt + (long long)r * spatial, v0, spatial, 0.f);
#pragma unroll
    for (int j = 0; j < 4; ++j) y |= (t.v[j] >= 0.5f) ? (1u << j) : 0u;
  }
  return y;
}

// p = sigmoid(l) and sp = log1p(exp(-|l|)), the softplus tail of BCEWithLogits, from one exponential and one division.
// log1p(e) = log(u) + (e - (u - 1)) / u with u = fl(1 + e): the second term restores what the rounding of 1 + e lost, so the
// sum keeps log1pf's precision where e is tiny (measured on 2 x 3 x 128^3: log1pf itself cost a third of the reduction)
__device__ __forceinline__ float sigmoid_parts(float l, float& sp) {
  const float e = expf(-fabsf(l));            // in (0, 1]: no overflow at any logit
  const float u = 1.f + e;
  const float inv = 1.f / u;
  sp = logf(u) + (e - (u - 1.f)) * inv;
  return l >= 0.f ? inv : e * inv;
}

template <int RB, bool LABELS, bool VEC>
__global__ __launch_bounds__(256) void dc_bce_reduce_kernel(const float* __restrict__ logits, const float* __restrict__ target,
                                                            const unsigned* __restrict__ words, double* __restrict__ acc, int R,
                                                            long long spatial) {
  const int n = blockIdx.y;
  const float* lp = logits + (long long)n * R * spatial;
  const float* tg = target + (long long)n * (LABELS ? 1 : R) * spatial;
  unsigned wd[RB];
#pragma unroll
  for (int r = 0; r < RB; ++r) wd[r] = (LABELS && r < R) ? words[r] : 0u;
  float tp[RB], fp[RB], fn[RB];
  double dtp[RB], dfp[RB], dfn[RB];
#pragma unroll
  for (int r = 0; r < RB; ++r) { tp[r] = 0.f; fp[r] = 0.f; fn[r] = 0.f; dtp[r] = 0.0; dfp[r] = 0.0; dfn[r] = 0.0; }
  double bce = 0.0;
  int it = 0;
  const long long groups = (spatial + 3) >> 2;
  for (long long gi = (long long)blockIdx.x * 256 + threadIdx.x; gi < groups; gi += (long long)gridDim.x * 256) {
    const long long v0 = gi << 2;
    unsigned lbits[4] = {0u, 0u, 0u, 0u};
    unsigned valid = 15u;
    if (!VEC) valid = (spatial - v0 >= 4) ? 15u : ((1u << (int)(spatial - v0)) - 1u);
    if (LABELS) {
      const Quad t = load_quad<VEC>(tg, v0, spatial, -1.f);
#pragma unroll
      for (int j = 0; j < 4; ++j) lbits[j] = label_bit(t.v[j]);
    }
    float bsum = 0.f;
#pragma unroll
    for (int r = 0; r < RB; ++r) {
      if (r < R) {
        const Quad l = load_quad<VEC>(lp + (long long)r * spatial, v0, spatial, 0.f);
        const unsigned y = region_hits<LABELS, VEC>(tg, lbits, wd[r], r, v0, spatial);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if (valid & (1u << j)) {
            float sp;
            const float p = sigmoid_parts(l.v[j], sp);
            const bool hit = (y >> j) & 1u;
            // BCEWithLogits, stable form: max(l, 0) - l y + log1p(exp(-|l|))
            bsum += fmaxf(l.v[j], 0.f) - (hit ? l.v[j] : 0.f) + sp;
            if (hit) { tp[r] += p; fn[r] += 1.f - p; }
            else fp[r] += p;
          }
        }
      }
    }
    bce += (double)bsum;
    if ((++it & 7) == 0) {
#pragma unroll
      for (int r = 0; r < RB; ++r) {
        dtp[r] += tp[r]; dfp[r] += fp[r]; dfn[r] += fn[r];
        tp[r] = 0.f; fp[r] = 0.f; fn[r] = 0.f;
      }
    }
  }
  __shared__ double sh[4][3 * RB + 1];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
  for (int r = 0; r < RB; ++r) {
    const double a = e2e::wave_sum_d(dtp[r] + (double)tp[r]);
    const double b = e2e::wave_sum_d(dfp[r] + (double)fp[r]);
    const double c = e2e::wave_sum_d(dfn[r] + (double)fn[r]);
    if (lane == 0) { sh[wave][3 * r] = a; sh[wave][3 * r + 1] = b; sh[wave][3 * r + 2] = c; }
  }
  bce = e2e::wave_sum_d(bce);
  if (lane == 0) sh[wave][3 * RB] = bce;
  __syncthreads();
  if (threadIdx.x < 3 * R) {
    const int i = threadIdx.x;
    atomicAdd(&acc[(long long)n * R * 3 + i], sh[0][i] + sh[1][i] + sh[2][i] + sh[3][i]);
  }
  if (threadIdx.x == 255) atomicAdd(&acc[(long long)gridDim.y * R * 3], sh[0][3 * RB] + sh[1][3 * RB] + sh[2][3 * RB] + sh[3][3 * RB]);
}

// gradient: dlogit_r = weight * [ (p_r - y_r) / (B * R * spatial) + p_r (1 - p_r) g_r ], g_r of dice_grads (K0 = 0)
template <int RB, bool LABELS, bool VEC>
__global__ __launch_bounds__(256) void dc_bce_grad_kernel(const float* __restrict__ logits, const float* __restrict__ target,
                                                          const unsigned* __restrict__ words, const double* __restrict__ acc,
                                                          float weight, int batch_dice, float smooth, float* __restrict__ dlogits,
                                                          float* __restrict__ loss_out, int B, int R, long long spatial) {
  const int n = blockIdx.y;
  __shared__ float g_hit[RB], g_miss[RB];
  dice_prologue<RB>(acc, weight, batch_dice, smooth, loss_out, n, B, R, 0, (double)B * (double)R * (double)spatial, g_hit, g_miss);
  if (dlogits == nullptr) return;                      // value only (validation batches)
  const float inv_cnt = 1.f / ((float)B * (float)R * (float)spatial);
  const float* lp = logits + (long long)n * R * spatial;
  float* dp = dlogits + (long long)n * R * spatial;
  const float* tg = target + (long long)n * (LABELS ? 1 : R) * spatial;
  unsigned wd[RB];
  load_words<RB, LABELS>(words, R, wd);
  const long long groups = (spatial + 3) >> 2;
  for (long long gi = (long long)blockIdx.x * 256 + threadIdx.x; gi < groups; gi += (long long)gridDim.x * 256) {
    const long long v0 = gi << 2;
    unsigned lbits[4];
    group_label_bits<LABELS, VEC>(tg, v0, spatial, lbits);
#pragma unroll
    for (int r = 0; r < RB; ++r) {
      if (r < R) {
        const Quad l = load_quad<VEC>(lp + (long long)r * spatial, v0, spatial, 0.f);
        const unsigned y = region_hits<LABELS, VEC>(tg, lbits, wd[r], r, v0, spatial);
        float d[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          float sp;
          const float p = sigmoid_parts(l.v[j], sp);
          const bool hit = (y >> j) & 1u;
          d[j] = weight * ((p - (hit ? 1.f : 0.f)) * inv_cnt + p * (1.f - p) * (hit ? g_hit[r] : g_miss[r]));
        }
        float* row = dp + (long long)r * spatial;
        if (VEC) {
          *reinterpret_cast<float4*>(row + v0) = make_float4(d[0], d[1], d[2], d[3]);
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (v0 + j < spatial) row[v0 + j] = d[j];
        }
      }
    }
  }
}

// a thread's packed counts of online_eval_regions_kernel -> the block's LDS counts; the packed counts restart at 0
template <int RB>
__device__ __forceinline__ void flush_counts(unsigned c[RB], unsigned int (*h)[3], int R) {
#pragma unroll
  for (int r = 0; r < RB; ++r) {
    if (r < R && c[r]) {
      if (c[r] & 1023u) atomicAdd(&h[r][0], c[r] & 1023u);
      if ((c[r] >> 10) & 1023u) atomicAdd(&h[r][1], (c[r] >> 10) & 1023u);
      if (c[r] >> 20) atomicAdd(&h[r][2], c[r] >> 20);
    }
    c[r] = 0u;
  }
}

// online evaluation of a region model (reference nnUNetTrainerV2BraTSRegions.run_online_evaluation, :168-189): hard tp / fp / fn
// per region of sigmoid(l) > 0.5 against y, summed over the batch.  sigmoid(l) > 0.5 <=> l > 0 (a logit of exactly 0 is a
// negative); the sign is tested, so the count does not hang on the last ulp of an exponential.
template <int RB, bool LABELS, bool VEC>
__global__ __launch_bounds__(256) void online_eval_regions_kernel(const float* __restrict__ logits, const float* __restrict__ target,
                                                                  const unsigned* __restrict__ words,
                                                                  unsigned long long* __restrict__ counts, int R, long long spatial) {
  __shared__ unsigned int h[RB][3];
  for (int i = threadIdx.x; i < 3 * RB; i += 256) (&h[0][0])[i] = 0u;
  __syncthreads();
  const int n = blockIdx.y;
  const float* lp = logits + (long long)n * R * spatial;
  const float* tg = target + (long long)n * (LABELS ? 1 : R) * spatial;
  unsigned wd[RB];
  load_words<RB, LABELS>(words, R, wd);
  unsigned c[RB];                                      // packed per-thread counts: tp | fp << 10 | fn << 20 (at most 4 * 128 each)
#pragma unroll
  for (int r = 0; r < RB; ++r) c[r] = 0u;
  int it = 0;
  const long long groups = (spatial + 3) >> 2;
  for (long long gi = (long long)blockIdx.x * 256 + threadIdx.x; gi < groups; gi += (long long)gridDim.x * 256) {
    const long long v0 = gi << 2;
    unsigned lbits[4];
    group_label_bits<LABELS, VEC>(tg, v0, spatial, lbits);
    const unsigned valid = group_valid<VEC>(v0, spatial);
#pragma unroll
    for (int r = 0; r < RB; ++r) {
      if (r < R) {
        const Quad l = load_quad<VEC>(lp + (long long)r * spatial, v0, spatial, 0.f);
        const unsigned y = region_hits<LABELS, VEC>(tg, lbits, wd[r], r, v0, spatial) & valid;
        unsigned pos = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) pos |= (l.v[j] > 0.f) ? (1u << j) : 0u;
        pos &= valid;
        c[r] += __popc(pos & y) + (__popc(pos & ~y) << 10) + (__popc(~pos & y) << 20);
      }
    }
    if ((++it & 127) == 0) flush_counts<RB>(c, h, R);  // 128 groups: a field holds at most 512 < 1024
  }
  flush_counts<RB>(c, h, R);
  __syncthreads();
  for (int i = threadIdx.x; i < 3 * R; i += 256)
    if ((&h[0][0])[i]) atomicAdd(&counts[i], (unsigned long long)(&h[0][0])[i]);
}

// ConvertSegmentationToRegionsTransform (custom_transforms.py:96-123) for callers who want its output: label map
// [B,1,spatial] -> multi-hot [B,R,spatial] float 0/1
__global__ __launch_bounds__(256) void seg_to_regions_kernel(const float* __restrict__ seg, const unsigned* __restrict__ words,
                                                             float* __restrict__ out, int R, long long spatial) {
  const int n = blockIdx.y;
  const float* sp = seg + (long long)n * spatial;
  float* op = out + (long long)n * R * spatial;
  for (long long v = (long long)blockIdx.x * 256 + threadIdx.x; v < spatial; v += (long long)gridDim.x * 256) {
    const unsigned bit = label_bit(sp[v]);
    for (int r = 0; r < R; ++r) op[(long long)r * spatial + v] = (bit & words[r]) ? 1.f : 0.f;
  }
}

inline bool quad_aligned(const void* a, const void* b, const void* c, long long spatial) {
  return (spatial & 3) == 0 && (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c) & 15u) == 0;
}

// blocks.x covers the voxels of a sample with grid-stride loops, blocks.y the batch; a single block where only the prologue runs
inline dim3 loss_grid(long long spatial, int B, bool whole = true) {
  long long b = e2e::cdivll(spatial, 256 * 8);
  if (b > 512) b = 512;
  if (b < 1) b = 1;
  return whole ? dim3((unsigned)b, B) : dim3(1, 1);
}
}  // namespace

// argument checks of the entry points over [B][K or R][spatial] tensors (expects B and spatial in scope)
#define LOSS_REQUIRE(name, pointers, K, kmin, sym)                \
  E2E_REQUIRE(pointers, name ": null pointer");                   \
  E2E_REQUIRE(B > 0 && (K) >= kmin && (K) <= KMAX && spatial > 0, name ": need " #kmin " <= " sym " <= 32")

#define DISPATCH_LK(K, ...)                                    \
  if ((K) <= 4) { constexpr int KB = 4; __VA_ARGS__; }         \
  else if ((K) <= 8) { constexpr int KB = 8; __VA_ARGS__; }    \
  else if ((K) <= 16) { constexpr int KB = 16; __VA_ARGS__; }  \
  else { constexpr int KB = 32; __VA_ARGS__; }

// region count -> register block, target form and load width -> template instance
#define DISPATCH_REGIONS(R, labels, vec, ...)                                        \
  DISPATCH_LK(R, {                                                                   \
    constexpr int RB = KB;                                                           \
    if (labels) {                                                                    \
      if (vec) { constexpr bool LABELS = true, VEC = true; __VA_ARGS__; }            \
      else { constexpr bool LABELS = true, VEC = false; __VA_ARGS__; }               \
    } else {                                                                         \
      if (vec) { constexpr bool LABELS = false, VEC = true; __VA_ARGS__; }           \
      else { constexpr bool LABELS = false, VEC = false; __VA_ARGS__; }              \
    }                                                                                \
  })

extern "C" long long e2e_loss_ws_bytes(int B, int K) { return ((long long)B * K * 3 + 1) * (long long)sizeof(double); }

extern "C" int e2e_dc_ce_reduce(const float* logits, const float* target, void* acc, int B, int K, long long spatial,
                                void* stream) {
  LOSS_REQUIRE("dc_ce_reduce", logits && target && acc, K, 2, "K");
  hipStream_t st = (hipStream_t)stream;
  e2e::zero_async(acc, (size_t)e2e_loss_ws_bytes(B, K), st);
  DISPATCH_LK(K, hipLaunchKernelGGL((dc_ce_reduce_kernel<KB>), loss_grid(spatial, B), dim3(256), 0, st, logits, target, (double*)acc,
                                    K, spatial));
  return e2e::check_launch("dc_ce_reduce_kernel");
}

extern "C" int e2e_dc_ce_grad(const float* logits, const float* target, const void* acc, float weight, int batch_dice,
                              float smooth, float* dlogits, float* loss_out, int B, int K, long long spatial,
                              void* stream) {
  LOSS_REQUIRE("dc_ce_grad", logits && target && acc && loss_out, K, 2, "K");
  DISPATCH_LK(K, hipLaunchKernelGGL((dc_ce_grad_kernel<KB>), loss_grid(spatial, B, dlogits != nullptr), dim3(256), 0,
                                    (hipStream_t)stream, logits, target, (const double*)acc, weight, batch_dice, smooth, dlogits,
                                    loss_out, B, K, spatial));
  return e2e::check_launch("dc_ce_grad_kernel");
}

extern "C" int e2e_dc_ce_fold_batch(void* acc, int B, int K, void* stream) {
  E2E_REQUIRE(acc, "dc_ce_fold_batch: null pointer");
  E2E_REQUIRE(B > 0 && K >= 1 && K <= KMAX, "dc_ce_fold_batch: need 1 <= K <= 32");     // (K = 1: a single region, K8r)
  hipLaunchKernelGGL(dc_ce_fold_batch_kernel, dim3(1), dim3(128), 0, (hipStream_t)stream, (double*)acc, B, K);
  return e2e::check_launch("dc_ce_fold_batch_kernel");
}

extern "C" int e2e_online_eval_counts(const float* logits, const float* target, long long* counts, int B, int K,
                                      long long spatial, void* stream) {
  LOSS_REQUIRE("online_eval_counts", logits && target && counts, K, 2, "K");
  hipStream_t st = (hipStream_t)stream;
  e2e::zero_async(counts, (size_t)K * 3 * sizeof(long long), st);
  DISPATCH_LK(K, hipLaunchKernelGGL((online_eval_kernel<KB>), loss_grid(spatial, B), dim3(256), 0, st, logits, target,
                                    (unsigned long long*)counts, K, spatial));
  return e2e::check_launch("online_eval_kernel");
}

extern "C" int e2e_dc_bce_reduce(const float* logits, const float* target, const unsigned* region_words, void* acc, int B, int R,
                                 long long spatial, void* stream) {
  LOSS_REQUIRE("dc_bce_reduce", logits && target && acc, R, 1, "R");
  hipStream_t st = (hipStream_t)stream;
  e2e::zero_async(acc, (size_t)e2e_loss_ws_bytes(B, R), st);
  const bool labels = region_words != nullptr, vec = quad_aligned(logits, target, nullptr, spatial);
  DISPATCH_REGIONS(R, labels, vec, hipLaunchKernelGGL((dc_bce_reduce_kernel<RB, LABELS, VEC>), loss_grid(spatial, B), dim3(256), 0, st,
                                                      logits, target, region_words, (double*)acc, R, spatial));
  return e2e::check_launch("dc_bce_reduce_kernel");
}

extern "C" int e2e_dc_bce_grad(const float* logits, const float* target, const unsigned* region_words, const void* acc,
                               float weight, int batch_dice, float smooth, float* dlogits, float* loss_out, int B, int R,
                               long long spatial, void* stream) {
  LOSS_REQUIRE("dc_bce_grad", logits && target && acc && loss_out, R, 1, "R");
  const bool labels = region_words != nullptr, vec = quad_aligned(logits, target, dlogits, spatial);
  DISPATCH_REGIONS(R, labels, vec, hipLaunchKernelGGL((dc_bce_grad_kernel<RB, LABELS, VEC>), loss_grid(spatial, B, dlogits != nullptr),
                                                      dim3(256), 0, (hipStream_t)stream, logits, target, region_words,
                                                      (const double*)acc, weight, batch_dice, smooth, dlogits, loss_out, B, R, spatial));
  return e2e::check_launch("dc_bce_grad_kernel");
}

extern "C" int e2e_online_eval_regions(const float* logits, const float* target, const unsigned* region_words, long long* counts,
                                       int B, int R, long long spatial, void* stream) {
  LOSS_REQUIRE("online_eval_regions", logits && target && counts, R, 1, "R");
  hipStream_t st = (hipStream_t)stream;
  e2e::zero_async(counts, (size_t)R * 3 * sizeof(long long), st);
  const bool labels = region_words != nullptr, vec = quad_aligned(logits, target, nullptr, spatial);
  DISPATCH_REGIONS(R, labels, vec, hipLaunchKernelGGL((online_eval_regions_kernel<RB, LABELS, VEC>), loss_grid(spatial, B), dim3(256), 0,
                                                      st, logits, target, region_words, (unsigned long long*)counts, R, spatial));
  return e2e::check_launch("online_eval_regions_kernel");
}

extern "C" int e2e_seg_to_regions(const float* seg, const unsigned* region_words, float* out, int B, int R, long long spatial,
                                  void* stream) {
  LOSS_REQUIRE("seg_to_regions", seg && region_words && out, R, 1, "R");
  hipLaunchKernelGGL(seg_to_regions_kernel, loss_grid(spatial, B), dim3(256), 0, (hipStream_t)stream, seg, region_words, out, R,
                     spatial);
  return e2e::check_launch("seg_to_regions_kernel");
}


// ---- deep-supervision targets: nearest-neighbour gather through per-axis index vectors (downsampling.py:87-107) ----
namespace {
__global__ __launch_bounds__(256) void ds_target_gather_kernel(const float* __restrict__ seg, float* __restrict__ out,
                                                               const int* __restrict__ idx_d, const int* __restrict__ idx_h,
                                                               const int* __restrict__ idx_w, int D, int H, int W, int d, int h,
                                                               int w, long long total) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int x = (int)(i % w);
  long long t = i / w;
  const int y = (int)(t % h);
  t /= h;
  const int z = (int)(t % d);
  const long long bc = t / d;
  out[i] = seg[((bc * D + idx_d[z]) * H + idx_h[y]) * W + idx_w[x]];
}
}  // namespace

extern "C" int e2e_ds_target_gather(const float* seg, float* out, const int* idx_d, const int* idx_h, const int* idx_w,
                                    int BC, int D, int H, int W, int d, int h, int w, void* stream) {
  E2E_REQUIRE(seg && out && idx_d && idx_h && idx_w, "ds_target_gather: null pointer");
  E2E_REQUIRE(BC > 0 && D > 0 && H > 0 && W > 0 && d > 0 && h > 0 && w > 0, "ds_target_gather: bad dims");
  const long long total = (long long)BC * d * h * w;
  hipLaunchKernelGGL(ds_target_gather_kernel, dim3((unsigned)e2e::cdivll(total, 256)), dim3(256), 0, (hipStream_t)stream, seg, out,
                     idx_d, idx_h, idx_w, D, H, W, d, h, w, total);
  return e2e::check_launch("ds_target_gather_kernel");
}
