// N3: the training loader's crop of one whole batch out of cases that live on the device (gfx950).
// Reference: DataLoader3D.generate_train_batch (e2enet/training/dataloading/dataset_loading.py:283-372): per sample np.copy of the
// valid box of the case, np.pad of the data (any numpy mode; the trainer uses 'constant') and np.pad of the seg with -1.
//
// Shape of the code.  Nothing is computed: every output word is a source word or a fill word, moved as 32-bit integers so that no bit
// of a NaN changes.  blockIdx.y names one output volume (sample b, channel c; channel C is the seg and goes to out_seg), blockIdx.x a
// span of LOADER_SPAN consecutive words of it.  The spans are cut on 16-byte boundaries of the OUTPUT ADDRESS, not of the volume: a
// volume of an odd patch (205^3) starts on any 4-byte phase, so a thread owns the aligned quad of words [4 g - a, 4 g - a + 4) of its
// volume (a = word phase of the volume's first word) and writes it with one 16-byte store; the up to three words in front of the first
// whole quad and behind the last one are written one by one by the threads that own those quads.  One writer per word, no atomics.
// A quad that lies in one output row takes one of three uniform routes: the row is outside the box (constant mode) -> four fill words
// and no load; the four source words are inside the row -> one 16-byte load that needs 4-byte alignment only (source rows start
// anywhere); otherwise, and for a quad that runs over the end of its row, word by word with the clamped / tested coordinate.  A wave
// covers 256 consecutive words, about one row of a training patch, so the lanes of a wave agree on the route except where a row meets
// the border of the box.  Coordinates: the span's first word is divided once per workgroup (uniform); a thread only divides numbers
// below 2^22 by the row length and the row count, which a float reciprocal and one correction do exactly.
#include "e2e_common.h"
#include <cstdint>

namespace {

constexpr int LOADER_MAX_BATCH = 32;
constexpr int LOADER_THREADS = 256;
constexpr int LOADER_UNROLL = 4;                                          // quads per thread
constexpr int LOADER_SPAN = LOADER_THREADS * LOADER_UNROLL * 4;          // words per workgroup: 16 KiB of output
constexpr int LOADER_MAX_EXTENT = 1 << 21;                               // per patch axis: small_div's numerators stay below 2^22

struct LoaderBatch { e2e_loader_rec_t rec[LOADER_MAX_BATCH]; };

// four words at any 4-byte boundary (global_load_dwordx4 needs no more)
struct __attribute__((packed, aligned(4))) Words4 { unsigned x, y, z, w; };

// n / d for n < 2^22 and 1 <= d: the float quotient is within one of the integer one
__device__ __forceinline__ int small_div(int n, int d, float rd) {
  int q = (int)((float)n * rd);
  const int r = n - q * d;
  if (r < 0) --q;
  if (r >= d) ++q;
  return q;
}

struct Box {
  const unsigned* chan;        // first word of the source channel
  int d, h, w, od, oh, ow;
  int mode;                    // 0: fill outside the box, 1: nearest voxel of the box
  unsigned fill;
};

__device__ __forceinline__ unsigned one_word(const Box& s, int z, int y, int x) {
  const int qz = s.od + z, qy = s.oh + y, qx = s.ow + x;
  const bool in = (unsigned)qz < (unsigned)s.d && (unsigned)qy < (unsigned)s.h && (unsigned)qx < (unsigned)s.w;
  if (s.mode == 0 && !in) return s.fill;
  const int cz = min(max(qz, 0), s.d - 1), cy = min(max(qy, 0), s.h - 1), cx = min(max(qx, 0), s.w - 1);
  return s.chan[((long long)cz * s.h + cy) * (long long)s.w + cx];
}

__global__ __launch_bounds__(LOADER_THREADS) void loader_crop_kernel(const LoaderBatch batch, int C, int pd, int ph, int pw, float rph,
                                                                     float rpw, unsigned* __restrict__ out_data,
                                                                     unsigned* __restrict__ out_seg, int data_mode, unsigned data_fill,
                                                                     unsigned seg_fill) {
  const int b = (int)blockIdx.y / (C + 1), c = (int)blockIdx.y - b * (C + 1);
  const e2e_loader_rec_t rec = batch.rec[b];
  const int n_vol = pd * ph * pw;                                        // (below 2^31 - LOADER_SPAN: checked by the caller)
  const bool is_seg = c == C;
  unsigned* __restrict__ out = is_seg ? out_seg + (long long)b * n_vol : out_data + ((long long)b * C + c) * n_vol;
  Box s;
  s.chan = reinterpret_cast<const unsigned*>(rec.src) + (long long)c * rec.d * rec.h * (long long)rec.w;
  s.d = rec.d; s.h = rec.h; s.w = rec.w;
  s.od = rec.off_d; s.oh = rec.off_h; s.ow = rec.off_w;
  s.mode = is_seg ? 0 : data_mode;
  s.fill = is_seg ? seg_fill : data_fill;

  const int a = (int)(((uintptr_t)out >> 2) & 3u);                       // word phase of the volume inside its 16-byte line
  const int v0 = (int)blockIdx.x * LOADER_SPAN;                          // first word of the span, counted from the line's start
  // the coordinates of the span's first word inside the volume (uniform)
  const int eb = max(v0 - a, 0);
  const int rowb = eb / pw, xb = eb - rowb * pw;
  const int zb = rowb / ph, yb = rowb - zb * ph;

#pragma unroll
  for (int u = 0; u < LOADER_UNROLL; ++u) {
    const int e = v0 + (u * LOADER_THREADS + (int)threadIdx.x) * 4 - a;   // the quad is words e .. e + 3 of the volume
    if (e >= n_vol) continue;
    const int ef = max(e, 0);                                            // (e < 0: only the volume's first quad)
    const int t = xb + (ef - eb);
    const int rows = small_div(t, pw, rpw);
    const int x = t - rows * pw;
    const int yy = yb + rows;
    const int planes = small_div(yy, ph, rph);
    const int y = yy - planes * ph;
    const int z = zb + planes;

    if (e >= 0 && e + 3 < n_vol && x + 3 < pw) {                         // a whole quad inside one output row
      uint4 v = make_uint4(s.fill, s.fill, s.fill, s.fill);
      const int qz = s.od + z, qy = s.oh + y, qx = s.ow + x;
      const bool row_in = (unsigned)qz < (unsigned)s.d && (unsigned)qy < (unsigned)s.h;
      if (s.mode == 1 || (row_in && qx + 3 >= 0 && qx < s.w)) {
        const int cz = min(max(qz, 0), s.d - 1), cy = min(max(qy, 0), s.h - 1);
        const unsigned* __restrict__ row = s.chan + ((long long)cz * s.h + cy) * (long long)s.w;
        if (qx >= 0 && qx + 3 < s.w) {
          const Words4 r = *reinterpret_cast<const Words4*>(row + qx);
          v = make_uint4(r.x, r.y, r.z, r.w);
        } else {
          unsigned r[4];
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const int xi = qx + i;
            const unsigned w = row[min(max(xi, 0), s.w - 1)];
            r[i] = (s.mode == 0 && (unsigned)xi >= (unsigned)s.w) ? s.fill : w;
          }
          v = make_uint4(r[0], r[1], r[2], r[3]);
        }
      }
      *reinterpret_cast<uint4*>(out + e) = v;
    } else {                                                             // over a row's end, or cut by the volume's ends
      int zi = z, yi = y, xi = x;
      const int last = min(e + 3, n_vol - 1);
      unsigned r[4];
      bool whole = e >= 0 && e + 3 < n_vol;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int ei = e + i;
        r[i] = 0u;
        if (ei >= ef && ei <= last) {
          r[i] = one_word(s, zi, yi, xi);
          if (++xi == pw) {
            xi = 0;
            if (++yi == ph) {
              yi = 0;
              ++zi;
            }
          }
        }
      }
      if (whole) {
        *reinterpret_cast<uint4*>(out + e) = make_uint4(r[0], r[1], r[2], r[3]);
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if (e + i >= ef && e + i <= last) out[e + i] = r[i];
      }
    }
  }
}

}  // namespace

extern "C" int e2e_loader_crop_max_batch(void) { return LOADER_MAX_BATCH; }

extern "C" int e2e_loader_crop(const e2e_loader_rec_t* recs, int B, int C, int pd, int ph, int pw, float* out_data, float* out_seg,
                               int data_mode, float data_fill, float seg_fill, void* stream) {
  E2E_REQUIRE(recs && out_data && out_seg, "loader_crop: null pointer");
  E2E_REQUIRE(B >= 1 && B <= LOADER_MAX_BATCH, "loader_crop: batch %d is outside [1, %d]", B, LOADER_MAX_BATCH);
  E2E_REQUIRE(C >= 1 && C + 1 <= 65535 / B, "loader_crop: %d data channels of %d samples are outside what one launch takes", C, B);
  E2E_REQUIRE((((uintptr_t)out_data | (uintptr_t)out_seg) & 3u) == 0u, "loader_crop: an output is not 4-byte aligned");
  E2E_REQUIRE(data_mode == 0 || data_mode == 1, "loader_crop: data_mode %d is neither 0 (constant) nor 1 (edge)", data_mode);
  E2E_REQUIRE(pd >= 1 && ph >= 1 && pw >= 1, "loader_crop: patch extent %d x %d x %d is not positive", pd, ph, pw);
  E2E_REQUIRE(pd <= LOADER_MAX_EXTENT && ph <= LOADER_MAX_EXTENT && pw <= LOADER_MAX_EXTENT &&
                  (long long)pd * ph * pw < (1ll << 31) - 2 * LOADER_SPAN,
              "loader_crop: patch %d x %d x %d has an axis above %d or 2^31 voxels", pd, ph, pw, LOADER_MAX_EXTENT);
  LoaderBatch batch;
  for (int b = 0; b < B; ++b) {
    const e2e_loader_rec_t& r = recs[b];
    E2E_REQUIRE(r.src, "loader_crop: sample %d has a null source", b);
    E2E_REQUIRE(r.d >= 1 && r.h >= 1 && r.w >= 1, "loader_crop: sample %d has the box extent %d x %d x %d, not positive", b, r.d, r.h,
                r.w);
    const int lim = 1 << 30;
    E2E_REQUIRE(r.off_d >= -lim && r.off_d <= lim && r.off_h >= -lim && r.off_h <= lim && r.off_w >= -lim && r.off_w <= lim,
                "loader_crop: sample %d has an offset (%d, %d, %d) outside [-2^30, 2^30]", b, r.off_d, r.off_h, r.off_w);
    batch.rec[b] = r;
  }
  for (int b = B; b < LOADER_MAX_BATCH; ++b) batch.rec[b] = recs[0];
  const long long n_vol = (long long)pd * ph * pw;
  const unsigned spans = (unsigned)e2e::cdivll(n_vol + 3, LOADER_SPAN);
  hipLaunchKernelGGL(loader_crop_kernel, dim3(spans, (unsigned)(B * (C + 1))), dim3(LOADER_THREADS), 0, (hipStream_t)stream, batch, C, pd, ph,
                     pw, 1.0f / (float)ph, 1.0f / (float)pw, reinterpret_cast<unsigned*>(out_data), reinterpret_cast<unsigned*>(out_seg),
                     data_mode, __builtin_bit_cast(unsigned, data_fill), __builtin_bit_cast(unsigned, seg_fill));
  return e2e::check_launch("loader_crop_kernel");
}
