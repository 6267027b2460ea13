// E2: label census of one (prediction, ground truth) pair of uint8 label volumes (gfx950): the joint table of (reference slot, test
// slot) voxel counts behind every confusion-matrix metric, and per slot the bounding box of its voxels in either volume (what
// scipy.ndimage.find_objects gives evaluation/surface_distance.py's label_boxes), in ONE pass that reads 2 B per voxel.
// Reference: ConfusionMatrix.compute (e2enet/evaluation/metrics.py:67-80) per label, i.e. four boolean passes per label and volume.
//
// Shape of the code.  The flat volume is cut into spans of 16 voxels (one 16-byte load of each volume per span; the voxels in front
// of the first 16-byte boundary and behind the last one are spans of fewer voxels, read byte by byte).  A thread keeps ONE open run
// in registers -- slot pair, voxel count, box -- across all its spans: a span whose 32 bytes are one pair (label maps are piecewise
// constant) extends the run with a handful of integer operations and touches no memory.  A run that ends goes to the workgroup's LDS
// histogram (4096 32-bit bins) and LDS boxes; a box word is written only when a plain read says the run lies outside it (a stale
// read only costs the atomic it could have saved).  The runs still open at the end are first summed across the wave per distinct
// pair, so 64 lanes of background are one LDS add.  The grid is fixed (CENSUS_WGS workgroups striding over chunks of CENSUS_CHUNK
// voxels); at the end a workgroup sends one global atomic per non-zero bin and per box word of a slot it met.  Integer atomics only:
// the same bits on every run.
#include "e2e_common.h"
#include <climits>
#include <cstdint>

namespace {

constexpr int CENSUS_SLOTS = 64;                       // 64 * 64 32-bit bins = 16 KiB of LDS
constexpr int CENSUS_THREADS = 256;
constexpr int CENSUS_UNROLL = 4;                       // spans a thread has in flight: 8 16-byte loads
constexpr int CENSUS_CHUNK = CENSUS_THREADS * CENSUS_UNROLL * 16;      // voxels a workgroup takes per loop trip
constexpr int CENSUS_WGS = 512;                        // two workgroups per CU

struct CensusLut { unsigned char slot[256]; };

struct Run {
  int key;                 // reference slot * 64 + test slot; -1: no run open
  unsigned count;
  int lo[3], hi[3];        // d, h, w; hi inclusive
};

struct CensusLds {
  unsigned hist[CENSUS_SLOTS * CENSUS_SLOTS];
  int lo[CENSUS_SLOTS][3];
  int hi[CENSUS_SLOTS][3];  // inclusive; -1: the workgroup met no voxel of the slot
  unsigned char lut[256];
};

__device__ __forceinline__ void lds_box(CensusLds& s, int slot, const Run& r) {
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    if (r.lo[a] < *(volatile int*)&s.lo[slot][a]) atomicMin(&s.lo[slot][a], r.lo[a]);
    if (r.hi[a] > *(volatile int*)&s.hi[slot][a]) atomicMax(&s.hi[slot][a], r.hi[a]);
  }
}

// the run's boxes go to LDS; its count too unless the caller sums counts across the wave first
__device__ __forceinline__ void flush(CensusLds& s, const Run& r, bool with_count) {
  if (r.key < 0) return;
  if (with_count) atomicAdd(&s.hist[r.key], r.count);
  const int rs = r.key >> 6, ts = r.key & 63;
  lds_box(s, rs, r);
  if (ts != rs) lds_box(s, ts, r);
}

__device__ __forceinline__ void open_run(Run& r, int key, int d, int h, int w) {
  r.key = key;
  r.count = 0u;
  r.lo[0] = r.hi[0] = d;
  r.lo[1] = r.hi[1] = h;
  r.lo[2] = r.hi[2] = w;
}

__device__ __forceinline__ void add_point(Run& r, int d, int h, int w) {
  r.lo[0] = min(r.lo[0], d); r.hi[0] = max(r.hi[0], d);
  r.lo[1] = min(r.lo[1], h); r.hi[1] = max(r.hi[1], h);
  r.lo[2] = min(r.lo[2], w); r.hi[2] = max(r.hi[2], w);
}

__device__ __forceinline__ unsigned byte_of(const uint4& v, int j) {
  const unsigned word = (j >> 2) == 0 ? v.x : (j >> 2) == 1 ? v.y : (j >> 2) == 2 ? v.z : v.w;
  return (word >> (8 * (j & 3))) & 255u;
}

__device__ __forceinline__ bool one_byte(const uint4& v) {
  return v.x == v.y && v.x == v.z && v.x == v.w && v.x == (v.x & 255u) * 0x01010101u;
}

// `count` (1..16) voxels from flat index i, whose coordinates are (d, h, w): bytes 0..count-1 of tv / rv
__device__ __forceinline__ void take_span(CensusLds& s, Run& run, const uint4& tv, const uint4& rv, int count, int d, int h, int w, int H,
                                          int W) {
  if (count == 16 && one_byte(tv) && one_byte(rv)) {
    const int key = (int)s.lut[rv.x & 255u] * 64 + (int)s.lut[tv.x & 255u];
    if (key != run.key) {
      flush(s, run, true);
      open_run(run, key, d, h, w);
    }
    run.count += 16u;
    // the last voxel of the span; a span that leaves its row holds that row's last voxel and the next row's first one, and the
    // same for planes: the endpoints and those full ranges are the exact box
    int d1 = d, h1 = h, w1 = w + 15;
    if (w1 >= W) {
      const int rows = w1 / W;
      w1 -= rows * W;
      h1 += rows;
      if (h1 >= H) {
        const int planes = h1 / H;
        h1 -= planes * H;
        d1 += planes;
      }
      add_point(run, d, h, 0);
      add_point(run, d, h, W - 1);
      if (d1 != d) {
        add_point(run, d, 0, 0);
        add_point(run, d, H - 1, 0);
      }
    }
    add_point(run, d, h, w);
    add_point(run, d1, h1, w1);
    return;
  }
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    if (j < count) {
      const int key = (int)s.lut[byte_of(rv, j)] * 64 + (int)s.lut[byte_of(tv, j)];
      if (key != run.key) {
        flush(s, run, true);
        open_run(run, key, d, h, w);
      }
      run.count += 1u;
      add_point(run, d, h, w);
      if (++w == W) {
        w = 0;
        if (++h == H) {
          h = 0;
          ++d;
        }
      }
    }
  }
}

__device__ __forceinline__ uint4 load_bytes(const unsigned char* __restrict__ p, int count) {
  unsigned w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
  for (int j = 0; j < 16; ++j)
    if (j < count) w[j >> 2] |= (unsigned)p[j] << (8 * (j & 3));
  return make_uint4(w[0], w[1], w[2], w[3]);
}

__global__ void census_init_kernel(unsigned long long* joint, int* boxes, int slots) {
  for (int i = threadIdx.x; i < slots * slots; i += blockDim.x) joint[i] = 0ull;
  for (int i = threadIdx.x; i < slots * 6; i += blockDim.x) boxes[i] = (i % 6) < 3 ? INT_MAX : 0;
}

// head: voxels in front of span 0 (0..15; they are span -1, taken by thread 0 of workgroup 0).  Spans 0 .. spans-1 start at
// head + 16 s; spans below vec_spans are whole and 16-byte aligned in BOTH volumes.
__global__ __launch_bounds__(CENSUS_THREADS) void census_kernel(const unsigned char* __restrict__ test, const unsigned char* __restrict__ ref,
                                                                const CensusLut lut, int slots, long long n, int head, long long spans,
                                                                long long vec_spans, int H, int W, unsigned long long* __restrict__ joint,
                                                                int* __restrict__ boxes) {
  __shared__ CensusLds s;
  for (int i = threadIdx.x; i < CENSUS_SLOTS * CENSUS_SLOTS; i += CENSUS_THREADS) s.hist[i] = 0u;
  for (int i = threadIdx.x; i < CENSUS_SLOTS * 3; i += CENSUS_THREADS) {
    s.lo[i / 3][i % 3] = INT_MAX;
    s.hi[i / 3][i % 3] = -1;
  }
  s.lut[threadIdx.x] = lut.slot[threadIdx.x];
  __syncthreads();

  Run run;
  run.key = -1;
  run.count = 0u;
#pragma unroll
  for (int a = 0; a < 3; ++a) { run.lo[a] = INT_MAX; run.hi[a] = -1; }

  if (blockIdx.x == 0 && threadIdx.x == 0 && head > 0) {
    const uint4 tv = load_bytes(test, head), rv = load_bytes(ref, head);
    take_span(s, run, tv, rv, head, 0, 0, 0, H, W);
  }
  const long long spans_per_chunk = CENSUS_THREADS * CENSUS_UNROLL;
  for (long long base = (long long)blockIdx.x * spans_per_chunk; base < spans; base += (long long)gridDim.x * spans_per_chunk) {
    uint4 tv[CENSUS_UNROLL], rv[CENSUS_UNROLL];
#pragma unroll
    for (int u = 0; u < CENSUS_UNROLL; ++u) {
      const long long sp = base + u * CENSUS_THREADS + threadIdx.x;
      if (sp < vec_spans) {
        tv[u] = *reinterpret_cast<const uint4*>(test + head + sp * 16);
        rv[u] = *reinterpret_cast<const uint4*>(ref + head + sp * 16);
      }
    }
#pragma unroll
    for (int u = 0; u < CENSUS_UNROLL; ++u) {
      const long long sp = base + u * CENSUS_THREADS + threadIdx.x;
      if (sp >= spans) continue;
      const long long i = head + sp * 16;
      const long long left = n - i;
      const int count = left < 16 ? (int)left : 16;
      if (sp >= vec_spans) {
        tv[u] = load_bytes(test + i, count);
        rv[u] = load_bytes(ref + i, count);
      }
      int d, h, w;
      if (n <= 0xFFFFFFFFll) {                       // (uniform: the 32-bit divisions are a fraction of the 64-bit ones)
        const unsigned row = (unsigned)i / (unsigned)W;
        w = (int)((unsigned)i - row * (unsigned)W);
        d = (int)(row / (unsigned)H);
        h = (int)(row - (unsigned)d * (unsigned)H);
      } else {
        const long long row = i / W;
        w = (int)(i - row * W);
        d = (int)(row / H);
        h = (int)(row - (long long)d * H);
      }
      take_span(s, run, tv[u], rv[u], count, d, h, w, H, W);
    }
  }

  // the runs still open: boxes lane by lane, counts summed per distinct pair across the wave (the loop is wave-uniform)
  flush(s, run, false);
  const int lane = threadIdx.x & 63;
  unsigned long long todo = __ballot(run.key >= 0);
  while (todo != 0ull) {
    const int leader = __ffsll((long long)todo) - 1;
    const int key = __shfl(run.key, leader, 64);
    const bool same = run.key == key;
    unsigned v = same ? run.count : 0u;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    if (lane == leader) atomicAdd(&s.hist[key], v);
    todo &= ~__ballot(same);
  }
  __syncthreads();

  for (int i = threadIdx.x; i < CENSUS_SLOTS * CENSUS_SLOTS; i += CENSUS_THREADS) {
    const unsigned c = s.hist[i];
    const int rs = i >> 6, ts = i & 63;
    if (c != 0u && rs < slots && ts < slots) atomicAdd(&joint[rs * slots + ts], (unsigned long long)c);
  }
  for (int i = threadIdx.x; i < CENSUS_SLOTS * 3; i += CENSUS_THREADS) {
    const int slot = i / 3, a = i % 3;
    if (slot < slots && s.hi[slot][a] >= 0) {
      atomicMin(&boxes[slot * 6 + a], s.lo[slot][a]);
      atomicMax(&boxes[slot * 6 + 3 + a], s.hi[slot][a] + 1);
    }
  }
}

}  // namespace

extern "C" int e2e_eval_census_max_slots(void) { return CENSUS_SLOTS; }
extern "C" long long e2e_eval_census_chunk(void) { return CENSUS_CHUNK; }
extern "C" int e2e_eval_census_workgroups(void) { return CENSUS_WGS; }

extern "C" int e2e_eval_census(const unsigned char* test, const unsigned char* reference, const unsigned char* lut, int slots, int D, int H,
                               int W, unsigned long long* joint, int* boxes, void* stream) {
  E2E_REQUIRE(D >= 1 && H >= 1 && W >= 1, "eval_census: every axis needs at least one voxel (got %d x %d x %d)", D, H, W);
  E2E_REQUIRE(test && reference && lut && joint && boxes, "eval_census: null pointer");
  E2E_REQUIRE(slots >= 1 && slots <= CENSUS_SLOTS, "eval_census: slots %d is outside [1, %d]", slots, CENSUS_SLOTS);
  CensusLut l;
  for (int v = 0; v < 256; ++v) {
    E2E_REQUIRE((int)lut[v] < slots, "eval_census: value %d maps to slot %d, there are %d slots", v, (int)lut[v], slots);
    l.slot[v] = lut[v];
  }
  const long long n = (long long)D * H * W;
  // 16-byte loads need both volumes on one 16-byte phase; otherwise every span is read byte by byte
  const int phase = (int)((16u - (unsigned)((uintptr_t)test & 15u)) & 15u);
  const bool vec = (((uintptr_t)test ^ (uintptr_t)reference) & 15u) == 0u;
  const int head = vec ? (int)(phase < n ? phase : n) : 0;
  const long long spans = e2e::cdivll(n - head, 16);
  const long long vec_spans = vec ? (n - head) / 16 : 0;
  const long long chunks = e2e::cdivll(spans * 16, CENSUS_CHUNK);
  const int wgs = (int)(chunks < 1 ? 1 : chunks < CENSUS_WGS ? chunks : CENSUS_WGS);
  // the LDS bins and a thread's run count are 32-bit: one workgroup must see fewer than 2^32 voxels
  E2E_REQUIRE((e2e::cdivll(chunks, wgs) + 1) * (long long)CENSUS_CHUNK < (1ll << 32),
              "eval_census: %lld voxels give one of %d workgroups 2^32 voxels or more", n, wgs);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(census_init_kernel, dim3(1), dim3(256), 0, st, joint, boxes, slots);
  hipLaunchKernelGGL(census_kernel, dim3((unsigned)wgs), dim3(CENSUS_THREADS), 0, st, test, reference, l, slots, n, head, spans, vec_spans, H,
                     W, joint, boxes);
  return e2e::check_launch("census_kernel");
}
