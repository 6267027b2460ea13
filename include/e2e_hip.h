/*
 * e2e_hip.h -- C ABI of libe2e_hip.so: the MI355X (gfx950) kernels of the E2ENet
 * shiftConvPP + DSFF hot path.
 *
 * The reference (boqian333/E2ENet-Medical) has no FFI: its hot path bottoms out in
 * PyTorch operators.  Every entry point below names the reference call site(s) whose
 * arithmetic it replaces (paths relative to the reference repo root).  Conventions:
 *   - all pointers are DEVICE pointers unless marked host; fp32 NCDHW activations;
 *   - no ownership transfer: the caller (PyTorch-ROCm tensors) owns every buffer,
 *     workspaces are passed in; nothing is allocated or synchronised inside;
 *   - `stream` is a hipStream_t passed as void*; calls are asynchronous on it and
 *     graph-capturable;
 *   - return 0 on success, negative E2E_ERR_* otherwise; e2e_last_error() returns a
 *     thread-local message.
 */
#ifndef E2E_HIP_H
#define E2E_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

#define E2E_OK 0
#define E2E_ERR_ARG (-1)
#define E2E_ERR_LAUNCH (-2)
#define E2E_ERR_UNSUPPORTED (-3)

const char* e2e_last_error(void);
int e2e_abi_version(void);
/* Diagnostics: name and launch shape of the kernel variant the last conv133 / convT entry point called on this
 * thread selected (size-dependent dispatch; the parity tests assert that the benchmarked shapes reach the intended
 * variants).  Thread-local, valid until the next call. */
const char* e2e_last_kernel(void);

/* One input plane (channel) of a convolution whose input is the *virtual* concatenation
 * [skip, up, down] (unetpp_d.py:453-478) followed by the restricted depth shift
 * (unetpp_d.py:45-59).  Neither the concat nor the shift is ever materialised: the load
 * stage reads plane `ptr` at depth d - dshift and applies the producer's InstanceNorm
 * affine + LeakyReLU on the fly (unetpp_d.py:111).                                      */
typedef struct {
  const float* ptr;     /* element [n=0, this channel, 0,0,0] of the source tensor        */
  const float* scale;   /* IN scale for (n=0, channel); NULL => raw source (no transform)  */
  const float* shift;   /* IN shift, same indexing                                        */
  long long nstride;    /* elements between batch items of the source tensor              */
  int ab_nstride;       /* elements between batch items of scale/shift (= source C)       */
  int dshift;           /* s(c): shifted[d] = x[d - s], zero outside                      */
  float slope;          /* LeakyReLU negative slope applied after the affine (1 = none)   */
  int reserved;
} e2e_in_chan_t;

/* One output plane of a scatter epilogue (conv dgrad): the gradient of virtual-concat
 * channel c computed at depth d is stored at depth d - dshift of `ptr` (un-shift on
 * store), `accumulate` != 0 adds to what is there.                                      */
typedef struct {
  float* ptr;
  long long nstride;
  int dshift;
  int accumulate;
} e2e_out_chan_t;

/* One channel of a fused InstanceNorm-backward reduction (round 4): the LAST writer of a gradient buffer holds the final dz of
 * every element it stores and writes, per 16 x 32 tile of every depth slice, this channel's  sum dz * lrelu'(u)  and
 * sum dz * lrelu'(u) * xhat  (u = scale * y + shift, xhat = (y - mean) * rstd; autograd of unetpp_d.py:99-100, :111) -- the
 * first pass of e2e_in_lrelu_bwd, which then only adds the tile records up (fixed order: deterministic) and runs its apply pass.
 * Records: part[((n * C + c) * np + tile) * 2 + {0, 1}], np = e2e_conv133_num_partials(D, H, W, 1, 1), every record of a
 * channel is written exactly once per launch (plain stores).  y == NULL: nothing to do for this channel.                    */
typedef struct {
  const float* y;        /* pre-norm plane of this channel (batch item 0) */
  const float* scale;    /* per-(n, c) coefficients of the channel at n = 0 ... */
  const float* shift;
  const float* mean;
  const float* rstd;
  double* part;          /* tile records of (n = 0, c) */
  long long nstride;     /* floats between batch items of y */
  long long part_nstride;   /* doubles between batch items of part (= 2 * C * np) */
  int ab_nstride;        /* elements between batch items of the coefficients (= C) */
  float slope;
} e2e_in_sum_chan_t;

/* ---- K1: 1x3x3 convolution, forward ------------------------------------------------
 * Replaces: torch_shift.forward (unetpp_d.py:45-59) + torch.cat (unetpp_d.py:453-478) +
 * nn.Conv3d k(1,3,3) pad(0,1,1) stride (sd,sh,sw) bias (unetpp_d.py:93,108) and the
 * statistics pass of nn.InstanceNorm3d (unetpp_d.py:99,111).
 *   chans   [Cin]            device table (see e2e_in_chan_t)
 *   w       [Cout,Cin,1,3,3] (DSFF-masked weights; dead kernels are exact zeros)
 *   live    quad words [ceil(Cout/4), ceil(Cin/8)] (quads_rows of e2e_dsff_expand_quads): bit (c%8)*4 + o%4 of
 *           word [o/4][c/8] set <=> kernel (o,c) is alive; NULL => dense
 *   y       [B,Cout,Do,Ho,Wo] pre-norm output, Do=(Di-1)/sd+1, Ho=(Hi-1)/sh+1, ...
 *   part    [B,Cout,np,3] per-tile (count, mean, M2) partials, fp64 (ABI 9; fp32 before), np =
 *           e2e_conv133_num_partials(Do,Ho,Wo,sh,sw); NULL => no statistics
 */
int e2e_conv133_num_partials(int Do, int Ho, int Wo, int sh, int sw);
int e2e_conv133_fwd(const e2e_in_chan_t* chans, int Cin, const float* w, const float* bias,
                    const unsigned* live, float* y, double* part, int B, int Cout, int Di, int Hi,
                    int Wi, int sd, int sh, int sw, void* stream);

/* Forward with a workspace: on the deep levels (planes no larger than a 16 x 16 tile, hundreds of input planes) the
 * input-plane chunks of a tile are split over several workgroups that store raw partial sums in `ws`
 * ([parts][B][Cout][Do][Ho][Wo]); a second kernel adds them up in a fixed order (deterministic), adds the bias and
 * writes the InstanceNorm partials.  e2e_conv133_fwd_ws_bytes returns the bytes this shape wants (0: it does not
 * split and e2e_conv133_fwd_splitk behaves exactly like e2e_conv133_fwd).                                              */
long long e2e_conv133_fwd_ws_bytes(int B, int Cin, int Cout, int Di, int Hi, int Wi, int sd, int sh, int sw);
int e2e_conv133_fwd_splitk(const e2e_in_chan_t* chans, int Cin, const float* w, const float* bias,
                           const unsigned* live, float* y, double* part, int B, int Cout, int Di, int Hi, int Wi,
                           int sd, int sh, int sw, float* ws, long long ws_bytes, void* stream);


/* ---- K6a: 1x3x3 convolution, data gradient ------------------------------------------
 * Replaces: autograd of the Conv3d + cat + torch_shift chain w.r.t. its inputs
 * (nnUNetTrainer_simple.py:572 l.backward()).
 *   dy    [B,Cout,Do,Ho,Wo] gradient w.r.t. the pre-norm conv output
 *   outs  [Cin] destinations, one per virtual-concat input channel (un-shift on store)
 *   live_t quad words [ceil(Cin/4), ceil(Cout/8)] (quads_cols of e2e_dsff_expand_quads); NULL => dense
 */
int e2e_conv133_dgrad(const float* dy, const float* w, const unsigned* live_t, const e2e_out_chan_t* outs,
                      int B, int Cin, int Cout, int Di, int Hi, int Wi, int sd, int sh, int sw, void* stream);

/* Data gradient with a workspace: the split-K form of the deep levels (see e2e_conv133_fwd_splitk); the parts hold raw
 * sums per virtual-concat channel, a second kernel adds them in a fixed order and applies the scatter epilogue (un-shift
 * on store, zero-fill, accumulate flag).  ws_bytes from e2e_conv133_dgrad_ws_bytes (0: this shape does not split).      */
long long e2e_conv133_dgrad_ws_bytes(int B, int Cin, int Cout, int Di, int Hi, int Wi, int sd, int sh, int sw);
int e2e_conv133_dgrad_splitk(const float* dy, const float* w, const unsigned* live_t, const e2e_out_chan_t* outs,
                             int B, int Cin, int Cout, int Di, int Hi, int Wi, int sd, int sh, int sw, float* ws,
                             long long ws_bytes, void* stream);


/* ---- K1s: DSFF-masked 1x3x3 convolution on a load-balanced plan (conv133_sparse.hip) ---------------------------------
 * The same operators as e2e_conv133_fwd / e2e_conv133_dgrad (unetpp_d.py:45-59, :453-478, :93/:108 and their autograd; the
 * mask is Masking's, core_channel.py:427-434) for stride-1 layers with planes wider than 16 voxels, Wi % 4 == 0 and more than
 * 8 channels on both sides (e2e_conv133_sparse_eligible).  The order in which input planes are chunked and the assignment of
 * output planes to the eight waves of a workgroup are chosen on the HOST from the kernel map so that every wave carries the same
 * work in every chunk; weights are read from a packed copy in that order.
 *   e2e_conv133_sparse_plan    host function.  kmask [R][Cc] uint8 in HOST memory (weight dims 0 and 1); transpose 0: forward
 *       (Q = R output planes, P = Cc input planes), 1: data gradient (Q = Cc virtual-concat channels, P = R dy channels).  Writes
 *       (host arrays) qslot [groups*32] (output plane of slot wave*4 + a, -1 empty), pslot [groups*nchunks*8] (input plane of each
 *       chunk slot, -1 empty; the same chunking for every group: they share the staged planes through L2), quads
 *       [groups*8*nchunks] (bit cl*4 + a of word [group][wave][chunk] <=> kernel alive), woff [groups*nchunks*8] (first slot of
 *       each wave's kernel list inside the chunk's packed block), kmax (slots of a block = the most live kernels of any chunk) and
 *       flush_every (chunks per flush of the two-level summation); groups = ceil(Q/32), nchunks = ceil(P/8).  A pure function of
 *       the kernel map (every data-parallel rank derives the same plan).
 *   e2e_conv133_sparse_pack    device: packed weights [groups][nchunks][kmax][12] -- only the LIVE kernels, wave by wave in walk
 *       order -- for a TABLE of jobs in one launch (run it after every optimizer step / parameter load).  reverse = 1 flips the
 *       taps (data gradient).
 *   e2e_conv133_fwd_sparse     chans_plan [groups][nchunks*8]: the e2e_in_chan_t of pslot's planes (ptr NULL for empty slots)
 *   e2e_conv133_dgrad_sparse   pslot_t as returned by the plan (dy channels); outs_plan [groups][32]: the e2e_out_chan_t of
 *       qslot's channels (ptr NULL for empty slots); insum_plan (optional, same order): channels whose gradient buffer this
 *       launch writes LAST also get their InstanceNorm-backward sums here (e2e_in_sum_chan_t)                                                                          */
typedef struct {
  const float* w;            /* the layer's weight tensor */
  float* wpk;                /* e2e_conv133_sparse_wpk_floats(P, Q) floats */
  const int* qslot;          /* device copies of the plan arrays */
  const int* pslot;
  const unsigned* quads;
  const int* woff;
  int groups, nchunks;
  int wq_stride, wp_stride;  /* element strides of w for (output plane, input plane): forward (Cin*9, 9), data gradient (9, Cin*9) */
  int reverse;
  int kmax;
} e2e_sparse_pack_job_t;
int e2e_conv133_sparse_eligible(int Cin, int Cout, int Di, int Hi, int Wi, int sd, int sh, int sw);
long long e2e_conv133_sparse_wpk_floats(int P, int Q, int kmax);
int e2e_conv133_sparse_plan(const unsigned char* kmask_host, int R, int Cc, int transpose, int* qslot, int* pslot, unsigned* quads,
                            int* woff, int* kmax, int* flush_every);
int e2e_conv133_sparse_pack(const e2e_sparse_pack_job_t* jobs, int njobs, long long max_threads, void* stream);
int e2e_conv133_fwd_sparse(const e2e_in_chan_t* chans_plan, int Cin, const float* wpk, const float* bias, const unsigned* quads,
                           const int* woff, int kmax, const int* qslot, int flush_every, float* y, double* part, int B, int Cout,
                           int Di, int Hi, int Wi, void* stream);
int e2e_conv133_dgrad_sparse(const float* dy, const float* wpk_t, const unsigned* quads_t, const int* woff_t, int kmax_t,
                             const int* pslot_t, const e2e_out_chan_t* outs_plan, const e2e_in_sum_chan_t* insum_plan /* [groups][32] or NULL */,
                             int flush_every, int B, int Cin, int Cout, int Di, int Hi, int Wi, void* stream);

/* ---- K1m (round 5): the same operators as e2e_conv133_fwd / e2e_conv133_dgrad (unetpp_d.py:45-59, :453-478, :93/:108 and their
 * autograd; DSFF-pruned kernels contribute nothing: they are packed as zeros from `live`, core_channel.py:427-434) as a GEMM on the
 * fp16 matrix pipe with fp32-exact two-piece operands (three matrix products per fp32 product; conv133_mm.hip) -- every stride-1
 * layer with Wi % 32 == 0, Hi % 16 == 0, Hi > 16 and 17..320 channels on both sides, masked or not.
 *   wpk         the layer's packed weights of this direction: a buffer of e2e_conv133_mm_ws_bytes(...) bytes (0: shape not served)
 *               that e2e_conv133_mm_pack filled -- ONE launch pair for all layers and both directions, after an optimizer step or a
 *               parameter load (round 6; until round 5 every conv launch re-packed its weights)
 *   w_absmax    the device word e2e_conv133_mm_pack recorded max |w| in (its power-of-two scale); NULL: packed with the fixed 2^8
 *   x_absmax    NULL, or a device word holding (a bound of) max |x| over all input planes after normalise-on-load
 *               (e2e_conv133_input_ranges derives one from the parameters; e2e_absmax_word measures one): the activations are
 *               moved into the fp16 range by the power of two it implies.  NULL keeps the fixed 2^3 of round 5: |x| > 8188 -> Inf
 *   dy_absmax   NULL, or the word e2e_in_lrelu_bwd(dy_absmax) left behind for this dy: its power-of-two scale (without it dy is
 *               taken as it is: only for O(1) test data -- full-resolution gradients of 1e-7 are below the fp16 range)
 *   outs        as e2e_conv133_dgrad; destinations with `accumulate` set are updated by no-return global_atomic_add_f32 -- every element
 *               by exactly one lane per launch, launches stream-ordered: the same value as a load / add / store and deterministic;
 *               the buffers must be device (coarse-grained) memory */
typedef struct {
  const float* w;            /* the layer's weight tensor [Cout, Cin, 1, 3, 3] */
  const unsigned* quads;     /* DSFF liveness quad words of this direction (e2e_dsff_expand_quads) or NULL (dense) */
  void* wpk;                 /* e2e_conv133_mm_ws_bytes(...) bytes */
  unsigned* w_absmax;        /* one word per layer (shared by its two directions) */
  int P, Q;                  /* reduction-side / output-side channels: forward (Cin, Cout), data gradient (Cout, Cin) */
  int wq_stride, wp_stride;  /* element strides of w for (output-side, reduction-side) channel: forward (Cin*9, 9), data gradient (9, Cin*9) */
  int reverse;               /* data gradient: taps reversed */
  int owns_absmax;           /* this job computes *w_absmax (one job per layer) */
} e2e_mm_pack_job_t;
typedef struct {
  int kind;                  /* 0 none, 1 normalised source (or its max-pool), 2 transposed conv of a normalised source, 3 measured word,
                              * 4 max |w| over N floats, 5 max over channels [C, C + wks) of sum_{o, tap} |w[o, c, tap]|, w [wCout][N][9] */
  int C;                     /* channels of the normalised tensor */
  long long N;               /* voxels per instance of the normalised tensor */
  const float* gamma;        /* [C] instnorm.weight of its producer */
  const float* beta;         /* [C] instnorm.bias */
  const float* w;            /* kind 2: transposed-conv weight [C, wCout, wks] */
  int wCout, wks;
  const unsigned* word;      /* kind 3 */
} e2e_range_src_t;
typedef struct {
  e2e_range_src_t src[3];    /* the concat sources of one conv (reference unetpp_d.py:453-478) */
  unsigned* out;             /* bit pattern of the bound of |x| over all of them */
} e2e_range_job_t;
long long e2e_conv133_mm_ws_bytes(int B, int Cin, int Cout, int Di, int Hi, int Wi, int sd, int sh, int sw);
/* jobs: DEVICE table; max_elems >= the largest ceil(Q/32)*ceil(P/16)*9*512 of the table */
int e2e_conv133_mm_pack(const e2e_mm_pack_job_t* jobs, int njobs, long long max_elems, void* stream);
/* jobs: DEVICE table, one per range word (a conv's input planes; a transposed conv's activations, weights, dy factor);
 * ws: e2e_conv133_input_ranges_ws_bytes(njobs) bytes of scratch (two launches: partial maxima, fold) */
long long e2e_conv133_input_ranges_ws_bytes(int njobs);
int e2e_conv133_input_ranges(const e2e_range_job_t* jobs, int njobs, void* ws, void* stream);
/* *word = bit pattern of max |x| over n floats (a non-finite element gives +Inf) */
int e2e_absmax_word(const float* x, long long n, unsigned* word, void* stream);
int e2e_conv133_fwd_mm(const e2e_in_chan_t* chans, int Cin, const void* wpk, const unsigned* w_absmax, const float* bias,
                       const unsigned* x_absmax, float* y, double* part, int B, int Cout, int Di, int Hi, int Wi, void* stream);
int e2e_conv133_dgrad_mm(const float* dy, const unsigned* dy_absmax, const void* wpk_t, const unsigned* w_absmax,
                         const e2e_out_chan_t* outs, int B, int Cin, int Cout, int Di, int Hi, int Wi, void* stream);

/* ---- K6b: 1x3x3 convolution, weight gradient (dense: also for dead kernels, because the
 * reference's clip_grad_norm_ runs over all gradients, nnUNetTrainer_simple.py:573) ----
 *   dw   [Cout,Cin,1,3,3] (overwritten)
 *   ws   workspace of e2e_conv133_wgrad_ws_bytes(...) bytes
 */
long long e2e_conv133_wgrad_ws_bytes(int B, int Cin, int Cout, int Di, int Hi, int Wi, int sd, int sh, int sw);
/*   dy_absmax  NULL, or the device word e2e_in_lrelu_bwd(dy_absmax) left behind for this dy (bit pattern of max |dy|).  With it,
 *              the shapes served by the matrix-pipe kernel run on fp16 two-piece operands (three products per fp32 product, dy
 *              pre-scaled by the power of two that puts its maximum in [2^14, 2^15)); without it on bf16 three-piece operands
 *              (six products, no range assumption).  Both are fp32-exact to the last two bits of an operand. */
/*   x_absmax   NULL, or the word e2e_conv133_input_ranges / e2e_absmax_word produced for this conv's input planes: the power-of-two
 *              scale of the activations in the fp16 two-piece kernel (NULL: the fixed 2^3 of round 5, |x| > 8188 -> Inf) */
int e2e_conv133_wgrad(const e2e_in_chan_t* chans, const float* dy, float* dw, void* ws, int B, int Cin,
                      int Cout, int Di, int Hi, int Wi, int sd, int sh, int sw, const unsigned* dy_absmax,
                      const unsigned* x_absmax, void* stream);

/* Diagnostic (the numerics gate of the split-operand matrix paths, tests/test_gpu_ops.py): D[32][32] = A[32][K] Bt[32][K]^T through the
 * split functions of csrc/e2e_split.h and the product orders of the matrix-pipe kernels.  mode 0: bf16 three-piece operands, six
 * products (the bf16 weight gradient K6b, the bf16 transposed convs, the dense conv K1d); 1: fp16 two-piece operands split by
 * convert-and-subtract, three products, Bt pre-scaled by the power of two derived from *absmax_b (NULL: unscaled) exactly as dy is
 * in e2e_conv133_wgrad (the fp16 weight gradient K6b); 2: fp32-input MFMA (an fp32 FMA chain: the fp32 kernels); 3: as 1 with the
 * fma-mix split (K1m, the fp16 transposed convs).  K % 16 == 0.  No reference counterpart (torch computes in fp32). */
int e2e_diag_split_gemm(const float* A, const float* Bt, float* D, int K, int mode, const unsigned* absmax_b, void* stream);

/* Diagnostic, host only (no GPU call): the store rule of e2e_out_chan_t as every data-gradient kernel applies it
 * (csrc/e2e_concat.h: concat_store_slice).  The workgroups of (shifted) depth d of a D-slice volume, destination shift `dshift`:
 * *dd = the source slice they own; returns what they do with it: 0 store, 1 add (accumulate != 0), 2 zero-fill (the slice
 * receives nothing and this launch is the buffer's first writer), 3 skip (it receives nothing and holds earlier writers' values). */
int e2e_diag_concat_slice(int d, int dshift, int D, int accumulate, int* dd);

/* Diagnostic, host only (no GPU call): the tile walk and slab layout of e2e_conv133_wgrad for a shape, through the plan the size
 * query and the launch share and the functions the kernels walk with (csrc/e2e_wgrad.h).  For workgroup column `chunk` of the
 * launch grid and the `tile`-th tile it walks: out[0..19] = chunks, pairs (the launch grid), slabs (what e2e_conv133_wgrad_ws_bytes
 * counts), 1 if chunks never cross a batch item else 0, tiles per batch item, tiles in all, the chunk's tile range [lo, hi) as indices
 * over all tiles, the batch items of its first and last tile, the first and last slab its workgroups write, the tile's batch item and
 * origin (n, d0, h0, w0) in the output volume, the tile's extent (nd, th, tw), slabs per workgroup.  Returns the path (0 s2, 1 smallc,
 * 2 split-operand on 4 x 32 tiles, 3 v3, 4 split-operand on 8 x 16 tiles, 5 v2, 6 v1), or -1 when chunk or tile is out of range. */
int e2e_diag_wgrad_walk(int B, int Cin, int Cout, int Di, int Hi, int Wi, int sd, int sh, int sw, int chunk, int tile, long long out[20]);

/* Diagnostic: the shader clock the hot kernels ran at.  Workgroup 0 of every launch of family 0 (K1m, conv133_mm) / 1 (the
 * matrix-pipe K1w, conv133_wgrad v5) adds its s_memtime span (shader-clock cycles) and its s_memrealtime span (100 MHz) to a
 * device-side pair; this call synchronises the device and returns *mhz = cycles / time over all launches since the last reset
 * (0 if none) and *busy_ms = that time (may be NULL).  bench.py prices roofline.frac_at_measured_clock with it.  No reference
 * counterpart. */
int e2e_diag_kernel_clock(int family, double* mhz, double* busy_ms, int reset);

/* ---- K2: InstanceNorm statistics finalize --------------------------------------------
 * Replaces: nn.InstanceNorm3d(eps, affine, instance statistics) (unetpp_d.py:99,111):
 * combines the per-tile partials (Chan) in fp64 and emits per-(n,c)
 *   scale = gamma * rstd, shift = beta - mean * gamma * rstd   (consumed on load), mean, rstd.
 */
int e2e_in_stats_finalize(const double* part, int np, const float* gamma, const float* beta, float eps,
                          float* scale, float* shift, float* mean, float* rstd, int B, int C, void* stream);

/* ---- K7: InstanceNorm + LeakyReLU backward -------------------------------------------
 * Given dz = dL/d(lrelu(IN(y))) and the saved pre-norm y, overwrite dz with dy = dL/dy and
 * produce dgamma, dbeta (accumulated over the batch) and dbias = sum(dy).
 *   sums  workspace of e2e_in_lrelu_bwd_ws_doubles(B, C) doubles (s1 = sum du, s2 = sum du*xhat per (n, c); the per-block
 *         records of the first pass; the per-block sum dy records of the apply pass); no state survives a call (round 6: every
 *         sum is formed from per-block records in a fixed order -- no atomics, no zeroing launch, bit-reproducible gradients)
 *   tile_sums  NULL: the first pass (s1, s2) runs here.  Otherwise the per-tile records [B][C][np][2] that the last writers of
 *              dz have produced (e2e_in_sum_chan_t): they are added up in a fixed order and only the apply pass runs
 *   dy_absmax  NULL, or one device word that receives the bit pattern of max |dy| over the tensor (consumed by e2e_conv133_wgrad)
 *   scale, shift  the arrays e2e_in_stats_finalize produced for this tensor: the LeakyReLU branch of an element is decided from
 *              u = fma(y, scale, shift) -- bit for bit the value every forward consumer formed (normalise-on-load), so the backward
 *              differentiates exactly the function the forward evaluated (until round 5 it was re-derived as gamma * xhat + beta,
 *              whose sign differs for |u| ~ 1e-7: found by the same-branch gradient check of tests/test_gpu_configs.py)
 */
long long e2e_in_lrelu_bwd_ws_doubles(int B, int C);
int e2e_in_lrelu_bwd(float* dz_dy, const float* y, const float* mean, const float* rstd, const float* scale, const float* shift,
                     const float* gamma, float slope, float* dgamma, float* dbeta, float* dbias, float* sums,
                     int B, int C, long long spatial, const double* tile_sums, int np, unsigned* dy_absmax, void* stream);

/* ---- K3: transposed convolution, kernel == stride in {1,2}^3, no bias ------------------
 * Replaces: nn.ConvTranspose3d(Cin,Cout,k,k,bias=False) (unetpp_d.py:521-522).
 *   x   [B,Cin,D,H,W] pre-norm producer output + (scale,shift) [B,Cin] (NULL => raw), slope
 *   w   [Cin,Cout,kd,kh,kw];  live [Cout, ceil(Cin/32)] bits or NULL
 *   y   [B,Cout,D*kd,H*kh,W*kw]
 * Operand ranges (round 6): the matrix-pipe kernels (kw == 2, W % 32 == 0 ...) run on fp16 TWO-piece operands -- three matrix
 * products per fp32 product instead of the six of the bf16 three-piece form -- when the caller hands over the device words that
 * bound their operands (e2e_conv133_input_ranges: x_absmax = kind 1 of the source, w_absmax = kind 4 of w, dy_bound_b = kind 5 of
 * the conv that consumes y, dy_bound_a = that conv's dy_absmax word of e2e_in_lrelu_bwd; the bound of dy is their product); with
 * NULL words (or E2E_CT_H2=0) they keep the bf16 form, which needs no range. */
int e2e_convT_fwd(const float* x, const float* scale, const float* shift, float slope, const float* w,
                  const unsigned* live, float* y, int B, int Cin, int Cout, int D, int H, int W, int kd,
                  int kh, int kw, const unsigned* x_absmax, const unsigned* w_absmax, void* stream);
/* dgrad: dx (gradient w.r.t. the *post-activation* input) [B,Cin,D,H,W]; accumulate != 0 adds.
 * live_t [Cin, ceil(Cout/32)] or NULL. */
int e2e_convT_dgrad(const float* dy, const float* w, const unsigned* live_t, float* dx, int accumulate, int B,
                    int Cin, int Cout, int D, int H, int W, int kd, int kh, int kw, const unsigned* w_absmax,
                    const unsigned* dy_bound_a, const unsigned* dy_bound_b, void* stream);
/* wgrad (dense): dw [Cin,Cout,kd,kh,kw] overwritten; ws of e2e_convT_wgrad_ws_bytes bytes. */
long long e2e_convT_wgrad_ws_bytes(int B, int Cin, int Cout, int D, int H, int W, int kd, int kh, int kw);
int e2e_convT_wgrad(const float* x, const float* scale, const float* shift, float slope, const float* dy,
                    float* dw, void* ws, int B, int Cin, int Cout, int D, int H, int W, int kd, int kh, int kw,
                    const unsigned* x_absmax, const unsigned* dy_bound_a, const unsigned* dy_bound_b, void* stream);

/* ---- K4: max pooling, kernel == stride ------------------------------------------------
 * Replaces: nn.MaxPool3d(k) (unetpp_d.py:523-524) on a normalise-on-load source. */
int e2e_maxpool_fwd(const float* x, const float* scale, const float* shift, float slope, float* y, int B, int C,
                    int D, int H, int W, int kd, int kh, int kw, void* stream);
/* dx [B,C,D,H,W] (w.r.t. the post-activation input; first maximum in scan order wins, as ATen). */
/* mean / rstd / tile_sums (all NULL: plain pooling backward): when this launch writes dx LAST it also forms the per-block records
 * of the source's InstanceNorm-backward sums (see e2e_in_sum_chan_t; records [B*C][e2e_maxpool_bwd_num_records(..)][2], consumed
 * by e2e_in_lrelu_bwd(tile_sums, np)); e2e_maxpool_bwd_num_records returns 0 for shapes that cannot carry them.            */
int e2e_maxpool_bwd_num_records(int D, int H, int W, int kd, int kh, int kw);
int e2e_maxpool_bwd(const float* x, const float* scale, const float* shift, float slope, const float* dy,
                    float* dx, int accumulate, int B, int C, int D, int H, int W, int kd, int kh, int kw,
                    const float* mean, const float* rstd, double* tile_sums, void* stream);

/* ---- K5: 1x1x1 segmentation head, no bias ----------------------------------------------
 * Replaces: nn.Conv3d(C,K,1,bias=False) (unetpp_d.py:394-401, used :480-483). */
int e2e_head1x1_fwd(const float* x, const float* scale, const float* shift, float slope, const float* w,
                    float* logits, int B, int C, int K, long long spatial, void* stream);
int e2e_head1x1_dgrad(const float* dlogits, const float* w, float* dx, int accumulate, int B, int C, int K,
                      long long spatial, void* stream);
long long e2e_head1x1_wgrad_ws_bytes(int B, int C, int K, long long spatial);
int e2e_head1x1_wgrad(const float* x, const float* scale, const float* shift, float slope,
                      const float* dlogits, float* dw, void* ws, int B, int C, int K, long long spatial,
                      void* stream);

/* ---- K8: softmax + soft-Dice + cross-entropy, forward and gradient ----------------------
 * Replaces: DC_and_CE_loss (dice_loss.py:302-359, :156-192, :100-153, crossentropy.py:4-12) for one
 * deep-supervision scale; MultipleOutputLoss2 weights (deep_supervision.py:31-43) enter as `weight`.
 *   target  [B,1,spatial] float labels;  acc [B,K,3]+[1] fp64 workspace (tp,fp,fn ; ce sum) zeroed by caller
 *   loss_out: *loss_out += weight * (ce + dice)   (device scalar, fp32)
 *   dlogits [B,K,spatial] = weight * dL/dlogits
 */
long long e2e_loss_ws_bytes(int B, int K);
int e2e_dc_ce_reduce(const float* logits, const float* target, void* acc, int B, int K, long long spatial,
                     void* stream);
int e2e_dc_ce_grad(const float* logits, const float* target, const void* acc, float weight, int batch_dice,
                   float smooth, float* dlogits, float* loss_out, int B, int K, long long spatial, void* stream);
/* dlogits may be NULL: loss value only (validation batches, nnUNetTrainer_simple.py:980-988).  A label outside [0, K)
 * turns the loss NaN (torch's CrossEntropyLoss raises).
 * Data-parallel batch dice (reference nnUNetTrainerV2_DDP.py:263-268 all-gathers the per-sample dice numerators and
 * denominators): e2e_dc_ce_fold_batch folds acc's [B][K][3] rows into row 0 (rows 1.. zeroed, K >= 1); the host all-reduces the
 * 3*K doubles of row 0 over the ranks (RCCL) between e2e_dc_ce_reduce and e2e_dc_ce_grad(batch_dice = 1).           */
int e2e_dc_ce_fold_batch(void* acc, int B, int K, void* stream);
/* Online evaluation of a validation batch (nnUNetTrainer_simple.py:373-405): hard tp / fp / fn voxel counts of
 * argmax(softmax(logits)) against the target per class, summed over the batch.  counts [K][3] int64 (zeroed by callee). */
int e2e_online_eval_counts(const float* logits, const float* target, long long* counts, int B, int K,
                           long long spatial, void* stream);

/* ---- K8r: sigmoid + soft-Dice + binary cross-entropy over overlapping label regions -----
 * Replaces: DC_and_BCE_loss (dice_loss.py:362-387) = BCEWithLogitsLoss() + SoftDiceLoss(sigmoid, batch_dice, do_bg=True,
 * smooth) for one deep-supervision scale, the loss of nnUNetTrainerV2BraTSRegions; 1 <= R <= 32 regions, which may overlap.
 *   logits  [B,R,spatial];  acc as K8: [B,R,3]+[1] fp64 (tp,fp,fn ; BCE sum), e2e_loss_ws_bytes(B, R), zeroed by the callee;
 *           e2e_dc_ce_fold_batch(acc, B, R) serves the data-parallel batch dice as for K8
 *   target, region_words: two forms of the same targets, which give bit-identical results on equivalent inputs
 *     region_words != NULL: target is the [B,1,spatial] float label map and region_words a device uint32[R], bit t of
 *           word r = "label t belongs to region r"; y_r = (word[r] >> t) & 1 is formed on load and no R-channel target is
 *           written or read (ConvertSegmentationToRegionsTransform, custom_transforms.py:96-123, fused).  Labels outside
 *           [0, 32) and values that are not whole numbers belong to no region, as in the reference's `seg == l` loop
 *     region_words == NULL: target is a multi-hot [B,R,spatial] float tensor, y = (value >= 0.5)
 *   loss = mean over B*R*spatial of [max(l,0) - l y + log1p(exp(-|l|))] - mean over the M dice terms of
 *          (2tp + smooth) / (2tp + fp + fn + smooth + 1e-8), M = B*R (batch_dice: R); finite at |l| = 100 and for a region
 *          absent from a sample with smooth = 0 (dc = 0, zero dice gradient)
 *   loss_out: *loss_out += weight * loss;   dlogits [B,R,spatial] = weight * dL/dlogits, NULL = loss value only
 *   Planes whose pointers and spatial size allow it are read as dwordx4; the order of the sums does not depend on that.   */
int e2e_dc_bce_reduce(const float* logits, const float* target, const unsigned* region_words, void* acc, int B, int R,
                      long long spatial, void* stream);
int e2e_dc_bce_grad(const float* logits, const float* target, const unsigned* region_words, const void* acc, float weight,
                    int batch_dice, float smooth, float* dlogits, float* loss_out, int B, int R, long long spatial,
                    void* stream);
/* Online evaluation of a region model (nnUNetTrainerV2BraTSRegions.py:168-189): hard tp / fp / fn voxel counts per region of
 * sigmoid(l) > 0.5 against y, summed over the batch; both target forms.  The kernel tests l > 0, the same predicate (a logit
 * of exactly 0 is a negative).  counts [R][3] int64 (zeroed by callee).                                                    */
int e2e_online_eval_regions(const float* logits, const float* target, const unsigned* region_words, long long* counts, int B,
                            int R, long long spatial, void* stream);
/* ConvertSegmentationToRegionsTransform (custom_transforms.py:96-123): seg [B,1,spatial] float labels -> out [B,R,spatial]
 * float 0/1 through the region words (see above).                                                                        */
int e2e_seg_to_regions(const float* seg, const unsigned* region_words, float* out, int B, int R, long long spatial,
                       void* stream);

/* Deep-supervision targets (the loss-side end of the input feed): reference
 * e2enet/training/data_augmentation/downsampling.py:87-107 (downsample_seg_for_ds_transform2, order 0) resizes the label
 * map to every deep-supervision scale with batchgenerators' resize_segmentation -> skimage.transform.resize(order=0,
 * mode="edge", anti_aliasing=False), which in scikit-image 0.19.3 is scipy.ndimage.zoom(order=0, mode="nearest",
 * grid_mode=True): out[j] = in[floor((j + 0.5) * in_size / out_size)] per axis.  The host computes the three index vectors
 * in float64 exactly like scipy's zoom; this kernel gathers.  seg [BC][D][H][W] -> out [BC][d][h][w].                 */
int e2e_ds_target_gather(const float* seg, float* out, const int* idx_d, const int* idx_h, const int* idx_w,
                         int BC, int D, int H, int W, int d, int h, int w, void* stream);


/* ---- K10: clip_grad_norm_ + SGD(nesterov) + DSFF mask, multi-tensor ---------------------
 * Replaces: torch.nn.utils.clip_grad_norm_(params, 12) + torch.optim.SGD.step (nnUNetTrainer_simple.py:573-574,
 * :369-370) + Masking.apply_mask (core_channel.py:427-434).
 *   table: device array of n entries {param, grad, momentum, mask-or-NULL, numel} */
typedef struct {
  float* param;
  const float* grad;
  float* momentum;
  const float* mask;
  long long numel;
} e2e_param_t;
int e2e_grad_sqnorm(const e2e_param_t* table, int n, double* sq_out /* device, zeroed by callee */, void* stream);
int e2e_sgd_clip_mask_step(const e2e_param_t* table, int n, const double* sq_norm, float max_norm, float lr,
                           float weight_decay, float momentum, int nesterov, int first_step, void* stream);
int e2e_apply_mask(const e2e_param_t* table, int n, void* stream);

/* ---- K9: DSFF kernel statistics ---------------------------------------------------------
 * Replaces: the three chained torch.sum(|w|, dim=-1) of kernel_death (core_channel.py:652-655; the association
 * order is reproduced bit for bit), torch.sort + threshold (:658-661) as an exact k-th order statistic
 * (radix select), and the liveness bit tables consumed by K1/K3/K6.
 *   w [R, Cc, kd,kh,kw] -> l1 [R*Cc] */
int e2e_dsff_kernel_l1(const float* w, float* l1, int R, int Cc, int kd, int kh, int kw, void* stream);
/* kth: value of the k-th smallest (0-based) of n non-negative floats; ws >= 4096 bytes */
int e2e_dsff_kth_value(const float* v, int n, int k, float* out, void* ws, void* stream);
/* kmask [R*Cc] u8: kmask &= !(l1 <= *thr) */
int e2e_dsff_death(const float* l1, const float* thr, unsigned char* kmask, int n, void* stream);
/* growth_mode='gradient' (Masking.kernel_grad_growth, core_channel.py:771-790): score [R*Cc*kd] = sum_kh(sum_kw |grad|) of
 * dead kernels (0 for live ones; two chained sums, the kernel's depth extent stays), grad [R,Cc,kd,kh,kw] scaled by the
 * clip_grad_norm_ coefficient max_norm / (sqrt(*sq_norm) + 1e-6) clamped to 1 (sq_norm NULL: taken as it is);
 * then kmask[i / kd] = 1 where score[i] > *thr (thr = the (num_growth)-th largest score: e2e_dsff_kth_value) */
int e2e_dsff_grad_score(const float* grad, const double* sq_norm, float max_norm, const unsigned char* kmask, float* score,
                        int R, int Cc, int kd, int kh, int kw, void* stream);
int e2e_dsff_grow_above(const float* score, const float* thr, unsigned char* kmask, int R, int Cc, int kd, void* stream);
/* expand a kernel-granular u8 map to the fp32 element mask [R,Cc,ks] and to liveness bit tables:
 * bits_rows [R, ceil(Cc/32)] and bits_cols [Cc, ceil(R/32)] (either may be NULL) */
int e2e_dsff_expand(const unsigned char* kmask, float* mask, unsigned* bits_rows, unsigned* bits_cols, int R,
                    int Cc, int ks, void* stream);
/* liveness "quad words" consumed by e2e_conv133_fwd / e2e_conv133_dgrad (4 output planes x 8 input planes per word,
 * input-plane-major so that the kernel walks the live kernels of one staged input plane back to back):
 *   quads_rows [ceil(R/4), ceil(Cc/8)], bit (c % 8) * 4 + r % 4 = kmask[r][c]   (forward: R = Cout, Cc = Cin)
 *   quads_cols [ceil(Cc/4), ceil(R/8)], bit (r % 8) * 4 + c % 4 = kmask[r][c]   (data gradient)
 * either may be NULL */
int e2e_dsff_expand_quads(const unsigned char* kmask, unsigned* quads_rows, unsigned* quads_cols, int R, int Cc,
                          void* stream);
/* kernel map from weights (inference: live <=> any nonzero tap) */
int e2e_dsff_kmask_from_weights(const float* w, unsigned char* kmask, int R, int Cc, int ks, void* stream);

/* ---- K11: sliding-window aggregation ------------------------------------------------------
 * Replaces: _internal_maybe_mirror_and_pred_3D accumulation (neural_network.py:529-563) and the overlap-add /
 * normalise / argmax of _internal_predict_3D_3Dconv_tiled (neural_network.py:383-407).            */
/* dst[n,c,flip(x)] = src  (torch.flip over the set bits of `axes`: bit0=X(dim2), bit1=Y, bit2=Z)   */
int e2e_flip3d(const float* src, float* dst, int NC, int X, int Y, int Z, int axes, void* stream);
/* result (+)= w * flip(softmax_c(logits));  first != 0 overwrites */
int e2e_softmax_flip_acc(const float* logits, float* result, float w, int first, int K, int X, int Y, int Z,
                         int axes, void* stream);
/* the same with the network's `inference_apply_nonlin` named (neural_network.py:531-560 applies whatever the attribute
 * holds, the constructor default at :80 is the identity): nonlin 0 = identity, 1 = softmax over the classes (the call
 * above), 2 = sigmoid */
int e2e_nonlin_flip_acc(const float* logits, float* result, float w, int first, int K, int X, int Y, int Z,
                        int axes, int nonlin, void* stream);
/* agg[:, x0:x0+px, ...] += patch * gauss (gauss NULL => 1); cnt[x..] += gauss (or 1); patch NULL: the weight map cnt
 * only (a tile whose probabilities another rank adds into ITS partial volume, parallel.run_tiles_partial) */
int e2e_sw_accumulate(const float* patch, const float* gauss, float* agg, float* cnt, int K, int X, int Y, int Z,
                      int px, int py, int pz, int x0, int y0, int z0, void* stream);
/* probs = agg[crop]/cnt[crop]; seg = argmax_k (first max), int64 */
int e2e_sw_finalize_argmax(const float* agg, const float* cnt, float* probs, long long* seg, int K, int X, int Y,
                           int Z, int cx0, int cy0, int cz0, int CX, int CY, int CZ, void* stream);

/* ---- N1: fold ensembling and segmentation export on device --------------------------------------------------
 * Replaces: the per-fold softmax accumulation and average of predict_cases (e2enet/inference/predict.py:282-296; a
 * multi-GB device->host copy per fold in the reference) and transpose_backward + argmax / region thresholds + crop-box
 * placement into the uint8 volume of save_segmentation_nifti_from_softmax (e2enet/inference/segmentation_export.py:
 * 118-136, predict.py:298-301), and the resampling to the original grid (:84-104).  The NIfTI writer stays on the host.
 *   dst (+)= src over n floats (first != 0 overwrites); n_folds > 0 additionally divides by n_folds (float32 division) */
int e2e_ensemble_accumulate(float* dst, const float* src, long long n, int first, int n_folds, void* stream);
/*   probs [K, ...] with class stride kstride; output voxel (a,b,c) of the TRANSPOSED [A,B,C] frame reads source offset
 *   a*sa + b*sb + c*sc; seg is the zero-initialised uint8 volume [OA,OB,OC] of the original (uncropped) size, written at
 *   offset (a0,b0,c0) and clipped to it; regions (device int[n_regions]) != NULL selects the region-threshold rule   */
int e2e_export_argmax_u8(const float* probs, unsigned char* seg, int K, long long kstride, int A, int B, int C,
                         long long sa, long long sb, long long sc, int OA, int OB, int OC, int a0, int b0, int c0,
                         const int* regions, int n_regions, void* stream);
/*   Softmax volume resampled to another grid (order 1; nearest along one optional low-resolution axis) -- replaces
 *   resample_data_or_seg(is_seg=False, order=1, order_z=0) as called by save_segmentation_nifti_from_softmax
 *   (e2enet/inference/segmentation_export.py:84-104, e2enet/preprocessing/preprocessing.py:113-202; skimage resize =
 *   scipy.ndimage.zoom(order=1, mode='nearest', grid_mode=True) on float64, result cast to float32).
 *   src: [K] volumes of the frame [A,B,C] read with strides (sa,sb,sc) (folds transpose_backward), class stride kstride;
 *   dst: contiguous [K,OA,OB,OC]; lowres_axis: -1 = trilinear, 0..2 = nearest along that axis, bilinear in the plane.   */
int e2e_resample_linear(const float* src, float* dst, int K, long long kstride, int A, int B, int C, long long sa,
                        long long sb, long long sc, int OA, int OB, int OC, int lowres_axis, void* stream);

/* ---- N2: ensembling of saved class probabilities (csrc/ensemble.hip) -------------------------------------------
 * Replaces: `seg_old_spacing.astype(np.float16)` of save_segmentation_nifti_from_softmax (e2enet/inference/
 * segmentation_export.py:117-122, the `-z` export) and merge_files (e2enet/inference/ensemble_predictions.py:28-30: np.vstack of N
 * fp16 volumes, np.mean over them) followed by the argmax / region thresholds and the crop-box placement of
 * segmentation_export.py:124-140.  fp16 volumes are passed as void* (IEEE binary16).
 *   softmax_to_f16: out (contiguous [K, A, B, C], fp16) = probs read as e2e_export_argmax_u8 reads it (class stride kstride, voxel
 *     (a,b,c) of the transposed frame at a*sa + b*sb + c*sc), each value rounded to nearest even, fp16 subnormals included:
 *     the bits of softmax.transpose(...).astype(np.float16).
 *   merge_softmax_f16: srcs is a HOST array of n_src (1 .. E2E_MERGE_MAX_SOURCES) device pointers, read before the call returns
 *     and carried into the launch by value; each source is a contiguous fp16 [K, A, B, C].  Per class and voxel: fp32 sum of the
 *     sources in source order, one fp32 division by n_src, one rounding to fp16 -- what numpy forms for np.mean over fp16 input.
 *     Every decision is taken on that fp16 mean: without regions the first maximum over k (a NaN counts as a maximum), with
 *     regions (device int[n_regions], n_regions <= K) the last region whose mean is > 0.5, else 0.  seg (zero-initialised uint8
 *     [OA, OB, OC]) receives the label at (a0+a, b0+b, c0+c), clipped to its size; mean ([K, A, B, C] fp16) receives the mean.
 *     Either of seg and mean may be NULL, not both.  A*B*C need not be a multiple of 8 (the width of one lane's load).           */
#define E2E_MERGE_MAX_SOURCES 16
int e2e_softmax_to_f16(const float* probs, void* out, int K, long long kstride, int A, int B, int C, long long sa, long long sb,
                       long long sc, void* stream);
int e2e_merge_softmax_f16(const void* const* srcs, int n_src, int K, int A, int B, int C, unsigned char* seg, int OA, int OB,
                          int OC, int a0, int b0, int c0, const int* regions, int n_regions, void* mean, void* stream);


/* ---- K1d: dense 1x3x3 convolution on the bf16 matrix pipe (fp32-exact three-piece operands) --------------------------
 * Same operator as e2e_conv133_fwd / e2e_conv133_dgrad (unetpp_d.py:45-59, :453-478, :93/:108 and their autograd) for layers
 * without DSFF sparsity to exploit (the encoder; masked layers at high density -- `live` / `live_t` are the quad words of
 * e2e_conv133_fwd / e2e_conv133_dgrad, null for a dense layer: pruned kernels are packed as zeros whatever `w` holds):
 * stride (1,1,1), Wi % 32 == 0, Hi % 16 == 0, >= 16 channels on both sides.  e2e_conv133_dense_ws_bytes returns the
 * workspace (packed weights) these calls need, 0 when the shape is not served (use the e2e_conv133_* entry points then).
 * `part` as e2e_conv133_fwd (the partial records are those of its 16 x 32 tiles).                                        */
long long e2e_conv133_dense_ws_bytes(int B, int Cin, int Cout, int Di, int Hi, int Wi, int sd, int sh, int sw);
int e2e_conv133_fwd_dense(const e2e_in_chan_t* chans, int Cin, const float* w, const float* bias, const unsigned* live, float* y,
                          double* part, int B, int Cout, int Di, int Hi, int Wi, void* ws, long long ws_bytes, void* stream);
int e2e_conv133_dgrad_dense(const float* dy, const float* w, const unsigned* live_t, const e2e_out_chan_t* outs, int B, int Cin,
                            int Cout, int Di, int Hi, int Wi, void* ws, long long ws_bytes, void* stream);

/* ---- N3: training input feed on the device ------------------------------------------------------------------------
 * Replaces the spatial and intensity transforms of get_moreDA_augmentation
 * (e2enet/training/data_augmentation/data_augmentation_moreDA.py:66-111; batchgenerators 0.24 transforms executed by 24 CPU
 * worker processes in the reference).  All tensors float32 [B, C, D, H, W] contiguous; parameters are drawn on the host.
 *   e2e_aug_spatial: SpatialTransform (:66-79) as one affine gather: source coordinate = A (o - (size_out - 1) / 2) + t per
 *     sample (mat: B x 12 doubles, row-major 3 x 4); data cval 0, order 3 (the reference's order_data, :43) for the samples
 *     flagged in `cubic` (B ints; NULL = all) when `coef` -- the B-spline coefficient image of `data`, three
 *     e2e_aug_bspline_prefilter_axis passes -- is given, order 1 otherwise; seg (may be NULL) order `order_seg` (0: nearest;
 *     1: batchgenerators' per-label linear interpolation thresholded at 0.5), outside the volume cval_seg (order 0) / 0 (order 1)
 *   e2e_aug_bspline_prefilter_axis: scipy.ndimage.spline_filter1d(order 3, mode 'mirror') along `axis` of nvol volumes
 *     [D, H, W], src -> dst (may alias): what scipy's map_coordinates / zoom run in front of an order-3 interpolation
 *   e2e_aug_stats: per (sample, channel) min, max, mean, std (ddof 0) as 4 doubles; ws of e2e_aug_stats_ws_bytes(nbc) bytes
 *   e2e_aug_pointwise: op 1 GaussianNoise (:85), 2 BrightnessMultiplicative (:88), 3 ContrastAugmentation (:96), 4 / 5 the
 *     power and retain_stats steps of GammaTransform (:102-109); prm: nbc x 8 doubles, prm[0] == 0 leaves the channel untouched
 *   e2e_aug_blur_axis: one axis of GaussianBlurTransform (:86-87) = scipy gaussian_filter1d (truncate 4, 'reflect');
 *     wts: nbc x 16 floats (radius, w[0..radius])
 *   e2e_aug_lowres: SimulateLowResolutionTransform (:97-100): nearest down to lo_shape (nbc x 3 ints, 0 = untouched), linear up
 *   e2e_aug_lowres_down / e2e_aug_lowres_up3: the same with the reference's order_upsample = 3 (:99), one volume per call: the
 *     low-resolution volume materialised edge-padded by `pad` (scipy: 12) -> [prefilter, 3 axes] -> cubic up-sampling clipped to
 *     minmax[0..1] (skimage resize clip=True: the low-resolution volume's range, e.g. from e2e_aug_stats)
 *   e2e_aug_finish: MaskTransform (:117-119; use_mask: C ints or NULL) and RemoveLabelTransform(-1, 0) (:121)               */
int e2e_aug_spatial(const float* data, const float* coef, const int* cubic, const float* seg, float* out_data, float* out_seg,
                    const double* mat, int B, int C, int CS, int Di, int Hi, int Wi, int Do, int Ho, int Wo, int order_seg,
                    float cval_seg, void* stream);
int e2e_aug_bspline_prefilter_axis(const float* src, float* dst, int nvol, int D, int H, int W, int axis, void* stream);
long long e2e_aug_stats_ws_bytes(int nbc);
int e2e_aug_stats(const float* x, double* stats, double* ws, int nbc, long long vol, void* stream);
int e2e_aug_pointwise(float* x, const double* prm, int op, int nbc, long long vol, unsigned long long seed, void* stream);
int e2e_aug_blur_axis(const float* src, float* dst, const float* wts, int nbc, int D, int H, int W, int axis, void* stream);
int e2e_aug_lowres(const float* src, float* dst, const int* lo_shape, int nbc, int D, int H, int W, void* stream);
int e2e_aug_lowres_down(const float* src, float* dst, int D, int H, int W, int ld, int lh, int lw, int pad, void* stream);
int e2e_aug_lowres_up3(const float* coef, float* dst, const double* minmax, int D, int H, int W, int ld, int lh, int lw, int pad,
                       void* stream);
int e2e_aug_finish(float* data, float* seg, const int* use_mask, int B, int C, int CS, long long vol, void* stream);

/* ---- E1: surface-distance scoring of exported label volumes ---------------------------------------------------
 * Replaces: medpy's surface distances behind hausdorff_distance / hausdorff_distance_95 / avg_surface_distance /
 * avg_surface_distance_symmetric (e2enet/evaluation/metrics.py:792-861) and normalized_surface_dice
 * (e2enet/evaluation/surface_dice.py:20-56): binary_erosion with the 6-neighbour cross (connectivity 1) and one
 * scipy.ndimage.distance_transform_edt over the whole volume per label and direction.  Volumes are [D,H,W], W contiguous.
 *   surface_border: border [D,H,W] u8 = m & ~erode(m) of m = (labels == label), voxels outside the volume count as 0;
 *     the binary map is formed on load.  *count (device int64, zeroed by the callee) = number of border voxels
 *   distance_transform_edt_sq: dt2 [D,H,W] fp32 = squared distance to the nearest set voxel of mask under spacing (sd,sh,sw),
 *     exact up to one fp32 rounding of each axis term and of each of the two sums (integers below 2^24 at unit spacing are
 *     exact); +inf everywhere for a mask without a set voxel.  One lower-envelope pass per axis, lines staged in LDS: an
 *     axis longer than the value surface_max_line returns is E2E_ERR_UNSUPPORTED
 *   surface_distances_stats: with d1 = sqrt(dt2_b) at border_a and d2 = sqrt(dt2_a) at border_b (n voxels each):
 *     out[0..3] = count, sum (fp64), max, count <= threshold of d1; out[4..7] the same of d2; out[8], out[9] = the values
 *     of 0-based rank rank_lo and rank_hi in the sorted concatenation of d1 and d2 (the neighbours HD95 interpolates
 *     between; ranks past the number of border voxels are the caller's error and give an unspecified value).  All ten are
 *     doubles and the same bits on every run.  ws: surface_distances_ws_bytes bytes                                     */
int e2e_surface_border(const unsigned char* labels, int label, unsigned char* border, long long* count, int D, int H,
                       int W, void* stream);
int e2e_surface_max_line(void);
int e2e_distance_transform_edt_sq(const unsigned char* mask, float* dt2, int D, int H, int W, double sd, double sh,
                                  double sw, void* stream);
long long e2e_surface_distances_ws_bytes(void);
int e2e_surface_distances_stats(const unsigned char* border_a, const float* dt2_b, const unsigned char* border_b,
                                const float* dt2_a, long long n, double threshold, long long rank_lo, long long rank_hi,
                                double* out, void* ws, void* stream);

/* ---- E2: label census of a (prediction, ground truth) pair; border of a label set ---------------------------------------
 * Replaces: ConfusionMatrix.compute (e2enet/evaluation/metrics.py:67-80: four boolean passes per label and volume) and the
 * scipy.ndimage.find_objects pass that finds the label boxes surface scoring works in.  test / reference: uint8 [D,H,W] on the
 * device, W contiguous, any byte alignment (16-byte loads where both pointers share their phase modulo 16, byte loads otherwise).
 *   eval_census: one pass, 2 B read per voxel.  lut: 256 bytes on the HOST (read before the call returns), value -> slot in
 *     [0, slots); 1 <= slots <= eval_census_max_slots (values nobody evaluates share one slot).  joint (device, slots * slots
 *     64-bit words) [reference slot * slots + test slot] = number of voxels with that pair, exact.  boxes (device, slots * 6
 *     ints) [slot] = lo d, h, w then exclusive hi d, h, w over the voxels that carry the slot in EITHER volume; a slot nobody
 *     carries has lo = INT_MAX >= hi = 0 on every axis.  Both are initialised by the callee.  Integer atomics only: the same
 *     bits on every run.  A fixed grid of at most eval_census_workgroups workgroups strides over chunks of eval_census_chunk
 *     voxels; a volume that would give one workgroup 2^32 voxels or more is refused (32-bit bins in LDS).
 *   surface_border_set: surface_border on the mask "the value's bit is set in members" (8 HOST words, bit v of the 256 = value
 *     v belongs; the empty set gives an empty border).  One kernel serves both entry points.                                  */
int e2e_eval_census_max_slots(void);
long long e2e_eval_census_chunk(void);
int e2e_eval_census_workgroups(void);
int e2e_eval_census(const unsigned char* test, const unsigned char* reference, const unsigned char* lut, int slots, int D, int H,
                    int W, unsigned long long* joint, int* boxes, void* stream);
int e2e_surface_border_set(const unsigned char* labels, const unsigned* members, unsigned char* border, long long* count, int D,
                           int H, int W, void* stream);

/* ---- P1: connected-component post-processing of exported label volumes -------------------------------------------
 * Replaces: remove_all_but_the_largest_connected_component (e2enet/postprocessing/connected_components.py:50-107): one
 * scipy.ndimage.label over the whole volume per class entry and one (lmap == id).sum() per object.  volume: uint8 [D,H,W], W
 * contiguous, edited in place.  The entry's mask is class_words[x >> 5] >> (x & 31) & 1 (class_words: 8 HOST words, a 256-bit
 * class set; a joint region sets several bits), formed on load.  6-neighbour connectivity (scipy's default structure).
 *   cc_ws_bytes: bytes of `ws` for a volume of that shape: 8 per voxel (32-bit parent and size arrays) plus 64 for the result
 *     words; 0 for a shape cc_remove_all_but_largest refuses
 *   cc_remove_all_but_largest: every mask voxel of a component whose size differs from the largest size and, when
 *     min_valid >= 0, whose size * volume_per_voxel (fp64) is < min_valid, becomes 0; min_valid < 0: no minimum.  All components
 *     of the largest size stay.  result (device, four 64-bit words, written by the callee): number of components, largest size
 *     in voxels, largest removed size in voxels (0: nothing removed), give-up flag.  The flag is a backstop: non-zero means the
 *     union-find met a link it must never meet or ran out of its V + 64 step budget; the volume is then left as it was and the
 *     caller, who reads the words after the stream has run, must treat the call as failed.  Same bits on every run.
 *     Refused before anything is launched: an axis < 1 (E2E_ERR_ARG), more than 2^31 - 2 voxels (E2E_ERR_UNSUPPORTED), class 0 in
 *     the set, an empty set, a volume_per_voxel that is not positive and finite, a NaN min_valid (E2E_ERR_ARG)                  */
long long e2e_cc_ws_bytes(int D, int H, int W);
int e2e_cc_remove_all_but_largest(unsigned char* volume, int D, int H, int W, const unsigned* class_words,
                                  double volume_per_voxel, double min_valid, void* ws, unsigned long long* result,
                                  void* stream);

/* ---- P5: the component table of a prediction, for the post-processing search over a folder ---------------------------------
 * Replaces: what determine_postprocessing (connected_components.py:124-399) gets from removing, writing, reading and scoring every
 * case once per sweep: the confusion counts after a removal follow from the prediction's components, their sizes and their own
 * true positives.  pred, gt: uint8 [D,H,W], W contiguous, read only.  class_words: the foreground classes S as in P1 (8 HOST words).
 * Two labellings of pred in one call: the foreground components (x in S as one mask, the kernels of P1) and the class components
 * (two 6-neighbours unite only when both are in S and carry the same value), the latter with size and tp = voxels with gt == pred.
 *   ct_ws_bytes: bytes of `ws`: 20 per voxel (five 32-bit arrays) plus 128 for the two sets of result words; 0 for a refused shape
 *   ct_label: result (device, four 64-bit words, written by the callee): number of class components, number of foreground
 *     components, give-up flag (non-zero: the call failed, see P1; never retried), 0
 *   ct_emit: after ct_label on the same ws and pred, and after the caller has read its result: class_records [class_count][5]
 *     32-bit words (first voxel = flat index of the component's first voxel in raster order, label, size, tp, first voxel of the
 *     foreground component it lies in), fg_records [fg_count][2] (first voxel, size).  The order of the records is not fixed; sorted
 *     by first voxel the table is the same bits on every run (integer atomics only).  Nothing is truncated: a capacity (in records)
 *     below its count is E2E_ERR_ARG, and no record is written at or past its count.
 *   Refused before anything is launched: an axis < 1, a null pointer, an empty set, class 0 in the set, counts that are no
 *     component counts of the shape (E2E_ERR_ARG); more than 2^31 - 2 voxels (E2E_ERR_UNSUPPORTED)                              */
long long e2e_ct_ws_bytes(int D, int H, int W);
int e2e_ct_label(const unsigned char* pred, const unsigned char* gt, int D, int H, int W, const unsigned* class_words, void* ws,
                 unsigned long long* result, void* stream);
int e2e_ct_emit(const unsigned char* pred, int D, int H, int W, void* ws, unsigned* class_records, long long class_capacity,
                long long class_count, unsigned* fg_records, long long fg_capacity, long long fg_count, void* stream);

/* ---- P2: preprocessing of a raw case (crop to non-zero, resample, normalise) ----------------------------------------
 * Replaces: e2enet/preprocessing/cropping.py (create_nonzero_mask, get_bbox_from_mask, crop_to_nonzero) and
 * e2enet/preprocessing/preprocessing.py (resample_data_or_seg, GenericPreprocessor.resample_and_normalize).  Volumes are fp32,
 * masks uint8; "strided" sources give a channel stride and one element stride per axis (a transposed view needs no copy), every
 * destination is contiguous.  lowres_axis: -1, or the axis (0..2) that is resampled with order 0 while the planes across it are
 * resampled in 2-D (the reference's do_separate_z).
 *   pp_nonzero_mask: mask[D,H,W] = OR over the C contiguous modalities of x != 0 (NaN counts as non-zero), then
 *     scipy.ndimage.binary_fill_holes (6 neighbours): every background component without a voxel on a face of the volume
 *     becomes mask.  ws: pp_nonzero_ws_bytes bytes (5 per voxel; 0: shape refused).  result (device, 8 words): word 6 is the
 *     union-find's give-up flag (see cc_remove_all_but_largest): non-zero means the call failed; it is never retried.
 *   pp_bbox: result[0..5] = lo, hi of axis 0, 1, 2 with hi exclusive, over the voxels mask != outside_value; result[7] = their
 *     number (0: the box words are meaningless).  Integer atomics only.
 *   pp_crop: out_data[C,d,h,w] = data[:, z0:z0+d, y0:y0+h, x0:x0+w]; out_seg[S,d,h,w] = the cropped seg with nonzero_label
 *     where seg == 0 and the mask is off; seg == NULL: out_seg[1,d,h,w] = nonzero_label off the mask, 0 on it.
 *   pp_label_hist: hist[v + 256] += 1 for whole-number labels v in [-256, 255], hist[512] += 1 for anything else (hist: 513
 *     words, zeroed by the caller); fix_below != 0 additionally writes seg[seg < -1] = 0.
 *   pp_nan_to_zero: x[isnan(x)] = 0 in place.
 *   pp_minmax: dst[2 g], dst[2 g + 1] = min, max of group g = modality k (lowres_axis < 0) or k * n[lowres_axis] + slice.
 *     ws: pp_minmax_ws_bytes bytes.
 *   pp_pad_edge: dst[K, A + 2 pa, B + 2 pb, C + 2 pc] = src continued by its edge values (np.pad mode 'edge').
 *   pp_resize_cubic: src = the B-spline coefficients of the volume padded by `pad` on every axis but lowres_axis
 *     (pp_pad_edge, then aug_bspline_prefilter_axis on those axes); dst[K,OA,OB,OC] = the cubic spline at
 *     (o + 0.5) * in / out - 0.5 + pad, which is scipy.ndimage.zoom(order=3, mode='nearest', grid_mode=True) for pad = 12,
 *     clipped to the group's range in minmax (pp_minmax of the same lowres_axis); along lowres_axis the plane
 *     floor(c + 0.5) of the clamped coordinate.
 *   pp_resize_seg: per voxel the largest label whose binary mask, resampled like resample_linear does (order 1, order 0 along
 *     lowres_axis), is >= 0.5, else 0; a result < -1 is written as 0.
 *   pp_norm_stats: stats[4 c ..] = (voxels counted, mean, std with ddof 0) of channel c for the schemes that need them:
 *     prm[8 c ..] = (scheme: 0 default, 1 CT, 2 CT2, 3 noNorm; lower bound; upper bound; mean; sd; use_nonzero_mask; 0; 0).
 *     Scheme 0 counts seg >= 0 when use_nonzero_mask is set and every voxel otherwise, scheme 2 counts lb < x < ub.  Two passes,
 *     fp64 per-block records folded in a fixed order: the same bits on every run.  ws: pp_norm_ws_bytes bytes.
 *   pp_normalize: in place.  0: (x - mean) / (std + 1e-8); 1: (clip(x, lb, ub) - prm mean) / prm sd; 2: (clip(x, lb, ub) - mean) /
 *     std; 3: untouched.  With use_nonzero_mask, voxels with seg < 0 become 0 (schemes 0..2).  seg: one channel [vol] or NULL. */
long long e2e_pp_nonzero_ws_bytes(int D, int H, int W);
int e2e_pp_nonzero_mask(const float* data, int C, int D, int H, int W, unsigned char* mask, void* ws, unsigned* result,
                        void* stream);
int e2e_pp_bbox(const unsigned char* mask, int outside_value, int D, int H, int W, unsigned* result, void* stream);
int e2e_pp_crop(const float* data, const float* seg, const unsigned char* mask, float* out_data, float* out_seg, int C, int S,
                int D, int H, int W, int z0, int y0, int x0, int d, int h, int w, float nonzero_label, void* stream);
int e2e_pp_label_hist_bins(void);
int e2e_pp_label_hist(float* seg, long long n, unsigned* hist, int fix_below, void* stream);
int e2e_pp_nan_to_zero(float* x, long long n, void* stream);
long long e2e_pp_minmax_ws_bytes(int K, int A, int B, int C, int lowres_axis);
int e2e_pp_minmax(const float* src, double* dst, void* ws, int K, long long kstride, int A, int B, int C, long long sa,
                  long long sb, long long sc, int lowres_axis, void* stream);
int e2e_pp_pad_edge(const float* src, float* dst, int K, long long kstride, int A, int B, int C, long long sa, long long sb,
                    long long sc, int pa, int pb, int pc, void* stream);
int e2e_pp_resize_cubic(const float* src, float* dst, const double* minmax, int K, int A, int B, int C, int OA, int OB, int OC,
                        int pad, int lowres_axis, void* stream);
int e2e_pp_resize_seg(const float* src, float* dst, int K, long long kstride, int A, int B, int C, long long sa, long long sb,
                      long long sc, int OA, int OB, int OC, int lowres_axis, void* stream);
long long e2e_pp_norm_ws_bytes(int C);
int e2e_pp_norm_stats(const float* x, const float* seg, const double* prm, double* stats, void* ws, int C, long long vol,
                      void* stream);
int e2e_pp_normalize(float* x, const float* seg, const double* prm, const double* stats, int C, long long vol, void* stream);

/* ---- P3: class locations of a preprocessed training case ------------------------------------------------------------
 * Replaces: e2enet/preprocessing/preprocessing.py:343-361 (GenericPreprocessor._run_internal): per class c of all_classes,
 * np.argwhere(seg == c), which lists the class's voxels in raster order, and rows of it drawn by one RandomState.  seg: the
 * contiguous fp32 label volume [D,H,W] (n = D*H*W voxels, whole-number labels) on the device.  classes: K fp32 values on the
 * HOST (read before the call returns), 1 <= K <= pp_select_max_classes; the caller loops over longer lists.  A voxel equal to
 * none of them belongs to no class (-1, 0, stray values, NaN).  All indices, offsets and counts are 64-bit.
 *   pp_select_chunk: voxels per workgroup (a chunk of the flat volume; wave w of pass p owns voxels 256 p + 64 w .. + 63 of it).
 *   pp_select_ws_bytes: workspace of one (n, K) pair: per chunk and class a 32-bit count and a 64-bit offset.  0: refused
 *     (n < 1, K outside 1 .. pp_select_max_classes, or more than 2^24 - 1 chunks).
 *   pp_select_count: counts[k] (device, K 64-bit words) = number of voxels equal to classes[k]; ws keeps the per-chunk counts
 *     and their exclusive prefix sums for pp_select_coords.  One read of the volume.
 *   pp_select_coords: for class k and every p in [class_offsets[k], class_offsets[k+1]): ranks[p] (device, ascending within a
 *     class) is a position in the raster order of the class's voxels, slots[p] (device) in [0, class_offsets[k+1] -
 *     class_offsets[k]) the row of the class it goes to: out[(class_offsets[k] + slots[p]) * 3 ..] = (i, j, k) of that voxel,
 *     64-bit.  class_offsets: K + 1 non-decreasing 64-bit words on the HOST.  ws: as pp_select_count of the same seg, n and
 *     classes left it.  A workgroup none of whose voxels was drawn leaves without reading the volume: at most one read.  Every
 *     row has one writer and there are no atomics: the same bits on every run.  A rank that is not below the class's count
 *     and a slot outside the class's rows write nothing.                                                                    */
int e2e_pp_select_chunk(void);
int e2e_pp_select_max_classes(void);
long long e2e_pp_select_ws_bytes(long long n, int K);
int e2e_pp_select_count(const float* seg, long long n, const float* classes, int K, long long* counts, void* ws, void* stream);
int e2e_pp_select_coords(const float* seg, int D, int H, int W, const float* classes, int K, const long long* ranks,
                         const long long* slots, const long long* class_offsets, long long* out, const void* ws, void* stream);

/* ---- P4: the dataset fingerprint of a cropped training folder --------------------------------------------------------
 * Replaces: e2enet/experiment_planning/DatasetAnalyzer.py:161-179 (_get_voxels_in_foreground: modality[seg > 0][::10] per case
 * and modality; _compute_stats: np.median / mean / std / min / max / percentile over a Python list of the samples).  A cropped
 * case is [C + 1, X, Y, Z] fp32 on the device with the seg last; n = X*Y*Z voxels.  All indices, offsets and counts are 64-bit.
 *   fingerprint_sample_chunk: voxels per workgroup (a chunk of the flat seg, laid out like pp_select_chunk's).
 *   fingerprint_sample_ws_bytes: workspace of a volume of n voxels: per chunk a 32-bit count and a 64-bit offset.  0: refused
 *     (n < 1 or more than 2^24 - 1 chunks).
 *   fingerprint_sample_count: *n_fg (device, one 64-bit word) = number of voxels with seg > 0 (a NaN is not); ws keeps the
 *     per-chunk counts and their exclusive prefix sums for fingerprint_sample_gather.  One read of the seg.
 *   fingerprint_sample_gather: out[c * out_len + r / stride] = data[c * n + v] for c < C and every voxel v with seg > 0 whose
 *     rank r in the raster order of those voxels is a multiple of stride (1 .. 2^30): out[c] is data[c][seg > 0][::stride] when
 *     out_len = ceil(n_fg / stride); a column >= out_len is not written.  ws: as fingerprint_sample_count of the same seg and n
 *     left it.  A chunk without a sampled rank is not read; the seg is read once whatever C is.  One writer per element.
 *   fingerprint_stats: over the n (1 .. 2^32 - 1) values of x (device).  out (device, 16 doubles): [0] number of NaNs, [1] min,
 *     [2] max, [3] sum (NaNs left out of all three), [4] sum of (x - out[3] / n)^2, [5..7] 0, [8 + r] the value at position
 *     ranks[r] of the sorted array (exact, as stored; -0.0 sorts in front of 0.0, a NaN behind +inf).  ranks: num_ranks (1 ..
 *     fingerprint_stats_max_ranks) positions in [0, n) on the HOST, read before the call returns; duplicates are allowed.
 *     Sums are fp64 per-workgroup partials added in workgroup order; the order statistics come from a byte-wise radix select (four
 *     sweeps of x for all ranks together, integer histograms).  ws: fingerprint_stats_ws_bytes bytes.  The same bits on every run. */
int e2e_fingerprint_sample_chunk(void);
long long e2e_fingerprint_sample_ws_bytes(long long n);
int e2e_fingerprint_sample_count(const float* seg, long long n, long long* n_fg, void* ws, void* stream);
int e2e_fingerprint_sample_gather(const float* data, const float* seg, int C, long long n, int stride, float* out,
                                  long long out_len, const void* ws, void* stream);
int e2e_fingerprint_stats_max_ranks(void);
long long e2e_fingerprint_stats_ws_bytes(void);
int e2e_fingerprint_stats(const float* x, long long n, const long long* ranks, int num_ranks, double* out, void* ws,
                          void* stream);

/* ---- N3: the training loader's crop, out of cases that live on the device ----------------------------------------------
 * Replaces: e2enet/training/dataloading/dataset_loading.py:283-372 (DataLoader3D.generate_train_batch: per sample np.copy of the
 * valid box, np.pad of the data and np.pad of the seg with -1, into a host batch that is then uploaded).  One launch cuts a whole
 * batch.  recs: B records on the HOST, read before the call returns, 1 <= B <= loader_crop_max_batch.  A record names a source box
 * src = [C + 1, d, h, w] fp32 on the device, contiguous, the seg as its last channel (a whole preprocessed case, or any box cut
 * out of one), and the box coordinates off_d, off_h, off_w of patch voxel 0, 0, 0; they may be negative or beyond the extent
 * (-2^30 .. 2^30).  out_data [B, C, pd, ph, pw] and out_seg [B, 1, pd, ph, pw], fp32, contiguous; every patch axis is at most 2^21
 * and the patch has fewer than 2^31 voxels.  With q = off + p per axis:
 *   out_seg: the source seg where q lies in the box on all three axes, seg_fill elsewhere;
 *   out_data, data_mode 0 (np.pad 'constant'): the source value inside the box, data_fill outside;
 *   out_data, data_mode 1 (np.pad 'edge'): the source value at q clamped per axis to [0, extent - 1].
 * Values are copied as 32-bit words: every bit of a NaN or of -0.0 comes out as it went in.  Source offsets are 64-bit (a source
 * may hold more than 2^31 elements).  One writer per element and no atomics: the same bits on every run.  Refused: B outside its
 * range, a data_mode other than 0 and 1, an extent of a box or of the patch below 1, a null pointer.                          */
typedef struct {
  const float* src;
  int d, h, w;
  int off_d, off_h, off_w;
} e2e_loader_rec_t;
int e2e_loader_crop_max_batch(void);
int e2e_loader_crop(const e2e_loader_rec_t* recs, int B, int C, int pd, int ph, int pw, float* out_data, float* out_seg,
                    int data_mode, float data_fill, float seg_fill, void* stream);

/* ---- N4: decoding of NIfTI-1 voxel payloads (csrc/nifti.hip) -------------------------------------------------------------
 * Replaces: the host pass of e2enet/preprocessing/cropping.py:61-81 (sitk.GetArrayFromImage, np.vstack, astype(np.float32)) and
 * the upload of its fp32 copy.  raw: nvox elements on the device exactly as the file stores them (the host has inflated the file
 * and parsed the header, e2enet_medical_amd/nifti.py), aligned to the element size.  datatype: the NIfTI-1 code, one of 2 uint8,
 * 4 int16, 8 int32, 16 float32, 64 float64, 256 int8, 512 uint16, 768 uint32, 1024 int64, 1280 uint64.  swap != 0: the bytes of
 * every element are reversed first (a file of the other byte order).
 *   scale == 0: out[i] = the element converted with one rounding to nearest even (ndarray.astype(np.float32)): the 32- and 64-bit
 *     integers directly, not through fp64; float32 bit for bit; NaN and Inf of float64 pass through.  slope and inter are not read.
 *   scale != 0: out[i] = fp32(fp64(element) * slope + inter), the product and the sum each rounded to fp64 (never an FMA), then one
 *     rounding to fp32: numpy's (raw.astype(np.float64) * slope + inter).astype(np.float32).
 *   decode_f32: out fp32, nvox elements (a channel of a [C, Z, Y, X] tensor: only these nvox floats are written).
 *   decode_u8: out uint8; the fp32 value above when it is a whole number in [0, 255], else 0 and *rejected (device, 64-bit, zeroed
 *     by the caller) is incremented: one integer atomic per workgroup that rejected something, the same total on every run.
 * elsize bytes read and 4 or 1 written per voxel.  Refused with E2E_ERR_ARG before anything is launched: another datatype, nvox < 0
 * or > 2^40, a null pointer, raw not aligned to the element size.  nvox == 0 launches nothing.                                  */
int e2e_nifti_decode_f32(const void* raw, long long nvox, int datatype, int swap, int scale, double slope, double inter, float* out,
                         void* stream);
int e2e_nifti_decode_u8(const void* raw, long long nvox, int datatype, int swap, int scale, double slope, double inter,
                        unsigned char* out, unsigned long long* rejected, void* stream);

/* The integrity scan of a payload: what np.isnan, np.unique and the label rule of decode_u8 say about a volume, from one pass over the
 * stored bytes (same arguments, same per-voxel value as decode_f32) with nothing of volume size written.
 * Replaces: np.any(np.isnan(sitk.GetArrayFromImage(...))) and np.unique of e2enet/preprocessing/sanity_checks.py:79-87, 136-145.
 * out: 4 + 256 64-bit words on the device, written whole by the call (no need to zero them):
 *   [0] voxels whose fp32 value is NaN               [1] raster index of the first of them, ~0 when there is none
 *   [2] voxels that are not NaN and are no whole number in [0, 255] (what decode_u8 rejects, less the NaNs)
 *   [3] raster index of the first of them, ~0 when there is none
 *   [4 + v] voxels whose value is the label v
 * so [0] + [2] + sum [4..259] == nvox.  Integer sums and minima only: the words are the same on every run.  The 256 counts are kept
 * in LDS, 16 copies per workgroup, each lane adding a run of equal values at once; a workgroup adds its counts to out once.  16 bytes
 * per lane and load, four loads requested at a time, from the first 16-byte boundary of raw on; the elements in front of it and behind the last whole vector are read
 * one by one.  elsize bytes read per voxel.  One small kernel sets out before the scan; nvox == 0 runs only that one (raw is not
 * read and may be null).  Refused with E2E_ERR_ARG before anything is launched: another datatype, nvox < 0 or > 2^40, a null pointer,
 * raw not aligned to the element size, out not aligned to 8 bytes.
 * e2e_nifti_scan_grid_voxels: the voxels one full grid of the scan takes in one step of its walk, four vectors per lane (0 for a
 * datatype that is not decoded): in a larger volume lanes take a second step.                                                  */
long long e2e_nifti_scan_grid_voxels(int datatype);
int e2e_nifti_scan(const void* raw, long long nvox, int datatype, int swap, int scale, double slope, double inter,
                   unsigned long long* out, void* stream);

/* ---- N5: raw DEFLATE (RFC 1951) of a device buffer (csrc/deflate.hip) ----------------------------------------------------
 * Replaces: the download of an uncompressed volume and the host's zlib pass over it (np.savez_compressed of the -z
 * probabilities, gzip of a label volume).  The stream is the simplest one every inflater takes: the input is cut into chunks of
 * e2e_deflate_chunk_bytes() bytes, one workgroup per chunk, no workgroup waits for another.  A chunk is one non-final
 * fixed-Huffman block whose only matches have distance `elem` ("the same element again": byte i equals byte i - elem; a match may
 * reach back in front of the chunk, the window is the input), lengths 3..258, a maximal run inside the chunk cut into 258s and one
 * match for the rest (literals when fewer than 3 bytes are left); everything else is a literal.  An empty stored block behind the
 * end-of-block symbol byte-aligns the chunk.  A chunk whose fixed-Huffman form is longer than 5 + its bytes is one stored block.
 * The caller closes the stream with the bytes 03 00 (an empty final fixed block).
 *   encode: slots [nchunks][e2e_deflate_slot_bytes()] receives every chunk's bytes, counts[nchunks] their number; nchunks =
 *     ceil(nbytes / chunk).  *crc (device) receives zlib's CRC-32 of the input: one CRC per chunk (chunk_crcs[nchunks], workspace),
 *     combined by one small kernel with the shift operator of a whole chunk, applied once per chunk.  elem: 1, 2, 4 or 8, a
 *     divisor of nbytes.  nbytes == 0 only sets *crc = 0.  The bytes depend on the input and elem only.
 *   gather: out[offsets[c] .. offsets[c] + counts[c]) = slot c, offsets the exclusive prefix sum of counts (64-bit, device); a chunk
 *     that would end behind out_bytes is not copied.
 * Refused with E2E_ERR_ARG before anything is launched: elem not 1, 2, 4, 8 or no divisor of nbytes, nbytes < 0 or > 2^37, a null
 * pointer, slots not aligned to 16 bytes.                                                                                      */
int e2e_deflate_chunk_bytes(void);
int e2e_deflate_slot_bytes(void);
int e2e_deflate_encode(const void* src, long long nbytes, int elem, unsigned char* slots, unsigned* counts, unsigned* chunk_crcs,
                       unsigned* crc, void* stream);
int e2e_deflate_gather(const unsigned char* slots, const unsigned* counts, const long long* offsets, long long nchunks,
                       unsigned char* out, long long out_bytes, void* stream);

/* ---- N5b: the same stream with one Huffman code per chunk (csrc/deflate.hip) -------------------------------------------------
 * e2e_deflate_encode_dynamic is e2e_deflate_encode with a third form of a chunk: one dynamic-Huffman block (RFC 1951, 3.2.7) over
 * exactly the tokens of the fixed form, with a literal/length code built from the chunk's own token counts (symbol 256 counts
 * once).  A chunk is written in the shortest of its three forms: fixed where fixed <= stored as before, dynamic only where it is
 * strictly shorter than both others; kinds[nchunks] (bytes) receives 0 for stored, 1 for fixed, 2 for dynamic.  A chunk that is not
 * dynamic carries the bytes e2e_deflate_encode gives it, so slots, counts, chunk_crcs, crc, the gather and the closing 03 00 are
 * those of N5, and counts[c] never exceeds N5's.  tests/deflate_dynamic_oracle.py restates the format in Python.
 *   code lengths, for the literal/length code (286 symbols, at most 15 bits) and the code-length code (19 symbols, at most 7):
 *     the used symbols are ordered by count descending, equal counts by symbol number ascending; their counts go through the
 *     two-queue Huffman construction, a leaf before an internal node of the same weight; only the number of leaves per depth is
 *     kept.  Leaves deeper than the limit count at the limit, and for every 2^-limit that the Kraft sum then exceeds 1 by, the
 *     deepest level below the limit that has a leaf gives one up: it becomes an internal node with two leaves one level down, one
 *     of them taken from the limit's level (the step of zlib's gen_bitlen).  The lengths are then dealt out along the order,
 *     shortest first: of two symbols with equal counts the smaller symbol number never has the longer code.  Codes are the
 *     canonical ones of 3.2.2; both codes are complete.
 *   distance code: one symbol, the one of distance elem (0, 1, 3, 5), with length 1 and HDIST = that symbol + 1, when the chunk has
 *     a match (distance 8 carries its extra bit, set); HDIST = 1 and one zero length when it has none.
 *   header: BFINAL 0, BTYPE 10, HLIT (the last used symbol, at least 257 symbols), HDIST, HCLEN (at least 4), the code-length
 *     code's lengths in the permuted order, then the literal/length lengths and the distance lengths, each sequence on its own in
 *     the run codes 16, 17, 18 as zlib's scan_tree cuts runs (zeros: up to 138 per code 18, 3..10 per code 17; a non-zero length
 *     once and then up to 6 repeats per code 16).
 *   ending: the end-of-block code, an empty stored block as byte alignment (00 00 FF FF), as in the fixed form.
 * Refusals as e2e_deflate_encode's, and kinds null with nbytes > 0.                                                            */
int e2e_deflate_encode_dynamic(const void* src, long long nbytes, int elem, unsigned char* slots, unsigned* counts,
                               unsigned char* kinds, unsigned* chunk_crcs, unsigned* crc, void* stream);

/* ---- N8: inflate on the device what N5 / N5b wrote (csrc/inflate.hip), and zlib's CRC-32 of a device buffer --------------------
 * Replaces: the host's single-threaded zlib pass over a .npz member this package wrote, and the upload of the inflated bytes.
 * General DEFLATE is serial; the stream of N5 is a sequence of byte-aligned chunk records, each inflating to exactly
 * e2e_deflate_chunk_bytes() bytes (the last to the remainder), each one stored block or one fixed / dynamic Huffman block closed by
 * the empty stored block 00 00 FF FF, every match of a record at one distance d of 1, 2, 4 or 8.  A record needs nothing from
 * outside itself but the 8 bytes in front of it, so one wave inflates one record and no wave waits for another.  The stream has
 * no index: the host proposes candidate offsets (e2enet_medical_amd/deflate.py), scan parses one record at each, the host walks
 * the chain of valid records from offset 0 and resolves every record's 8 front bytes from the tail descriptors.
 *   scan: records[c] (e2e_inflate_record_words() = 8 words) for the candidate starts[c] (64-bit byte offsets, device):
 *     word 0  status: 0 a valid record, 1 invalid (all other words are 0 then);
 *     word 1  kind (0 stored, 1 fixed, 2 dynamic) | d << 8 (0: no match) | reach << 16 (how many bytes in front of the record its
 *             matches read, 0 .. 8);
 *     word 2  output bytes, 1 .. chunk;  words 3, 4  the end offset (the byte behind the record), low and high half;
 *     words 5, 6  the values and word 7 the dependences of the record's last 8 output bytes, oldest first: nibble i of word 7 is
 *             15 when byte i of words 5, 6 is the value, else j = 0 .. 7 and the byte equals byte j of the 8 bytes in front of the
 *             record (the byte of words 5, 6 is 0).  A record shorter than 8 bytes passes the front bytes on; a match copies the
 *             dependence with the value, so the dependent bytes need not be a prefix of the record.
 *     No output byte is written.  Invalid: BFINAL set; BTYPE 11; HLIT > 286 or HDIST > 30 symbols; a code-length or
 *     literal/length code that is over-subscribed or incomplete, a distance code that is over-subscribed, or incomplete other than
 *     by having one code of length 1 or none (zlib's rules); a repeat with nothing to repeat or lengths running over HLIT + HDIST;
 *     no end-of-block code; a bit pattern without a symbol; a symbol > 285, a distance code > 29; a distance that is not 1, 2, 4
 *     or 8, or two different distances; more than chunk output bytes, or none; a stored block with LEN != ~NLEN, LEN = 0 or
 *     LEN > chunk; a Huffman block not followed by 000, padding and 00 00 FF FF; a record that ends behind ncomp (bytes behind
 *     ncomp read as zeros meanwhile); a start outside [0, ncomp).
 *   chunks: record k of the chain, at starts[k], is parsed again with the same rules (nothing of the scan is trusted) into an LDS
 *     image that begins with prev_tails[k][8], the bytes in front of it (record 0: not read by a valid stream; a record 0 that
 *     reaches in front of itself is bad), and the image is stored to out + k chunk when the record is valid and gives exactly
 *     min(chunk, nbytes - k chunk) bytes.  Otherwise nothing of that record is stored and *status (device, zeroed by the call)
 *     counts it.  nchunks = ceil(nbytes / chunk).  out is aligned to 16 bytes.
 *   crc32: *crc (device) = zlib.crc32 of buf[0, nbytes); chunk_crcs[ceil(nbytes / chunk)] is workspace.  The kernels are those
 *     of e2e_deflate_encode.  nbytes == 0 only sets *crc = 0.
 * Refused with E2E_ERR_ARG before anything is launched: a null pointer, ncomp > 2^38, nbytes > 2^37, more than 2^26 candidates,
 * nchunks != ceil(nbytes / chunk), starts not aligned to 8 bytes, out not aligned to 16.                                        */
int e2e_inflate_record_words(void);
int e2e_inflate_scan(const unsigned char* comp, long long ncomp, const long long* starts, long long nstarts, unsigned* records,
                     void* stream);
int e2e_inflate_chunks(const unsigned char* comp, long long ncomp, const long long* starts, const unsigned char* prev_tails,
                       long long nchunks, unsigned char* out, long long nbytes, unsigned* status, void* stream);
int e2e_crc32(const void* buf, long long nbytes, unsigned* chunk_crcs, unsigned* crc, void* stream);

/* ---- N9: inflate any raw DEFLATE stream (RFC 1951) on the device (csrc/inflate_any.hip) ------------------------------------------
 * Replaces: the host's single-threaded zlib pass over a zlib-written .npz member or a .nii.gz, and the upload of the inflated bytes.
 * comp[0, n) is the stream; bit position p is bit p mod 8 (least significant first) of comp[p / 8]; bytes behind n read as zero.
 * W = e2e_inflate_any_window_bytes() = 32768.  All buffers are device buffers; the host only compacts and sums small tables.
 *   find: the compressed bytes are cut into nseg = ceil(n / segment_bytes) segments.  starts[s], s = 1 .. nseg - 1, receives the
 *     first bit position p with 8 s S <= p < 8 (s + 1) S at which a non-final dynamic block header is valid, or -1: BFINAL 0,
 *     BTYPE 10, HLIT <= 29, HDIST <= 29, a complete code-length code, no run over HLIT + HDIST, no repeat of nothing, symbol 256
 *     present, a complete literal/length code, a distance code that is complete, empty or one code of length 1 (zlib's rules, the
 *     ones N8 applies), and the header ends at or before bit 8 n.  starts[0] is not written (the host sets it to 0).
 *   spans_count: starts[0, m) are ascending bit positions (the compacted result of find).  Span k is parsed block by block (stored,
 *     fixed, dynamic; distances 1 .. 32768) from starts[k] until a block ends exactly at starts[k + 1]; the last span until a block
 *     with BFINAL set, which must end in byte n - 1.  records[k] (e2e_inflate_any_record_words() = 8 words): word 0 status, word 1
 *     whether the span ended with the final block, words 2, 3 the bit position behind its last block (low, high), words 4, 5 its
 *     output length (low, high), words 6, 7 zero; words 1 .. 7 are zero when the status is not 0.  Status: 0 good; 1 BTYPE 11; 2 a header rule above; 3 a bit pattern without a symbol;
 *     4 a symbol > 285; 5 a distance code > 29; 6 stored LEN != ~NLEN; 7 BFINAL in a span that is not the last, or a final block
 *     that does not end in the last byte; 8 a block that runs behind n; 9 overshoot: a block end behind starts[k + 1]; 10 more
 *     than max_span_bytes compressed bytes, or more than 8 max_span_bytes + 64 blocks and symbols; 13 a start outside [0, 8 n).
 *     Nothing but the record is written.
 *   spans_write: offs[0, m] is the exclusive prefix sum of the counted lengths (offs[m] = nbytes).  Span k is parsed again with the
 *     same rules (nothing of the count is trusted but the offsets) into sym[offs[k], offs[k + 1]): a literal is its value; a match
 *     copies symbols of the span; a source q < 0 (span-relative) is the marker 0x8000 | (W + q), "byte W + q of the W bytes in front
 *     of this span".  A span that is invalid, reaches in front of absolute position 0 (status 12), gives another length than its
 *     offsets say (11) or whose offsets leave [0, nbytes] stores nothing outside its own range of sym and adds 1 to *status
 *     (device, zeroed by the call).
 *   windows: wins[k W + j], 1 <= k < m, = the byte at absolute position offs[k] - W + j (0 in front of the output), from
 *     win_{k-1} and the symbols of span k - 1, spans in order, one workgroup.  A marker in span 0 counts in *status.
 *   resolve: out[i] = sym[i] < 0x8000 ? sym[i] : wins[k(i) W + (sym[i] & 0x7FFF)], k(i) the last span with offs[k] <= i.
 * Refused with E2E_ERR_ARG before anything is launched: a null pointer, segment_bytes outside 16 .. 2^24, nseg != ceil(n /
 * segment_bytes), n > 2^38, nbytes > 2^37, m > 2^26, max_span_bytes outside 1 .. 2^31, starts / offs not aligned to 8 bytes, sym
 * or out not aligned to 16.                                                                                                       */
int e2e_inflate_any_record_words(void);
int e2e_inflate_any_window_bytes(void);
int e2e_inflate_find(const unsigned char* comp, long long n, long long segment_bytes, long long nseg, long long* starts, void* stream);
int e2e_inflate_spans_count(const unsigned char* comp, long long n, const long long* starts, long long m, long long max_span_bytes,
                            unsigned* records, void* stream);
int e2e_inflate_spans_write(const unsigned char* comp, long long n, const long long* starts, const long long* offs, long long m,
                            long long max_span_bytes, unsigned short* sym, long long nbytes, unsigned* status, void* stream);
int e2e_inflate_windows(const unsigned short* sym, const long long* offs, long long m, long long nbytes, unsigned char* wins,
                        unsigned* status, void* stream);
int e2e_inflate_resolve(const unsigned short* sym, const long long* offs, long long m, const unsigned char* wins, unsigned char* out,
                        long long nbytes, unsigned* status, void* stream);

/* ---- N7: the two-stage cascade (csrc/cascade.hip) -------------------------------------------------------------------------------
 * Replaces: resample_and_save of the 3d_lowres hand-over (e2enet/training/cascade_stuff/predict_next_stage.py:31-43:
 * resample_data_or_seg(order 1) of the [K, ...] softmax on the host, argmax(0), uint8) and the three transforms of
 * e2enet/training/data_augmentation/pyramid_augmentations.py:23-136 (skimage's ball / binary_dilation / binary_erosion /
 * binary_closing / binary_opening / label on every one-hot channel of the previous stage's segmentation).  Every result is an integer
 * or a bit, all atomics are integer: the same bits on every run.
 *   resample_argmax_u8: src as e2e_resample_linear reads it ([K] volumes of the frame [A,B,C] through strides, class stride kstride);
 *     seg (contiguous uint8 [OA,OB,OC]) = first maximum over k of the K order-1 values e2e_resample_linear(lowres_axis = -1) forms
 *     (the same expression, e2e_resample.h; a NaN counts as a maximum, as in e2e_export_argmax_u8).  1 <= K <= 256.
 *   seg_onehot: out[b, c0 + l, i] = (seg[b, channel, i] == labels[l]) as 0.0 / 1.0; seg [B, CS, vol], out [B, CO, vol]; labels is a
 *     HOST array of n_labels (1 .. 64) ints, read before the call returns.
 *   morph_*: binary morphology of one fp32 channel [D, H, W] on bit-packed rows.  pack: bits[(z H + y) ceil(W / 64) + w] holds
 *     x != 0 of voxels 64 w .. 64 w + 63 of the row, zero behind its end; e2e_morph_bits_words is the word count.  pass: the
 *     footprint of N^3 voxels with origin c = N / 2 is a HOST table of n_rows x (oz, oy, x_lo, x_hi), offsets from the origin, one
 *     contiguous x-run per (z, y) row.  dst[p] = OR over footprint offsets o of src[p - o], 0 outside the volume (scipy's
 *     binary_dilation); reflect != 0 reads src[p + o]; complement != 0 complements the source on load and the result on store, so
 *     that reflect = complement = 1 is binary_erosion(border_value = 1): AND over o of src[p + o], 1 outside.  src != dst.
 *     E2E_ERR_UNSUPPORTED, nothing launched: N > e2e_morph_max_footprint() (17), two runs in one (oz, oy) row (a row with a gap).
 *     unpack: sample[channel][i] = bit as 0.0 / 1.0 of a sample [n_channels, D, H, W]; where the bit is 1 and the channel was 0
 *     ("was added") the n_others (0 .. 64) channels of the HOST list `others` are set to 0 at that voxel.
 *   rcc_remove: x, one fp32 channel [D, H, W], is labelled with 26-neighbour connectivity (x != 0).  Of the components with
 *     (double)size < threshold, in the order of their first voxel in raster order (the label order of skimage and scipy), number
 *     floor(u * count) is set to 0 in x and, when fill != NULL, to 1 in fill.  0 <= u < 1.  result (device, 4 x u64): components,
 *     eligible components, size of the removed component (0: none), give-up word of the union-find (then nothing is removed).
 *     ws: e2e_rcc_ws_bytes(D, H, W) bytes; D H W <= 2^31 - 2.                                                                    */
int e2e_resample_argmax_u8(const float* src, unsigned char* seg, int K, long long kstride, int A, int B, int C, long long sa,
                           long long sb, long long sc, int OA, int OB, int OC, void* stream);
int e2e_seg_onehot(const float* seg, float* out, const int* labels, int n_labels, int B, int CS, int channel, int CO, int c0,
                   long long vol, void* stream);
int e2e_morph_max_footprint(void);
long long e2e_morph_bits_words(int D, int H, int W);
int e2e_morph_pack(const float* x, unsigned long long* bits, int D, int H, int W, void* stream);
int e2e_morph_pass(const unsigned long long* src, unsigned long long* dst, int D, int H, int W, const int* table, int n_rows, int N,
                   int reflect, int complement, void* stream);
int e2e_morph_unpack(const unsigned long long* bits, float* sample, int n_channels, int channel, const int* others, int n_others,
                     int D, int H, int W, void* stream);
long long e2e_rcc_ws_bytes(int D, int H, int W);
int e2e_rcc_remove(float* x, float* fill, int D, int H, int W, double threshold, double u, void* ws, unsigned long long* result,
                   void* stream);

#ifdef __cplusplus
}
#endif
#endif /* E2E_HIP_H */
