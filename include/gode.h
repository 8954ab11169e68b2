/* gode.h -- C ABI of libgode.so, the MI355X (gfx950) native library behind the MoCoGAN + Neural-ODE hot path.
 *
 * The reference (chechaohp/gan-ode) is pure Python on PyTorch and has no FFI of its own; its seam for this path is
 * the class surface imported by mnist_moco_ode.py:5-6 / ucf_moco_ode.py:5-6.  The Python host code in
 * gan-ode_amd/ mirrors that surface and lowers every call to the entry points below through ctypes.  Each entry
 * point cites the reference arithmetic it replaces.
 *
 * Conventions
 *  - plain pointers and sizes only; every pointer is DEVICE memory owned by the caller (PyTorch's allocator);
 *    the library never allocates, frees or keeps memory and has no mutable global state (the one object it owns is
 *    the caller-created lanes object of the two-lane runner: a stream and three events, no device memory);
 *  - every call only ENQUEUES work on `stream` (a hipStream_t passed as void*) and never synchronises;
 *  - return value: 0 ok, <0 argument error (GODE_E_*), >0 a hipError_t from a launch;
 *  - activations are channels-last fp32: [N][D][H][W][C]; weights stay in PyTorch's canonical layout
 *    W[co][ci][kd][kh][kw] (Conv) == W[in][out][kh][kw] (ConvTranspose, seen as the conv whose dgrad it is) and
 *    are re-packed on the device by gode_pack_* into the K-contiguous panels the GEMM kernels read.
 */
#ifndef GODE_H
#define GODE_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define GODE_VERSION 105

enum { GODE_OK = 0, GODE_E_ARG = -1, GODE_E_SHAPE = -2, GODE_E_KIND = -3 };
enum { GODE_ACT_NONE = 0, GODE_ACT_RELU = 1, GODE_ACT_LRELU = 2,              /* LeakyReLU slope is 0.2 */
       GODE_ACT_TANH_OUT = 3 /* bn_bwd only: y holds tanh OUTPUT, g *= 1-y^2 */,
       GODE_ACT_TANH = 4, GODE_ACT_SIGMOID = 5 /* gode_fc_act / gode_fc_act_bwd only */,
       GODE_ACT_LRELU01 = 6 /* LeakyReLU with slope 0.1: wherever the convolution stack takes GODE_ACT_LRELU (gode_igemm, gode_wgrad,
                               gode_bn_apply, gode_bn_bwd, gode_dnoise); not gode_fc_act / gode_cbn_* */ };
enum { GODE_EPI_RAW = 0, GODE_EPI_TANH = 1 };
enum { GODE_FPROP = 0, GODE_DGRAD = 1 };
/* or'ed into the `dir` of gode_pack_size / gode_pack_weights / gode_pack_op: the pack an igemm op with border != 0 reads */
enum { GODE_PACK_BORDER = 0x100 };

/* A regular convolution x[N,Di,Hi,Wi,Ci] -> y[N,Do,Ho,Wo,Co].  2-D layers use D=1,kd=1,sd=1,pd=0.  A
 * ConvTranspose layer is described by the convolution whose data-gradient it is (x = its output). */
typedef struct gode_conv_geom {
  int32_t N, Ci, Co;
  int32_t Di, Hi, Wi;
  int32_t Do, Ho, Wo;
  int32_t kd, kh, kw;
  int32_t sd, sh, sw;
  int32_t pd, ph, pw; /* may be negative (ConvTranspose k=1,p=2 of mocogan_ode.py:82 is a crop) */
} gode_conv_geom;

/* ---- implicit-GEMM convolution (fp32 MFMA 32x32x2) ---------------------------------------------------------
 * dir=GODE_FPROP: out=y, gathers x.  dir=GODE_DGRAD: out=x, gathers y (one sub-GEMM per stride phase; this is
 * the ConvTranspose2d forward of models/mocogan.py:200-215 and the Conv3d/Conv2d input-gradient).
 * The gathered operand is read through element strides gs[5] = {N,D,H,W,C} (lets the first discriminator layer
 * read the caller's [B,C,T,H,W] / transposed views in place, mnist_moco_ode.py:136-139) and transformed on load:
 *   a = act(v*scale[c] + shift[c])   (train-mode BatchNorm + ReLU/LeakyReLU of the PREVIOUS layer; nullable).
 * Zero padding is applied after the transform.  `wpack` comes from gode_pack_weights for the same geom/dir.
 * If stats != NULL, per-column partial sums (sum, sum of squares) of the raw outputs are written to
 * stats[2][ncols][rows] (row = m-block, rows = gode_igemm_stats_rows(op); deterministic), feeding
 * gode_bn_finalize, which reads each channel's rows contiguously. */
typedef struct gode_igemm_op {
  gode_conv_geom g;
  int32_t dir, act, epilogue, tile; /* tile: 0 auto; 1 128x128, 2 128x64, 3 128x32, 4 64x64, 6 256x128; else GODE_E_ARG */
  const float* src;
  const float* wpack;
  float* out;
  const float* scale;
  const float* shift;
  float* stats;
  int64_t gs[5];
  /* nullable; >= gode_igemm_work_size(op) floats.  When that size is > 0 the launch plan splits K (it is made from the
   * geometry alone: it sees no pointer) and the split launch needs `work`, and src, scale and shift on 16-byte boundaries.
   * Without either the op is served all the same, unsplit on the generic kernel (slower): out, the statistics layout and
   * gode_igemm_stats_rows / _rows0 stay those of the plan. */
  float* work;
  /* groups == 2 (FPROP with stats only, N even): the batch is two image groups [0, N/2) and [N/2, N) whose BatchNorm
   * partial statistics must stay separate -- one discriminator pass over [real; fake] keeps the per-pass batch
   * statistics of the reference's two calls (mnist_moco_ode.py:119-124,137-143).  The partial-statistics rows of group 0
   * are the first gode_igemm_stats_rows0(op) rows of every column, group 1 the rest.  0 / 1: one group. */
  int32_t groups;
  /* border != 0 (DGRAD; ignored by FPROP, fullk, groups == 2, live-tap and split-K launches): the launch may run the
   * border-split phase table -- every stride phase cut into interior / edge / corner sub-phases that hold only in-range
   * taps, so no MFMA multiplies zero padding.  `wpack` must then be packed with dir = GODE_DGRAD | GODE_PACK_BORDER (that
   * pack extends the plain one, so the launch is free to stay plain when its cost model says so).  Raw outputs are bit-identical to
   * border == 0; the partial-statistics rows are grouped differently: gode_igemm_stats_rows / _rows0 / _work_size /
   * _model_cycles all follow the flag.  0: as before.
   * border == 2: the caller has measured the layer and decides.  The launch takes the border-split table whenever the op has
   * one, every sub-phase runs on the MFMA kernel's fast path (channels and every K in whole 32-deep slabs, vector strides) and K is not
   * split -- with the tile of the border cost model (tile == 0; the plain plan when that model offers none: fewer than 4/3
   * tiles per workgroup slot), or the requested one -- without comparing the two forms' modelled cost.  Its grid is
   * phase-interleaved where the table allows: the sub-phases of one border class (interior, h-edge, w-edge, corner) of all
   * stride phases, which gather the same input rows, run back to back on one XCD per m-block, classes in descending K;
   * tables whose classes do not hold one sub-phase of every stride phase (k3 s2 p1, temporal taps off both ends) keep the
   * order of border == 1.  Same pack as border == 1; at equal tile raw outputs AND partial-statistics rows are bit-identical
   * to border == 1.  Any other nonzero value: as 1. */
  int32_t border;
} gode_igemm_op;
int gode_igemm(const gode_igemm_op* op, void* stream);
/* floats of workspace the op needs to split K (0: it never splits).  Deterministic from the op's geometry. */
int64_t gode_igemm_work_size(const gode_igemm_op* op);
/* number of partial-stats rows gode_igemm writes for this op (host-side, no GPU work) */
int gode_igemm_stats_rows(const gode_igemm_op* op);
/* rows of those that belong to image group 0 (== gode_igemm_stats_rows unless op->groups == 2) */
int gode_igemm_stats_rows0(const gode_igemm_op* op);
/* A stack whose batch is [first `split_images` images; the rest] with SEPARATE BatchNorm statistics per part (the generator's
 * video and image paths decoded in one pass): which partial-statistics rows belong to which part.  Writes up to 8 segments
 * {begin, split, end} (gode_bn_finalize_op.seg) and returns their number; GODE_E_SHAPE when a tile (or split-K statistics
 * chunk) of this op would straddle the boundary -- the caller then runs the two parts separately. */
int gode_igemm_stats_segments(const gode_igemm_op* op, int32_t split_images, int32_t* seg);
/* The launch-time estimate (GPU cycles) of the tile / split-K cost model for this op, or -1 when the op does not take the
 * modelled path.  Host-side, no GPU work: such a caller compares one launch over the whole batch with two over its parts. */
double gode_igemm_model_cycles(const gode_igemm_op* op);
/* The kernel family the launch plan gives the op: 0 tiled GEMM, 1 LDS-patch FPROP, 2 pointwise (thin-output streaming),
 * 3 tiny-K, 4 dot.  Host-side, no GPU work; unaligned pointers can still take a launch from its family to the tiled GEMM
 * (src / scale / shift off a 16-byte boundary: pointwise and dot; out: tiny-K; the LDS-patch kernel reads scalars and
 * stays), and there from the vector kernels to the scalar generic one (a plan that splits K then runs unsplit: see
 * gode_igemm_op.work). */
int gode_igemm_family(const gode_igemm_op* op);
/* The launch cell: what gode_igemm(op) launches, decided by the function the launch itself dispatches on.  Returns what
 * gode_igemm would return before launching anything (0, GODE_E_ARG, GODE_E_SHAPE); on 0, cell[8] =
 *   {kernel, tile, reduce, ksplit, xcd_mode, table, interleave, tapskip}
 * kernel: -1 nothing (empty op); 0 FAST LDS-DMA, 1 FAST LDS-DMA over live taps, 2 FAST register-staged with the transform on
 *   load, 3 FAST register-staged plain (an operand beyond 2 GiB), 4 generic float4, 5 generic scalar, 6 / 7 / 8 pointwise
 *   (one tap and one column / one tap / several taps), 9 tiny-K, 10 dot, 11 LDS-patch.
 * tile: the tile id of a tiled launch (kernels 0-5), else 0.  reduce: the split-K finish, 0 none, 1 float4, 2 scalar
 *   (with ksplit == 1 on kernels 4 / 5: a plan that splits K served unsplit, the finish run over that one slab).
 * table: 0 plain, 1 border-split, 2 border-split phase-interleaved (`interleave` sub-phases per entry).  xcd_mode: the
 * FAST kernels' grid order.  Host-side, no GPU work; the op's pointers are looked at (null, alignment), never through. */
int gode_igemm_launch_cell(const gode_igemm_op* op, int32_t* cell);
/* Share of the op's multiply-adds that gather zero padding at the tensor's borders: 1 - (sum of M*K over the border-split
 * table) / (sum of M*K over the plain table); 0 when the op has no border-split table (gode_igemm_op.border).  Host-side. */
double gode_igemm_dead_taps(const gode_igemm_op* op);
/* The shape of the op's launch plan: info = {1 if it runs the border-split table, tile id, tiles of the GEMM launch,
 * workgroups the chip holds at once with that tile (256 CUs x resident workgroups per CU)}.  Host-side; 0 or an error. */
int gode_igemm_launch_info(const gode_igemm_op* op, int32_t* info);
/* floats needed for the packed weights of (geom, dir) */
int64_t gode_pack_size(const gode_conv_geom* g, int dir);
/* canonical W[co][ci][taps] -> packed panels.  co_perm (nullable, length g->Co): internal y-side channel c is
 * canonical output channel co_perm[c] (zero weights when co_perm[c] < 0); g->Co counts INTERNAL channels.  Used for
 * the generator's first layer, whose latent buffer is stored [motion 16|content 50|pad 6] while the reference
 * concatenates content first (models/mocogan.py:267). */
int gode_pack_weights(const gode_conv_geom* g, int dir, const float* w, float* wpack, const int32_t* co_perm,
                      int32_t co_canon, void* stream);

/* ---- weight gradient: dW[co][ci][taps] = sum_m y_grad[m][co] * act(x*scale+shift)[pos(m,tap)][ci] ----------
 * split over the reduction (output positions) into `splits` slabs of a workspace, then reduced deterministically
 * and scattered into the canonical layout (accumulate!=0 adds to dW).  xform_on_y!=0 applies the transform to
 * the y-side operand instead (ConvTranspose layers: their *input* is the y side). */
typedef struct gode_wgrad_op {
  gode_conv_geom g;
  int32_t act, xform_on_y, splits, accumulate;
  const float* x;  /* x side tensor (channels-last unless xs given) */
  const float* y;  /* y side tensor, channels-last */
  const float* scale;
  const float* shift;
  float* work;     /* >= gode_wgrad_work_size floats */
  float* dw;       /* canonical layout */
  const int32_t* co_perm; int64_t co_canon; /* as in gode_pack_weights, nullable / g.Co */
  int64_t xs[5];   /* element strides of x {N,D,H,W,C}; all zero = channels-last contiguous */
} gode_wgrad_op;
int gode_wgrad(const gode_wgrad_op* op, void* stream);
int64_t gode_wgrad_work_size(const gode_wgrad_op* op);
int gode_wgrad_auto_splits(const gode_conv_geom* g);

/* ---- BatchNorm (train mode: batch statistics, eps, momentum as nn.BatchNorm2d/3d defaults) ------------------
 * finalize: partial sums -> mean, invstd, and the fused affine scale=gamma*invstd, shift=beta-mean*scale that the
 * NEXT layer's operand load applies; updates running_mean/var (unbiased var) and num_batches_tracked.
 * training==0: scale/shift from the running statistics (genSamples' eval mode, mnist_moco_ode.py:31-35). */
typedef struct gode_bn_finalize_op {
  const float* stats; int32_t rows, ncols, C; int64_t count;
  const float* gamma; const float* beta;
  float* running_mean; float* running_var; int64_t* num_batches_tracked;
  float* mean; float* invstd; float* scale; float* shift;
  float momentum, eps; int32_t training, pad_;
  /* groups == 2: the first rows0 partial rows belong to image group 0, the rest to group 1 (count = elements per channel
   * and GROUP); mean / invstd / scale / shift are [2][C] (group-major); the running statistics receive the two
   * momentum updates in group order (what two successive forward calls do), num_batches_tracked += 2. */
  int32_t groups, rows0;
  /* groups == 2, general form (nseg > 0 overrides rows0): up to 8 row segments {begin, split, end} -- rows [begin, split) are
   * group 0, [split, end) group 1 (gode_igemm_stats_segments: one per stride phase of a transposed-convolution stack whose
   * rows are [first batch; second batch]); count1 (> 0): elements per channel of group 1 when the groups differ in size
   * (count: group 0); order != 0: group 1's momentum update is applied first (the reference called that batch first). */
  int32_t nseg, order; int64_t count1; int32_t seg[24];   /* 8 x {begin, split, end} */
  /* groups == 2, two-launch form (overrides nseg / rows0): group 1's partial sums are an array of their own,
   * stats1[2][ncols][rows1], written by a second gode_igemm launch over that batch alone; `stats` / `rows` are group 0's. */
  const float* stats1; int32_t rows1, pad3_;
  /* deferred form (non-null; training mode, one group, no segments -- anything else is GODE_E_ARG): the unbiased batch
   * variance goes to batch_var[C] as float, the batch mean is mean[] as always, and running_mean / running_var /
   * num_batches_tracked are neither read nor written -- gode_bn_running applies their updates later.  Nothing then orders
   * two passes over the same module layer by layer. */
  float* batch_var;
} gode_bn_finalize_op;
int gode_bn_finalize(const gode_bn_finalize_op* op, void* stream);

/* The momentum updates that deferred finalizes left out, for up to GODE_BN_RUNNING_MAX layers in ONE launch (one workgroup,
 * layers in order):  running_mean = (1 - momentum) * running_mean + momentum * mean,  running_var likewise from var (the slot
 * a deferred finalize wrote),  num_batches_tracked += 1 -- operation for operation what the in-place finalize does, so the
 * running tensors hold the same bits either way.  running_mean == NULL: that layer only counts its batch. */
#define GODE_BN_RUNNING_MAX 8
typedef struct gode_bn_running_layer {
  const float* mean; const float* var; float* running_mean; float* running_var; int64_t* num_batches_tracked;
  int32_t C, pad_;
} gode_bn_running_layer;
typedef struct gode_bn_running_op {
  gode_bn_running_layer layer[8];   /* GODE_BN_RUNNING_MAX rows, the first n used */
  int32_t n; float momentum;
} gode_bn_running_op;
int gode_bn_running(const gode_bn_running_op* op, void* stream);

/* out = act(y*scale[c] + shift[c]) over [M][C] (C % 4 == 0): materialises an activated tensor for consumers that are
 * MFMA-bound and re-read every element several times (the heavy GEMMs run ~10-20 % faster without the transform
 * in their operand path; light layers keep it fused).  scale==NULL: plain activation. */
typedef struct gode_bn_apply_op {
  const float* y; float* out; const float* scale; const float* shift; int64_t M; int32_t C, act;
  int64_t M0; /* > 0: rows >= M0 use scale + C / shift + C (second image group of a grouped pass); 0: one group */
} gode_bn_apply_op;
int gode_bn_apply(const gode_bn_apply_op* op, void* stream);

/* Overlap-add of per-pixel tap contributions: the second half of a thin-output ConvTranspose2d (the UCF generator's
 * RGB head, models/mocogan.py:213) computed as ONE plain GEMM over the input pixels -- gode_igemm, DGRAD of the geometry
 * {N = pixels, Di x Hi x Wi = 1 x kh x kw, Do = Ho = Wo = 1}: cols[pixel][(kh, kw, c)] -- followed by
 *   out[n][oh][ow][c] = epilogue( sum over taps with oh = ih*sh - ph + kh, ow = iw*sw - pw + kw of cols[(n, ih, iw)][(kh, kw, c)] )
 * in fixed tap order.  Every input activation is then read once instead of once per tap and phase. */
typedef struct gode_col2im_op {
  const float* cols; float* out;
  int32_t N, Hi, Wi, Ho, Wo, C, kh, kw, sh, sw, ph, pw;   /* Hi x Wi: the pixels of cols; Ho x Wo: out */
  int32_t epilogue, pad_;                                  /* GODE_EPI_RAW / GODE_EPI_TANH */
  /* 3-D form (kd > 0; all zero: the 2-D op above): cols pixels are (n, id, ih, iw) over Di x Hi x Wi with kd*kh*kw*C values
   * each (tap order kd, kh, kw), out is Do x Ho x Wo, od = id*sd - pd + kd.  The input gradient of a thin-INPUT Conv3d (the UCF
   * video discriminator's first layer, models/mocogan.py:100: 3 channels, 4x4x4 taps) is one GEMM over its output positions
   * + this overlap-add, instead of a gather of 1,024 values per input voxel. */
  int32_t Di, Do, kd, sd, pd, pad2_;
} gode_col2im_op;
int gode_col2im(const gode_col2im_op* op, void* stream);
/* The launch plan: which kernel gode_col2im(op) launches and why, decided by the function the launch itself dispatches on.
 * Returns what gode_col2im would return before launching anything (0, GODE_E_ARG, GODE_E_SHAPE); on 0, kind[2] =
 *   kind[0]: 0 row-group LDS kernel (2-D), 1 per-pixel 2-D, 2 3-D with fixed 4x4x4 taps / strides 1x2x2 / C == 3, 3 3-D generic;
 *   kind[1]: why a 2-D op left the row-group kernel (0: it did not) -- bit 0 the row length Wi*kh*kw*C is no multiple of 4,
 *     bit 1 cols is off a 16-byte boundary, bit 2 its R = ceil(kh/sh) input rows exceed 48 KiB of LDS, bit 3 N * row groups
 *     >= 2^31; for a 3-D op why it left the fixed kernel -- bit 0 taps or strides are not the fixed ones, bit 1 C != 3, bit 2
 *     N*Do*Ho*Wo >= 2^31.
 * All four kernels add an output element's taps in the same order ((kd,) kh, kw ascending from 0.f): the kind changes no bit
 * of a raw output.  Host-side, no GPU work; cols is looked at (null, alignment), never through. */
int gode_col2im_launch_kind(const gode_col2im_op* op, int32_t* kind);

/* backward of y -> BN -> act given g_a = dL/d(act output), all [M][C] channels-last:
 *   g_z = g_a * act'(scale*y+shift);  dbeta = sum g_z;  dgamma = sum g_z*xhat;
 *   g_y = gamma*invstd*(g_z - dbeta/M - xhat*dgamma/M)     written in place over g_a.
 * With mean==NULL the layer has no BN: g_y = g_a*act'(y).  work: >= gode_bn_bwd_work_size floats, 8-byte aligned
 * (the two sums are accumulated in fp64).
 * accumulate!=0 adds into dgamma/dbeta.
 * eval_mode!=0: the forward normalised with the RUNNING statistics (mean/invstd hold them), which are constants:
 *   g_y = gamma*invstd*g_z  (dgamma/dbeta as above, with xhat from the running statistics). */
typedef struct gode_bn_bwd_op {
  float* g; const float* y; int64_t M; int32_t C, act;
  const float* gamma; const float* mean; const float* invstd; const float* scale; const float* shift;
  float* dgamma; float* dbeta; float* work; int32_t accumulate, eval_mode;
  const float* gin; /* nullable: read g_a from here instead of g (g is then write-only); lets the caller's upstream
                       gradient tensor be consumed in place without being modified */
  /* groups == 2 (M even): rows [0, M/2) and [M/2, M) are two BatchNorm batches of one grouped pass -- mean / invstd /
   * scale / shift are [2][C] (group-major, as gode_bn_finalize writes them), the batch terms use each group's own sums,
   * dgamma / dbeta receive both groups' sums in group order (what the reference's two backward passes add up to). */
  int32_t groups, pad2_;
  int64_t M0;   /* groups == 2: rows of group 0 (0: M / 2) */
  /* Rank-1 upstream gradient (r1_s != NULL; g is then write-only and gin ignored): the layer feeds a 1x1 convolution to ONE
   * channel whose output is a centre crop (the MNIST generator's head, models/mocogan.py:151), so g_a[row][c] =
   * r1_w[c] * r1_s[crop(row)] and the [M][C] gradient tensor need not be written and read back before this op.  Rows are
   * (image, h, w) over r1_H x r1_W; r1_s is (image, h - r1_off, w - r1_off) over r1_h x r1_w, zero outside. */
  const float* r1_s; const float* r1_w; int32_t r1_H, r1_W, r1_h, r1_wd, r1_off, pad3_;
} gode_bn_bwd_op;
int gode_bn_bwd(const gode_bn_bwd_op* op, void* stream);
int64_t gode_bn_bwd_work_size(int64_t M, int32_t C);

/* ---- motion-latent ODE (models/mocogan_ode.py:6-17,123-148; torchdiffeq fixed-grid rk4 = Kutta 3/8) --------
 * forward: x[N][16] host-drawn noise -> pre-net Linear(16,64)/LReLU/Linear(64,16)/LReLU -> T-1 RK4(3/8) steps
 * of f(y)=W2 tanh(W1 y+b1)+b2 with step sizes dt[T-1] -> latent rows.  z is the generator's latent buffer
 * [rows][zcols] = [motion 16 | content 50 | zero pad] (zcols % 4 == 0, >= 68; the Python side uses 96 so that the
 * first decoder GEMM has K % 32 == 0); row n*T+t (sel_t==NULL) or row n holding time sel_t[n]
 * (sample_images' row selection, models/mocogan.py:287-295).  content[N][50] is broadcast over the T rows.
 * traj[N][T][16] (nullable) keeps the whole trajectory for the adjoint pass. */
typedef struct gode_ode_params {
  const float* Wa; const float* ba; const float* Wb; const float* bb; /* pre-net: [64,16],[64],[16,64],[16] */
  const float* W1; const float* b1; const float* W2; const float* b2; /* ODEFunc: [16,16],[16],[16,16],[16] */
} gode_ode_params;
typedef struct gode_ode_fwd_op {
  gode_ode_params p;
  const float* x; const float* content; const float* dt; const int32_t* sel_t;
  float* z; float* traj; int32_t N, T, substeps, prenet; /* prenet==0: linear=False (nn.Identity) */
  int32_t zcols, G;
  /* optional solver grid (torchdiffeq options={'step_size': h}: FixedGridODESolver integrates on its own grid and
   * interpolates the outputs linearly).  grid_dt[G] = step sizes of the grid; output j >= 1 is produced after grid
   * step emit_at[j] as y0 + emit_w[j]*(y1 - y0) (emit_w == 1: y1 itself).  grid_dt == NULL: the grid is the output
   * times (dt[T-1], `substeps` equal sub-steps each) -- the reference's own call. */
  const float* grid_dt; const int32_t* emit_at; const float* emit_w;
  /* method 1: torchdiffeq's dopri5 (adaptive Dormand-Prince 5(4), controller and 4th-order dense output as in
   * gode_odernn_fwd) over the T output times tout[T] (increasing, tout[0] = start); the error norm is taken jointly
   * over the trajectories of a workgroup (<= 64; torchdiffeq: over the whole batch).  nsteps[ceil(N/64)] (nullable)
   * receives the number of trial steps.  method 0: fixed-grid rk4 (above).
   * method 2: torchdiffeq's euler, y1 = y0 + dt f(y0); method 3: its midpoint, y1 = y0 + dt f(y0 + (dt/2) f(y0)).  Both
   * walk the grids of method 0 (dt / substeps, or grid_dt / emit_at / emit_w) and take the same arguments; they run on
   * the vector-ALU kernels at every N.  Any other code: GODE_E_ARG.
   * rhs: the right-hand side.  0: f(y) = W2 tanh(W1 y + b1) + b2 (above; what a zero-initialised op asks for).
   * 1: f(y) = tanh(W1 y + b1), the one-layer ODEFunc of models/mocogan_mnist.py:6-16 -- its weight in p.W1, its bias in
   * p.b1; p.W2 and p.b2 are never dereferenced (NULL is fine).  Served for methods 0, 2 and 3, on the vector-ALU kernels at
   * every N; rhs 1 with method 1 (the adaptive kernels integrate u = W1 y + b1, the two-layer function's algebra) and any
   * rhs other than 0 or 1: GODE_E_ARG, from gode_ode_fwd and gode_ode_fwd_multi alike, before any launch. */
  int32_t method, rhs; float rtol, atol; const float* tout; int32_t* nsteps;
  /* method 1 with N > 32: >= gode_odernn_sync_size(N) words through which the workgroups exchange the whole-batch error norm
   * (see the ODE-RNN ops below; NULL or more than GODE_ODERNN_SYNC_MAX_N trajectories per launch: one norm per
   * 64-trajectory workgroup, nsteps per such workgroup).  With it nsteps[0] = trial steps of the call (negative: stalled). */
  int32_t* sync;
} gode_ode_fwd_op;
int gode_ode_fwd(const gode_ode_fwd_op* op, void* stream);
/* `count` (<= 8) independent method-1 solves in ONE launch (ops: HOST array): the dopri5 counterpart of
 * gode_odernn_fwd_multi below */
int gode_ode_fwd_multi(const gode_ode_fwd_op* ops, int32_t count, void* stream);
/* adjoint backward (torchdiffeq odeint_adjoint semantics: per output interval ONE reverse-time RK4(3/8) step of
 * (y, a, g_theta), y reset to the stored trajectory, a += upstream grad) followed by the pre-net backward.
 * gz[rows][zcols]: gradient wrt the latent rows (only the 16 motion columns are read).  Parameter gradients are
 * reduced deterministically through work (>= gode_ode_bwd_work_size floats) and written (accumulate!=0: added) to
 * grads, laid out as the 8 tensors of gode_ode_params in order (2672 floats).  prenet == 0: the first 2128 floats of
 * grads (the pre-net block) are neither read nor written, on every path (rk4 and dopri5, single and _multi calls) --
 * grads may point 2128 floats before a region that holds only the ODEFunc block. */
typedef struct gode_ode_bwd_op {
  gode_ode_params p;
  const float* x; const float* traj; const float* dt; const int32_t* sel_t; const float* gz;
  float* work; float* grads; int32_t N, T, substeps, prenet, accumulate, zcols;
  /* optional per-interval reverse step lists (same option: the adjoint solve of output interval j -> j-1 runs on the
   * grid torchdiffeq builds for the reversed span): steps bstep_dt[bstep_off[j-1] .. bstep_off[j]) for j = 1..T-1.
   * NULL: `substeps` equal steps of dt[j-1]/substeps. */
  const int32_t* bstep_off; const float* bstep_dt;
  /* method 1 with substeps == 0: torchdiffeq's ADAPTIVE adjoint of a dopri5 solve -- the augmented state (y, a, g_theta)
   * of the one adjoint call is integrated backwards over the output times tout[T] with dopri5 (rtol, atol), mixed norm
   * (max over the RMS norms of y, a and each ODEFunc parameter tensor, joint over a workgroup's <= 64 trajectories);
   * the theta state is carried across the output intervals, the solver restarts on each.  method 1 with substeps > 0:
   * the same adjoint discretised with `substeps` fixed Kutta-3/8 steps per interval (round-1 behaviour; dt required).
   * method 2 (euler) / 3 (midpoint): the adjoint of method 0 with the reverse-time steps of (y, a, g_theta) taken by that
   * method (the parameter integrals get its b-weights: euler's one stage 1; midpoint's first stage 0, its second 1);
   * same arguments as method 0 (dt, substeps >= 1, bstep_off / bstep_dt).  Any other code: GODE_E_ARG.
   * rhs: as in gode_ode_fwd_op.  rhs 1 (f(y) = tanh(W1 y + b1)): p.W2 / p.b2 are never dereferenced, and the gradient
   * block is the first 2400 floats of the layout above (pre-net block, W1, b1): floats [2400, 2672) of grads are neither
   * read nor written, on every path (the two-level reduce included) -- grads may end at float 2400.  `work` rows keep
   * their stride of GODE_ODE_NPARAM floats (gode_ode_bwd_work_size does not depend on rhs).  rhs 1 with method 1
   * (substeps 0 or not) and any rhs other than 0 or 1: GODE_E_ARG from gode_ode_bwd and gode_ode_bwd_multi, before any
   * launch. */
  int32_t method, rhs; float rtol, atol; const float* tout;
  int32_t* nsteps;   /* nullable, adaptive adjoint only: trial steps of the adjoint call (nsteps[0]; without `sync` and N > 32:
                        [ceil(N/64)], one per workgroup); a negative entry reports a call that stalled (trial-step limit /
                        step-size underflow: torchdiffeq asserts there) */
  int32_t* sync;     /* adaptive adjoint with N > 32: as in gode_ode_fwd_op */
  /* backprop: 0 (what a zero-initialised op asks for) = the continuous adjoint above.  1 = DISCRETE backprop: the exact
   * reverse-mode gradient of the fixed-grid forward solve (what autograd through torchdiffeq's odeint gives), step by step in
   * reverse order from each step's start state: the stage inputs u_s and h_s = tanh(W1 u_s + b1) are recomputed, then with
   * J_s^T g the vector-Jacobian product of f at u_s and lambda = dL/dy1
   *   euler:    g1 = dt lambda;                            lambda += J1^T g1
   *   midpoint: g2 = dt lambda, gu2 = J2^T g2, g1 = (dt/2) gu2;   lambda += gu2 + J1^T g1
   *   rk4:      g4 = dt/8 lambda, gu4 = J4^T g4;  g3 = 3dt/8 lambda + dt gu4, gu3 = J3^T g3;
   *             g2 = 3dt/8 lambda - dt gu4 + dt gu3, gu2 = J2^T g2;
   *             g1 = dt/8 lambda + dt gu4 - dt/3 gu3 + dt/3 gu2, gu1 = J1^T g1;   lambda += gu1 + gu2 + gu3 + gu4
   * and every stage adds its parameter VJP with g_s.  Methods 0, 2 and 3, both rhs, on the vector-ALU kernel at every N
   * (GODE_ODE_MFMA does not apply).  The grid is the FORWARD solve's: dt / substeps, or G / grid_dt / emit_at / emit_w as in
   * gode_ode_fwd_op, grid_dt != NULL needing emit_at, emit_w and G >= 1; an interpolated output y0 + w (y1 - y0) hands w gz to the
   * step's lambda before the reverse step and (1 - w) gz after it; bstep_off / bstep_dt are ignored.  With substeps == 1 and
   * grid_dt == NULL the step-start states are traj itself and ysteps may be NULL; otherwise the launch re-runs the forward
   * from traj[n][0] and keeps every step's start state in ysteps (>= gode_ode_bwd_steps_size floats, caller-owned
   * scratch).  grads / work / accumulate / prenet == 0 / rhs == 1 / determinism: exactly as for backprop 0.
   * GODE_E_ARG before any launch: backprop other than 0 or 1; backprop 1 with method 1; backprop 1 with ysteps needed and
   * NULL; any op with backprop != 0 in gode_ode_bwd_multi. */
  int32_t backprop, G;
  const float* grid_dt; const int32_t* emit_at; const float* emit_w;
  float* ysteps;
} gode_ode_bwd_op;
int gode_ode_bwd(const gode_ode_bwd_op* op, void* stream);
/* floats of gode_ode_bwd_op.ysteps for a discrete-backprop op: 16 per trajectory and solver step -- N * G * 16 on a grid_dt
 * grid (G >= 1), N * (T-1) * substeps * 16 with substeps > 1, and 0 where the grid is the output times themselves (G == 0,
 * substeps <= 1: ysteps may be NULL) */
int64_t gode_ode_bwd_steps_size(int32_t N, int32_t T, int32_t substeps, int32_t G);
/* the adaptive adjoints (method 1, substeps 0) of `count` (<= 8) solves in one launch; ops sharing a grads pointer form a
 * group under the group rule stated at gode_odernn_bwd_multi */
int gode_ode_bwd_multi(const gode_ode_bwd_op* ops, int32_t count, void* stream);
int64_t gode_ode_bwd_work_size(int32_t N);
#define GODE_ODE_NPARAM 2672

/* ---- ODE-RNN motion latent (models/mocogan_ode_rnn.py:41-53) -------------------------------
 * per frame: h' = odeint_adjoint(ODEFunc, h, [0,1])[-1] with torchdiffeq's default dopri5 (rtol, atol), then
 * h = GRUCell(e_t, h').  noise[T+1][N][16] = h_0, e_0..e_{T-1} drawn on the host.  z / content / sel_t as in
 * gode_ode_fwd (row t = h_{t+1}).  hs[N][T+1][16] (nullable), hp[N][T][16] (post-ODE states, kept for the backward).
 * Error norm: the RMS over ALL N trajectories of the call, as torchdiffeq takes it (models/mocogan_ode_rnn.py:47-48 hands
 * the whole batch to one odeint call): a workgroup integrates 32 trajectories; for N > 32 the workgroups of a call
 * exchange their partial sums of squares through `sync` (gode_odernn_sync_size(N) 4-byte words, caller-owned, zeroed by
 * the launch) and add them in fixed order, so every workgroup takes bit-identical accept / reject decisions and re-runs
 * are bit-identical.  All workgroups of a launch must be co-resident: N <= GODE_ODERNN_SYNC_MAX_N per launch (summed
 * over the ops of a _multi launch); above that the call falls back to one norm per 64-trajectory workgroup (a recorded
 * deviation, unused by any configuration).  nsteps[T] (nullable): dopri5 trial steps per frame (of workgroup 0 in the
 * fallback); a negative entry reports a solve that hit the trial-step limit or whose step size underflowed. */
typedef struct gode_odernn_params {
  const float* W1; const float* b1; const float* W2; const float* b2;         /* ODEFunc */
  const float* Wih; const float* Whh; const float* bih; const float* bhh;     /* GRUCell(16,16): [48,16]x2, [48]x2 */
} gode_odernn_params;
typedef struct gode_odernn_fwd_op {
  gode_odernn_params p;
  const float* noise; const float* content; const int32_t* sel_t;
  float* z; float* hs; float* hp; int32_t* nsteps;
  int32_t N, T; float rtol, atol; int32_t zcols, pad_;
  int32_t* sync;    /* N > 32: >= gode_odernn_sync_size(N) words; ignored (may be NULL) for N <= 32 */
} gode_odernn_fwd_op;
int gode_odernn_fwd(const gode_odernn_fwd_op* op, void* stream);
#define GODE_ODERNN_SYNC_MAX_N 4096
int64_t gode_odernn_sync_size(int32_t N);
/* `count` (<= 8) independent solves in ONE launch, each with its own whole-batch norm: one training iteration's
 * sample_videos / sample_images latents depend only on the generator's weights at the start of the iteration, so their
 * one-workgroup solves run side by side on different CUs instead of back to back (ops: HOST array). */
int gode_odernn_fwd_multi(const gode_odernn_fwd_op* ops, int32_t count, void* stream);
/* backward: GRU backward + continuous adjoint of every unit-interval solve.  substeps == 0 (what the Python side
 * uses): integrated ADAPTIVELY as torchdiffeq does -- per frame one adjoint call, dopri5 (rtol, atol) on the augmented
 * state (y, a, g_theta), mixed norm (max over the RMS norms of y, a and each ODEFunc parameter tensor) over the whole
 * batch of the call (sync as above).  substeps > 0: `substeps` fixed reverse-time Kutta-3/8 steps per frame (32 agree
 * with the adaptive result to ~1e-6).  grads: 2176 floats = W1,b1,W2,b2,Wih,Whh,bih,bhh.
 * work >= gode_odernn_bwd_work_size floats.  nsteps[T] (nullable, adaptive only): trial steps per frame's adjoint call,
 * negative = the solve stalled (trial-step limit / step-size underflow; torchdiffeq asserts there). */
typedef struct gode_odernn_bwd_op {
  gode_odernn_params p;
  const float* noise; const float* hp; const int32_t* sel_t; const float* gz;
  float* work; float* grads; int32_t N, T, substeps, accumulate, zcols, pad_;
  float rtol, atol;   /* substeps == 0: adaptive adjoint (dopri5 on (y, a, g_theta) per frame, mixed norm), as torchdiffeq */
  int32_t* sync;      /* adaptive adjoint with N > 32: as in the forward op */
  int32_t* nsteps;
} gode_odernn_bwd_op;
int gode_odernn_bwd(const gode_odernn_bwd_op* op, void* stream);
int64_t gode_odernn_bwd_work_size(int32_t N);
/* the adjoints of `count` (<= 8) independent solves (the video and the image path of one generator step) in one launch.
 * The group rule (gode_odernn_bwd_multi and gode_ode_bwd_multi, on every route a call can take): the ops of a call that share
 * a grads pointer form a group, reduced in array order -- the FIRST op of a group stores into grads or adds to it as its
 * accumulate flag says; every later op of the group adds, whatever its flag. */
int gode_odernn_bwd_multi(const gode_odernn_bwd_op* ops, int32_t count, void* stream);
/* Which route gode_odernn_fwd_multi / gode_odernn_bwd_multi would take with these ops: host arithmetic on the decisions the
 * launchers dispatch on, no pointer dereferenced but `ops` and `route`, no HIP call.  Returns what the launch would return
 * before launching anything (0, GODE_E_ARG for a refused op or count); on 0, route[count + 2] =
 *   route[k], k < count:  0 op k runs on the vector-ALU kernel in the call's shared launch; 1 on the MFMA kernels, with
 *                         launches of its own
 *   route[count]:         workgroups of the shared vector-ALU launch (0: there is none)
 *   route[count + 1]:     adjoint: 0 work rows added by latent_rows_kernel; 1 the launch's one workgroup writes grads itself;
 *                         2 the ops run one at a time in array order (a call with an MFMA op).  Forward: 0. */
int gode_odernn_fwd_route(const gode_odernn_fwd_op* ops, int32_t count, int32_t* route);
int gode_odernn_bwd_route(const gode_odernn_bwd_op* ops, int32_t count, int32_t* route);
#define GODE_ODERNN_NPARAM 2176

/* ---- Neural-SDE motion latent (models/mocogan_sde.py: sdeint_adjoint(SDEFunc, x, linspace(0, 1, T), method='euler',
 * dt=2.5e-2); Ito, diagonal noise) ---------------------------------------------------------------------------------
 * forward: x[1+S][N][16] = the host-drawn initial noise x0 followed by the standard-normal stack xi_0..xi_{S-1} ->
 * pre-net (as gode_ode_fwd; prenet==0: nn.Identity) -> S Euler-Maruyama steps
 *   y_{k+1} = y_k + dt[k] f(y_k) + g(y_k) * sqrt_dt[k] * xi_k,   f = Wf2 tanh(Wf1 y + bf1) + bf2,  g = Wg2 tanh(Wg1 y + bg1) + bg2
 * with the host schedule dt[S], sqrt_dt[S] (torchsde's fixed-step loop in fp32; the Brownian increment is
 * sqrt(dt_k) xi_k, a documented deviation from torchsde's BrownianInterval).  Output 0 is y_0; output j >= 1 is produced
 * after step emit_at[j] as emit_w0[j] y_k + emit_w1[j] y_{k+1} (torchsde's linear_interp).  z / content / sel_t / zcols as
 * in gode_ode_fwd.  states[N][S+1][16] (nullable in the forward) keeps every state for the backward. */
typedef struct gode_sde_params {
  const float* Wa; const float* ba; const float* Wb; const float* bb;       /* pre-net (NULL when prenet == 0) */
  const float* Wf1; const float* bf1; const float* Wf2; const float* bf2;   /* drift_fn: [16,16],[16],[16,16],[16] */
  const float* Wg1; const float* bg1; const float* Wg2; const float* bg2;   /* diffusion_fn: the same shapes */
} gode_sde_params;
typedef struct gode_sde_fwd_op {
  gode_sde_params p;
  const float* x; const float* content; const int32_t* sel_t;
  const float* dt; const float* sqrt_dt; const int32_t* emit_at; const float* emit_w0; const float* emit_w1;
  float* z; float* states;
  int32_t N, T, S, prenet, zcols, pad_;
} gode_sde_fwd_op;
int gode_sde_fwd(const gode_sde_fwd_op* op, void* stream);
/* backward: the exact gradient of the discrete forward above (not torchsde's continuous adjoint), the reverse sweep
 *   a_k = a_{k+1} + dt_k Jf(y_k)^T a_{k+1} + Jg(y_k)^T (a_{k+1} * dW_k)  + the interpolation weights' share of gz,
 * then the pre-net backward.  gz[rows][zcols] as in gode_ode_bwd (full or sel_t rows; 16 motion columns read).  Parameter
 * gradients are reduced in fixed order through work (>= gode_sde_bwd_work_size(N) floats) and written (accumulate != 0:
 * added) to grads, which points at the FIRST PRESENT tensor of gode_sde_params: 3216 floats with the pre-net, 1088
 * (drift + diffusion) without.  Nothing outside that span is touched. */
typedef struct gode_sde_bwd_op {
  gode_sde_params p;
  const float* x; const float* states; const int32_t* sel_t;
  const float* dt; const float* sqrt_dt; const int32_t* emit_at; const float* emit_w0; const float* emit_w1;
  const float* gz; float* work; float* grads;
  int32_t N, T, S, prenet, accumulate, zcols;
} gode_sde_bwd_op;
int gode_sde_bwd(const gode_sde_bwd_op* op, void* stream);
int64_t gode_sde_bwd_work_size(int32_t N);
#define GODE_SDE_NPARAM 3216

/* ---- Neural-CDE motion latent (models/mocogan_cde.py: torchcde.cdeint(X, f([0, x_0]), CDEFunc, t=arange(T)) on the
 * backward-difference Hermite cubic spline of the path [linspace(0, 1, T), x]; dopri5, rtol/atol from the caller) -----
 * forward, ONE launch: z0 = f([tt_0, x_0]) (Linear(2,64) -> LReLU -> Linear(64,16) -> LReLU), then dopri5 on
 *   dz/dt = tanh(W2 relu(W1 z + b1) + b2).view(16, 2) @ dX/dt(t)
 * with torchdiffeq's controller (_select_initial_step, safety 0.9, ifactor 10, dfactor 0.2, exponent -1/5), the RMS error
 * norm over ALL N*16 values of the call (workgroups exchange partial sums through `sync`, fixed order: bit-identical
 * decisions) and the 4th-order dense output at t = 0..T-1, written into z (content / sel_t / zcols as in gode_ode_fwd).
 * The clock and the step size are fp64, the state fp32.  x[N][T]: the noise channel's knots; tslope[T-1]: the time
 * channel's per-interval slopes (fp32 differences of linspace(0, 1, T)).  Recorded for the backward: states[N][S_cap+1][16]
 * (the state at the start of every accepted step, then the final one), sched[2][S_cap] (fp64: t_k, then h_k; one schedule
 * for the whole batch) and counts[2] = {accepted, trials}.  More than S_cap accepted steps, a trial limit or a step-size
 * underflow stop the solve cleanly: counts[0] = -(accepted) - 1, nothing is written past the buffers.
 * 2 <= T <= 16, 1 <= N <= GODE_CDE_MAX_N (all workgroups must be co-resident). */
typedef struct gode_cde_params {
  const float* Wa; const float* ba; const float* Wb; const float* bb;   /* f: Linear(2,64) [64,2],[64]; Linear(64,16) [16,64],[16] */
  const float* W1; const float* b1; const float* W2; const float* b2;   /* CDEFunc: linear1 [128,16],[128]; linear2 [32,128],[32] */
} gode_cde_params;
typedef struct gode_cde_fwd_op {
  gode_cde_params p;
  const float* x; const float* tslope; const float* content; const int32_t* sel_t;
  float* z; float* states; double* sched; int32_t* counts;
  int32_t* sync;    /* N > 16: >= gode_cde_sync_size(N) words (zeroed by the call); may be NULL for N <= 16 */
  int32_t N, T, S_cap, zcols;
  float rtol, atol;
} gode_cde_fwd_op;
int gode_cde_fwd(const gode_cde_fwd_op* op, void* stream);
int64_t gode_cde_sync_size(int32_t N);
int64_t gode_cde_state_size(int32_t N, int32_t S_cap);   /* floats of states */
/* backward: the exact gradient of the discrete forward above (step sizes held constant; not torchdiffeq's continuous
 * adjoint): for every accepted step in reverse, the 7 stages are recomputed from the stored state and back-propagated,
 * with the dense-output interpolant's share of gz and, at the end, the pre-net.  gz[rows][zcols] as in gode_ode_bwd.
 * The parameter sums are reduced in fixed order through work (>= gode_cde_bwd_work_size(N) floats) and written
 * (accumulate != 0: added) to grads[GODE_CDE_NPARAM] = Wa, ba, Wb, bb, W1, b1, W2, b2; nothing outside it is touched.
 * counts is the forward's (read on the device; a failed forward leaves grads untouched). */
typedef struct gode_cde_bwd_op {
  gode_cde_params p;
  const float* x; const float* tslope; const int32_t* sel_t;
  const float* states; const double* sched; const int32_t* counts;
  const float* gz; float* work; float* grads;
  int32_t N, T, S_cap, accumulate, zcols, pad_;
} gode_cde_bwd_op;
int gode_cde_bwd(const gode_cde_bwd_op* op, void* stream);
int64_t gode_cde_bwd_work_size(int32_t N);
#define GODE_CDE_NPARAM 7536
#define GODE_CDE_MAX_N 4096

/* ---- GRU motion latent (models/mocogan.py:217-229: MoCoGAN's VideoGenerator.sample_z_m) ---------------------------
 * h_0 ~ N(0,1); for t < T: h_{t+1} = GRUCell(e_t, h_t) (torch's definition, gate order r, z, n); latent row t = h_{t+1}.
 * noise[T+1][N][16] = h_0, e_0..e_{T-1} drawn on the host.  z / content / sel_t / zcols as in gode_ode_fwd (content NULL:
 * only the 16 motion columns of each row are written, zcols >= 16).  hs[N][T+1][16] (nullable) keeps every h_t for the
 * backward.  Trajectories are independent: any N >= 1, T >= 1. */
typedef struct gode_gru_params {
  const float* Wih; const float* Whh; const float* bih; const float* bhh;   /* GRUCell(16,16): [48,16]x2, [48]x2 */
} gode_gru_params;
typedef struct gode_gru_fwd_op {
  gode_gru_params p;
  const float* noise; const float* content; const int32_t* sel_t;
  float* z; float* hs;
  int32_t N, T, zcols, pad_;
} gode_gru_fwd_op;
int gode_gru_fwd(const gode_gru_fwd_op* op, void* stream);
/* `count` (<= 8) independent chains in ONE launch (one training iteration's prefetched latents; ops: HOST array) */
int gode_gru_fwd_multi(const gode_gru_fwd_op* ops, int32_t count, void* stream);
/* backward: backpropagation through time from gz[rows][zcols] (the decoder's input gradient, full or sel_t rows as in
 * gode_ode_bwd; 16 motion columns read), gates recomputed from hs and noise.  No gradient for the noise.  The parameter
 * sums are reduced in fixed order (trajectories within a workgroup, then workgroups in order through work, >=
 * gode_gru_bwd_work_size(N) floats, one buffer per op) and written (accumulate != 0: added) to
 * grads[GODE_GRU_NPARAM] = Wih, Whh, bih, bhh; nothing outside it is touched. */
typedef struct gode_gru_bwd_op {
  gode_gru_params p;
  const float* noise; const float* hs; const int32_t* sel_t; const float* gz;
  float* work; float* grads;
  int32_t N, T, accumulate, zcols;
} gode_gru_bwd_op;
int gode_gru_bwd(const gode_gru_bwd_op* op, void* stream);
int64_t gode_gru_bwd_work_size(int32_t N);
/* the BPTT of `count` (<= 8) chains (the video and the image path of one generator step) in one launch; ops sharing a
 * grads pointer are applied in array order, each op's rows reduced into its own partial first and stored / added under
 * its own accumulate flag: bit-identical to the same ops launched one by one */
int gode_gru_bwd_multi(const gode_gru_bwd_op* ops, int32_t count, void* stream);
#define GODE_GRU_NPARAM 1632

/* ---- loss and optimiser (mnist_moco_ode.py:86-89) ------------------------------------------------------------
 * BCE-with-logits, mean reduced, constant target: loss (+)= mean(max(x,0) - x*t + log1p(exp(-|x|))) and
 * g[i] = gscale*(sigmoid(x[i]) - t)/n.  loss is one device float; accumulate!=0 adds to it.  stride > 1: logit i and its
 * gradient sit at element i*stride of their arrays (column 0 of a [B][1+C] categorical head); 0 or 1: contiguous. */
typedef struct gode_bce_op {
  const float* logits; float* grad; float* loss; int64_t n; float target, gscale; int32_t accumulate, stride;
} gode_bce_op;
int gode_bce_logits(const gode_bce_op* op, void* stream);
/* ---- categorical MoCoGAN (models/mocogan.py:167-182,231-247) ----------------------------------------------------
 * One-hot columns of the latent rows: row r (trajectory r / rows_per; rows_per = T, or 1 when one row per trajectory
 * was selected) receives z[r*zcols + col0 + c] = (cls[trajectory] == c), c < C; col0 + C <= zcols.  Runs after the
 * latent solve of the same rows on the same stream.  labels_out (nullable): cls widened to int64[n_traj]. */
typedef struct gode_categ_op {
  const int32_t* cls; float* z; int64_t* labels_out; int32_t n_traj, rows_per, C, zcols, col0, pad_;
} gode_categ_op;
int gode_categ_onehot(const gode_categ_op* op, void* stream);
/* nn.CrossEntropyLoss(): loss (+)= mean over rows r < n_lab of -log_softmax(logits[r*ld .. r*ld+C))[labels[r]], summed
 * in a fixed order (no atomics).  grad (nullable) rows r < n_lab: gscale*(softmax - onehot)/n_lab at grad[r*gld + c];
 * rows n_lab <= r < B: zeros (n_lab == 0: only that, the loss is not touched).  labels are int64 on the device.
 * rows_per_label = P > 1: row r takes labels[r / P] (the P output positions of a video's patch head share its class);
 * 0 or 1: one label per row.  loss is one device float; accumulate != 0 adds to it. */
typedef struct gode_ce_op {
  const float* logits; const int64_t* labels; float* grad; float* loss;
  int32_t B, n_lab, C, ld, gld; float gscale; int32_t accumulate, rows_per_label;
} gode_ce_op;
int gode_ce_logits(const gode_ce_op* op, void* stream);
/* torch.optim.Adam with L2-coupled weight_decay on one tensor: g+=wd*p; m,v update; bias-corrected step. */
typedef struct gode_adam_op {
  float* p; const float* g; float* m; float* v; int64_t n;
  float lr, beta1, beta2, eps, weight_decay, gscale; int32_t step, pad_; /* step >= 1; gscale: 1/world for DP */
} gode_adam_op;
int gode_adam_l2(const gode_adam_op* op, void* stream);
/* the same update on `count` tensors in ONE launch; `table` is a DEVICE array of {p, g, m, v, n} records */
typedef struct gode_adam_tensor { float* p; const float* g; float* m; float* v; int64_t n; } gode_adam_tensor;
int gode_adam_multi(const gode_adam_tensor* table, int32_t count, int64_t max_n, float lr, float beta1, float beta2,
                    float eps, float weight_decay, float gscale, int32_t step, void* stream);

/* gode_adam_multi with the step-dependent coefficients read from device memory: coef[0] = lr / (1 - beta1^step),
 * coef[1] = sqrt(1 - beta2^step), both evaluated in double and rounded to float exactly as gode_adam_multi does.  A
 * launch captured in a HIP graph then stays valid across steps (the host rewrites coef before every replay). */
int gode_adam_multi_dev(const gode_adam_tensor* table, int32_t count, int64_t max_n, float beta1, float beta2, float eps,
                        float weight_decay, float gscale, const float* coef, void* stream);

/* ---- Wasserstein loss (torchgan.losses.WassersteinGeneratorLoss / WassersteinDiscriminatorLoss, reduction "mean" or
 * "sum", no clipping; mnist_moco_ode_wgan.py:97-98,138,159,174) ----------------------------------------------------
 *   real == NULL: loss (+)= sign * reduce(fake)            (generator: sign = -1)
 *   real != NULL: loss (+)= sign * reduce(fake - real)     (discriminator: sign = +1; the difference is taken per element)
 * reduce = mean (reduction 0) or sum (1), summed in double in one workgroup.  Gradients (each nullable):
 * grad_fake[i] = sign * (gscale / n) (sum: sign * gscale), grad_real[i] = -grad_fake[i].  A joint [real; fake] tensor of
 * 2n elements is passed as real = x, fake = x + n.  loss is one device float; accumulate != 0 adds to it. */
typedef struct gode_wgan_op {
  const float* fake; const float* real; float* grad_fake; float* grad_real; float* loss; int64_t n;
  float sign, gscale; int32_t reduction, accumulate;
} gode_wgan_op;
int gode_wgan_logits(const gode_wgan_op* op, void* stream);

/* ---- parameter noise (add_noise of mnist_moco_ode_noise.py / mnist_moco_ode_wgan.py: p += randn_like(p) * sigma after
 * every optimiser step) ------------------------------------------------------------------------------------------------
 * The stream: element e of a param group (e = noise_off + local index; noise_off of tensor k is the sum of
 * roundup4(numel) over the tensors before it) takes output lane e & 3 of Philox4x32-10 with key (seed_lo, seed_hi) and
 * counter (e >> 2 low word, step, stream, e >> 2 high word); each output word x becomes u = ((x >> 9) + 0.5) * 2^-23
 * (exact in fp32, never 0 or 1), Box-Muller maps (u0, u1) -> (r cos 2 pi u1, r sin 2 pi u1), r = sqrt(-2 ln u0), and (u2, u3)
 * alike.  Independent of the grid, the vector width and the arena layout.  The update is t = fp32(n * sigma),
 * p = fp32(p + t): two roundings, no FMA, as the reference's two torch ops.
 *
 * Adam + noise on `count` tensors in ONE launch: rows with g == NULL are noise-only (no Adam update; m and v are neither
 * read nor written and may be NULL).  The noise is added after the Adam update of the row. */
typedef struct gode_adam_noise_tensor { float* p; const float* g; float* m; float* v; int64_t n; int64_t noise_off; } gode_adam_noise_tensor;
int gode_adam_noise_multi(const gode_adam_noise_tensor* table, int32_t count, int64_t max_n, float lr, float beta1,
                          float beta2, float eps, float weight_decay, float gscale, int32_t step, uint64_t seed,
                          uint32_t noise_stream, uint32_t noise_step, float sigma, void* stream);
/* the same with coef[0], coef[1] as in gode_adam_multi_dev and the noise step read as the raw 32-bit word coef[2] (a graph
 * replay advances it with the Adam coefficients) */
int gode_adam_noise_multi_dev(const gode_adam_noise_tensor* table, int32_t count, int64_t max_n, float beta1, float beta2,
                              float eps, float weight_decay, float gscale, const float* coef, uint64_t seed,
                              uint32_t noise_stream, float sigma, void* stream);
/* the stream alone over elements [noise_off, noise_off + n): accumulate 0: out[i] = n_e * sigma; 1: out[i] = out[i] + n_e * sigma
 * (the rounding above); 2: out[i] receives the raw Philox word of element e (bit pattern, for tests) */
int gode_param_noise(float* out, int64_t n, uint64_t seed, uint32_t noise_stream, uint32_t noise_step, int64_t noise_off,
                     float sigma, int32_t accumulate, void* stream);

/* ---- discriminator instance noise (Noise(use_noise=True, sigma) of models/mocogan.py:20-29: x + sigma * N(0, 1) in front of
 * the discriminators' convolutions, train and eval mode alike) ----------------------------------------------------------
 * The stream: element e of a noised tensor is its flat channels-last index ([N][D][H][W][C], C fastest) plus e_off (the
 * shard's first global sample times D*H*W*C).  It takes lane e & 3 of Philox4x32-10 with key (seed lo, seed hi) and counter
 * (q low word, call, 0x80000000 | stream << 8 | layer, q high word), q = e >> 2; uniforms and Box-Muller as the parameter
 * noise above (the tag bit keeps the two families of streams disjoint).  The noisy value is fp32(a + fp32(sigma * z)), no
 * FMA, where a is bit for bit what the noise-free path feeds the convolution.
 * Two modes, one struct:
 *  - gather (N > 0, layer 0): x is the caller's [N][D][H][W][C] tensor read through element strides xs {N, D, H, W, C};
 *    out[N*D*H*W][C] receives the channels-last noisy copy (a = x);
 *  - apply (N == 0, layers >= 1): x is a raw output y[M][C] (C % 4 == 0); a = act(y * scale[c] + shift[c]) exactly as
 *    gode_bn_apply (scale == NULL: act(y)); M0 > 0: rows >= M0 are the second group of a paired pass -- scale + C /
 *    shift + C, call + 1, and e restarts at e_off.
 * call = (call_dev ? call_dev[0] : 0) + call: a launch captured in a graph reads its base call from device memory, which
 * the host rewrites before every replay.  stream < 2^23, layer < 256. */
typedef struct gode_dnoise_op {
  const float* x; float* out; const float* scale; const float* shift; const int32_t* call_dev;
  int64_t M; int32_t C, act;
  int64_t M0, e_off;
  int64_t xs[5];
  int32_t N, D, H, W;
  int64_t seed;
  int32_t stream, layer, call; float sigma;
} gode_dnoise_op;
int gode_dnoise(const gode_dnoise_op* op, void* stream);
/* the stream alone: out[i] = z of element e_off + i for i < n (raw != 0: the raw Philox word of that element, bit pattern) */
int gode_dnoise_normals(float* out, int64_t n, uint64_t seed, uint32_t noise_stream, uint32_t layer, uint32_t call,
                        int64_t e_off, int32_t raw, void* stream);

/* ---- generator latents drawn on the device (latent_rng = "device" of the generator classes) ----------
 * The latent stream: key (seed low word, seed high word); element e of a field takes output lane e & 3 of Philox4x32-10 with
 * counter (q low word, call, tag, q high word), q = e >> 2, tag = 0x60000000 | stream << 8 | field, stream < 2^21, field < 256.
 * The family is disjoint from the parameter-noise streams (small indices, far below 2^29), from dropout (0x40000000 | layer,
 * layer < 256: bit 29 clear) and from the instance noise (>= 0x80000000: bit 31 set) -- here bits 30 and 29 are set and
 * bit 31 is clear.  Words become normals as above: u = ((x >> 9) + 0.5) * 2^-23, lanes 0 / 1 = r0 cos 2 pi u1, r0 sin 2 pi u1
 * with r0 = sqrt(-2 ln u0), lanes 2 / 3 likewise from (u2, u3).  call = (call_dev ? call_dev[0] : 0) + call in 32-bit
 * wrap-around arithmetic, as in gode_dnoise_op.
 * Fields, g being the global index of a trajectory among those the call draws:
 *   0 content:   element g*50 + j, j < 50 -> normal, content[row][j];
 *   1 motion:    element g*XW + k, XW = outer*inner, k = o*inner + i -> normal, x[o][row][i] ((outer, inner): ODE (1, 16),
 *                GRU / ODE-RNN (T + 1, 16), SDE (1 + S, 16), CDE (1, T));
 *   2 class:     element g -> cls[row] = umulhi(word, C);
 *   3 selection: select mode only (n_all > 0, sample_images): n rows are picked from R = n_all*T by Floyd's algorithm -- for
 *                m = 0 .. n-1: j = R - n + m, t = umulhi(word of element m, j + 1), take t if it was not taken before, else
 *                j -- and sorted ascending, r_0 < ... < r_{n-1}; plan row b is trajectory g_b = traj0 + r_b / T at time
 *                sel_t[b] = r_b % T.  Two rows may share a trajectory and then carry the same content / motion / class.
 * Full mode (n_all == 0): g_b = traj0 + b.  The values of a trajectory are a pure function of (seed, stream, call, g): a
 * select-mode draw is bit for bit the chosen trajectories of the full draw of all n_all.
 * gode_latent_draw writes exactly x[outer][n][inner], content[n][50] (nullable), sel_t[n] (select mode) and cls[n] (C > 0,
 * nullable) -- the four sub-blocks of a sampling plan's input block -- in ONE launch, O(n) work (select mode: every workgroup
 * repeats the selection in LDS), plain stores, independent of the grid.
 * GODE_E_ARG: a null op or x; n, outer, inner or T below 1; C or n_all below 0; stream outside [0, 2^21); traj0 < 0; select
 * mode without sel_t.  GODE_E_SHAPE: n * (outer*inner + 52) >= 2^31; select mode with n > 4096, n > n_all*T or
 * n_all*T >= 2^31.  All are returned before any launch. */
typedef struct gode_latent_draw_op {
  float* x; float* content; int32_t* sel_t; int32_t* cls;
  const int32_t* call_dev;
  int64_t seed, traj0;
  int32_t n, outer, inner, T;
  int32_t n_all;
  int32_t C, stream, call;
} gode_latent_draw_op;
int gode_latent_draw(const gode_latent_draw_op* op, void* stream);

/* ---- differentiable augmentation in front of the discriminators (DiffAugment, Zhao et al., NeurIPS 2020)
 * A sample is one image [C][H][W] (D = 1) or one clip [C][D][H][W]; all its frames and channels share ONE parameter set.  The
 * parameters of global sample g = g0 + (position in the batch) come from Philox4x32-10 with key (seed low word, seed high
 * word) and counter (g low word, call, tag, g high word), tag = 0x20000000 | stream << 8 | field, stream < 2^21: bit 29 set,
 * bits 30 and 31 clear -- disjoint from the parameter noise (far below 2^29), dropout (0x40000000), the latents (0x60000000)
 * and the instance noise (0x80000000).  U(w) = ((w >> 9) + 0.5) * 2^-23.  All seven are drawn whatever the mask says:
 *   field 0: u_b = U(w0), u_s = U(w1), u_c = U(w2)   (w3 unused)
 *   field 1: tx = umulhi(w0, 2 Sx + 1) - Sx, ty = umulhi(w1, 2 Sy + 1) - Sy, cx = umulhi(w2, W + 1 - cw % 2),
 *            cy = umulhi(w3, H + 1 - ch % 2), with Sx = (W + 4) / 8, Sy = (H + 4) / 8, cw = (W + 1) / 2, ch = (H + 1) / 2
 * The components, in this order, selected by the bits of `mask`:
 *   1  brightness   x <- x + (u_b - 0.5)
 *   2  saturation   m = mean over the C channels at each (d, h, w); x <- (x - m) * (2 u_s) + m
 *   4  contrast     M = mean over all C*D*H*W elements of the sample; x <- (x - M) * (u_c + 0.5) + M
 *   8  translation  y[c][d][h][w] = x[c][d][h - ty][w - tx] where that source lies inside the map, else 0
 *   16 cutout       y = 0 for cy - ch/2 <= h < cy - ch/2 + ch and cx - cw/2 <= w < cx - cw/2 + cw (clipped to the map)
 * backward == 1: x is the cotangent of the forward's output and out receives the cotangent of its input -- zero under the
 * cutout, shifted back (g'[h][w] = g[h + ty][w + tx], 0 outside), g <- s g + (1 - s) mean_sample(g) with s = u_c + 0.5,
 * g <- s g + (1 - s) mean_channels(g) with s = 2 u_s; brightness is the identity.
 * x is read through the element strides xs {N, D, H, W, C} (any view, as gode_dnoise_op's gather mode); out is contiguous
 * channels-last [N][D][H][W][C].  call = (call_dev ? call_dev[0] : 0) + call, as in gode_dnoise_op.  Nothing but (seed,
 * stream, call, g) enters a sample's parameters: a batch drawn in parts with g0 set equals the whole.
 * The sample sums that contrast needs (forward: of x; backward: of the masked, shifted cotangent) are fp64, formed in a
 * fixed order without atomics -- a sample is cut into gode_diffaug_chunks(D, H, W) chunks of positions, one workgroup each,
 * whose partial sums go to work ([N][chunks] doubles) and are added in index order by the second launch -- so two runs give the
 * same bits.  work: >= gode_diffaug_work_size(N, D, H, W, mask) floats, 8-byte aligned; 0 for a mask without bit 4, which
 * launches once and never touches work (it may be NULL).  Masks within 8 | 16 move data only: out holds x's bits or +0.
 * GODE_E_ARG: a null op / x / out; any of N, C, D, H, W below 1; mask outside [1, 31]; backward not 0 or 1; stream outside
 * [0, 2^21); g0 < 0; bit 4 with a null or misaligned work.  GODE_E_SHAPE: D*H*W*C >= 2^31 or N * chunks >= 2^31.  All are
 * returned before any launch. */
typedef struct gode_diffaug_op {
  const float* x; float* out; float* work; const int32_t* call_dev;
  int64_t xs[5];
  int64_t seed, g0;
  int32_t N, C, D, H, W;
  int32_t mask, backward, stream, call, pad_;
} gode_diffaug_op;
int gode_diffaug(const gode_diffaug_op* op, void* stream);
int32_t gode_diffaug_chunks(int32_t D, int32_t H, int32_t W);
int64_t gode_diffaug_work_size(int32_t N, int32_t D, int32_t H, int32_t W, int32_t mask);
/* the parameters alone, on the host (no launch): ints[n][4] = tx, ty, cx, cy and unis[n][3] = u_b, u_s, u_c of samples
 * g0 .. g0 + n - 1.  GODE_E_ARG: a null pointer, n < 0, stream >= 2^21, g0 < 0, H or W below 1. */
int gode_diffaug_params(int32_t* ints, float* unis, int64_t n, uint64_t seed, uint32_t stream, uint32_t call, int64_t g0,
                        int32_t H, int32_t W);

/* ---- ODE-GAN training (GANODETrainer of stage2/ode_training.py: Euler / Heun / RK4 steps in parameter space) ---------
 * One stage update of a whole network in ONE launch, on `count` fp32 tensors described by a DEVICE table:
 *   p += c1*g[0] + c2*g[1] + c3*g[2] + c4*g[3] + cq*(qp - qm)
 * terms: bit k (k < 4) says that g[k] takes part, bit 4 that the q pair does; an absent term is neither read nor added.  The
 * sum is formed left to right with fused multiply-adds (the first present term is a plain product), then added to p: at
 * most 4 + 2 + 1 roundings.  A record in which a participating pointer is NULL is skipped: that tensor is not touched
 * (autograd returned None for it).  cq_dev != NULL: cq is multiplied by the device float cq_dev[0] (the reciprocal
 * difference step written by gode_axpy_multi), so no value has to travel to the host.
 * Tensors need 4-byte alignment only; those whose participating pointers share p's offset within 16 bytes move as 16-byte
 * vectors between a scalar head and tail, the others element by element.  chunk0 of record k is the sum of
 * gode_ode_step_chunks(p, n) over the records before it, and `chunks` the sum over all of them: the workgroups stride over
 * that concatenated space. */
#define GODE_STEP_QUADS 256
#define GODE_AXPY_MAX_BLOCKS 512
typedef struct gode_ode_step_tensor {
  float* p; const float* g[4]; const float* qp; const float* qm; int64_t n; int64_t chunk0;
} gode_ode_step_tensor;
int64_t gode_ode_step_chunks(const void* p, int64_t n);
int gode_ode_step(const gode_ode_step_tensor* table, int32_t count, int64_t chunks, int32_t terms, float c1, float c2,
                  float c3, float c4, float cq, const float* cq_dev, void* stream);
/* p = base + a*v on `count` tensors (one fused multiply-add; a == 0 or v == NULL copies base bit for bit; p may alias base),
 * a multiplied by the device float a_dev[0] when a_dev != NULL.  sums != NULL: sums[0] = sum v^2, sums[1] = sum base^2 over
 * all tensors, accumulated in double in a fixed order (two passes, no atomics: two runs give the same bits).  step != NULL
 * (needs sums): step[0] = fp32(h * (1 + sqrt(sums[1])) / sqrt(sums[0])), the central-difference step of DESIGN section 14,
 * and step[1] = fp32(1 / step[0]); both 0 when sums[0] == 0.  work: 2 * GODE_AXPY_MAX_BLOCKS doubles of device scratch.
 * chunk0 / chunks as above. */
typedef struct gode_axpy_tensor { float* p; const float* base; const float* v; int64_t n; int64_t chunk0; } gode_axpy_tensor;
int gode_axpy_multi(const gode_axpy_tensor* table, int32_t count, int64_t chunks, float a, const float* a_dev, double* sums,
                    float h, float* step, double* work, void* stream);

/* ---- stage 1: DVD-GAN generator residual block (stage1/GResBlock.py: SpectralNorm :10-64, ConditionalNorm :66-88,
 * GResBlock :90-167) -- the pieces around gode_igemm / gode_wgrad, which run the 3x3 and 1x1 convolutions on materialised
 * channels-last tensors.  2-D maps; strides are ELEMENT strides {N, H, W, C}, all zero = channels-last contiguous (so a tensor
 * whose genuine strides are all zero -- one element expanded -- must be materialised by the caller first).  Every C is accepted.  Reductions run in a fixed order without float atomics: two runs give the same bits. */

/* Per-channel partial sums of a strided tensor: stats[2][C][rows] (sum, then sum of squares; row r covers positions
 * [r*chunk, (r+1)*chunk) of the N*H*W positions, chunk = ceil(N*H*W / rows)) -- the layout gode_bn_finalize reads
 * (ncols = C).  rows >= 1 is the caller's choice (gode_chstats_rows: the default). */
typedef struct gode_chstats_op {
  const float* x; float* stats; int64_t xs[4]; int32_t N, H, W, C, rows, pad_;
} gode_chstats_op;
int gode_chstats(const gode_chstats_op* op, void* stream);
int gode_chstats_rows(int64_t positions);

/* ConditionalNorm's embedding: gb[n][2C] = condition[n][K] . W[2C][K]^T + b[2C]  ([gamma | beta] per sample). */
typedef struct gode_cbn_embed_op {
  const float* cond; const float* W; const float* b; float* gb; int32_t N, K, C2, pad_;
} gode_cbn_embed_op;
int gode_cbn_embed(const gode_cbn_embed_op* op, void* stream);
/* its backward from dgb[n][2C] (gode_cbn_bwd writes it): dW[2C][K] = dgb^T cond, db[2C] = column sums, dcond[n][K] =
 * dgb W (each nullable), every sum in index order. */
typedef struct gode_cbn_embed_bwd_op {
  const float* cond; const float* W; const float* dgb; float* dW; float* db; float* dcond; int32_t N, K, C2, pad_;
} gode_cbn_embed_bwd_op;
int gode_cbn_embed_bwd(const gode_cbn_embed_bwd_op* op, void* stream);

/* Conditional BatchNorm + activation + nearest upsample on the store:
 *   a[n][h*f+i][w*f+j][c] = act(gamma[n,c] * (v + bias[c] - mean[c]) * invstd[c] + beta[n,c]),  i, j < f,  f in {1, 2}
 * v = src[n,h,w,c] read through ss.  gb = [gamma | beta][N][2C] (gode_cbn_embed).  mean == NULL: no normalisation,
 * a = act(v + bias).  bias nullable.  (Train mode over a convolution output: its bias cancels against the batch mean, so the
 * caller passes the raw output, the raw mean and bias = NULL.)  out is channels-last [N][H*f][W*f][C]. */
typedef struct gode_cbn_apply_op {
  const float* src; const float* bias; const float* mean; const float* invstd; const float* gb; float* out;
  int64_t ss[4]; int32_t N, H, W, C, f, act;
} gode_cbn_apply_op;
int gode_cbn_apply(const gode_cbn_apply_op* op, void* stream);

/* Backward of the above from g_a[N][H*f][W*f][C] (channels-last): g_z = act'(a) * (sum of the f x f replicas of g_a), with a the
 * forward's output (ReLU: a > 0);  dgb[n][2C] = [sum_hw g_z * xhat | sum_hw g_z];  with g_xhat = gamma[n,c] * g_z
 *   g_v = invstd * (g_xhat - mean(g_xhat) - xhat * mean(g_xhat * xhat))        (eval_mode != 0: invstd * g_xhat)
 * the means over all N*H*W positions of a channel; mean == NULL (no normalisation): g_v = g_z.  g_out = g_v (+ gadd, a
 * channels-last [N][H][W][C] tensor: the skip path's input gradient), written through gos (the caller's x layout or
 * channels-last).  dbias (nullable, [C]): the gradient of `bias`, sum of g_v -- exactly 0 behind a train-mode normalisation.
 * work: >= gode_cbn_bwd_work_size floats, 8-byte aligned. */
typedef struct gode_cbn_bwd_op {
  const float* g_a; const float* a; const float* src; const float* bias; const float* mean; const float* invstd;
  const float* gb; const float* gadd; float* work; float* dgb; float* dbias; float* g_out;
  int64_t ss[4]; int64_t gos[4]; int32_t N, H, W, C, f, act, eval_mode, pad_;
} gode_cbn_bwd_op;
int gode_cbn_bwd(const gode_cbn_bwd_op* op, void* stream);
int64_t gode_cbn_bwd_work_size(int32_t N, int32_t H, int32_t W, int32_t C);

/* Block output: main[N][H*f][W*f][C] = conv1's raw output, sc[N][H][W][C] = the 1x1 skip convolution's raw output at the INPUT
 * resolution (a 1x1 convolution commutes with nearest upsampling), both channels-last:
 *   down == 1: y[n][p][q][c] = main[n][p][q][c] + b_main[c] + sc[n][p/f][q/f][c] + b_sc[c]
 *   down == 2 (f == 1): y = avg_pool2(main + b_main) + avg_pool2(sc + b_sc), [N][H/2][W/2][C]. */
typedef struct gode_gres_out_op {
  const float* main; const float* sc; const float* b_main; const float* b_sc; float* y; int32_t N, H, W, C, f, down;
} gode_gres_out_op;
int gode_gres_out(const gode_gres_out_op* op, void* stream);
/* its inverse from g_y[N][Ho][Wo][C] read through gys: db[C] = column sums of g_y (the gradient of BOTH biases);
 * g_sc[N][H][W][C] = the f x f sums of g_y (down == 2: 0.25 * g_y[p/2][q/2], zero on an odd last row / column; f == down == 1:
 * a copy); g_main (nullable, down == 1 only): the channels-last copy of g_y ([N][H*f][W*f][C]; down == 2: conv1's output
 * gradient IS g_sc).  work: >= gode_gres_out_bwd_work_size floats (needed only with db). */
typedef struct gode_gres_out_bwd_op {
  const float* g_y; float* g_sc; float* g_main; float* db; float* work; int64_t gys[4]; int32_t N, H, W, C, f, down;
} gode_gres_out_bwd_op;
int gode_gres_out_bwd(const gode_gres_out_bwd_op* op, void* stream);
int64_t gode_gres_out_bwd_work_size(int32_t N, int32_t H, int32_t W, int32_t C, int32_t f, int32_t down);

/* Spectral normalisation, one power iteration on wbar[h][w] (l2n(x) = x / (|x| + 1e-12)), launches in stream order:
 *   v <- l2n(wbar^T u);  u <- l2n(wbar v);  sigma = u . (wbar v);  wout = wbar / sigma  (a true division).
 * u[h], v[w] are updated in place, sigma is one device float.  work: >= h + w floats. */
typedef struct gode_sn_op {
  const float* wbar; float* u; float* v; float* wout; float* sigma; float* work; int32_t h, w;
} gode_sn_op;
int gode_sn_fwd(const gode_sn_op* op, void* stream);
/* dwbar = G / sigma - (<G, wbar> / sigma^2) u v^T  (u, v constants), <G, wbar> reduced in double in a fixed order.
 * work: >= 2 * GODE_SN_BWD_BLOCKS floats, 8-byte aligned. */
#define GODE_SN_BWD_BLOCKS 64
typedef struct gode_sn_bwd_op {
  const float* G; const float* wbar; const float* u; const float* v; const float* sigma; float* dwbar; float* work;
  int32_t h, w;
} gode_sn_bwd_op;
int gode_sn_bwd(const gode_sn_bwd_op* op, void* stream);

/* ---- stage 2: the fully-connected MNIST GAN (stage2/test_ODE_training_with_MNIST_GAN.ipynb: Generator 100-256-512-1024-784
 * with LeakyReLU(0.2) / tanh, Discriminator 784-1024-512-256-1 with LeakyReLU(0.2) + F.dropout(x, 0.3) / sigmoid, nn.BCELoss) --
 * the passes around the products, which are gode_igemm (FPROP / DGRAD of the geometry {N = M, Ci, Co, everything else 1}) and
 * gode_wgrad on row-major blocks [M][C].  M * C < 2^31, any C >= 1 (16-byte vectors when C % 4 == 0 and the pointers allow).
 *
 * The dropout stream: element e = m*C + c of a layer's [M][C] block takes output lane e & 3 of Philox4x32-10 with key
 * (key low word, key high word) and counter (q low word, 0, 0x40000000 | layer, q high word), q = e >> 2; the word x becomes
 * u = ((x >> 9) + 0.5) * 2^-23 as for the noise streams above, and the element is KEPT iff u >= p, compared in fp32; kept values
 * are multiplied by fp32(1 / (1 - p)).  layer < 256.  The stream word has bit 31 clear (the instance noise sets it) and bit 30
 * set (a parameter-noise stream is a small index), so the three families never share a counter; independent of the grid and of
 * the vector width.  No mask is stored: the backward recomputes the bits.
 *
 *   out[m][c] = drop(act(y[m][c] + b[c]))     act: GODE_ACT_NONE / _LRELU / _TANH / _SIGMOID;  b nullable;  p == 0: no dropout;
 *                                             out may alias y. */
typedef struct gode_fc_act_op {
  const float* y; const float* b; float* out; int64_t M; int32_t C, act;
  int64_t key; int32_t layer; float p;
} gode_fc_act_op;
int gode_fc_act(const gode_fc_act_op* op, void* stream);
/* its backward from g_out[M][C] and the forward's out[M][C]:  g_y = g_out * keep / (1 - p) * act', with act' taken from the
 * activation's output a (= out, or out * (1 - p) behind a dropout): a > 0 ? 1 : 0.2 for LeakyReLU, 1 - a^2 for tanh,
 * a (1 - a) for sigmoid.  g_y may alias g_out.  db (nullable, [C]): the column sums of g_y, stored or (accumulate != 0) added;
 * they are reduced in a fixed order without atomics -- row lanes, then chunks of 128 rows through work (>=
 * gode_fc_act_bwd_work_size floats; 0 for M <= 128: work may be NULL) -- so two runs give the same bits. */
typedef struct gode_fc_act_bwd_op {
  const float* g_out; const float* out; float* g_y; float* db; float* work; int64_t M; int32_t C, act;
  int64_t key; int32_t layer; float p; int32_t accumulate, pad_;
} gode_fc_act_bwd_op;
int gode_fc_act_bwd(const gode_fc_act_bwd_op* op, void* stream);
int64_t gode_fc_act_bwd_work_size(int64_t M, int32_t C);
/* the keep values alone: out[e] = 1 or 0 for elements e < n of (key, layer, p) */
int gode_dropout_mask(float* out, int64_t n, uint64_t key, uint32_t layer, float p, void* stream);
/* nn.BCELoss() on probabilities p[n] against targets t[n], mean reduction, torch's clamps:
 *   loss (+)= mean(-(t * max(log p, -100) + (1 - t) * max(log(1 - p), -100)))
 *   grad[i] = gscale * (p - t) / max(p (1 - p), 1e-12) / n          (grad nullable)
 * summed in double in one workgroup in a fixed order.  loss is one device float; accumulate != 0 adds to it. */
typedef struct gode_bce_prob_op {
  const float* p; const float* t; float* grad; float* loss; int64_t n; float gscale; int32_t accumulate;
} gode_bce_prob_op;
int gode_bce_prob(const gode_bce_prob_op* op, void* stream);

/* ---- stage 2: the CIFAR DCGAN (stage2/test_ODE_training_with_cifar_GAN.ipynb) runs on the convolution stack above with
 * GODE_ACT_LRELU01; its criterion is nn.BCEWithLogitsLoss() against a target TENSOR: gode_bce_logits with target[n] in place of
 * the constant --
 *   loss (+)= mean(max(x,0) - x*t[i] + log1p(exp(-|x|))),   g[i] = gscale*(sigmoid(x[i]) - t[i])/n          (grad nullable)
 * the same device code, so a tensor that holds one value gives gode_bce_logits' loss and gradient bit for bit.  Summed in double
 * by one workgroup in a fixed order (no atomics: two runs give the same bits).  loss is one device float; accumulate != 0 adds. */
typedef struct gode_bce_t_op {
  const float* logits; const float* target; float* grad; float* loss; int64_t n; float gscale; int32_t accumulate;
} gode_bce_t_op;
int gode_bce_logits_t(const gode_bce_t_op* op, void* stream);

/* ---- device-resident UCF-101 feed (dataset/ucf101new.py:73-98,162-180: Resize((64, 85), BICUBIC) on uint8 frames, crop of
 * columns 10..73, (x - 128) / 128) -- DESIGN section 21 -------------------------------------------------------------------
 * Separable resize of uint8 frames through two tap tables (bicubic_taps of gan-ode_amd/data.py: the weights of
 * torch.nn.functional.interpolate(mode="bicubic", align_corners=False, antialias=...) evaluated in double and rounded once to
 * fp32; the horizontal table lists the KEPT output columns only, so the crop costs nothing).  Output row i reads input rows
 * [y_first[i], y_first[i] + y_count[i]) with weights y_w[i*ky ..], output column j reads input columns [x_first[j], x_first[j] +
 * x_count[j]) with weights x_w[j*kx ..]:
 *   v = sum_y wy * (sum_x wx * in)      the horizontal sum first, taps ascending, each an fp32 fused-multiply-add chain from 0
 *   dst     = uint8(round_half_even(clamp(v, 0, 255)))       (torchvision's order for uint8 tensors: clamp, round, cast)
 *   dst_f32 = v
 * src: uint8 read through ELEMENT strides ss {frame, row, column, channel} -- the decoder's [F][Hin][Win][C] and the reference's
 * permuted [F][C][Hin][Win] both go in without a copy.  dst, dst_f32: [F][out_h][out_w][C] contiguous, each nullable, not both.
 * C is 1 or 3; 1 <= ky, kx <= GODE_RESIZE_MAX_TAPS (antialiased downscales up to 8x).  The tables are DEVICE memory, which the
 * entry point does not read; the kernel checks every table row it uses instead: a count outside [1, k], or a range that leaves
 * the input, turns the outputs that row feeds into NaN (dst_f32) / 0 (dst), and nothing outside src is read.  (The Python side
 * builds the tables and refuses such rows before any upload.)  GODE_E_SHAPE: ky or kx above the maximum, ky rows of fp32
 * partial sums (ky * out_w * C floats) beyond the kernel's 48 KiB of LDS, or F * bands of 8 rows >= 2^31. */
#define GODE_RESIZE_MAX_TAPS 32
typedef struct gode_resize_u8_op {
  const uint8_t* src; uint8_t* dst; float* dst_f32;
  const int32_t* y_first; const int32_t* y_count; const float* y_w;
  const int32_t* x_first; const int32_t* x_count; const float* x_w;
  int64_t ss[4];
  int32_t F, Hin, Win, C, out_h, out_w, ky, kx;
} gode_resize_u8_op;
int gode_resize_u8(const gode_resize_u8_op* op, void* stream);
/* Window gather and normalise: out[b][t][e] = (frames[first[b] + t][e] - sub) * inv for t < T, e < frame_elems -- with sub = 128,
 * inv = 1/128 exactly the reference's (x - 128.0) / 128.0 (the difference is an integer, the divisor a power of two).  frames:
 * uint8 [n_frames][frame_elems]; first: int64 [B] on the DEVICE, the first stored frame of every clip (T == 1: image batches);
 * out: fp32 [B][T][frame_elems] contiguous.  A clip whose range [first, first + T) leaves [0, n_frames) is filled with NaN and
 * nothing outside the buffer is read (the idiom of gode_ce_logits' bad label).  frame_elems % 16 == 0 with frames and out on
 * 16-byte boundaries: 16-byte loads and stores; otherwise element by element.  Same values either way. */
typedef struct gode_clip_gather_op {
  const uint8_t* frames; const int64_t* first; float* out;
  int64_t n_frames, frame_elems; int32_t B, T; float sub, inv;
} gode_clip_gather_op;
int gode_clip_gather(const gode_clip_gather_op* op, void* stream);

/* ---- Rotated-MNIST clips built on the device (utils/images.py:101-173, rotate_data: every digit through K angles with
 * scipy.ndimage.rotate(image, angle, reshape=False, cval=-0.5), every frame normalised min-max) -- DESIGN section 25 ---------
 * images: [n][H][W], uint8 (in_u8 = 1) or fp32 (in_u8 = 0), one channel.  On load a = v * in_scale + in_shift (one fused
 * multiply-add), where for uint8 v is first taken through the reference's own fp32 expression (byte - 127.5f) / 255.0f
 * (utils/images.py:71); in_scale = 1, in_shift = 0 changes no value.  cs: fp32 [n][K][2] = (cos, sin) of every frame's angle,
 * evaluated in double on the host and rounded once.  Per digit:
 *   1. cubic B-spline prefilter along axis 0, then axis 1: gain 6, pole z = sqrt(3) - 2, the causal pass initialised for a mirror
 *      boundary (period 2n - 2), the anticausal one from z / (z^2 - 1) * (c[n-1] + z c[n-2])   (scipy.ndimage.spline_filter,
 *      order 3, mode 'mirror');
 *   2. output pixel (y, x) of frame k reads p_y = cy + cos (y - cy) + sin (x - cx), p_x = cx - sin (y - cy) + cos (x - cx), with
 *      cy = (H - 1) / 2, cx = (W - 1) / 2, each two fp32 fused multiply-adds;
 *   3. p_y outside [0, H - 1] or p_x outside [0, W - 1] (or not a number): cval.  Otherwise f = floor(p), t = p - f, weights
 *      ((1-t)^3, 3t^3 - 6t^2 + 4, -3t^3 + 3t^2 + 3t + 1, t^3) / 6 per axis on the coefficients f - 1 .. f + 2, indices outside
 *      [0, n - 1] mirrored (i -> -i, i -> 2(n - 1) - i);
 *   4. out = x / (max - min) - min / (max - min) over the frame's H * W values, both IEEE divisions (utils/images.py:166-167:
 *      the quotient first, then minus ITS minimum).  A frame of equal values divides by zero and comes out non-finite, as in the
 *      reference; it is not special-cased.
 * out: fp32 [n][K][H][W], the normalised frames; raw: the same shape, the rotated frames before step 4; each nullable, not both;
 * the values of either do not depend on the presence of the other.  Element offsets are 64-bit.
 * GODE_E_ARG: a null op / images / cs, both outputs null, n < 1, K < 1, in_u8 not 0 or 1.  GODE_E_SHAPE: H or W outside
 * [4, 64].  Both are returned before any launch. */
typedef struct gode_rot_clips_op {
  const void* images; const float* cs; float* out; float* raw;
  int32_t n, K, H, W, in_u8; float in_scale, in_shift, cval;
} gode_rot_clips_op;
int gode_rot_clips(const gode_rot_clips_op* op, void* stream);

/* ---- sample grid of a batch of videos, as 8-bit frames (the drivers' genSamples, mnist_moco_ode.py:31-48) -- DESIGN section 26
 * src: fp32 videos (b, c, t, h, w) read in place through the element strides xs[5] (any view: sample_videos' channels-last
 * permuted view, a contiguous [B, C, T, H, W] tensor, an expanded one).  Video b fills tile (b / cols, b % cols) of a grid of
 * rows x cols tiles; C == 1 is broadcast to the three colour channels; a tile with b >= B holds source value 0 (the reference's
 * zero-initialised `out`).  Per value, in float64 and operation for operation as NumPy evaluates the reference's expression:
 *   mode 0: v = ((double)x + 1.0) / 2.0 * 255.0     (generator output, UCF reals: [-1, 1])
 *   mode 1: v = (double)x * 255.0                   (Rot-MNIST reals: [0, 1])
 * then v < 0 -> 0, v > 255 -> 255 and truncation toward zero to uint8 (the writer's clip(0, 255).astype(uint8)).  A NaN input
 * is outside the contract: NumPy's own cast of NaN is undefined, and what comes out here is unspecified (nothing faults).
 * rgb: uint8 [T][rows*H][cols*W][3], the frames.  idx: uint8 [T][rows*H][cols*W], palette indices: C == 1 the gray value itself
 * (a 256-gray palette); C == 3 the cell of a fixed 6 x 7 x 6 colour cube, in integers: with L = (6, 7, 6),
 * q_c = (v_c * (L_c - 1) + 127) / 255 and idx = (q_r * 7 + q_g) * 6 + q_b, whose palette entry is level
 * (k * 255 + (L_c - 1) / 2) / (L_c - 1) per channel (entries 252..255 unused, black).  No dithering.  Each output is nullable,
 * not both; neither depends on the presence of the other.
 * Launch: four pixels per thread with 16-byte loads and dword stores when W % 4 == 0, the source has unit stride along w
 * (C == 1) or is channels-last (C == 3: xs[1] == 1, xs[4] == 3), src is 16-byte aligned with xs[0], xs[2], xs[3] multiples of
 * 4, and the outputs are 4-byte aligned; one pixel per thread through the strides otherwise.  The values are the same.
 * gode_video_grid_launch_kind returns what gode_video_grid would return before launching anything and, on 0, kind[0] = 1 for
 * the four-pixel kernel, 0 for the strided one.
 * GODE_E_ARG: a null op or src; both outputs null; C not 1 or 3; mode not 0 or 1; B < 1; B > rows * cols.  GODE_E_SHAPE: any
 * of T, H, W, rows, cols below 1; rows * H or cols * W above 16384.  (rows or cols below 1 is GODE_E_SHAPE, whatever B.)  All
 * are returned before any launch. */
typedef struct gode_video_grid_op {
  const float* src; int64_t xs[5];
  uint8_t* rgb;
  uint8_t* idx;
  int32_t B, C, T, H, W, rows, cols, mode;
} gode_video_grid_op;
int gode_video_grid(const gode_video_grid_op* op, void* stream);
int gode_video_grid_launch_kind(const gode_video_grid_op* op, int32_t* kind);

/* ---- GIF variable-width LZW on the host (csrc/gif_lzw.h; gan_ode_amd.video_io.write_gif frames the result) -----------------
 * gode_gif_lzw encodes n palette indices (each below 1 << min_code_size, 2 <= min_code_size <= 8) into `out`: a clear code
 * first, codes from min_code_size + 1 to 12 bits wide, a clear code when the table reaches 4096 entries, the
 * end-of-information code last, bits packed LSB first.  Returns the byte count; GODE_E_ARG for a null pointer, n < 0, a
 * min_code_size outside [2, 8] or an index the code size cannot hold; GODE_E_SHAPE when `cap` bytes do not hold the stream.
 * Nothing is ever written at or behind out + cap.  gode_gif_lzw_bound(n): a cap that always suffices (n < 0: GODE_E_ARG). */
int64_t gode_gif_lzw_bound(int64_t n);
int64_t gode_gif_lzw(const uint8_t* idx, int64_t n, int32_t min_code_size, uint8_t* out, int64_t cap);

/* out[i] = a[i]*alpha (+ out[i] if accumulate); small utility for gradient bucket handling */
int gode_scale(float* out, const float* a, int64_t n, float alpha, int accumulate, void* stream);

/* ---- program runner: executes n ops back to back on the stream (one host call per network pass) -------------
 * The op kinds, one row each: X(NAME, GODE_OP_NAME's value, op struct, its `int fn(const op*, void* stream)`).  The enum
 * below, gode_sizeof and gode_run's dispatch expand from this table, and scripts/gen_binding_stub.py reads it. */
#define GODE_OPS(X) \
  X(IGEMM,          1, gode_igemm_op,         gode_igemm)         \
  X(WGRAD,          2, gode_wgrad_op,         gode_wgrad)         \
  X(BN_FINALIZE,    3, gode_bn_finalize_op,   gode_bn_finalize)   \
  X(BN_BWD,         4, gode_bn_bwd_op,        gode_bn_bwd)        \
  X(ODE_FWD,        5, gode_ode_fwd_op,       gode_ode_fwd)       \
  X(ODE_BWD,        6, gode_ode_bwd_op,       gode_ode_bwd)       \
  X(BCE,            7, gode_bce_op,           gode_bce_logits)    \
  X(ADAM,           8, gode_adam_op,          gode_adam_l2)       \
  X(ODERNN_FWD,    10, gode_odernn_fwd_op,    gode_odernn_fwd)    \
  X(ODERNN_BWD,    11, gode_odernn_bwd_op,    gode_odernn_bwd)    \
  X(BN_APPLY,      12, gode_bn_apply_op,      gode_bn_apply)      \
  X(COL2IM,        13, gode_col2im_op,        gode_col2im)        \
  X(SDE_FWD,       14, gode_sde_fwd_op,       gode_sde_fwd)       \
  X(SDE_BWD,       15, gode_sde_bwd_op,       gode_sde_bwd)       \
  X(CDE_FWD,       16, gode_cde_fwd_op,       gode_cde_fwd)       \
  X(CDE_BWD,       17, gode_cde_bwd_op,       gode_cde_bwd)       \
  X(WGAN,          18, gode_wgan_op,          gode_wgan_logits)   \
  X(GRU_FWD,       19, gode_gru_fwd_op,       gode_gru_fwd)       \
  X(GRU_BWD,       20, gode_gru_bwd_op,       gode_gru_bwd)       \
  X(DNOISE,        21, gode_dnoise_op,        gode_dnoise)        \
  X(CATEG,         22, gode_categ_op,         gode_categ_onehot)  \
  X(CE,            23, gode_ce_op,            gode_ce_logits)     \
  X(CHSTATS,       24, gode_chstats_op,       gode_chstats)       \
  X(CBN_EMBED,     25, gode_cbn_embed_op,     gode_cbn_embed)     \
  X(CBN_EMBED_BWD, 26, gode_cbn_embed_bwd_op, gode_cbn_embed_bwd) \
  X(CBN_APPLY,     27, gode_cbn_apply_op,     gode_cbn_apply)     \
  X(CBN_BWD,       28, gode_cbn_bwd_op,       gode_cbn_bwd)       \
  X(GRES_OUT,      29, gode_gres_out_op,      gode_gres_out)      \
  X(GRES_OUT_BWD,  30, gode_gres_out_bwd_op,  gode_gres_out_bwd)  \
  X(SN_FWD,        31, gode_sn_op,            gode_sn_fwd)        \
  X(SN_BWD,        32, gode_sn_bwd_op,        gode_sn_bwd)        \
  X(FC_ACT,        33, gode_fc_act_op,        gode_fc_act)        \
  X(FC_ACT_BWD,    34, gode_fc_act_bwd_op,    gode_fc_act_bwd)    \
  X(BCE_PROB,      35, gode_bce_prob_op,      gode_bce_prob)      \
  X(BCE_T,         36, gode_bce_t_op,         gode_bce_logits_t)  \
  X(RESIZE_U8,     37, gode_resize_u8_op,     gode_resize_u8)     \
  X(CLIP_GATHER,   38, gode_clip_gather_op,   gode_clip_gather)   \
  X(BN_RUNNING,    39, gode_bn_running_op,    gode_bn_running)    \
  X(ROT_CLIPS,     40, gode_rot_clips_op,     gode_rot_clips)     \
  X(VIDEO_GRID,    41, gode_video_grid_op,    gode_video_grid)    \
  X(LATENT_DRAW,   42, gode_latent_draw_op,   gode_latent_draw)   \
  X(DIFFAUG,       43, gode_diffaug_op,       gode_diffaug)
/* GODE_OP_PACK stays outside the table: it has no (op*, stream) entry point, gode_run sends every run of consecutive pack
 * ops out as batched launches instead. */
#define GODE_ENUM_ROW_(name, value, op_t, fn) GODE_OP_##name = value,
enum { GODE_OPS(GODE_ENUM_ROW_) GODE_OP_PACK = 9 };
#undef GODE_ENUM_ROW_
typedef struct gode_pack_op {
  gode_conv_geom g; int32_t dir /* may carry GODE_PACK_BORDER */, co_canon; const float* w; float* wpack; const int32_t* co_perm;
} gode_pack_op;
int gode_run(const int32_t* kinds, const void* const* ops, int32_t n, void* stream);

/* ---- two-lane runner: the front of a program on a side stream --------------------------------------------------
 * A program whose first n_front ops depend on nothing the PREVIOUS program on `stream` computed (a sampling call's noise
 * upload, latent solve and first GEMM) can run them under that program's tail.  A lanes object -- the one piece of state
 * the library owns: a non-blocking side stream and three events without timing -- carries the ordering from call to call:
 *   ops [0, n_front) go to the side stream, which then records ev_front; `stream` waits for ev_front and runs ops
 *   [n_front, n); behind op `release_after` (the last op on `stream` that touches a buffer the side lane writes) `stream`
 *   records ev_release.
 *   mode GODE_LANES_OVERLAP: the side lane first waits for the ev_release of the previous call on this object, and for
 *   nothing else -- the caller vouches that nothing but that call's ops [n_front, release_after] uses what the front
 *   writes, and that nothing queued since then writes what the front reads.
 *   mode GODE_LANES_ORDERED: the side lane first waits for an event recorded on `stream` at entry, i.e. for everything
 *   queued so far.  The first call on an object, and the call after one that failed, is ORDERED whatever `mode` says.
 * Runs of consecutive pack ops are batched and error codes carry the op index as in the one-stream runner.  Argument errors
 * (a null object, n_front > n, release_after outside [n_front, n), an unknown mode) return GODE_E_ARG before any HIP call.
 * A `stream` that is being captured takes all n ops itself, in order: a capture never forks.
 * The stream handle lets the caller put its own work (the H2D copy of the front's input) on the side lane ahead of a call.
 * Destroying the object drains the side stream first. */
typedef struct gode_lanes gode_lanes;
enum { GODE_LANES_ORDERED = 0, GODE_LANES_OVERLAP = 1 };
int gode_lanes_create(gode_lanes** out);
int gode_lanes_destroy(gode_lanes* lanes);
void* gode_lanes_stream(gode_lanes* lanes);
int gode_run_lanes(gode_lanes* lanes, const int32_t* kinds, const void* const* ops, int32_t n, int32_t n_front,
                   int32_t release_after, int32_t mode, void* stream);
/* Pair mode: two whole programs in flight on two lanes objects used in turn.  Ops [0, n - n_tail) run on `lanes`' own stream,
 * which then records its done event; `stream` waits for that event and runs the last n_tail ops (>= 1: the program's
 * gode_bn_running, the one op that touches state two programs share).  At entry `stream` records `lanes`' entry event.
 *   mode GODE_LANES_OVERLAP: the lane first waits for the entry event of `peer` -- the object the PREVIOUS call ran on, so
 *   for everything queued on `stream` before that call -- and for nothing else: the previous call's program keeps running
 *   next to this one.  The caller vouches that the two programs share no buffer they write, and that nothing queued on
 *   `stream` since the previous call's entry writes what this program reads.
 *   mode GODE_LANES_ORDERED, a null `peer`, or a `peer` whose entry event holds no record: the lane waits for this call's own
 *   entry event, i.e. for everything queued on `stream` so far.
 * Whatever is queued on `stream` behind the call is behind the whole program.  A `stream` that is being captured takes all n
 * ops itself, in order.  Argument errors (a null object, peer == lanes, n_tail outside [1, n), an unknown mode) return
 * GODE_E_ARG before any HIP call; error codes carry the op index as in gode_run. */
int gode_run_pair(gode_lanes* lanes, gode_lanes* peer, const int32_t* kinds, const void* const* ops, int32_t n,
                  int32_t n_tail, int32_t mode, void* stream);

int gode_version(void);
/* size of every op struct as compiled, so the ctypes mirror can assert it matches (index = GODE_OP_*; -1: the
 * gode_adam_noise_tensor table record) */
int gode_sizeof(int kind);

#ifdef __cplusplus
}
#endif
#endif
