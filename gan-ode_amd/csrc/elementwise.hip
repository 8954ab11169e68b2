// elementwise.hip -- the HBM-bound companions of the GEMM kernels: BatchNorm statistics finalisation and backward,
// BCE-with-logits, Adam(L2).  All reductions are fixed-order (partials -> one reducer), so results are
// run-to-run reproducible.  Reference semantics: nn.BatchNorm2d/3d train mode (models/mocogan.py:76-85,143-156,
// 202-212), nn.BCEWithLogitsLoss (mnist_moco_ode.py:89), torch.optim.Adam(weight_decay) (mnist_moco_ode.py:86-88).
#include "common.h"
#include "philox.h"
#include "col2im_plan.h"

// ---------------------------------------------------------------------------------------------------------------
// BatchNorm finalize
// The momentum update of the running statistics with its roundings pinned: under -ffp-contract=fast the compiler is free to
// fuse `(1 - m) * run + m * batch` either way, and it chose differently for the two tensors (the mean: two rounded products
// and an add; the variance: one rounded product and a fused multiply-add).  These helpers switch contraction OFF and state
// the one fused operation explicitly, so that choice no longer rests with the compiler.  gode_bn_running applies the same
// update from a deferred finalize's slots and must give the same bits, so both kernels call these.
__device__ __forceinline__ float bn_running_mean_update(float run, float momentum, float batch_mean) {
#pragma clang fp contract(off)
  const float keep = (1.f - momentum) * run;
  const float add = momentum * batch_mean;
  return add + keep;
}
__device__ __forceinline__ float bn_running_var_update(float run, float momentum, float unbiased) {
#pragma clang fp contract(off)
  const float keep = (1.f - momentum) * run;
  return __builtin_fmaf(momentum, unbiased, keep);
}

__global__ void __launch_bounds__(256) bn_finalize_kernel(const gode_bn_finalize_op a) {
  const int c = blockIdx.x, tid = threadIdx.x;
  __shared__ double red[2][256];
  if (a.training) {
    // stats[which][column][row] (column = rep*C + c): consecutive threads read consecutive rows of one column.
    // groups == 2: two BatchNorm batches in one launch.  Their partial rows are described by up to 8 segments
    // (begin, split, end): rows [begin, split) of a segment belong to group 0, [split, end) to group 1 -- one segment with
    // begin = 0, split = rows0, end = rows for a grouped FPROP pass (gode_igemm groups == 2), one per stride phase for a
    // transposed-convolution stack whose rows are [first batch; second batch] (gode_igemm_stats_segments).  The groups are
    // finalised one after the other in `order` (0: group 0 first), so the running statistics see the two momentum updates
    // in the order of the reference's two forward calls.
    const int reps = a.ncols / a.C;
    const int ngroups = a.groups == 2 ? 2 : 1;
    for (int gi = 0; gi < ngroups; ++gi) {
      const int grp = ngroups == 2 ? (a.order ? 1 - gi : gi) : 0;
      double s1 = 0.0, s2 = 0.0;
      const int nseg = (ngroups == 2 && !a.stats1) ? (a.nseg > 0 ? a.nseg : 1) : 1;
      for (int sg = 0; sg < nseg; ++sg) {
        int r_lo, r_hi;
        if (ngroups == 1 || a.stats1) { r_lo = 0; r_hi = (grp == 1 && a.stats1) ? a.rows1 : a.rows; }
        else if (a.nseg > 0) { r_lo = grp == 0 ? a.seg[3 * sg] : a.seg[3 * sg + 1]; r_hi = grp == 0 ? a.seg[3 * sg + 1] : a.seg[3 * sg + 2]; }
        else { r_lo = grp == 0 ? 0 : a.rows0; r_hi = grp == 0 ? a.rows0 : a.rows; }
        // (stats1: the second group's partial sums are an array of their own, written by a launch of its own)
        const float* st = (grp == 1 && a.stats1) ? a.stats1 : a.stats;
        const int stride = (grp == 1 && a.stats1) ? a.rows1 : a.rows;
        const int nr = r_hi - r_lo;
        const int64_t items = (int64_t)nr * reps;
        for (int64_t i = tid; i < items; i += 256) {
          const int rep = (int)(i / nr); const int r = r_lo + (int)(i - (int64_t)rep * nr);
          const int64_t o = (int64_t)(rep * a.C + c) * stride + r;
          s1 += (double)st[o];
          s2 += (double)st[(int64_t)a.ncols * stride + o];
        }
      }
      __syncthreads();
      red[0][tid] = s1; red[1][tid] = s2;
      __syncthreads();
      for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) { red[0][tid] += red[0][tid + s]; red[1][tid] += red[1][tid + s]; }
        __syncthreads();
      }
      if (tid == 0) {
        const double n = (double)((grp == 1 && a.count1 > 0) ? a.count1 : a.count);
        const double mean = red[0][0] / n;
        double var = red[1][0] / n - mean * mean;
        if (var < 0.0) var = 0.0;
        const float invstd = (float)(1.0 / sqrt(var + (double)a.eps));
        const float g = a.gamma ? a.gamma[c] : 1.f, b = a.beta ? a.beta[c] : 0.f;
        const float sc = g * invstd;
        const int o = grp * a.C + c;
        a.mean[o] = (float)mean; a.invstd[o] = invstd;
        a.scale[o] = sc; a.shift[o] = b - (float)mean * sc;
        if (a.batch_var) {
          // deferred form: the unbiased variance goes to the slot (the mean already is in mean[]); gode_bn_running applies
          // the momentum updates later, the running tensors and num_batches_tracked are not touched here
          a.batch_var[c] = (float)(n > 1.0 ? var * n / (n - 1.0) : var);
        } else {
          if (a.running_mean) {
            const double unbiased = n > 1.0 ? var * n / (n - 1.0) : var;
            a.running_mean[c] = bn_running_mean_update(a.running_mean[c], a.momentum, (float)mean);
            a.running_var[c] = bn_running_var_update(a.running_var[c], a.momentum, (float)unbiased);
          }
          if (c == 0 && a.num_batches_tracked) *a.num_batches_tracked += 1;
        }
      }
    }
  } else if (tid == 0) {
    const float invstd = 1.f / sqrtf(a.running_var[c] + a.eps);
    const float g = a.gamma ? a.gamma[c] : 1.f, b = a.beta ? a.beta[c] : 0.f;
    const float sc = g * invstd;
    const int ngroups = a.groups == 2 ? 2 : 1;
    for (int grp = 0; grp < ngroups; ++grp) {      // eval mode: both groups normalise with the running statistics
      const int o = grp * a.C + c;
      if (a.mean) a.mean[o] = a.running_mean[c];
      if (a.invstd) a.invstd[o] = invstd;
      a.scale[o] = sc; a.shift[o] = b - a.running_mean[c] * sc;
    }
  }
}

extern "C" int gode_bn_finalize(const gode_bn_finalize_op* op, void* stream) {
  if (!op || op->C <= 0 || !op->scale || !op->shift) return GODE_E_ARG;
  if (op->training) {
    if (!op->stats || !op->mean || !op->invstd || op->ncols % op->C != 0 || op->count <= 0) return GODE_E_ARG;
    if (op->stats1 && (op->groups != 2 || op->rows1 <= 0 || op->rows <= 0)) return GODE_E_ARG;
    if (op->groups == 2 && !op->stats1 && op->nseg == 0 && (op->rows0 <= 0 || op->rows0 >= op->rows)) return GODE_E_ARG;
    if (op->groups == 2 && (op->nseg < 0 || op->nseg > 8)) return GODE_E_ARG;
    for (int i = 0; op->groups == 2 && i < op->nseg; ++i)
      if (!(0 <= op->seg[3 * i] && op->seg[3 * i] <= op->seg[3 * i + 1] && op->seg[3 * i + 1] <= op->seg[3 * i + 2] && op->seg[3 * i + 2] <= op->rows)) return GODE_E_ARG;
  } else if (!op->running_mean || !op->running_var) return GODE_E_ARG;
  // the deferred form serves one training-mode batch: no groups, no segments, no eval mode
  if (op->batch_var && (!op->training || op->groups == 2 || op->nseg != 0 || op->stats1)) return GODE_E_ARG;
  hipLaunchKernelGGL(bn_finalize_kernel, dim3(op->C), dim3(256), 0, (hipStream_t)stream, *op);
  GODE_LAUNCH_CHECK();
  return 0;
}

// The momentum updates a run of deferred finalizes left out, all layers of a stack in one launch: one workgroup, layers in
// order, a thread per channel.  Same operations on the same floats as the in-place form (bn_running_*_update).
__global__ void __launch_bounds__(256) bn_running_kernel(const gode_bn_running_op a) {
  for (int l = 0; l < a.n; ++l) {
    const gode_bn_running_layer& y = a.layer[l];
    if (y.running_mean)
      for (int c = threadIdx.x; c < y.C; c += 256) {
        y.running_mean[c] = bn_running_mean_update(y.running_mean[c], a.momentum, y.mean[c]);
        y.running_var[c] = bn_running_var_update(y.running_var[c], a.momentum, y.var[c]);
      }
    if (threadIdx.x == 0 && y.num_batches_tracked) *y.num_batches_tracked += 1;
    __syncthreads();     // (two rows may name the same module: its updates then apply in row order)
  }
}

extern "C" int gode_bn_running(const gode_bn_running_op* op, void* stream) {
  if (!op || op->n <= 0 || op->n > GODE_BN_RUNNING_MAX) return GODE_E_ARG;
  for (int l = 0; l < op->n; ++l) {
    const gode_bn_running_layer& y = op->layer[l];
    if (y.C <= 0 || (y.running_mean && (!y.running_var || !y.mean || !y.var))) return GODE_E_ARG;
  }
  hipLaunchKernelGGL(bn_running_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, *op);
  GODE_LAUNCH_CHECK();
  return 0;
}

__global__ void __launch_bounds__(256) bn_apply_kernel(const gode_bn_apply_op a) {
  const int64_t n4 = a.M * a.C / 4;
  const float neg = gode_act_neg_slope(a.act);
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
    const int c = (int)((i * 4) % a.C) + ((a.M0 > 0 && i * 4 >= a.M0 * a.C) ? a.C : 0);   // second image group: + C
    f32x4 v = *reinterpret_cast<const f32x4*>(a.y + i * 4);
    f32x4 sc = {1.f, 1.f, 1.f, 1.f}, sh = {0.f, 0.f, 0.f, 0.f};
    if (a.scale) { sc = *reinterpret_cast<const f32x4*>(a.scale + c); sh = *reinterpret_cast<const f32x4*>(a.shift + c); }
#pragma unroll
    for (int e = 0; e < 4; ++e) { const float t = v[e] * sc[e] + sh[e]; v[e] = fmaxf(t, t * neg); }
    *reinterpret_cast<f32x4*>(a.out + i * 4) = v;
  }
}

extern "C" int gode_bn_apply(const gode_bn_apply_op* op, void* stream) {
  if (!op || !op->y || !op->out || op->M <= 0 || op->C <= 0 || op->C % 4 != 0) return GODE_E_ARG;
  if ((op->scale == nullptr) != (op->shift == nullptr)) return GODE_E_ARG;
  int64_t b = (op->M * op->C / 4 + 255) / 256;
  hipLaunchKernelGGL(bn_apply_kernel, dim3((int)(b > 8192 ? 8192 : (b < 1 ? 1 : b))), dim3(256), 0, (hipStream_t)stream, *op);
  GODE_LAUNCH_CHECK();
  return 0;
}

// ---------------------------------------------------------------------------------------------------------------
// col2im of a thin-output transposed convolution (see gode_col2im_op): one thread per output pixel, <= ceil(kh/sh) *
// ceil(kw/sw) taps of C floats each; every element of cols is read exactly once per launch.
__global__ void __launch_bounds__(256) col2im_kernel(const gode_col2im_op a) {
  const int64_t total = (int64_t)a.N * a.Ho * a.Wo;
  const int KC = a.kh * a.kw * a.C;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int ow = (int)(i % a.Wo); const int64_t t = i / a.Wo;
    const int oh = (int)(t % a.Ho), n = (int)(t / a.Ho);
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int kh = (oh + a.ph) % a.sh; kh < a.kh; kh += a.sh) {
      const int ih = (oh + a.ph - kh) / a.sh;
      if (oh + a.ph - kh < 0 || ih >= a.Hi) continue;
      for (int kw = (ow + a.pw) % a.sw; kw < a.kw; kw += a.sw) {
        const int iw = (ow + a.pw - kw) / a.sw;
        if (ow + a.pw - kw < 0 || iw >= a.Wi) continue;
        const float* src = a.cols + ((int64_t)(n * a.Hi + ih) * a.Wi + iw) * KC + (kh * a.kw + kw) * a.C;
        for (int c = 0; c < a.C; ++c) acc[c] += src[c];
      }
    }
    float* dst = a.out + i * a.C;
    for (int c = 0; c < a.C; ++c) dst[c] = a.epilogue == GODE_EPI_TANH ? tanhf(acc[c]) : acc[c];
  }
}

// Row-group form: a workgroup owns the sh output rows q*sh - ph ... q*sh - ph + sh - 1 of one image; they draw on the
// R = ceil(kh / sh) input rows q, q-1, ... only, which are contiguous in cols ([Wi][kh*kw*C] each) and go to LDS with
// coalesced float4 loads (the per-pixel form above reads 12-byte pieces 192 B apart: 43 us for the UCF head's 50 MB;
// this one ~20).  Same tap order per output element, so the same sums bit for bit.
__global__ void __launch_bounds__(256) col2im_rows_kernel(const gode_col2im_op a, int R, int nq) {
  extern __shared__ __attribute__((aligned(16))) float c2i_lds[];
  const int KC = a.kh * a.kw * a.C, rowlen = a.Wi * KC;
  const int q = blockIdx.x % nq, n = blockIdx.x / nq;
  for (int j = 0; j < R; ++j) {
    const int ih = q - j;
    if (ih < 0 || ih >= a.Hi) continue;                         // (never read below)
    const f32x4* src = reinterpret_cast<const f32x4*>(a.cols + ((int64_t)(n * a.Hi + ih) * a.Wi) * KC);
    f32x4* dst = reinterpret_cast<f32x4*>(c2i_lds + j * rowlen);
    for (int i = threadIdx.x; i < rowlen / 4; i += 256) dst[i] = src[i];
  }
  __syncthreads();
  for (int o = threadIdx.x; o < a.sh * a.Wo; o += 256) {
    const int r = o / a.Wo, ow = o - r * a.Wo;
    const int oh = q * a.sh - a.ph + r;
    if (oh < 0 || oh >= a.Ho) continue;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int kh = (oh + a.ph) % a.sh; kh < a.kh; kh += a.sh) {   // ascending kh = ascending j: the per-pixel form's order
      const int ih = (oh + a.ph - kh) / a.sh, j = q - ih;
      if (ih < 0 || ih >= a.Hi) continue;
      for (int kw = (ow + a.pw) % a.sw; kw < a.kw; kw += a.sw) {
        const int iw = (ow + a.pw - kw) / a.sw;
        if (ow + a.pw - kw < 0 || iw >= a.Wi) continue;
        const float* src = c2i_lds + j * rowlen + iw * KC + (kh * a.kw + kw) * a.C;
        for (int c = 0; c < a.C; ++c) acc[c] += src[c];
      }
    }
    float* dst = a.out + (((int64_t)n * a.Ho + oh) * a.Wo + ow) * a.C;
    for (int c = 0; c < a.C; ++c) dst[c] = a.epilogue == GODE_EPI_TANH ? tanhf(acc[c]) : acc[c];
  }
}

// 3-D form, taps and strides known at compile time (the shape that matters: 4x4x4 taps, strides 1x2x2 -- the UCF video
// discriminator's first layer): no divisions by run-time values, the <= 16 loads of a voxel are issued together.  Same tap
// order (kd, kh, kw ascending) as the generic kernel below: bit-identical sums.
template <int KD, int KH, int KW, int SD, int SH, int SW, int CC>
__global__ void __launch_bounds__(256) col2im3d_fixed_kernel(const gode_col2im_op a) {
  const uint32_t total = (uint32_t)a.N * a.Do * a.Ho * a.Wo;           // (< 2^31: checked by the launcher)
  constexpr int KC = KD * KH * KW * CC;
  for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < total; i += gridDim.x * 256u) {
    const uint32_t ow = i % (uint32_t)a.Wo; uint32_t t = i / (uint32_t)a.Wo;
    const uint32_t oh = t % (uint32_t)a.Ho; t /= (uint32_t)a.Ho;
    const uint32_t od = t % (uint32_t)a.Do, n = t / (uint32_t)a.Do;
    float acc[CC];
#pragma unroll
    for (int c = 0; c < CC; ++c) acc[c] = 0.f;
    const int d0 = ((int)od + a.pd) % SD, h0 = ((int)oh + a.ph) % SH, w0 = ((int)ow + a.pw) % SW;
#pragma unroll
    for (int jd = 0; jd < (KD + SD - 1) / SD; ++jd) {
      const int kd = d0 + jd * SD, td = (int)od + a.pd - kd, id = td / SD;
      if (kd >= KD || td < 0 || id >= a.Di) continue;
#pragma unroll
      for (int jh = 0; jh < (KH + SH - 1) / SH; ++jh) {
        const int kh = h0 + jh * SH, th = (int)oh + a.ph - kh, ih = th / SH;
        if (kh >= KH || th < 0 || ih >= a.Hi) continue;
#pragma unroll
        for (int jw = 0; jw < (KW + SW - 1) / SW; ++jw) {
          const int kw = w0 + jw * SW, tw = (int)ow + a.pw - kw, iw = tw / SW;
          if (kw >= KW || tw < 0 || iw >= a.Wi) continue;
          const float* src = a.cols + ((((int64_t)n * a.Di + id) * a.Hi + ih) * a.Wi + iw) * KC + ((kd * KH + kh) * KW + kw) * CC;
#pragma unroll
          for (int c = 0; c < CC; ++c) acc[c] += src[c];
        }
      }
    }
    float* dst = a.out + (int64_t)i * CC;
#pragma unroll
    for (int c = 0; c < CC; ++c) dst[c] = a.epilogue == GODE_EPI_TANH ? tanhf(acc[c]) : acc[c];
  }
}

// 3-D form: one thread per output voxel, <= ceil(kd/sd) * ceil(kh/sh) * ceil(kw/sw) taps of C floats each, fixed tap order
__global__ void __launch_bounds__(256) col2im3d_kernel(const gode_col2im_op a) {
  const int64_t total = (int64_t)a.N * a.Do * a.Ho * a.Wo;
  const int KC = a.kd * a.kh * a.kw * a.C;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int ow = (int)(i % a.Wo); int64_t t = i / a.Wo;
    const int oh = (int)(t % a.Ho); t /= a.Ho;
    const int od = (int)(t % a.Do), n = (int)(t / a.Do);
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int kd = (od + a.pd) % a.sd; kd < a.kd; kd += a.sd) {
      const int id = (od + a.pd - kd) / a.sd;
      if (od + a.pd - kd < 0 || id >= a.Di) continue;
      for (int kh = (oh + a.ph) % a.sh; kh < a.kh; kh += a.sh) {
        const int ih = (oh + a.ph - kh) / a.sh;
        if (oh + a.ph - kh < 0 || ih >= a.Hi) continue;
        for (int kw = (ow + a.pw) % a.sw; kw < a.kw; kw += a.sw) {
          const int iw = (ow + a.pw - kw) / a.sw;
          if (ow + a.pw - kw < 0 || iw >= a.Wi) continue;
          const float* src = a.cols + ((((int64_t)n * a.Di + id) * a.Hi + ih) * a.Wi + iw) * KC + ((kd * a.kh + kh) * a.kw + kw) * a.C;
          for (int c = 0; c < a.C; ++c) acc[c] += src[c];
        }
      }
    }
    float* dst = a.out + i * a.C;
    for (int c = 0; c < a.C; ++c) dst[c] = a.epilogue == GODE_EPI_TANH ? tanhf(acc[c]) : acc[c];
  }
}

extern "C" int gode_col2im(const gode_col2im_op* op, void* stream) {
  Col2imPlan P;
  const int rc = col2im_plan(op, &P);            // col2im_plan.h: the kernel, the grid and the row-group kernel's LDS
  if (rc) return rc;
  const dim3 grid(P.grid), block(256);
  hipStream_t st = (hipStream_t)stream;
  switch (P.kind) {
    case C2I_ROWS: hipLaunchKernelGGL(col2im_rows_kernel, grid, block, (size_t)P.lds, st, *op, P.R, P.nq); break;
    case C2I_PIXEL: hipLaunchKernelGGL(col2im_kernel, grid, block, 0, st, *op); break;
    case C2I_3D_FIXED: hipLaunchKernelGGL((col2im3d_fixed_kernel<4, 4, 4, 1, 2, 2, 3>), grid, block, 0, st, *op); break;
    default: hipLaunchKernelGGL(col2im3d_kernel, grid, block, 0, st, *op); break;
  }
  GODE_LAUNCH_CHECK();
  return 0;
}

// The plan of the op, host-side: what gode_col2im(op) launches and why (gode.h)
extern "C" int gode_col2im_launch_kind(const gode_col2im_op* op, int32_t* kind) {
  if (!kind) return GODE_E_ARG;
  Col2imPlan P;
  const int rc = col2im_plan(op, &P);
  if (rc) return rc;
  kind[0] = P.kind; kind[1] = P.why;
  return 0;
}

// ---------------------------------------------------------------------------------------------------------------
// BatchNorm + activation backward
#define BNB_ROWS 256   // rows per reduction block
#define BNB_CL 16      // float4 channel lanes per block (64 channels)

__device__ __forceinline__ float gz_of(float g, float y, float sc, float sh, int act) {
  if (act == GODE_ACT_TANH_OUT) return g * (1.f - y * y);
  return g * gode_act_grad(y * sc + sh, act);
}

// rank-1 upstream gradient (gode_bn_bwd_op.r1_s): the scalar of row r = (image, h, w), zero outside the crop
__device__ __forceinline__ float r1_scalar(const gode_bn_bwd_op& a, uint32_t r) {       // (M < 2^31: 32-bit divisions)
  const uint32_t t = r / (uint32_t)a.r1_W, w = r - t * (uint32_t)a.r1_W;
  const uint32_t n = t / (uint32_t)a.r1_H, h = t - n * (uint32_t)a.r1_H;
  const int hh = (int)h - a.r1_off, ww = (int)w - a.r1_off;
  return ((unsigned)hh < (unsigned)a.r1_h && (unsigned)ww < (unsigned)a.r1_wd) ? a.r1_s[((int64_t)n * a.r1_h + hh) * a.r1_wd + ww] : 0.f;
}

// partial[blk][2][C] (DOUBLE): sum g_z, sum g_z * xhat   (C % 4 == 0, C/4 <= 256).
// Both sums cancel heavily (signed gradients), and their error is fed back into every element of g_y, so they are
// accumulated in fp64 end to end; the kernel stays HBM-bound (2 fp64 FMAs per 8 bytes read).
// groups == 2 (one discriminator pass over [real; fake], gode_bn_bwd_op.groups): rows [0, M/2) and [M/2, M) are two
// BatchNorm batches with their own statistics ([2][C] arrays, group-major) -- row chunks never straddle the halves
// (chunks [0, rows0) belong to group 0), the finalisation forms one coefficient set per group, and both groups' sums go
// into dgamma / dbeta in group order: the arithmetic of two separate backward passes in one launch triple.
struct BnbGroups { int groups, rows0, rows; int64_t M0; };
__device__ __forceinline__ BnbGroups bnb_groups(const gode_bn_bwd_op& a) {
  BnbGroups G;
  G.groups = a.groups == 2 ? 2 : 1;
  G.M0 = G.groups == 2 ? (a.M0 > 0 ? a.M0 : a.M / 2) : a.M;          // rows [0, M0): group 0, [M0, M): group 1
  G.rows0 = (int)((G.M0 + BNB_ROWS - 1) / BNB_ROWS);
  G.rows = G.groups == 2 ? G.rows0 + (int)((a.M - G.M0 + BNB_ROWS - 1) / BNB_ROWS) : G.rows0;
  return G;
}

__global__ void __launch_bounds__(256) bn_bwd_reduce_kernel(const gode_bn_bwd_op a) {
  // block = (row chunk blockIdx.x) x (channel group blockIdx.y); threads = CL float4 channel lanes x RL row lanes
  const int C4 = a.C >> 2, tid = threadIdx.x;
  const int CL = C4 < BNB_CL ? C4 : BNB_CL;
  const int rl = 256 / CL;
  const int cl = tid % CL, rlane = tid / CL;
  const int c4 = blockIdx.y * CL + cl;
  const BnbGroups G = bnb_groups(a);
  const int grp = (int)blockIdx.x >= G.rows0 ? 1 : 0;
  __shared__ double red[2][256][4];
  double s1[4] = {0, 0, 0, 0}, s2[4] = {0, 0, 0, 0};
  const bool active = rlane < rl && c4 < C4;
  if (active) {
    const int c = c4 * 4, cs = grp * a.C + c;
    const f32x4 sc = *reinterpret_cast<const f32x4*>(a.scale + cs), sh = *reinterpret_cast<const f32x4*>(a.shift + cs);
    const f32x4 mu = *reinterpret_cast<const f32x4*>(a.mean + cs), is = *reinterpret_cast<const f32x4*>(a.invstd + cs);
    const int64_t r0 = grp * G.M0 + (int64_t)((int)blockIdx.x - grp * G.rows0) * BNB_ROWS;
    const int64_t rend = grp == 0 ? G.M0 : a.M;
    const int64_t r1 = r0 + BNB_ROWS < rend ? r0 + BNB_ROWS : rend;
    const float* gsrc = a.gin ? a.gin : a.g;
    f32x4 w1 = {0.f, 0.f, 0.f, 0.f};
    if (a.r1_s) w1 = *reinterpret_cast<const f32x4*>(a.r1_w + c);
    for (int64_t r = r0 + rlane; r < r1; r += rl) {
      f32x4 g;
      if (a.r1_s) { const float s = r1_scalar(a, (uint32_t)r); g = w1 * s; }
      else g = *reinterpret_cast<const f32x4*>(gsrc + r * a.C + c);
      const f32x4 y = *reinterpret_cast<const f32x4*>(a.y + r * a.C + c);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float gz = gz_of(g[e], y[e], sc[e], sh[e], a.act);
        s1[e] += (double)gz;
        s2[e] += (double)gz * (double)((y[e] - mu[e]) * is[e]);
      }
    }
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) { red[0][tid][e] = s1[e]; red[1][tid][e] = s2[e]; }
  __syncthreads();
  if (tid < CL && blockIdx.y * CL + tid < C4) {
    double t1[4] = {0, 0, 0, 0}, t2[4] = {0, 0, 0, 0};
    for (int j = 0; j < rl; ++j)
#pragma unroll
      for (int e = 0; e < 4; ++e) { t1[e] += red[0][j * CL + tid][e]; t2[e] += red[1][j * CL + tid][e]; }
    double* dst = reinterpret_cast<double*>(a.work) + (int64_t)blockIdx.x * 2 * a.C + (blockIdx.y * CL + tid) * 4;
#pragma unroll
    for (int e = 0; e < 4; ++e) { dst[e] = t1[e]; dst[a.C + e] = t2[e]; }
  }
}

// one block per channel: reduce partials, write dgamma/dbeta and the three apply coefficients (per group)
__global__ void __launch_bounds__(256) bn_bwd_finalize_kernel(const gode_bn_bwd_op a) {
  const int c = blockIdx.x, tid = threadIdx.x;
  __shared__ double red[2][256];
  const double* part = reinterpret_cast<const double*>(a.work);
  const BnbGroups G = bnb_groups(a);
  float* coef = a.work + (int64_t)G.rows * 4 * a.C;
  float dbeta_acc = 0.f, dgamma_acc = 0.f;
  if (tid == 0 && a.accumulate) { dbeta_acc = a.dbeta ? a.dbeta[c] : 0.f; dgamma_acc = a.dgamma ? a.dgamma[c] : 0.f; }
  for (int grp = 0; grp < G.groups; ++grp) {
    double s1 = 0.0, s2 = 0.0;
    for (int r = (grp == 0 ? 0 : G.rows0) + tid; r < (grp == 0 ? G.rows0 : G.rows); r += 256) {
      s1 += part[(int64_t)r * 2 * a.C + c];
      s2 += part[(int64_t)r * 2 * a.C + a.C + c];
    }
    __syncthreads();
    red[0][tid] = s1; red[1][tid] = s2;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
      if (tid < s) { red[0][tid] += red[0][tid + s]; red[1][tid] += red[1][tid + s]; }
      __syncthreads();
    }
    if (tid == 0) {
      dbeta_acc += (float)red[0][0]; dgamma_acc += (float)red[1][0];          // group order: what two passes would add
      const double Mg = (double)(grp == 0 ? G.M0 : a.M - (G.groups == 2 ? G.M0 : 0));
      const double invM = 1.0 / Mg;
      const int cs = grp * a.C + c;
      const double g = a.gamma ? (double)a.gamma[c] : 1.0, is = (double)a.invstd[cs];
      const double k = g * is;
      float* cf = coef + (int64_t)grp * 3 * a.C;
      // eval mode (running statistics are constants of the forward): g_y = gamma*invstd * g_z, no batch terms
      cf[c] = (float)k;                                                      // * g_z
      cf[a.C + c] = a.eval_mode ? 0.f : (float)(k * is * red[1][0] * invM);  // * (mean - y)
      cf[2 * a.C + c] = a.eval_mode ? 0.f : (float)(k * red[0][0] * invM);   // subtracted constant
    }
  }
  if (tid == 0) {
    if (a.dbeta) a.dbeta[c] = dbeta_acc;
    if (a.dgamma) a.dgamma[c] = dgamma_acc;
  }
}

__global__ void __launch_bounds__(256) bn_bwd_apply_kernel(const gode_bn_bwd_op a) {
  const int64_t n4 = a.M * a.C / 4;
  const BnbGroups G = bnb_groups(a);
  const float* coef = a.work + (int64_t)G.rows * 4 * a.C;
  const float* gsrc = a.gin ? a.gin : a.g;
  const int64_t n4_0 = G.M0 * a.C / 4;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
    const int grp = (G.groups == 2 && i >= n4_0) ? 1 : 0;
    const int c = (int)((i * 4) % a.C), cs = grp * a.C + c;
    const float* cf = coef + (int64_t)grp * 3 * a.C;
    f32x4 g;
    if (a.r1_s) g = *reinterpret_cast<const f32x4*>(a.r1_w + c) * r1_scalar(a, (uint32_t)((i * 4) / a.C));
    else g = *reinterpret_cast<const f32x4*>(gsrc + i * 4);
    const f32x4 y = *reinterpret_cast<const f32x4*>(a.y + i * 4);
    const f32x4 sc = *reinterpret_cast<const f32x4*>(a.scale + cs), sh = *reinterpret_cast<const f32x4*>(a.shift + cs);
    const f32x4 mu = *reinterpret_cast<const f32x4*>(a.mean + cs);
    const f32x4 cA = *reinterpret_cast<const f32x4*>(cf + c), cB = *reinterpret_cast<const f32x4*>(cf + a.C + c),
                cC = *reinterpret_cast<const f32x4*>(cf + 2 * a.C + c);
    // g_y = k*g_z - k*dbeta/M - k*invstd*dgamma/M*(y - mean); (mean - y) is formed first so that a large |mean|
    // does not cancel against a separately rounded constant
#pragma unroll
    for (int e = 0; e < 4; ++e) g[e] = cA[e] * gz_of(g[e], y[e], sc[e], sh[e], a.act) + cB[e] * (mu[e] - y[e]) - cC[e];
    *reinterpret_cast<f32x4*>(a.g + i * 4) = g;
  }
}

// no BatchNorm: g *= act'(y) (or tanh-from-output), any C
__global__ void __launch_bounds__(256) act_bwd_kernel(float* g, const float* gin, const float* y, int64_t n, int act) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
    g[i] = gz_of(gin[i], y[i], 1.f, 0.f, act);
}

extern "C" int64_t gode_bn_bwd_work_size(int64_t M, int32_t C) {
  // (sized for the two-group form: one more chunk row, two coefficient sets)
  const int64_t rows = (M + BNB_ROWS - 1) / BNB_ROWS + 2;
  return rows * 4 * C + 6 * (int64_t)C;   // fp64 partials (2 floats each) + 3 coefficient vectors per group
}

static int ew_blocks(int64_t n) {
  int64_t b = (n + 255) / 256;
  return (int)(b > 4096 ? 4096 : (b < 1 ? 1 : b));
}

extern "C" int gode_bn_bwd(const gode_bn_bwd_op* op, void* stream) {
  if (!op || !op->g || !op->y || op->M <= 0 || op->C <= 0) return GODE_E_ARG;
  hipStream_t st = (hipStream_t)stream;
  if (!op->mean) {
    hipLaunchKernelGGL(act_bwd_kernel, dim3(ew_blocks(op->M * op->C)), dim3(256), 0, st, op->g,
                       op->gin ? op->gin : op->g, op->y, op->M * op->C, op->act);
    GODE_LAUNCH_CHECK();
    return 0;
  }
  if (op->C % 4 != 0 || !op->invstd || !op->scale || !op->shift || !op->work) return GODE_E_ARG;
  if (op->r1_s && (!op->r1_w || op->r1_H <= 0 || op->r1_W <= 0 || op->r1_h <= 0 || op->r1_wd <= 0 || op->r1_off < 0 ||
                   op->M % ((int64_t)op->r1_H * op->r1_W) != 0 || op->M >= (1ll << 31) || ((uintptr_t)op->r1_w % 16) != 0)) return GODE_E_ARG;
  if (op->groups == 2 && op->M0 == 0 && (op->M % 2 != 0)) return GODE_E_ARG;
  if (op->groups == 2 && (op->M0 < 0 || op->M0 >= op->M)) return GODE_E_ARG;
  const int C4 = op->C / 4, CL = C4 < BNB_CL ? C4 : BNB_CL;
  if (256 % CL != 0) return GODE_E_SHAPE;
  const int groups = op->groups == 2 ? 2 : 1;
  const int64_t M0 = groups == 2 ? (op->M0 > 0 ? op->M0 : op->M / 2) : op->M;
  const int rows = (int)((M0 + BNB_ROWS - 1) / BNB_ROWS) + (groups == 2 ? (int)((op->M - M0 + BNB_ROWS - 1) / BNB_ROWS) : 0);
  hipLaunchKernelGGL(bn_bwd_reduce_kernel, dim3(rows, (C4 + CL - 1) / CL), dim3(256), 0, st, *op);
  GODE_LAUNCH_CHECK();
  hipLaunchKernelGGL(bn_bwd_finalize_kernel, dim3(op->C), dim3(256), 0, st, *op);
  GODE_LAUNCH_CHECK();
  hipLaunchKernelGGL(bn_bwd_apply_kernel, dim3(ew_blocks(op->M * op->C / 4)), dim3(256), 0, st, *op);
  GODE_LAUNCH_CHECK();
  return 0;
}

// ---------------------------------------------------------------------------------------------------------------
// BCE with logits, mean reduction (single block: n is a few thousand at most).  One body for both ops: the target is the
// op's constant (tt == NULL) or element i of a tensor, so a constant-valued tensor gives gode_bce_logits' bits.
__device__ __forceinline__ void bce_body(const float* logits, const float* tt, float target, float* grad, float* loss,
                                         int64_t n, float gscale, int accumulate, int64_t ld) {
  __shared__ double red[256];
  const int tid = threadIdx.x;
  double s = 0.0;
  const float inv = 1.f / (float)n;
  for (int64_t i = tid; i < n; i += 256) {
    const float x = logits[i * ld];
    const float t = tt ? tt[i] : target;
    const float l = fmaxf(x, 0.f) - x * t + log1pf(expf(-fabsf(x)));
    s += (double)l;
    if (grad) {
      const float sig = 1.f / (1.f + expf(-x));
      grad[i * ld] = gscale * (sig - t) * inv;
    }
  }
  red[tid] = s;
  __syncthreads();
  for (int k = 128; k > 0; k >>= 1) {
    if (tid < k) red[tid] += red[tid + k];
    __syncthreads();
  }
  if (tid == 0 && loss) {
    const float v = (float)(red[0] / (double)n);
    *loss = accumulate ? *loss + v : v;
  }
}
__global__ void __launch_bounds__(256) bce_kernel(const gode_bce_op a) {
  // (stride: column 0 of a categorical head, one logit per row)
  bce_body(a.logits, nullptr, a.target, a.grad, a.loss, a.n, a.gscale, a.accumulate, a.stride > 1 ? a.stride : 1);
}
__global__ void __launch_bounds__(256) bce_t_kernel(const gode_bce_t_op a) {
  bce_body(a.logits, a.target, 0.f, a.grad, a.loss, a.n, a.gscale, a.accumulate, 1);
}

extern "C" int gode_bce_logits(const gode_bce_op* op, void* stream) {
  if (!op || !op->logits || op->n <= 0) return GODE_E_ARG;
  hipLaunchKernelGGL(bce_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, *op);
  GODE_LAUNCH_CHECK();
  return 0;
}

extern "C" int gode_bce_logits_t(const gode_bce_t_op* op, void* stream) {
  if (!op || !op->logits || !op->target || op->n <= 0) return GODE_E_ARG;
  hipLaunchKernelGGL(bce_t_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, *op);
  GODE_LAUNCH_CHECK();
  return 0;
}

// ---------------------------------------------------------------------------------------------------------------
// Wasserstein loss (torchgan: generator -reduce(fgz), discriminator reduce(fgz - fx)), same single-block pattern
__global__ void __launch_bounds__(256) wgan_kernel(const gode_wgan_op a) {
  __shared__ double red[256];
  const int tid = threadIdx.x;
  double s = 0.0;
  const float gv = a.sign * (a.reduction ? a.gscale : a.gscale / (float)a.n);
  for (int64_t i = tid; i < a.n; i += 256) {
    const float d = a.real ? a.fake[i] - a.real[i] : a.fake[i];
    s += (double)d;
    if (a.grad_fake) a.grad_fake[i] = gv;
    if (a.grad_real) a.grad_real[i] = -gv;
  }
  red[tid] = s;
  __syncthreads();
  for (int k = 128; k > 0; k >>= 1) {
    if (tid < k) red[tid] += red[tid + k];
    __syncthreads();
  }
  if (tid == 0 && a.loss) {
    const float v = a.sign * (float)(a.reduction ? red[0] : red[0] / (double)a.n);
    *a.loss = a.accumulate ? *a.loss + v : v;
  }
}

extern "C" int gode_wgan_logits(const gode_wgan_op* op, void* stream) {
  if (!op || !op->fake || op->n <= 0 || (op->reduction != 0 && op->reduction != 1) || (op->grad_real && !op->real))
    return GODE_E_ARG;
  hipLaunchKernelGGL(wgan_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, *op);
  GODE_LAUNCH_CHECK();
  return 0;
}

// ---------------------------------------------------------------------------------------------------------------
// Adam with L2-coupled weight decay (operation order of torch.optim.Adam's single-tensor path)
__global__ void __launch_bounds__(256) adam_kernel(float* p, const float* g, float* m, float* v, int64_t n, float b1,
                                                   float b2, float eps, float wd, float gscale, float step_size,
                                                   float bc2_sqrt) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const float pi = p[i];
    const float gi = g[i] * gscale + wd * pi;
    const float mi = m[i] + (gi - m[i]) * (1.f - b1);
    const float vi = v[i] * b2 + (1.f - b2) * gi * gi;
    m[i] = mi; v[i] = vi;
    const float denom = sqrtf(vi) / bc2_sqrt + eps;
    p[i] = pi - step_size * (mi / denom);
  }
}

extern "C" int gode_adam_l2(const gode_adam_op* op, void* stream) {
  if (!op || !op->p || !op->g || !op->m || !op->v || op->n <= 0 || op->step < 1) return GODE_E_ARG;
  const double bc1 = 1.0 - pow((double)op->beta1, (double)op->step);
  const double bc2 = 1.0 - pow((double)op->beta2, (double)op->step);
  const float step_size = (float)((double)op->lr / bc1);
  const float bc2_sqrt = (float)sqrt(bc2);
  hipLaunchKernelGGL(adam_kernel, dim3(ew_blocks(op->n)), dim3(256), 0, (hipStream_t)stream, op->p, op->g, op->m,
                     op->v, op->n, op->beta1, op->beta2, op->eps, op->weight_decay, op->gscale, step_size, bc2_sqrt);
  GODE_LAUNCH_CHECK();
  return 0;
}

// One update rule for both entry points; float4 lanes when the four pointers of a tensor are 16-byte aligned (torch
// allocations and arena slices of whole float4s are), scalar tail / fallback otherwise.  HBM-bound: 16 B read + 12 B
// written per parameter.
// Every multiply-add is spelled as the fused operation it is to be: under -ffp-contract=fast the compiler otherwise picks, per
// call site, WHICH product of a sum like v*b2 + (1-b2)*gi*gi it fuses -- the float4 body of adam_multi_kernel fused one way, its
// scalar tail not at all, lanes 2 and 3 of adam_noise_multi_kernel's float4 body another way -- so an element's bits depended
// on its place in the tensor and on the entry point (tests/test_gpu_elementwise_cells.py: sigma = 0 noise against plain).  The
// forms below are the ones the float4 body of adam_multi_kernel had, so the bulk of every aligned tensor keeps its bits.
__device__ __forceinline__ void adam_elem(float& p, float g, float& m, float& v, float b1, float b2, float eps, float wd,
                                          float gscale, float step_size, float bc2_sqrt) {
  const float gi = fmaf(wd, p, g * gscale);
  const float mi = fmaf(1.f - b1, gi - m, m);
  const float vi = fmaf(b2, v, (1.f - b2) * gi * gi);
  m = mi; v = vi;
  p = fmaf(-step_size, mi / (sqrtf(vi) / bc2_sqrt + eps), p);
}
__device__ __forceinline__ void adam_tensor(const gode_adam_tensor& t, float b1, float b2, float eps, float wd, float gscale,
                                            float step_size, float bc2_sqrt) {
  const bool vec = (((uintptr_t)t.p | (uintptr_t)t.g | (uintptr_t)t.m | (uintptr_t)t.v) & 15) == 0;
  const int64_t n4 = vec ? t.n >> 2 : 0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
    f32x4 p = reinterpret_cast<const f32x4*>(t.p)[i], m = reinterpret_cast<const f32x4*>(t.m)[i], v = reinterpret_cast<const f32x4*>(t.v)[i];
    const f32x4 g = reinterpret_cast<const f32x4*>(t.g)[i];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float pe = p[e], me = m[e], ve = v[e];
      adam_elem(pe, g[e], me, ve, b1, b2, eps, wd, gscale, step_size, bc2_sqrt);
      p[e] = pe; m[e] = me; v[e] = ve;
    }
    reinterpret_cast<f32x4*>(t.m)[i] = m; reinterpret_cast<f32x4*>(t.v)[i] = v; reinterpret_cast<f32x4*>(t.p)[i] = p;
  }
  for (int64_t i = n4 * 4 + (int64_t)blockIdx.x * 256 + threadIdx.x; i < t.n; i += (int64_t)gridDim.x * 256) {
    float p = t.p[i], m = t.m[i], v = t.v[i];
    adam_elem(p, t.g[i], m, v, b1, b2, eps, wd, gscale, step_size, bc2_sqrt);
    t.m[i] = m; t.v[i] = v; t.p[i] = p;
  }
}
static int adam_blocks(int64_t max_n) {       // the largest tensor sets the grid: ~2 float4 per thread, others leave early
  int64_t b = (max_n + 2047) / 2048;
  return (int)(b > 2048 ? 2048 : (b < 1 ? 1 : b));
}

__global__ void __launch_bounds__(256) adam_multi_kernel(const gode_adam_tensor* table, float b1, float b2, float eps,
                                                         float wd, float gscale, float step_size, float bc2_sqrt) {
  adam_tensor(table[blockIdx.y], b1, b2, eps, wd, gscale, step_size, bc2_sqrt);
}

extern "C" int gode_adam_multi(const gode_adam_tensor* table, int32_t count, int64_t max_n, float lr, float beta1,
                               float beta2, float eps, float weight_decay, float gscale, int32_t step, void* stream) {
  if (!table || count <= 0 || max_n <= 0 || step < 1) return GODE_E_ARG;
  const double bc1 = 1.0 - pow((double)beta1, (double)step), bc2 = 1.0 - pow((double)beta2, (double)step);
  const int bx = adam_blocks(max_n);
  hipLaunchKernelGGL(adam_multi_kernel, dim3(bx, count), dim3(256), 0, (hipStream_t)stream, table, beta1, beta2, eps,
                     weight_decay, gscale, (float)((double)lr / bc1), (float)sqrt(bc2));
  GODE_LAUNCH_CHECK();
  return 0;
}

// The same update with the two step-dependent coefficients read from DEVICE memory (coef[0] = lr / (1 - beta1^step),
// coef[1] = sqrt(1 - beta2^step), written by the host in the arithmetic of gode_adam_multi): a launch recorded in a
// HIP graph stays valid while the step count advances -- the host refreshes coef before each replay.
__global__ void __launch_bounds__(256) adam_multi_dev_kernel(const gode_adam_tensor* table, float b1, float b2, float eps,
                                                             float wd, float gscale, const float* coef) {
  adam_tensor(table[blockIdx.y], b1, b2, eps, wd, gscale, coef[0], coef[1]);
}

extern "C" int gode_adam_multi_dev(const gode_adam_tensor* table, int32_t count, int64_t max_n, float beta1, float beta2,
                                   float eps, float weight_decay, float gscale, const float* coef, void* stream) {
  if (!table || count <= 0 || max_n <= 0 || !coef) return GODE_E_ARG;
  const int bx = adam_blocks(max_n);
  hipLaunchKernelGGL(adam_multi_dev_kernel, dim3(bx, count), dim3(256), 0, (hipStream_t)stream, table, beta1, beta2, eps,
                     weight_decay, gscale, coef);
  GODE_LAUNCH_CHECK();
  return 0;
}

__global__ void __launch_bounds__(256) scale_kernel(float* out, const float* a, int64_t n, float alpha, int acc) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
    out[i] = acc ? out[i] + a[i] * alpha : a[i] * alpha;
}

extern "C" int gode_scale(float* out, const float* a, int64_t n, float alpha, int accumulate, void* stream) {
  if (!out || !a || n <= 0) return GODE_E_ARG;
  hipLaunchKernelGGL(scale_kernel, dim3(ew_blocks(n)), dim3(256), 0, (hipStream_t)stream, out, a, n, alpha, accumulate);
  GODE_LAUNCH_CHECK();
  return 0;
}

// ---------------------------------------------------------------------------------------------------------------
// Parameter noise (add_noise: p += randn_like(p) * sigma after the optimiser step), fused into Adam.  The stream is a
// function of (seed, stream, step, element index in the param group) alone -- see gode.h -- so the grid, the float4 path
// and the arena layout do not change a single value.  One Philox4x32-10 call feeds the four elements of one float4:
// ~100 integer ops + two log / sqrt / sincospi per 4 elements, well under the ~175 VALU ops per element that Adam's
// 28 B of HBM traffic per parameter leaves at 6.3 TB/s.
__device__ __forceinline__ void adam_noise_tensor(const gode_adam_noise_tensor& t, float b1, float b2, float eps, float wd,
                                                  float gscale, float step_size, float bc2_sqrt, const NoiseArgs& na) {
  const bool adam = t.g != nullptr;          // uniform per block (one tensor per blockIdx.y)
  const bool vec = (((uintptr_t)t.p | (uintptr_t)t.g | (uintptr_t)t.m | (uintptr_t)t.v) & 15) == 0 && (t.noise_off & 3) == 0;
  const int64_t n4 = vec ? t.n >> 2 : 0;
  const uint64_t q0 = (uint64_t)t.noise_off >> 2;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
    f32x4 p = reinterpret_cast<const f32x4*>(t.p)[i];
    if (adam) {
      f32x4 m = reinterpret_cast<const f32x4*>(t.m)[i], v = reinterpret_cast<const f32x4*>(t.v)[i];
      const f32x4 g = reinterpret_cast<const f32x4*>(t.g)[i];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float pe = p[e], me = m[e], ve = v[e];
        adam_elem(pe, g[e], me, ve, b1, b2, eps, wd, gscale, step_size, bc2_sqrt);
        p[e] = pe; m[e] = me; v[e] = ve;
      }
      reinterpret_cast<f32x4*>(t.m)[i] = m; reinterpret_cast<f32x4*>(t.v)[i] = v;
    }
    uint32_t c[4];
    philox_quad(q0 + (uint64_t)i, na, c);
    const f32x4 z = box_muller4(c);
#pragma unroll
    for (int e = 0; e < 4; ++e) p[e] = noise_add(p[e], z[e], na.sigma);
    reinterpret_cast<f32x4*>(t.p)[i] = p;
  }
  for (int64_t i = n4 * 4 + (int64_t)blockIdx.x * 256 + threadIdx.x; i < t.n; i += (int64_t)gridDim.x * 256) {
    float p = t.p[i];
    if (adam) {
      float m = t.m[i], v = t.v[i];
      adam_elem(p, t.g[i], m, v, b1, b2, eps, wd, gscale, step_size, bc2_sqrt);
      t.m[i] = m; t.v[i] = v;
    }
    t.p[i] = noise_add(p, noise_elem((uint64_t)t.noise_off + (uint64_t)i, na), na.sigma);
  }
}

__global__ void __launch_bounds__(256) adam_noise_multi_kernel(const gode_adam_noise_tensor* table, float b1, float b2,
                                                               float eps, float wd, float gscale, float step_size,
                                                               float bc2_sqrt, NoiseArgs na) {
  adam_noise_tensor(table[blockIdx.y], b1, b2, eps, wd, gscale, step_size, bc2_sqrt, na);
}

extern "C" int gode_adam_noise_multi(const gode_adam_noise_tensor* table, int32_t count, int64_t max_n, float lr,
                                     float beta1, float beta2, float eps, float weight_decay, float gscale, int32_t step,
                                     uint64_t seed, uint32_t noise_stream, uint32_t noise_step, float sigma, void* stream) {
  if (!table || count <= 0 || max_n <= 0 || step < 1) return GODE_E_ARG;
  const double bc1 = 1.0 - pow((double)beta1, (double)step), bc2 = 1.0 - pow((double)beta2, (double)step);
  const int bx = adam_blocks(max_n);
  hipLaunchKernelGGL(adam_noise_multi_kernel, dim3(bx, count), dim3(256), 0, (hipStream_t)stream, table, beta1, beta2,
                     eps, weight_decay, gscale, (float)((double)lr / bc1), (float)sqrt(bc2),
                     make_noise_args(seed, noise_stream, noise_step, sigma));
  GODE_LAUNCH_CHECK();
  return 0;
}

// coef[0], coef[1]: Adam's step-dependent coefficients as in adam_multi_dev_kernel; coef[2]: the noise step, raw 32 bits
__global__ void __launch_bounds__(256) adam_noise_multi_dev_kernel(const gode_adam_noise_tensor* table, float b1, float b2,
                                                                   float eps, float wd, float gscale, const float* coef,
                                                                   NoiseArgs na) {
  na.step = __float_as_uint(coef[2]);
  adam_noise_tensor(table[blockIdx.y], b1, b2, eps, wd, gscale, coef[0], coef[1], na);
}

extern "C" int gode_adam_noise_multi_dev(const gode_adam_noise_tensor* table, int32_t count, int64_t max_n, float beta1,
                                         float beta2, float eps, float weight_decay, float gscale, const float* coef,
                                         uint64_t seed, uint32_t noise_stream, float sigma, void* stream) {
  if (!table || count <= 0 || max_n <= 0 || !coef) return GODE_E_ARG;
  const int bx = adam_blocks(max_n);
  hipLaunchKernelGGL(adam_noise_multi_dev_kernel, dim3(bx, count), dim3(256), 0, (hipStream_t)stream, table, beta1, beta2,
                     eps, weight_decay, gscale, coef, make_noise_args(seed, noise_stream, 0, sigma));
  GODE_LAUNCH_CHECK();
  return 0;
}

// The stream on its own: one thread per Philox quad overlapping [noise_off, noise_off + n), any offset and length
__global__ void __launch_bounds__(256) param_noise_kernel(float* out, int64_t n, int64_t noise_off, NoiseArgs na, int mode) {
  const uint64_t q_lo = (uint64_t)noise_off >> 2, q_hi = ((uint64_t)noise_off + (uint64_t)n - 1) >> 2;
  for (uint64_t q = q_lo + (uint64_t)blockIdx.x * 256 + threadIdx.x; q <= q_hi; q += (uint64_t)gridDim.x * 256) {
    uint32_t c[4];
    philox_quad(q, na, c);
    f32x4 z;
    if (mode != 2) z = box_muller4(c);
#pragma unroll
    for (int l = 0; l < 4; ++l) {
      const int64_t i = (int64_t)(q * 4 + l) - noise_off;
      if (i < 0 || i >= n) continue;
      if (mode == 2) out[i] = __uint_as_float(c[l]);
      else if (mode == 1) out[i] = noise_add(out[i], z[l], na.sigma);
      else out[i] = noise_scale(z[l], na.sigma);
    }
  }
}

extern "C" int gode_param_noise(float* out, int64_t n, uint64_t seed, uint32_t noise_stream, uint32_t noise_step,
                                int64_t noise_off, float sigma, int32_t accumulate, void* stream) {
  if (!out || n <= 0 || noise_off < 0 || accumulate < 0 || accumulate > 2) return GODE_E_ARG;
  const int64_t quads = (((noise_off + n - 1) >> 2) - (noise_off >> 2)) + 1;
  const int64_t b = (quads + 255) / 256;
  hipLaunchKernelGGL(param_noise_kernel, dim3((unsigned)(b > 4096 ? 4096 : b)), dim3(256), 0, (hipStream_t)stream, out, n,
                     noise_off, make_noise_args(seed, noise_stream, noise_step, sigma), (int)accumulate);
  GODE_LAUNCH_CHECK();
  return 0;
}
