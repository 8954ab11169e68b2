// gres.hip -- stage 1: the pieces of DVD-GAN's generator residual block around the convolutions (stage1/GResBlock.py):
// channel statistics of a strided tensor, the ConditionalNorm embedding, conditional BatchNorm + ReLU + nearest upsample and
// its backward, the block output (biases + skip + pool) and its inverse, and spectral normalisation with its gradient.  The
// 3x3 / 1x1 convolutions themselves are gode_igemm / gode_wgrad on the channels-last tensors written here.
// All of these are HBM-bound passes; sums are formed per thread in index order, then by a fixed tree / a fixed block order
// (no float atomics), in double where a sum spans more than a few hundred terms.  Element indices are 32-bit (the
// convolutions that consume these tensors have the same 2^31-element limit), decoded with FastDiv.
#include "common.h"

static inline int gres_pow2_ge(int x) { int p = 1; while (p < x) p <<= 1; return p; }
// resolves "all zero = channels-last contiguous"; false on a negative stride
static inline bool gres_strides(const int64_t* s, int H, int W, int C, int64_t* o) {
  if (s[0] == 0 && s[1] == 0 && s[2] == 0 && s[3] == 0) { o[3] = 1; o[2] = C; o[1] = (int64_t)W * C; o[0] = (int64_t)H * W * C; return true; }
  for (int i = 0; i < 4; ++i) { if (s[i] < 0) return false; o[i] = s[i]; }
  return true;
}
static inline int gres_blocks(int64_t total, int cap = 16384) {
  int64_t b = (total + 255) / 256;
  return (int)(b > cap ? cap : (b < 1 ? 1 : b));
}
// threads of a 256-thread workgroup as a logical [TP positions][TC channels] grid, TC a function of C alone, so that the
// order of every sum is the same for every memory layout of the tensor
static inline int gres_tc(int C) { return C >= 256 ? 256 : gres_pow2_ge(C); }

// ---------------------------------------------------------------------------------------------------------------
// channel statistics.  pfast: the tensor is not channel-fastest -- the same logical grid is laid over the threads with the
// position index fastest, so that a wave still reads runs of consecutive addresses; the LDS tree is indexed logically and
// gives the same bits either way.  sq == 0: sums only (stats[C][rows]).
struct ChstatsArgs { const float* x; float* stats; int64_t s[4]; int32_t H, W, C, rows, TC, pfast, sq, pad_; int64_t P, chunk; };

__global__ void __launch_bounds__(256) chstats_kernel(const ChstatsArgs a) {
  __shared__ double red[2][256];
  const int tid = threadIdx.x, TC = a.TC, TP = 256 / TC;
  const int cl = a.pfast ? tid / TP : tid & (TC - 1), pl = a.pfast ? tid % TP : tid / TC;
  const int li = pl * TC + cl;
  const int64_t lo = (int64_t)blockIdx.x * a.chunk;
  const int64_t hi = lo + a.chunk < a.P ? lo + a.chunk : a.P;
  for (int cb = 0; cb < a.C; cb += TC) {
    const int c = cb + cl;
    double s1 = 0.0, s2 = 0.0;
    if (c < a.C)
      for (int64_t p = lo + pl; p < hi; p += TP) {
        const int w = (int)(p % a.W); const int64_t t = p / a.W;
        const int h = (int)(t % a.H); const int64_t n = t / a.H;
        const double v = (double)a.x[n * a.s[0] + h * a.s[1] + w * a.s[2] + c * a.s[3]];
        s1 += v; s2 += v * v;
      }
    red[0][li] = s1; red[1][li] = s2;
    __syncthreads();
    for (int s = TP >> 1; s > 0; s >>= 1) {
      if (pl < s) { red[0][li] += red[0][li + s * TC]; red[1][li] += red[1][li + s * TC]; }
      __syncthreads();
    }
    if (pl == 0 && c < a.C) {
      a.stats[(int64_t)c * a.rows + blockIdx.x] = (float)red[0][li];
      if (a.sq) a.stats[((int64_t)a.C + c) * a.rows + blockIdx.x] = (float)red[1][li];
    }
    __syncthreads();
  }
}

extern "C" int gode_chstats_rows(int64_t positions) {
  int64_t r = (positions + 63) / 64;
  return (int)(r > 1024 ? 1024 : (r < 1 ? 1 : r));
}

static int launch_chstats(const float* x, float* stats, const int64_t* s, int N, int H, int W, int C, int rows, int sq, hipStream_t st) {
  ChstatsArgs A;
  A.x = x; A.stats = stats; A.H = H; A.W = W; A.C = C; A.rows = rows;
  for (int i = 0; i < 4; ++i) A.s[i] = s[i];
  A.P = (int64_t)N * H * W; A.chunk = (A.P + rows - 1) / rows;
  A.TC = gres_tc(C); A.pfast = s[3] != 1 ? 1 : 0; A.sq = sq; A.pad_ = 0;
  hipLaunchKernelGGL(chstats_kernel, dim3(rows), dim3(256), 0, st, A);
  GODE_LAUNCH_CHECK();
  return 0;
}

extern "C" int gode_chstats(const gode_chstats_op* op, void* stream) {
  if (!op || !op->x || !op->stats || op->N <= 0 || op->H <= 0 || op->W <= 0 || op->C <= 0 || op->rows <= 0) return GODE_E_ARG;
  int64_t s[4];
  if (!gres_strides(op->xs, op->H, op->W, op->C, s)) return GODE_E_ARG;
  return launch_chstats(op->x, op->stats, s, op->N, op->H, op->W, op->C, op->rows, 1, (hipStream_t)stream);
}

// ---------------------------------------------------------------------------------------------------------------
// ConditionalNorm embedding (Linear(n_condition, 2C)) and its backward: a few thousand outputs of <= a few hundred terms
__global__ void __launch_bounds__(256) cbn_embed_kernel(const gode_cbn_embed_op a) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= a.N * a.C2) return;
  const int n = i / a.C2, j = i - n * a.C2;
  const float* x = a.cond + (int64_t)n * a.K;
  const float* w = a.W + (int64_t)j * a.K;
  float s = 0.f;
  for (int k = 0; k < a.K; ++k) s += x[k] * w[k];
  a.gb[i] = s + (a.b ? a.b[j] : 0.f);
}

extern "C" int gode_cbn_embed(const gode_cbn_embed_op* op, void* stream) {
  if (!op || !op->cond || !op->W || !op->gb || op->N <= 0 || op->K <= 0 || op->C2 <= 0 || op->C2 % 2 != 0) return GODE_E_ARG;
  if ((int64_t)op->N * op->C2 >= (1ll << 31)) return GODE_E_SHAPE;
  hipLaunchKernelGGL(cbn_embed_kernel, dim3((op->N * op->C2 + 255) / 256), dim3(256), 0, (hipStream_t)stream, *op);
  GODE_LAUNCH_CHECK();
  return 0;
}

__global__ void __launch_bounds__(256) cbn_embed_bwd_kernel(const gode_cbn_embed_bwd_op a) {
  int i = blockIdx.x * 256 + threadIdx.x;
  const int nW = a.C2 * a.K, nb = a.C2, nc = a.N * a.K;
  if (i < nW) {
    if (!a.dW) return;
    const int j = i / a.K, k = i - j * a.K;
    float s = 0.f;
    for (int n = 0; n < a.N; ++n) s += a.dgb[(int64_t)n * a.C2 + j] * a.cond[(int64_t)n * a.K + k];
    a.dW[i] = s;
    return;
  }
  i -= nW;
  if (i < nb) {
    if (!a.db) return;
    float s = 0.f;
    for (int n = 0; n < a.N; ++n) s += a.dgb[(int64_t)n * a.C2 + i];
    a.db[i] = s;
    return;
  }
  i -= nb;
  if (i < nc && a.dcond) {
    const int n = i / a.K, k = i - n * a.K;
    float s = 0.f;
    for (int j = 0; j < a.C2; ++j) s += a.dgb[(int64_t)n * a.C2 + j] * a.W[(int64_t)j * a.K + k];
    a.dcond[i] = s;
  }
}

extern "C" int gode_cbn_embed_bwd(const gode_cbn_embed_bwd_op* op, void* stream) {
  if (!op || !op->cond || !op->W || !op->dgb || op->N <= 0 || op->K <= 0 || op->C2 <= 0) return GODE_E_ARG;
  const int64_t total = (int64_t)op->C2 * op->K + op->C2 + (int64_t)op->N * op->K;
  if (total >= (1ll << 31)) return GODE_E_SHAPE;
  hipLaunchKernelGGL(cbn_embed_bwd_kernel, dim3((int)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, *op);
  GODE_LAUNCH_CHECK();
  return 0;
}

// ---------------------------------------------------------------------------------------------------------------
// conditional BatchNorm + activation + nearest upsample: one thread per SOURCE element (channel fastest), f x f stores
struct CbnApplyArgs {
  const float* src; const float* bias; const float* mean; const float* invstd; const float* gb; float* out;
  int64_t s[4]; int32_t H, W, C, f, act; uint32_t total; FastDiv dC, dW, dH;
};

__global__ void __launch_bounds__(256) cbn_apply_kernel(const CbnApplyArgs a) {
  const int Hf = a.H * a.f, Wf = a.W * a.f;
  for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < a.total; i += gridDim.x * 256u) {
    const uint32_t p = fdiv(i, a.dC), c = i - p * a.C;
    const uint32_t t = fdiv(p, a.dW), w = p - t * a.W;
    const uint32_t n = fdiv(t, a.dH), h = t - n * a.H;
    float v = a.src[(int64_t)n * a.s[0] + (int64_t)h * a.s[1] + (int64_t)w * a.s[2] + (int64_t)c * a.s[3]];
    if (a.bias) v += a.bias[c];
    if (a.mean) {
      const float xh = (v - a.mean[c]) * a.invstd[c];
      const float* gb = a.gb + (int64_t)n * 2 * a.C;
      v = gb[c] * xh + gb[a.C + c];
    }
    v = gode_act(v, a.act);
    for (int di = 0; di < a.f; ++di)
      for (int dj = 0; dj < a.f; ++dj)
        a.out[(((int64_t)n * Hf + h * a.f + di) * Wf + w * a.f + dj) * a.C + c] = v;
  }
}

extern "C" int gode_cbn_apply(const gode_cbn_apply_op* op, void* stream) {
  if (!op || !op->src || !op->out || op->N <= 0 || op->H <= 0 || op->W <= 0 || op->C <= 0 || (op->f != 1 && op->f != 2)) return GODE_E_ARG;
  if (op->mean && (!op->invstd || !op->gb)) return GODE_E_ARG;
  if (op->act != GODE_ACT_NONE && op->act != GODE_ACT_RELU && op->act != GODE_ACT_LRELU) return GODE_E_ARG;
  CbnApplyArgs A;
  if (!gres_strides(op->ss, op->H, op->W, op->C, A.s)) return GODE_E_ARG;
  const int64_t total = (int64_t)op->N * op->H * op->W * op->C;
  if (total * op->f * op->f >= (1ll << 31)) return GODE_E_SHAPE;
  A.src = op->src; A.bias = op->bias; A.mean = op->mean; A.invstd = op->invstd; A.gb = op->gb; A.out = op->out;
  A.H = op->H; A.W = op->W; A.C = op->C; A.f = op->f; A.act = op->act; A.total = (uint32_t)total;
  A.dC = make_fastdiv((uint32_t)op->C); A.dW = make_fastdiv((uint32_t)op->W); A.dH = make_fastdiv((uint32_t)op->H);
  hipLaunchKernelGGL(cbn_apply_kernel, dim3(gres_blocks(total)), dim3(256), 0, (hipStream_t)stream, A);
  GODE_LAUNCH_CHECK();
  return 0;
}

// ---------------------------------------------------------------------------------------------------------------
// conditional BatchNorm backward.  Pass 1 (one workgroup per (position chunk, sample)): g_z and the chunk's sums; 1b: per
// sample, chunks in order -> dgb; 1c: per channel, samples in order -> the batch terms (and dbias); pass 2: g_v.
struct CbnBwdArgs {
  gode_cbn_bwd_op o;
  int64_t s[4], go[4];
  double* part; double* nsum; double* csum; float* gz;
  int32_t nblk, chunk, TC, sums; uint32_t total; FastDiv dC, dW, dH;
};
static inline int cbn_bwd_nblk(int HW) { int b = (HW + 63) / 64; return b > 32 ? 32 : (b < 1 ? 1 : b); }

__global__ void __launch_bounds__(256) cbn_bwd_pass1_kernel(const CbnBwdArgs a) {
  __shared__ double red[2][256];
  const gode_cbn_bwd_op& o = a.o;
  const int tid = threadIdx.x, TC = a.TC, TP = 256 / TC, cl = tid & (TC - 1), pl = tid / TC;
  const int n = blockIdx.y, HW = o.H * o.W, f = o.f, Hf = o.H * f, Wf = o.W * f, C = o.C;
  const int lo = blockIdx.x * a.chunk, hi = lo + a.chunk < HW ? lo + a.chunk : HW;
  const bool direct = o.mean == nullptr;
  for (int cb = 0; cb < C; cb += TC) {
    const int c = cb + cl;
    double s1 = 0.0, s2 = 0.0;
    if (c < C)
      for (int p = lo + pl; p < hi; p += TP) {
        const int h = p / o.W, w = p - h * o.W;
        const int64_t up = (((int64_t)n * Hf + h * f) * Wf + w * f) * C + c;
        float g = 0.f;
        for (int di = 0; di < f; ++di)
          for (int dj = 0; dj < f; ++dj) g += o.g_a[up + ((int64_t)di * Wf + dj) * C];
        const float av = o.a[up];
        const float gz = o.act == GODE_ACT_RELU ? (av > 0.f ? g : 0.f) : (o.act == GODE_ACT_LRELU ? (av > 0.f ? g : 0.2f * g) : g);
        const int64_t e = ((int64_t)n * HW + p) * C + c;
        if (direct) {
          const float r = o.gadd ? gz + o.gadd[e] : gz;
          o.g_out[(int64_t)n * a.go[0] + (int64_t)h * a.go[1] + (int64_t)w * a.go[2] + (int64_t)c * a.go[3]] = r;
        } else {
          a.gz[e] = gz;
        }
        if (a.sums) {
          s1 += (double)gz;
          if (!direct) {
            float v = o.src[(int64_t)n * a.s[0] + (int64_t)h * a.s[1] + (int64_t)w * a.s[2] + (int64_t)c * a.s[3]];
            if (o.bias) v += o.bias[c];
            s2 += (double)(gz * ((v - o.mean[c]) * o.invstd[c]));
          }
        }
      }
    if (!a.sums) continue;
    red[0][tid] = s1; red[1][tid] = s2;
    __syncthreads();
    for (int s = TP >> 1; s > 0; s >>= 1) {
      if (pl < s) { red[0][tid] += red[0][tid + s * TC]; red[1][tid] += red[1][tid + s * TC]; }
      __syncthreads();
    }
    if (pl == 0 && c < C) {
      double* dst = a.part + ((int64_t)n * a.nblk + blockIdx.x) * 2 * C;
      dst[c] = red[0][tid]; dst[C + c] = red[1][tid];
    }
    __syncthreads();
  }
}

__global__ void __launch_bounds__(256) cbn_bwd_sample_kernel(const CbnBwdArgs a) {
  const int n = blockIdx.x, C = a.o.C;
  for (int c = threadIdx.x; c < C; c += 256) {
    double s1 = 0.0, s2 = 0.0;
    for (int b = 0; b < a.nblk; ++b) {
      const double* src = a.part + ((int64_t)n * a.nblk + b) * 2 * C;
      s1 += src[c]; s2 += src[C + c];
    }
    a.nsum[((int64_t)n * 2) * C + c] = s1; a.nsum[((int64_t)n * 2 + 1) * C + c] = s2;
    if (a.o.dgb) { a.o.dgb[(int64_t)n * 2 * C + c] = (float)s2; a.o.dgb[(int64_t)n * 2 * C + C + c] = (float)s1; }
  }
}

__global__ void __launch_bounds__(256) cbn_bwd_channel_kernel(const CbnBwdArgs a) {
  const int c = blockIdx.x * 256 + threadIdx.x, C = a.o.C;
  if (c >= C) return;
  double S1 = 0.0, S2 = 0.0;
  for (int n = 0; n < a.o.N; ++n) {
    const double gam = a.o.gb ? (double)a.o.gb[(int64_t)n * 2 * C + c] : 1.0;
    S1 += gam * a.nsum[((int64_t)n * 2) * C + c];
    S2 += gam * a.nsum[((int64_t)n * 2 + 1) * C + c];
  }
  a.csum[c] = S1; a.csum[C + c] = S2;
  if (a.o.dbias) a.o.dbias[c] = a.o.mean == nullptr ? (float)S1 : (a.o.eval_mode ? a.o.invstd[c] * (float)S1 : 0.f);
}

__global__ void __launch_bounds__(256) cbn_bwd_pass2_kernel(const CbnBwdArgs a) {
  const gode_cbn_bwd_op& o = a.o;
  const int C = o.C;
  const double invM = 1.0 / ((double)o.N * o.H * o.W);
  for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < a.total; i += gridDim.x * 256u) {
    const uint32_t p = fdiv(i, a.dC), c = i - p * C;
    const uint32_t t = fdiv(p, a.dW), w = p - t * o.W;
    const uint32_t n = fdiv(t, a.dH), h = t - n * o.H;
    float v = o.src[(int64_t)n * a.s[0] + (int64_t)h * a.s[1] + (int64_t)w * a.s[2] + (int64_t)c * a.s[3]];
    if (o.bias) v += o.bias[c];
    const float xh = (v - o.mean[c]) * o.invstd[c];
    float gx = o.gb[(int64_t)n * 2 * C + c] * a.gz[i];
    if (!o.eval_mode) gx = gx - (float)(a.csum[c] * invM) - xh * (float)(a.csum[C + c] * invM);
    float r = o.invstd[c] * gx;
    if (o.gadd) r += o.gadd[i];
    o.g_out[(int64_t)n * a.go[0] + (int64_t)h * a.go[1] + (int64_t)w * a.go[2] + (int64_t)c * a.go[3]] = r;
  }
}

extern "C" int64_t gode_cbn_bwd_work_size(int32_t N, int32_t H, int32_t W, int32_t C) {
  if (N <= 0 || H <= 0 || W <= 0 || C <= 0) return GODE_E_ARG;
  const int64_t nblk = cbn_bwd_nblk(H * W);
  return 2 * ((int64_t)N * nblk * 2 * C + (int64_t)N * 2 * C + 2 * C) + (int64_t)N * H * W * C;
}

extern "C" int gode_cbn_bwd(const gode_cbn_bwd_op* op, void* stream) {
  if (!op || !op->g_a || !op->a || !op->g_out || !op->work || op->N <= 0 || op->H <= 0 || op->W <= 0 || op->C <= 0 ||
      (op->f != 1 && op->f != 2) || ((uintptr_t)op->work % 8) != 0)
    return GODE_E_ARG;
  if (op->mean && (!op->invstd || !op->gb || !op->src)) return GODE_E_ARG;
  if (!op->mean && op->dgb) return GODE_E_ARG;
  if (op->act != GODE_ACT_NONE && op->act != GODE_ACT_RELU && op->act != GODE_ACT_LRELU) return GODE_E_ARG;
  CbnBwdArgs A;
  A.o = *op;
  if (!gres_strides(op->ss, op->H, op->W, op->C, A.s) || !gres_strides(op->gos, op->H, op->W, op->C, A.go)) return GODE_E_ARG;
  const int64_t total = (int64_t)op->N * op->H * op->W * op->C;
  if (total * op->f * op->f >= (1ll << 31) || op->N > 65535) return GODE_E_SHAPE;
  const int HW = op->H * op->W;
  A.nblk = cbn_bwd_nblk(HW); A.chunk = (HW + A.nblk - 1) / A.nblk;
  A.TC = gres_tc(op->C);                 // g_a, a and the g_z buffer are channels-last: channel-fastest threads
  A.sums = (op->mean != nullptr || op->dbias != nullptr) ? 1 : 0;
  A.total = (uint32_t)total;
  A.dC = make_fastdiv((uint32_t)op->C); A.dW = make_fastdiv((uint32_t)op->W); A.dH = make_fastdiv((uint32_t)op->H);
  A.part = reinterpret_cast<double*>(op->work);
  A.nsum = A.part + (int64_t)op->N * A.nblk * 2 * op->C;
  A.csum = A.nsum + (int64_t)op->N * 2 * op->C;
  A.gz = reinterpret_cast<float*>(A.csum + 2 * op->C);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(cbn_bwd_pass1_kernel, dim3(A.nblk, op->N), dim3(256), 0, st, A);
  GODE_LAUNCH_CHECK();
  if (A.sums) {
    hipLaunchKernelGGL(cbn_bwd_sample_kernel, dim3(op->N), dim3(256), 0, st, A);
    GODE_LAUNCH_CHECK();
    hipLaunchKernelGGL(cbn_bwd_channel_kernel, dim3((op->C + 255) / 256), dim3(256), 0, st, A);
    GODE_LAUNCH_CHECK();
  }
  if (op->mean) {
    hipLaunchKernelGGL(cbn_bwd_pass2_kernel, dim3(gres_blocks(total)), dim3(256), 0, st, A);
    GODE_LAUNCH_CHECK();
  }
  return 0;
}

// ---------------------------------------------------------------------------------------------------------------
// block output: one thread per element of y (channels-last)
struct GresOutArgs { gode_gres_out_op o; int32_t Ho, Wo; uint32_t total; FastDiv dC, dW, dH; };

__global__ void __launch_bounds__(256) gres_out_kernel(const GresOutArgs a) {
  const gode_gres_out_op& o = a.o;
  const int C = o.C;
  for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < a.total; i += gridDim.x * 256u) {
    const uint32_t p = fdiv(i, a.dC), c = i - p * C;
    const uint32_t t = fdiv(p, a.dW), q = p - t * a.Wo;
    const uint32_t n = fdiv(t, a.dH), r = t - n * a.Ho;
    const float bm = o.b_main ? o.b_main[c] : 0.f, bs = o.b_sc ? o.b_sc[c] : 0.f;
    float y;
    if (o.down == 1) {
      const int64_t e = (((int64_t)n * o.H + r / o.f) * o.W + q / o.f) * C + c;
      y = (o.main[i] + bm) + (o.sc[e] + bs);
    } else {
      const int64_t e = (((int64_t)n * o.H + 2 * r) * o.W + 2 * q) * C + c;
      const int64_t dw = C, dh = (int64_t)o.W * C;
      const float m = (((o.main[e] + bm) + (o.main[e + dw] + bm)) + (o.main[e + dh] + bm)) + (o.main[e + dh + dw] + bm);
      const float s = (((o.sc[e] + bs) + (o.sc[e + dw] + bs)) + (o.sc[e + dh] + bs)) + (o.sc[e + dh + dw] + bs);
      y = 0.25f * m + 0.25f * s;
    }
    o.y[i] = y;
  }
}

static int gres_out_dims(int H, int W, int f, int down, int* Ho, int* Wo) {
  if ((f != 1 && f != 2) || (down != 1 && down != 2) || (f == 2 && down == 2)) return GODE_E_ARG;
  *Ho = H * f / down; *Wo = W * f / down;
  return (*Ho > 0 && *Wo > 0) ? 0 : GODE_E_SHAPE;
}

extern "C" int gode_gres_out(const gode_gres_out_op* op, void* stream) {
  if (!op || !op->main || !op->sc || !op->y || op->N <= 0 || op->H <= 0 || op->W <= 0 || op->C <= 0) return GODE_E_ARG;
  GresOutArgs A;
  A.o = *op;
  const int rc = gres_out_dims(op->H, op->W, op->f, op->down, &A.Ho, &A.Wo);
  if (rc) return rc;
  const int64_t total = (int64_t)op->N * A.Ho * A.Wo * op->C;
  if (total >= (1ll << 31) || (int64_t)op->N * op->H * op->W * op->C >= (1ll << 31)) return GODE_E_SHAPE;
  A.total = (uint32_t)total;
  A.dC = make_fastdiv((uint32_t)op->C); A.dW = make_fastdiv((uint32_t)A.Wo); A.dH = make_fastdiv((uint32_t)A.Ho);
  hipLaunchKernelGGL(gres_out_kernel, dim3(gres_blocks(total)), dim3(256), 0, (hipStream_t)stream, A);
  GODE_LAUNCH_CHECK();
  return 0;
}

// its inverse: column sums of g_y through the statistics kernel above (sums only, rows in order), then one thread per element of g_sc
struct GresOutBwdArgs { gode_gres_out_bwd_op o; int64_t gy[4]; int32_t Ho, Wo; uint32_t total; FastDiv dC, dW, dH; };

__global__ void __launch_bounds__(256) gres_colsum_kernel(const float* stats, float* db, int C, int rows) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  double s = 0.0;
  for (int r = 0; r < rows; ++r) s += (double)stats[(int64_t)c * rows + r];
  db[c] = (float)s;
}

__global__ void __launch_bounds__(256) gres_out_bwd_kernel(const GresOutBwdArgs a) {
  const gode_gres_out_bwd_op& o = a.o;
  const int C = o.C, f = o.f;
  for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < a.total; i += gridDim.x * 256u) {
    const uint32_t p = fdiv(i, a.dC), c = i - p * C;
    const uint32_t t = fdiv(p, a.dW), w = p - t * o.W;
    const uint32_t n = fdiv(t, a.dH), h = t - n * o.H;
    float s = 0.f;
    if (o.down == 1) {
      for (int di = 0; di < f; ++di)
        for (int dj = 0; dj < f; ++dj) {
          const int r = h * f + di, q = w * f + dj;
          const float g = o.g_y[(int64_t)n * a.gy[0] + (int64_t)r * a.gy[1] + (int64_t)q * a.gy[2] + (int64_t)c * a.gy[3]];
          s += g;
          if (o.g_main) o.g_main[(((int64_t)n * a.Ho + r) * a.Wo + q) * C + c] = g;
        }
    } else {
      const int r = h >> 1, q = w >> 1;
      if (r < a.Ho && q < a.Wo)
        s = 0.25f * o.g_y[(int64_t)n * a.gy[0] + (int64_t)r * a.gy[1] + (int64_t)q * a.gy[2] + (int64_t)c * a.gy[3]];
    }
    o.g_sc[i] = s;
  }
}

extern "C" int64_t gode_gres_out_bwd_work_size(int32_t N, int32_t H, int32_t W, int32_t C, int32_t f, int32_t down) {
  int Ho, Wo;
  const int rc = gres_out_dims(H, W, f, down, &Ho, &Wo);
  if (rc || N <= 0 || C <= 0) return rc ? rc : GODE_E_ARG;
  return (int64_t)C * gode_chstats_rows((int64_t)N * Ho * Wo);
}

extern "C" int gode_gres_out_bwd(const gode_gres_out_bwd_op* op, void* stream) {
  if (!op || !op->g_y || !op->g_sc || (op->db && !op->work) || op->N <= 0 || op->H <= 0 || op->W <= 0 || op->C <= 0) return GODE_E_ARG;
  GresOutBwdArgs A;
  A.o = *op;
  const int rc = gres_out_dims(op->H, op->W, op->f, op->down, &A.Ho, &A.Wo);
  if (rc) return rc;
  if (op->down == 2 && op->g_main) return GODE_E_ARG;
  if (!gres_strides(op->gys, A.Ho, A.Wo, op->C, A.gy)) return GODE_E_ARG;
  const int64_t total = (int64_t)op->N * op->H * op->W * op->C;
  if (total * op->f * op->f >= (1ll << 31)) return GODE_E_SHAPE;
  hipStream_t st = (hipStream_t)stream;
  if (op->db) {
    const int rows = gode_chstats_rows((int64_t)op->N * A.Ho * A.Wo);
    const int r2 = launch_chstats(op->g_y, op->work, A.gy, op->N, A.Ho, A.Wo, op->C, rows, 0, st);
    if (r2) return r2;
    hipLaunchKernelGGL(gres_colsum_kernel, dim3((op->C + 255) / 256), dim3(256), 0, st, op->work, op->db, op->C, rows);
    GODE_LAUNCH_CHECK();
  }
  A.total = (uint32_t)total;
  A.dC = make_fastdiv((uint32_t)op->C); A.dW = make_fastdiv((uint32_t)op->W); A.dH = make_fastdiv((uint32_t)op->H);
  hipLaunchKernelGGL(gres_out_bwd_kernel, dim3(gres_blocks(total)), dim3(256), 0, st, A);
  GODE_LAUNCH_CHECK();
  return 0;
}

// ---------------------------------------------------------------------------------------------------------------
// spectral normalisation.  wbar[h][w] is too large for one workgroup's registers or LDS (100 x 900 in the reference's demo)
// and small against the GPU (360 KB): it is streamed from L2 twice per forward, with the lanes of a wave always on
// consecutive addresses -- wbar^T u: one thread per COLUMN walking the rows (lanes = neighbouring columns);  wbar v: one wave
// per ROW, lanes striding the columns, then a fixed shuffle tree.  The two norms are single-workgroup steps between them.
__global__ void __launch_bounds__(256) sn_wtu_kernel(const gode_sn_op a) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= a.w) return;
  double s = 0.0;
  for (int i = 0; i < a.h; ++i) s += (double)a.wbar[(int64_t)i * a.w + j] * (double)a.u[i];
  a.work[j] = (float)s;
}

__global__ void __launch_bounds__(256) sn_wv_kernel(const gode_sn_op a) {
  const int lane = threadIdx.x & 63, i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= a.h) return;                       // (whole waves leave together)
  double s = 0.0;
  for (int j = lane; j < a.w; j += 64) s += (double)a.wbar[(int64_t)i * a.w + j] * (double)a.v[j];
  for (int m = 32; m > 0; m >>= 1) s += __shfl_xor(s, m);
  if (lane == 0) a.work[a.w + i] = (float)s;
}

// out = in / (|in| + 1e-12); sigma != NULL: also sigma = out . in
__global__ void __launch_bounds__(256) sn_l2n_kernel(const float* in, float* out, int n, float* sigma) {
  __shared__ double red[256];
  const int tid = threadIdx.x;
  double s = 0.0;
  for (int i = tid; i < n; i += 256) { const double v = (double)in[i]; s += v * v; }
  red[tid] = s;
  __syncthreads();
  for (int k = 128; k > 0; k >>= 1) { if (tid < k) red[tid] += red[tid + k]; __syncthreads(); }
  const float nrm = (float)sqrt(red[0]);
  __syncthreads();
  double d = 0.0;
  for (int i = tid; i < n; i += 256) { const float o = in[i] / (nrm + 1e-12f); out[i] = o; d += (double)o * (double)in[i]; }
  if (!sigma) return;
  red[tid] = d;
  __syncthreads();
  for (int k = 128; k > 0; k >>= 1) { if (tid < k) red[tid] += red[tid + k]; __syncthreads(); }
  if (tid == 0) *sigma = (float)red[0];
}

__global__ void __launch_bounds__(256) sn_div_kernel(const float* wbar, const float* sigma, float* wout, int64_t n) {
  const float s = *sigma;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) wout[i] = wbar[i] / s;
}

extern "C" int gode_sn_fwd(const gode_sn_op* op, void* stream) {
  if (!op || !op->wbar || !op->u || !op->v || !op->wout || !op->sigma || !op->work || op->h <= 0 || op->w <= 0) return GODE_E_ARG;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(sn_wtu_kernel, dim3((op->w + 255) / 256), dim3(256), 0, st, *op);
  GODE_LAUNCH_CHECK();
  hipLaunchKernelGGL(sn_l2n_kernel, dim3(1), dim3(256), 0, st, (const float*)op->work, op->v, op->w, (float*)nullptr);
  GODE_LAUNCH_CHECK();
  hipLaunchKernelGGL(sn_wv_kernel, dim3((op->h + 3) / 4), dim3(256), 0, st, *op);
  GODE_LAUNCH_CHECK();
  hipLaunchKernelGGL(sn_l2n_kernel, dim3(1), dim3(256), 0, st, (const float*)(op->work + op->w), op->u, op->h, op->sigma);
  GODE_LAUNCH_CHECK();
  const int64_t n = (int64_t)op->h * op->w;
  hipLaunchKernelGGL(sn_div_kernel, dim3(gres_blocks(n, 1024)), dim3(256), 0, st, op->wbar, (const float*)op->sigma, op->wout, n);
  GODE_LAUNCH_CHECK();
  return 0;
}

// backward: <G, wbar> as GODE_SN_BWD_BLOCKS partial sums over contiguous spans (double), re-added in block order by every
// workgroup of the element-wise pass
__global__ void __launch_bounds__(256) sn_dot_kernel(const gode_sn_bwd_op a, int64_t n, int64_t span) {
  __shared__ double red[256];
  const int tid = threadIdx.x;
  const int64_t lo = (int64_t)blockIdx.x * span, hi = lo + span < n ? lo + span : n;
  double s = 0.0;
  for (int64_t i = lo + tid; i < hi; i += 256) s += (double)a.G[i] * (double)a.wbar[i];
  red[tid] = s;
  __syncthreads();
  for (int k = 128; k > 0; k >>= 1) { if (tid < k) red[tid] += red[tid + k]; __syncthreads(); }
  if (tid == 0) reinterpret_cast<double*>(a.work)[blockIdx.x] = red[0];
}

__global__ void __launch_bounds__(256) sn_bwd_kernel(const gode_sn_bwd_op a, int64_t n, int nblk) {
  __shared__ float coef;
  if (threadIdx.x == 0) {
    double d = 0.0;
    for (int b = 0; b < nblk; ++b) d += reinterpret_cast<const double*>(a.work)[b];
    const double s = (double)*a.sigma;
    coef = (float)(d / (s * s));
  }
  __syncthreads();
  const float s = *a.sigma, k = coef;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const int r = (int)(i / a.w), c = (int)(i - (int64_t)r * a.w);
    a.dwbar[i] = a.G[i] / s - k * (a.u[r] * a.v[c]);
  }
}

extern "C" int gode_sn_bwd(const gode_sn_bwd_op* op, void* stream) {
  if (!op || !op->G || !op->wbar || !op->u || !op->v || !op->sigma || !op->dwbar || !op->work || op->h <= 0 || op->w <= 0 ||
      ((uintptr_t)op->work % 8) != 0)
    return GODE_E_ARG;
  hipStream_t st = (hipStream_t)stream;
  const int64_t n = (int64_t)op->h * op->w;
  int64_t nblk = (n + 1023) / 1024;
  if (nblk > GODE_SN_BWD_BLOCKS) nblk = GODE_SN_BWD_BLOCKS;
  const int64_t span = (n + nblk - 1) / nblk;
  hipLaunchKernelGGL(sn_dot_kernel, dim3((int)nblk), dim3(256), 0, st, *op, n, span);
  GODE_LAUNCH_CHECK();
  hipLaunchKernelGGL(sn_bwd_kernel, dim3(gres_blocks(n, 1024)), dim3(256), 0, st, *op, n, (int)nblk);
  GODE_LAUNCH_CHECK();
  return 0;
}
