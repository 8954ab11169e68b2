// categ.hip -- the categorical (InfoGAN) half of MoCoGAN: the one-hot columns of the latent rows and the fused
// cross-entropy of the categorical discriminator's class logits (models/mocogan.py:167-182,231-247).
#include "common.h"

// ---------------------------------------------------------------------------------------------------------------
// One-hot columns: latent row r belongs to trajectory r / rows_per (full mode: rows_per = T; select mode: 1) and
// receives z[r][col0 + c] = (cls[trajectory] == c) for c < C.  Both values are stored, so a reused latent buffer needs no
// clearing, and the launch follows the latent solve (whose content broadcast zeroes the pad columns) on the same stream.
// labels_out (nullable): the classes widened to int64, the tensor sample_videos hands back.
__global__ void __launch_bounds__(256) categ_onehot_kernel(const gode_categ_op a) {
  const int64_t total = (int64_t)a.n_traj * a.rows_per * a.C;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < total) {
    const int64_t r = i / a.C;
    const int c = (int)(i - r * a.C);
    const int n = (int)(r / a.rows_per);
    a.z[r * a.zcols + a.col0 + c] = a.cls[n] == c ? 1.f : 0.f;
  }
  if (a.labels_out && i < a.n_traj) a.labels_out[i] = (int64_t)a.cls[i];
}

extern "C" int gode_categ_onehot(const gode_categ_op* op, void* stream) {
  if (!op || !op->cls || !op->z || op->n_traj <= 0 || op->rows_per <= 0 || op->C <= 0 || op->col0 < 0 ||
      op->col0 + op->C > op->zcols)
    return GODE_E_ARG;
  const int64_t total = (int64_t)op->n_traj * op->rows_per * op->C;
  if (total >= (1ll << 31)) return GODE_E_SHAPE;
  hipLaunchKernelGGL(categ_onehot_kernel, dim3((int)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, *op);
  GODE_LAUNCH_CHECK();
  return 0;
}

// ---------------------------------------------------------------------------------------------------------------
// nn.CrossEntropyLoss() (mean reduction) of rows [0, n_lab) of a [B][ld] logits block with C class columns, single block
// like the other losses (B is a batch size).  Per row in fp32: m = max, lse = m + log(sum exp(x - m)); the row losses are
// summed in double, per thread in row order, then over the threads by a fixed tree.  grad rows [0, n_lab) receive
// gscale * (softmax - onehot) / n_lab, rows [n_lab, B) zeros (the fake half of a paired discriminator pass carries no
// class term).  rows_per_label = P > 1: the head of video b is P consecutive rows (the output positions of a patch
// discriminator) that share labels[b]; n_lab and B still count rows.  A label outside [0, C) poisons the loss with NaN instead of reading out of bounds.
__global__ void __launch_bounds__(256) ce_kernel(const gode_ce_op a) {
  __shared__ double red[256];
  const int tid = threadIdx.x;
  double s = 0.0;
  const float inv = a.n_lab > 0 ? a.gscale / (float)a.n_lab : 0.f;
  const int rpl = a.rows_per_label > 1 ? a.rows_per_label : 1;     // (a patch head: every position of a video shares its label)
  for (int r = tid; r < a.B; r += 256) {
    float* g = a.grad ? a.grad + (int64_t)r * a.gld : nullptr;
    if (r >= a.n_lab) {
      if (g) for (int c = 0; c < a.C; ++c) g[c] = 0.f;
      continue;
    }
    const float* x = a.logits + (int64_t)r * a.ld;
    const int64_t lab = a.labels[r / rpl];
    const bool ok = lab >= 0 && lab < a.C;
    float m = x[0];
    for (int c = 1; c < a.C; ++c) m = fmaxf(m, x[c]);
    float se = 0.f;
    for (int c = 0; c < a.C; ++c) se += expf(x[c] - m);
    const float lse = m + logf(se);
    s += ok ? (double)(lse - x[lab]) : (double)__builtin_nanf("");
    if (g) {
      const float rs = 1.f / se;
      for (int c = 0; c < a.C; ++c) g[c] = (expf(x[c] - m) * rs - (c == lab ? 1.f : 0.f)) * inv;
    }
  }
  red[tid] = s;
  __syncthreads();
  for (int k = 128; k > 0; k >>= 1) {
    if (tid < k) red[tid] += red[tid + k];
    __syncthreads();
  }
  if (tid == 0 && a.loss && a.n_lab > 0) {     // (n_lab == 0: a block of unlabelled rows -- zero gradient, no loss term)
    const float v = (float)(red[0] / (double)a.n_lab);
    *a.loss = a.accumulate ? *a.loss + v : v;
  }
}

extern "C" int gode_ce_logits(const gode_ce_op* op, void* stream) {
  if (!op || !op->logits || (!op->labels && op->n_lab > 0) || op->B <= 0 || op->n_lab < 0 || op->n_lab > op->B ||
      op->C <= 0 || op->ld < op->C || (op->grad && op->gld < op->C))
    return GODE_E_ARG;
  hipLaunchKernelGGL(ce_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, *op);
  GODE_LAUNCH_CHECK();
  return 0;
}
