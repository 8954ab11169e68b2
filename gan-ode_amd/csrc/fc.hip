// fc.hip -- the passes around the matrix products of stage 2's fully-connected MNIST GAN
// (stage2/test_ODE_training_with_MNIST_GAN.ipynb: Generator 100-256-512-1024-784, Discriminator 784-1024-512-256-1 with
// F.dropout(x, 0.3) behind every hidden LeakyReLU, nn.BCELoss on the sigmoid output).  The products themselves are gode_igemm
// (FPROP / DGRAD of a 1x1x1 geometry) and gode_wgrad; here:
//   gode_fc_act      out = drop(act(y + b))                      one pass over [M][C], in place or not
//   gode_fc_act_bwd  g_y = g_out * keep / (1 - p) * act'(out)    and db[c] = sum_m g_y[m][c] in a fixed order
//   gode_bce_prob    nn.BCELoss() (mean) on probabilities, loss and gradient in one workgroup
// The dropout mask is never stored: both directions recompute the keep bit of element e = m*C + c from Philox4x32-10 with the
// counter layout of gode.h, so it does not depend on the grid or on the vector width.
//
// Roofline: all three are HBM / launch bound.  Forward: 8 B per element (read y, write out; the bias row stays in cache), one
// Philox call (~100 integer ops) per four elements when C % 4 == 0.  Backward: 12 B per element (read g_out and out, write g_y)
// plus C floats of db per 128 rows; a workgroup covers 128 rows x 32 columns, so C = 1024 gives 32 workgroups.  At the
// notebook's size (M = 100, C <= 1024) a pass moves at most 1.2 MB: a few microseconds of kernel time, of the order of the
// launch itself.
#include "common.h"
#include "philox.h"

#define FC_DROP_TAG 0x40000000u
#define FC_BWD_ROWS 128          // rows per workgroup of the backward pass: M <= 128 needs no second launch
#define FC_BWD_LANES 32          // row lanes of a workgroup
#define FC_BWD_COLT 8            // column threads of a workgroup (x FC_BWD_LANES = 256), V columns each: 128 B of a row at V = 4

static inline NoiseArgs fc_noise_args(int64_t key, int32_t layer) {
  return make_noise_args((uint64_t)key, FC_DROP_TAG | (uint32_t)layer, 0u, 0.f);
}

// keep bits of the quad that holds elements 4q .. 4q + 3 (bit l: element 4q + l is kept)
__device__ __forceinline__ uint32_t fc_keep_quad(uint64_t q, const NoiseArgs& na, float p) {
  uint32_t w[4];
  philox_quad(q, na, w);
  uint32_t bits = 0;
#pragma unroll
  for (int l = 0; l < 4; ++l) bits |= (noise_uniform(w[l]) >= p ? 1u : 0u) << l;
  return bits;
}
__device__ __forceinline__ bool fc_keep(uint64_t e, const NoiseArgs& na, float p) {
  return (fc_keep_quad(e >> 2, na, p) >> (uint32_t)(e & 3)) & 1u;
}

__device__ __forceinline__ float fc_activate(float v, int act) {
  if (act == GODE_ACT_LRELU) return v > 0.f ? v : 0.2f * v;
  if (act == GODE_ACT_TANH) return tanhf(v);
  if (act == GODE_ACT_SIGMOID) return 1.f / (1.f + expf(-v));
  return v;
}
// act' from the activation's OUTPUT a
__device__ __forceinline__ float fc_act_grad(float a, int act) {
  if (act == GODE_ACT_LRELU) return a > 0.f ? 1.f : 0.2f;
  if (act == GODE_ACT_TANH) return 1.f - a * a;
  if (act == GODE_ACT_SIGMOID) return a * (1.f - a);
  return 1.f;
}

static inline bool fc_act_ok(int act) {
  return act == GODE_ACT_NONE || act == GODE_ACT_LRELU || act == GODE_ACT_TANH || act == GODE_ACT_SIGMOID;
}

// ---------------------------------------------------------------------------------------------------------------
// forward.  V = 4: one float4 (one Philox quad) per thread and step; V = 1: any C, any alignment
template <int V>
__global__ void __launch_bounds__(256) fc_act_kernel(const gode_fc_act_op a, NoiseArgs na) {
  const int64_t n = a.M * a.C / V;
  const bool drop = a.p > 0.f;
  const float keep_scale = 1.f / (1.f - a.p);
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    if (V == 4) {
      const int c = (int)((i * 4) % a.C);
      f32x4 v = *reinterpret_cast<const f32x4*>(a.y + i * 4);
      if (a.b) { const f32x4 b = *reinterpret_cast<const f32x4*>(a.b + c); v += b; }
      const uint32_t bits = drop ? fc_keep_quad((uint64_t)i, na, a.p) : 15u;
#pragma unroll
      for (int l = 0; l < 4; ++l) {
        const float t = fc_activate(v[l], a.act);
        v[l] = drop ? ((bits >> l) & 1u ? t * keep_scale : 0.f) : t;
      }
      *reinterpret_cast<f32x4*>(a.out + i * 4) = v;
    } else {
      float v = a.y[i];
      if (a.b) v += a.b[i % a.C];
      v = fc_activate(v, a.act);
      if (drop) v = fc_keep((uint64_t)i, na, a.p) ? v * keep_scale : 0.f;
      a.out[i] = v;
    }
  }
}

static bool fc_args_ok(int64_t M, int32_t C, int32_t act, int32_t layer, float p) {
  return M > 0 && C > 0 && M * (int64_t)C < (1ll << 31) && fc_act_ok(act) && layer >= 0 && layer < 256 && p >= 0.f && p < 1.f;
}

static int fc_blocks(int64_t n) {
  const int64_t b = (n + 255) / 256;
  return (int)(b > 8192 ? 8192 : b);
}

extern "C" int gode_fc_act(const gode_fc_act_op* op, void* stream) {
  if (!op || !op->y || !op->out || !fc_args_ok(op->M, op->C, op->act, op->layer, op->p)) return GODE_E_ARG;
  const NoiseArgs na = fc_noise_args(op->key, op->layer);
  const bool vec = op->C % 4 == 0 && ((uintptr_t)op->y % 16) == 0 && ((uintptr_t)op->out % 16) == 0 &&
                   (op->b == nullptr || ((uintptr_t)op->b % 16) == 0);
  const int64_t n = op->M * op->C;
  if (vec) hipLaunchKernelGGL(fc_act_kernel<4>, dim3(fc_blocks(n / 4)), dim3(256), 0, (hipStream_t)stream, *op, na);
  else hipLaunchKernelGGL(fc_act_kernel<1>, dim3(fc_blocks(n)), dim3(256), 0, (hipStream_t)stream, *op, na);
  GODE_LAUNCH_CHECK();
  return 0;
}

// ---------------------------------------------------------------------------------------------------------------
// backward.  A workgroup owns FC_BWD_ROWS rows x FC_BWD_COLT*V columns (C = 1024: 32 workgroups, four rows per thread):
// thread (column lane, row lane) walks its rows top down, the row lanes' sums meet in LDS and are added in lane order.  One row chunk: db is written here; more: the chunk sums go to
// work[chunk][C] and fc_db_finish_kernel adds them in chunk order.  No atomics anywhere: reruns give the same bits.
template <int V>
__global__ void __launch_bounds__(256) fc_act_bwd_kernel(const gode_fc_act_bwd_op a, NoiseArgs na) {
  __shared__ float red[FC_BWD_LANES][FC_BWD_COLT * V];
  const int cl = threadIdx.x % FC_BWD_COLT, rl = threadIdx.x / FC_BWD_COLT;
  const int c = ((int)blockIdx.x * FC_BWD_COLT + cl) * V;
  const int64_t r0 = (int64_t)blockIdx.y * FC_BWD_ROWS;
  const int64_t r1 = r0 + FC_BWD_ROWS < a.M ? r0 + FC_BWD_ROWS : a.M;
  const bool drop = a.p > 0.f;
  const float keep_scale = 1.f / (1.f - a.p), undo = 1.f - a.p;
  float s[V];
#pragma unroll
  for (int l = 0; l < V; ++l) s[l] = 0.f;
  if (c < a.C) {
    for (int64_t r = r0 + rl; r < r1; r += FC_BWD_LANES) {
      const int64_t e = r * a.C + c;
      if (V == 4) {
        f32x4 g = *reinterpret_cast<const f32x4*>(a.g_out + e);
        const f32x4 o = *reinterpret_cast<const f32x4*>(a.out + e);
        const uint32_t bits = drop ? fc_keep_quad((uint64_t)e >> 2, na, a.p) : 15u;
#pragma unroll
        for (int l = 0; l < 4; ++l) {
          const float d = fc_act_grad(drop ? o[l] * undo : o[l], a.act);
          g[l] = drop ? ((bits >> l) & 1u ? g[l] * keep_scale * d : 0.f) : g[l] * d;
          s[l] += g[l];
        }
        *reinterpret_cast<f32x4*>(a.g_y + e) = g;
      } else {
        const float o = a.out[e];
        const float d = fc_act_grad(drop ? o * undo : o, a.act);
        float g = a.g_out[e];
        g = drop ? (fc_keep((uint64_t)e, na, a.p) ? g * keep_scale * d : 0.f) : g * d;
        s[0] += g;
        a.g_y[e] = g;
      }
    }
  }
  if (!a.db) return;
#pragma unroll
  for (int l = 0; l < V; ++l) red[rl][cl * V + l] = s[l];
  __syncthreads();
  if (rl == 0 && c < a.C) {
    float* dst = gridDim.y == 1 ? a.db : a.work + (int64_t)blockIdx.y * a.C;
#pragma unroll
    for (int l = 0; l < V; ++l) {
      float t = red[0][cl * V + l];
#pragma unroll
      for (int k = 1; k < FC_BWD_LANES; ++k) t += red[k][cl * V + l];
      dst[c + l] = (gridDim.y == 1 && a.accumulate) ? dst[c + l] + t : t;
    }
  }
}

__global__ void __launch_bounds__(256) fc_db_finish_kernel(const float* work, float* db, int chunks, int C, int accumulate) {
  const int c = (int)blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  float t = work[c];
  for (int k = 1; k < chunks; ++k) t += work[(int64_t)k * C + c];
  db[c] = accumulate ? db[c] + t : t;
}

extern "C" int64_t gode_fc_act_bwd_work_size(int64_t M, int32_t C) {
  if (M <= 0 || C <= 0) return GODE_E_ARG;
  const int64_t chunks = (M + FC_BWD_ROWS - 1) / FC_BWD_ROWS;
  return chunks > 1 ? chunks * C : 0;
}

extern "C" int gode_fc_act_bwd(const gode_fc_act_bwd_op* op, void* stream) {
  if (!op || !op->g_out || !op->out || !op->g_y || !fc_args_ok(op->M, op->C, op->act, op->layer, op->p)) return GODE_E_ARG;
  const int chunks = (int)((op->M + FC_BWD_ROWS - 1) / FC_BWD_ROWS);
  if (op->db && chunks > 1 && !op->work) return GODE_E_ARG;
  if (chunks > 65535) return GODE_E_SHAPE;
  const NoiseArgs na = fc_noise_args(op->key, op->layer);
  const bool vec = op->C % 4 == 0 && ((uintptr_t)op->g_out % 16) == 0 && ((uintptr_t)op->out % 16) == 0 &&
                   ((uintptr_t)op->g_y % 16) == 0;
  hipStream_t st = (hipStream_t)stream;
  if (vec) hipLaunchKernelGGL(fc_act_bwd_kernel<4>, dim3((op->C + 4 * FC_BWD_COLT - 1) / (4 * FC_BWD_COLT), chunks), dim3(256), 0, st, *op, na);
  else hipLaunchKernelGGL(fc_act_bwd_kernel<1>, dim3((op->C + FC_BWD_COLT - 1) / FC_BWD_COLT, chunks), dim3(256), 0, st, *op, na);
  GODE_LAUNCH_CHECK();
  if (op->db && chunks > 1) {
    hipLaunchKernelGGL(fc_db_finish_kernel, dim3((op->C + 255) / 256), dim3(256), 0, st, op->work, op->db, chunks, op->C,
                       op->accumulate);
    GODE_LAUNCH_CHECK();
  }
  return 0;
}

// ---------------------------------------------------------------------------------------------------------------
// the keep values alone (tests, and a caller that wants to look at a mask)
__global__ void __launch_bounds__(256) fc_mask_kernel(float* out, int64_t n, NoiseArgs na, float p) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
    out[i] = fc_keep((uint64_t)i, na, p) ? 1.f : 0.f;
}

extern "C" int gode_dropout_mask(float* out, int64_t n, uint64_t key, uint32_t layer, float p, void* stream) {
  if (!out || n <= 0 || layer > 255u || !(p >= 0.f && p < 1.f)) return GODE_E_ARG;
  hipLaunchKernelGGL(fc_mask_kernel, dim3(fc_blocks(n)), dim3(256), 0, (hipStream_t)stream, out, n,
                     fc_noise_args((int64_t)key, (int32_t)layer), p);
  GODE_LAUNCH_CHECK();
  return 0;
}

// ---------------------------------------------------------------------------------------------------------------
// nn.BCELoss() on probabilities, mean reduction, torch's clamps (log terms at -100, the gradient's denominator at 1e-12);
// one workgroup, the sum in double in a fixed order (n is the batch size)
__global__ void __launch_bounds__(256) bce_prob_kernel(const gode_bce_prob_op a) {
  __shared__ double red[256];
  const int tid = threadIdx.x;
  double s = 0.0;
  const float inv = 1.f / (float)a.n;
  for (int64_t i = tid; i < a.n; i += 256) {
    const float p = a.p[i], t = a.t[i];
    const float lp = fmaxf(logf(p), -100.f), lq = fmaxf(log1pf(-p), -100.f);
    s += (double)(-(t * lp + (1.f - t) * lq));
    if (a.grad) a.grad[i] = a.gscale * (p - t) / fmaxf((1.f - p) * p, 1e-12f) * inv;
  }
  red[tid] = s;
  __syncthreads();
  for (int k = 128; k > 0; k >>= 1) {
    if (tid < k) red[tid] += red[tid + k];
    __syncthreads();
  }
  if (tid == 0 && a.loss) {
    const float v = (float)(red[0] / (double)a.n);
    *a.loss = a.accumulate ? *a.loss + v : v;
  }
}

extern "C" int gode_bce_prob(const gode_bce_prob_op* op, void* stream) {
  if (!op || !op->p || !op->t || op->n <= 0) return GODE_E_ARG;
  hipLaunchKernelGGL(bce_prob_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, *op);
  GODE_LAUNCH_CHECK();
  return 0;
}
