// diffaug.hip -- differentiable augmentation in front of the discriminators (DiffAugment; gode.h): random
// brightness / saturation / contrast / translation / cutout with one parameter set per sample (a whole clip), forward and
// backward, as ONE pass over the caller's strided tensor into a channels-last copy.  The parameters are recomputed in the
// kernel from (seed, stream, call, global sample index) with the Philox of philox.h on the tag family 0x20000000: they
// depend on the sample alone, so every workgroup of a sample derives them from its block index (scalar ALU work).
//
// Roofline: 4 B read + 4 B written per element; contrast needs the sample's mean first, one more read (the sum launch).
// A sample is cut into gode_diffaug_chunks chunks of positions, one 256-thread workgroup each (a UCF clip of 65,536
// positions: 64 workgroups), so a batch of 16 clips fills the chip; the chunk sums are fp64, reduced in a fixed tree inside
// the workgroup, stored to work[sample][chunk] and added in index order by every workgroup of the second launch.  No atomics.
// One thread handles all C channels of a position (C = 1 or 3 in registers, any other C by reading twice): adjacent lanes
// touch adjacent positions in both the channels-last and the planar ([B,T,C,H,W] transposed) source layouts.
#include "common.h"

#define DA_THREADS 256
#define DA_CHUNK_MIN 1024       // positions per workgroup at least (4 per thread)
#define DA_CHUNKS_MAX 64        // partial sums per sample at most

struct DaParams { float ub, us, uc; int32_t tx, ty, cx, cy; };

// Philox4x32-10 as philox.h states it, in arithmetic the host pass compiles too (gode_diffaug_params)
__host__ __device__ static inline void da_philox(uint32_t c[4], uint32_t k0, uint32_t k1) {
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c[0], p1 = (uint64_t)0xCD9E8D57u * c[2];
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1;
    c[0] = n0; c[1] = (uint32_t)p1; c[2] = n2; c[3] = (uint32_t)p0;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
}
__host__ __device__ static inline uint32_t da_mulhi(uint32_t a, uint32_t b) { return (uint32_t)(((uint64_t)a * b) >> 32); }
__host__ __device__ static inline float da_uniform(uint32_t w) { return ((float)(w >> 9) + 0.5f) * 0x1p-23f; }

__host__ __device__ static inline uint32_t da_tag(uint32_t stream, uint32_t field) {
  return 0x20000000u | (stream << 8) | field;
}

// all seven parameters of global sample g (whatever the mask: switching a component off does not move the others)
__host__ __device__ static inline DaParams da_params(uint32_t k0, uint32_t k1, uint32_t stream, uint32_t call, uint64_t g,
                                                     int32_t H, int32_t W) {
  DaParams p;
  uint32_t c[4] = {(uint32_t)g, call, da_tag(stream, 0u), (uint32_t)(g >> 32)};
  da_philox(c, k0, k1);
  p.ub = da_uniform(c[0]); p.us = da_uniform(c[1]); p.uc = da_uniform(c[2]);
  uint32_t e[4] = {(uint32_t)g, call, da_tag(stream, 1u), (uint32_t)(g >> 32)};
  da_philox(e, k0, k1);
  const int32_t Sx = (W + 4) / 8, Sy = (H + 4) / 8, cw = (W + 1) / 2, ch = (H + 1) / 2;
  p.tx = (int32_t)da_mulhi(e[0], (uint32_t)(2 * Sx + 1)) - Sx;
  p.ty = (int32_t)da_mulhi(e[1], (uint32_t)(2 * Sy + 1)) - Sy;
  p.cx = (int32_t)da_mulhi(e[2], (uint32_t)(W + 1 - cw % 2));
  p.cy = (int32_t)da_mulhi(e[3], (uint32_t)(H + 1 - ch % 2));
  return p;
}

struct DaArgs { FastDiv dHW, dW; uint32_t k0, k1, S, chunk; int32_t P; };

// what a position gathers: the shift (source = position - (sy, sx)) and the cutout box [y0, y1) x [x0, x1)
struct DaBox { int32_t sx, sy, x0, x1, y0, y1; };

template <bool BWD>
__device__ __forceinline__ DaBox da_box(const gode_diffaug_op& a, const DaParams& p) {
  DaBox b = {0, 0, 0, 0, 0, 0};
  if (a.mask & 8) { b.sx = BWD ? -p.tx : p.tx; b.sy = BWD ? -p.ty : p.ty; }
  if (a.mask & 16) {
    const int32_t cw = (a.W + 1) / 2, ch = (a.H + 1) / 2;
    b.x0 = p.cx - cw / 2; b.x1 = b.x0 + cw; b.y0 = p.cy - ch / 2; b.y1 = b.y0 + ch;
  }
  return b;
}

// element offset (channel 0, within the sample) of what output position `pos` reads, or -1 where it is the constant zero.
// Forward: the cutout lies on the output position; backward: on the position the cotangent comes from.
template <bool BWD>
__device__ __forceinline__ int64_t da_source(const gode_diffaug_op& a, const DaArgs& A, const DaBox& b, uint32_t pos) {
  const uint32_t d = fdiv(pos, A.dHW), r = pos - d * A.dHW.d, h = fdiv(r, A.dW), w = r - h * A.dW.d;
  const int32_t hs = (int32_t)h - b.sy, ws = (int32_t)w - b.sx;
  if (hs < 0 || hs >= a.H || ws < 0 || ws >= a.W) return -1;
  const int32_t hc = BWD ? hs : (int32_t)h, wc = BWD ? ws : (int32_t)w;
  if (hc >= b.y0 && hc < b.y1 && wc >= b.x0 && wc < b.x1) return -1;
  return (int64_t)d * a.xs[1] + (int64_t)hs * a.xs[2] + (int64_t)ws * a.xs[3];
}

__device__ __forceinline__ uint32_t da_call(const gode_diffaug_op& a) {
  return (a.call_dev ? (uint32_t)a.call_dev[0] : 0u) + (uint32_t)a.call;
}

// phase 1 (masks with contrast): work[sample][chunk] = the fp64 sum of the chunk -- forward: of x; backward: of the masked,
// shifted cotangent.  Thread t adds positions lo + t, lo + t + 256, ... in order, channels in order; then a fixed tree.
template <bool BWD>
__global__ void __launch_bounds__(DA_THREADS) diffaug_sum_kernel(const gode_diffaug_op a, const DaArgs A) {
  __shared__ double s_part[DA_THREADS];
  const int tid = threadIdx.x;
  const uint32_t n = blockIdx.x / (uint32_t)A.P, k = blockIdx.x - n * (uint32_t)A.P;
  DaBox b = {0, 0, 0, 0, 0, 0};
  if (BWD) b = da_box<true>(a, da_params(A.k0, A.k1, (uint32_t)a.stream, da_call(a), (uint64_t)a.g0 + n, a.H, a.W));
  const float* xn = a.x + (int64_t)n * a.xs[0];
  const uint32_t lo = k * A.chunk, hi = min(lo + A.chunk, A.S);
  double acc = 0.0;
  for (uint32_t pos = lo + tid; pos < hi; pos += DA_THREADS) {
    const int64_t off = da_source<BWD>(a, A, b, pos);     // (forward: no shift, no box -- the plain offset)
    if (off < 0) continue;
    for (int c = 0; c < a.C; ++c) acc += (double)xn[off + (int64_t)c * a.xs[4]];
  }
  s_part[tid] = acc;
  __syncthreads();
  for (int s = DA_THREADS / 2; s > 0; s >>= 1) {
    if (tid < s) s_part[tid] += s_part[tid + s];
    __syncthreads();
  }
  if (tid == 0) reinterpret_cast<double*>(a.work)[blockIdx.x] = s_part[0];
}

// phase 2 (the only launch for masks without contrast): the transform itself.  CT: the channel count held in registers
// (0: any C, the source read twice).
template <bool BWD, int CT>
__global__ void __launch_bounds__(DA_THREADS) diffaug_apply_kernel(const gode_diffaug_op a, const DaArgs A) {
  const int tid = threadIdx.x;
  const int C = CT ? CT : a.C;
  const uint32_t n = blockIdx.x / (uint32_t)A.P, k = blockIdx.x - n * (uint32_t)A.P;
  const DaParams p = da_params(A.k0, A.k1, (uint32_t)a.stream, da_call(a), (uint64_t)a.g0 + n, a.H, a.W);
  const DaBox b = da_box<BWD>(a, p);
  const bool bright = a.mask & 1, sat = a.mask & 2, con = a.mask & 4;
  const float bo = p.ub - 0.5f, ss = 2.f * p.us, sc = p.uc + 0.5f;
  float M = 0.f;
  if (con) {                                              // the chunk sums of this sample, in index order
    const double* part = reinterpret_cast<const double*>(a.work) + (size_t)n * A.P;
    double s = 0.0;
    for (int j = 0; j < A.P; ++j) s += part[j];
    s /= (double)A.S * (double)C;
    if (!BWD && bright) s += (double)bo;                  // the mean behind brightness (saturation keeps it)
    M = (float)s;
  }
  const float inv_c = 1.f / (float)C;
  const float* xn = a.x + (int64_t)n * a.xs[0];
  float* on = a.out + (int64_t)n * A.S * C;
  const uint32_t lo = k * A.chunk, hi = min(lo + A.chunk, A.S);
  for (uint32_t pos = lo + tid; pos < hi; pos += DA_THREADS) {
    const int64_t off = da_source<BWD>(a, A, b, pos);
    float* o = on + (int64_t)pos * C;
    if (!BWD && off < 0) {
      for (int c = 0; c < C; ++c) o[c] = 0.f;
      continue;
    }
    // what comes in front of the channel mean / behind it
    auto load = [&](int c) -> float { return off < 0 ? 0.f : xn[off + (int64_t)c * a.xs[4]]; };
    auto pre = [&](float t) -> float { return BWD ? (con ? sc * t + (1.f - sc) * M : t) : (bright ? t + bo : t); };
    float v[CT ? CT : 1];
    if (CT) {
#pragma unroll
      for (int c = 0; c < CT; ++c) v[c] = pre(load(c));
    }
    float m = 0.f;
    if (sat) {
      if (CT) {
#pragma unroll
        for (int c = 0; c < CT; ++c) m += v[c];
      } else {
        for (int c = 0; c < C; ++c) m += pre(load(c));
      }
      m *= inv_c;
    }
#pragma unroll
    for (int c = 0; c < C; ++c) {
      float t = CT ? v[CT ? c : 0] : pre(load(c));
      if (sat) t = BWD ? ss * t + (1.f - ss) * m : (t - m) * ss + m;
      if (!BWD && con) t = (t - M) * sc + M;
      o[c] = t;
    }
  }
}

extern "C" int32_t gode_diffaug_chunks(int32_t D, int32_t H, int32_t W) {
  if (D < 1 || H < 1 || W < 1) return 0;
  const int64_t S = (int64_t)D * H * W;
  const int64_t P = (S + DA_CHUNK_MIN - 1) / DA_CHUNK_MIN;
  return (int32_t)(P > DA_CHUNKS_MAX ? DA_CHUNKS_MAX : P);
}

extern "C" int64_t gode_diffaug_work_size(int32_t N, int32_t D, int32_t H, int32_t W, int32_t mask) {
  if (N < 1 || !(mask & 4)) return 0;
  return 2 * (int64_t)N * gode_diffaug_chunks(D, H, W);              // floats: one double per (sample, chunk)
}

extern "C" int gode_diffaug_params(int32_t* ints, float* unis, int64_t n, uint64_t seed, uint32_t stream, uint32_t call,
                                   int64_t g0, int32_t H, int32_t W) {
  if (!ints || !unis || n < 0 || stream >= (1u << 21) || g0 < 0 || H < 1 || W < 1) return GODE_E_ARG;
  for (int64_t i = 0; i < n; ++i) {
    const DaParams p = da_params((uint32_t)seed, (uint32_t)(seed >> 32), stream, call, (uint64_t)g0 + (uint64_t)i, H, W);
    ints[4 * i + 0] = p.tx; ints[4 * i + 1] = p.ty; ints[4 * i + 2] = p.cx; ints[4 * i + 3] = p.cy;
    unis[3 * i + 0] = p.ub; unis[3 * i + 1] = p.us; unis[3 * i + 2] = p.uc;
  }
  return 0;
}

template <bool BWD>
static int da_launch(const gode_diffaug_op* op, const DaArgs& A, int grid, hipStream_t st) {
  if (op->mask & 4) {
    hipLaunchKernelGGL(diffaug_sum_kernel<BWD>, dim3(grid), dim3(DA_THREADS), 0, st, *op, A);
    GODE_LAUNCH_CHECK();
  }
  if (op->C == 1) hipLaunchKernelGGL((diffaug_apply_kernel<BWD, 1>), dim3(grid), dim3(DA_THREADS), 0, st, *op, A);
  else if (op->C == 3) hipLaunchKernelGGL((diffaug_apply_kernel<BWD, 3>), dim3(grid), dim3(DA_THREADS), 0, st, *op, A);
  else hipLaunchKernelGGL((diffaug_apply_kernel<BWD, 0>), dim3(grid), dim3(DA_THREADS), 0, st, *op, A);
  GODE_LAUNCH_CHECK();
  return 0;
}

extern "C" int gode_diffaug(const gode_diffaug_op* op, void* stream) {
  if (!op || !op->x || !op->out || op->N < 1 || op->C < 1 || op->D < 1 || op->H < 1 || op->W < 1 || op->mask < 1 ||
      op->mask > 31 || (op->backward != 0 && op->backward != 1) || op->stream < 0 || op->stream >= (1 << 21) || op->g0 < 0)
    return GODE_E_ARG;
  if ((op->mask & 4) && (!op->work || ((uintptr_t)op->work % 8) != 0)) return GODE_E_ARG;
  const int64_t S = (int64_t)op->D * op->H * op->W;
  const int32_t P = gode_diffaug_chunks(op->D, op->H, op->W);
  if (S * op->C >= (1ll << 31) || (int64_t)op->N * P >= (1ll << 31)) return GODE_E_SHAPE;
  DaArgs A;
  A.dHW = make_fastdiv((uint32_t)(op->H * op->W)); A.dW = make_fastdiv((uint32_t)op->W);
  A.k0 = (uint32_t)(uint64_t)op->seed; A.k1 = (uint32_t)((uint64_t)op->seed >> 32);
  A.S = (uint32_t)S; A.P = P; A.chunk = (uint32_t)((S + P - 1) / P);
  const int grid = (int)((int64_t)op->N * P);
  return op->backward ? da_launch<true>(op, A, grid, (hipStream_t)stream) : da_launch<false>(op, A, grid, (hipStream_t)stream);
}
