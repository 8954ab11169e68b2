// odestep.hip -- the parameter updates of ODE-GAN training (stage2/ode_training.py): one Euler / Heun / RK4 stage update of a
// whole network in ONE launch (gode_ode_step), and the parameter shift theta = theta0 + a*v of the gradient penalty's central
// difference with its two norms (gode_axpy_multi).  Both walk a device table of tensors as one concatenated index space.
#include "common.h"

static_assert(sizeof(gode_ode_step_tensor) == 9 * 8, "gode_ode_step_tensor is nine 8-byte words (the host writes int64 rows)");
static_assert(sizeof(gode_axpy_tensor) == 5 * 8, "gode_axpy_tensor is five 8-byte words (the host writes int64 rows)");

// The index space: a tensor is cut into quads of four consecutive floats counted from the 16-byte boundary at or below its
// p pointer, so quad q covers elements [4q - mis, 4q - mis + 4), mis = (p / 4) & 3.  Quads that lie inside the tensor and
// whose other pointers share p's offset within 16 bytes move as one 16-byte load / store; the partial quads at the head
// and the tail, and every quad of a tensor whose pointers disagree, move element by element.  GODE_STEP_QUADS quads (one
// per thread) are a chunk, chunk0 of a record is the number of chunks before it, and the workgroups stride over chunks.
static int64_t step_chunks(const void* p, int64_t n) {
  const int64_t mis = (int64_t)(((uintptr_t)p >> 2) & 3);
  return ((n + mis + 3) / 4 + GODE_STEP_QUADS - 1) / GODE_STEP_QUADS;
}
extern "C" int64_t gode_ode_step_chunks(const void* p, int64_t n) { return p && n > 0 ? step_chunks(p, n) : 0; }

// last record whose chunk0 <= c (chunk0 ascending, table[0].chunk0 == 0); uniform over the workgroup
template <class Rec>
__device__ __forceinline__ int find_record(const Rec* table, int count, int64_t c) {
  int lo = 0, hi = count;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (table[mid].chunk0 <= c) lo = mid; else hi = mid;
  }
  return lo;
}
__device__ __forceinline__ bool same_lane(const void* a, const void* p) { return (((uintptr_t)a ^ (uintptr_t)p) & 15) == 0; }

struct StepArgs { float c[4]; float cq; int terms; };

__device__ __forceinline__ float step_elem(float p, float g0, float g1, float g2, float g3, float qp, float qm, const StepArgs& a,
                                           float cq) {
  float u = 0.f;                       // terms are uniform over the launch: the branches cost nothing
  bool first = true;
  const float g[4] = {g0, g1, g2, g3};
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (a.terms >> k & 1) { u = first ? a.c[k] * g[k] : fmaf(a.c[k], g[k], u); first = false; }
  if (a.terms & 16) { const float d = qp - qm; u = first ? cq * d : fmaf(cq, d, u); }
  return p + u;
}

__global__ void __launch_bounds__(GODE_STEP_QUADS) ode_step_kernel(const gode_ode_step_tensor* table, int count, int64_t chunks,
                                                                   StepArgs a, const float* cq_dev) {
  const float cq = cq_dev ? a.cq * cq_dev[0] : a.cq;
  for (int64_t c = blockIdx.x; c < chunks; c += gridDim.x) {
    const gode_ode_step_tensor r = table[find_record(table, count, c)];
    bool skip = false, vec = true;
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (a.terms >> k & 1) { skip |= r.g[k] == nullptr; vec &= same_lane(r.g[k], r.p); }
    if (a.terms & 16) { skip |= r.qp == nullptr || r.qm == nullptr; vec &= same_lane(r.qp, r.p) && same_lane(r.qm, r.p); }
    if (skip) continue;                // a null gradient: the tensor is left untouched (the reference's `continue`)
    const int64_t mis = (int64_t)(((uintptr_t)r.p >> 2) & 3);
    const int64_t e0 = ((c - r.chunk0) * GODE_STEP_QUADS + threadIdx.x) * 4 - mis;
    if (e0 >= r.n) continue;
    if (vec && e0 >= 0 && e0 + 4 <= r.n) {
      f32x4 p = *reinterpret_cast<const f32x4*>(r.p + e0), g[4], qp = {0.f, 0.f, 0.f, 0.f}, qm = qp;
#pragma unroll
      for (int k = 0; k < 4; ++k) g[k] = (a.terms >> k & 1) ? *reinterpret_cast<const f32x4*>(r.g[k] + e0) : qp;
      if (a.terms & 16) { qp = *reinterpret_cast<const f32x4*>(r.qp + e0); qm = *reinterpret_cast<const f32x4*>(r.qm + e0); }
#pragma unroll
      for (int l = 0; l < 4; ++l) p[l] = step_elem(p[l], g[0][l], g[1][l], g[2][l], g[3][l], qp[l], qm[l], a, cq);
      *reinterpret_cast<f32x4*>(r.p + e0) = p;
    } else {
#pragma unroll
      for (int l = 0; l < 4; ++l) {
        const int64_t e = e0 + l;
        if (e < 0 || e >= r.n) continue;
        float g[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) g[k] = (a.terms >> k & 1) ? r.g[k][e] : 0.f;
        const float qp = (a.terms & 16) ? r.qp[e] : 0.f, qm = (a.terms & 16) ? r.qm[e] : 0.f;
        r.p[e] = step_elem(r.p[e], g[0], g[1], g[2], g[3], qp, qm, a, cq);
      }
    }
  }
}

static int step_blocks(int64_t chunks, int cap) { return (int)(chunks > cap ? cap : chunks); }

extern "C" int gode_ode_step(const gode_ode_step_tensor* table, int32_t count, int64_t chunks, int32_t terms, float c1,
                             float c2, float c3, float c4, float cq, const float* cq_dev, void* stream) {
  if (!table || count <= 0 || chunks <= 0 || terms <= 0 || terms > 31) return GODE_E_ARG;
  StepArgs a = {{c1, c2, c3, c4}, cq, terms};
  hipLaunchKernelGGL(ode_step_kernel, dim3(step_blocks(chunks, 2048)), dim3(GODE_STEP_QUADS), 0, (hipStream_t)stream, table,
                     count, chunks, a, cq_dev);
  GODE_LAUNCH_CHECK();
  return 0;
}

// ---------------------------------------------------------------------------------------------------------------
// p = base + a*v on every tensor, and sum v^2 / sum base^2 over all of them.  Pass 1: every workgroup adds the squares of its
// chunks in double (a product of two floats is exact in double) and reduces them over its 256 threads in a fixed tree; pass 2:
// one workgroup adds the per-workgroup sums in the same fixed order.  The grid is a function of `chunks` alone, so two runs
// give the same bits; no atomics.
__device__ __forceinline__ float axpy_elem(float b, float v, float a) { return a == 0.f ? b : fmaf(a, v, b); }

__device__ __forceinline__ void block_sum2(double& s0, double& s1, double (*sh)[GODE_STEP_QUADS]) {
  const int t = threadIdx.x;
  sh[0][t] = s0; sh[1][t] = s1;
  __syncthreads();
  for (int w = GODE_STEP_QUADS / 2; w > 0; w >>= 1) {
    if (t < w) { sh[0][t] += sh[0][t + w]; sh[1][t] += sh[1][t + w]; }
    __syncthreads();
  }
  s0 = sh[0][0]; s1 = sh[1][0];
}

__global__ void __launch_bounds__(GODE_STEP_QUADS) axpy_multi_kernel(const gode_axpy_tensor* table, int count, int64_t chunks,
                                                                     float a, const float* a_dev, double* work) {
  __shared__ double sh[2][GODE_STEP_QUADS];
  if (a_dev) a *= a_dev[0];
  double sv = 0.0, sb = 0.0;
  for (int64_t c = blockIdx.x; c < chunks; c += gridDim.x) {
    const gode_axpy_tensor r = table[find_record(table, count, c)];
    const bool vec = same_lane(r.base, r.p) && (!r.v || same_lane(r.v, r.p));
    const int64_t mis = (int64_t)(((uintptr_t)r.p >> 2) & 3);
    const int64_t e0 = ((c - r.chunk0) * GODE_STEP_QUADS + threadIdx.x) * 4 - mis;
    if (e0 >= r.n) continue;
    if (vec && e0 >= 0 && e0 + 4 <= r.n) {
      const f32x4 b = *reinterpret_cast<const f32x4*>(r.base + e0);
      f32x4 v = {0.f, 0.f, 0.f, 0.f}, p;
      if (r.v) v = *reinterpret_cast<const f32x4*>(r.v + e0);
#pragma unroll
      for (int l = 0; l < 4; ++l) {
        p[l] = r.v ? axpy_elem(b[l], v[l], a) : b[l];
        sv += (double)v[l] * (double)v[l]; sb += (double)b[l] * (double)b[l];
      }
      *reinterpret_cast<f32x4*>(r.p + e0) = p;
    } else {
#pragma unroll
      for (int l = 0; l < 4; ++l) {
        const int64_t e = e0 + l;
        if (e < 0 || e >= r.n) continue;
        const float b = r.base[e], v = r.v ? r.v[e] : 0.f;
        r.p[e] = r.v ? axpy_elem(b, v, a) : b;
        sv += (double)v * (double)v; sb += (double)b * (double)b;
      }
    }
  }
  block_sum2(sv, sb, sh);
  if (threadIdx.x == 0) { work[2 * blockIdx.x] = sv; work[2 * blockIdx.x + 1] = sb; }
}

__global__ void __launch_bounds__(GODE_STEP_QUADS) axpy_finish_kernel(const double* work, int nblk, double* sums, float h,
                                                                      float* step) {
  __shared__ double sh[2][GODE_STEP_QUADS];
  double sv = 0.0, sb = 0.0;
  for (int i = threadIdx.x; i < nblk; i += GODE_STEP_QUADS) { sv += work[2 * i]; sb += work[2 * i + 1]; }
  block_sum2(sv, sb, sh);
  if (threadIdx.x == 0) {
    sums[0] = sv; sums[1] = sb;
    if (step) {
      const double eps = sv > 0.0 ? (double)h * (1.0 + sqrt(sb)) / sqrt(sv) : 0.0;
      const float e32 = (float)eps;
      step[0] = e32; step[1] = e32 > 0.f ? (float)(1.0 / (double)e32) : 0.f;
    }
  }
}

extern "C" int gode_axpy_multi(const gode_axpy_tensor* table, int32_t count, int64_t chunks, float a, const float* a_dev,
                               double* sums, float h, float* step, double* work, void* stream) {
  if (!table || count <= 0 || chunks <= 0 || !work || (step && !sums)) return GODE_E_ARG;
  const int nblk = step_blocks(chunks, GODE_AXPY_MAX_BLOCKS);
  hipLaunchKernelGGL(axpy_multi_kernel, dim3(nblk), dim3(GODE_STEP_QUADS), 0, (hipStream_t)stream, table, count, chunks, a,
                     a_dev, work);
  GODE_LAUNCH_CHECK();
  if (sums) {
    hipLaunchKernelGGL(axpy_finish_kernel, dim3(1), dim3(GODE_STEP_QUADS), 0, (hipStream_t)stream, work, nblk, sums, h, step);
    GODE_LAUNCH_CHECK();
  }
  return 0;
}
