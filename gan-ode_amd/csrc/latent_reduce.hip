// latent_reduce.hip -- the fixed-order sums of per-workgroup gradient rows that end every motion-latent backward
// (declared in common.h).  No float atomics anywhere: results are bit-identical run to run.
#include "common.h"

// second level: grads[k - grads_bias] (+)= sum over the rows b = 0, stride, 2*stride, ... of work[b][k].  Entries below
// `first` are not touched (no pre-net: that block of grads is then not the caller's memory), nor are entries from `nparam`
// on; rows of `work` are `ld` >= nparam floats apart.
__global__ void __launch_bounds__(256) latent_reduce_kernel(const float* work, float* grads, int nblk, int stride, int nparam, int first,
                                                            int grads_bias, int accumulate, const int32_t* counts, int ld) {
  const int k = first + blockIdx.x * 256 + threadIdx.x;
  if (k >= nparam || (counts && counts[0] < 0)) return;
  float s = 0.f;
  for (int b = 0; b < nblk; b += stride) s += work[(int64_t)b * ld + k];
  grads[k - grads_bias] = accumulate ? grads[k - grads_bias] + s : s;
}
// Many workgroups (N >> 1024): a first level sums chunks of `chunk` consecutive partial rows in parallel, in place (the
// sum of rows [c*chunk, (c+1)*chunk) replaces row c*chunk; a thread only ever touches its own column of its own chunk),
// the kernel above then adds every chunk-th row.  Fixed order at both levels.  (A single level left 11 workgroups
// walking 65,536 rows each: 25 of the 28 ms of the N = 2^20 rk4 adjoint.)
__global__ void __launch_bounds__(256) latent_reduce_chunks_kernel(float* work, int nblk, int chunk, int nparam, int first,
                                                                   const int32_t* counts, int ld) {
  const int k = first + blockIdx.x * 256 + threadIdx.x;
  if (k >= nparam || (counts && counts[0] < 0)) return;
  const int b0 = blockIdx.y * chunk, b1 = b0 + chunk < nblk ? b0 + chunk : nblk;
  float s = 0.f;
#pragma unroll 8
  for (int b = b0; b < b1; ++b) s += work[(int64_t)b * ld + k];
  work[(int64_t)b0 * ld + k] = s;
}

int gode_reduce_rows(float* work, float* grads, int nblk, int nparam, int first, int grads_bias, int accumulate,
                     const int32_t* counts, int chunk_threshold, int chunk, hipStream_t st, int ld) {
  if (ld == 0) ld = nparam;
  const int gx = (nparam - first + 255) / 256;
  int stride = 1;
  if (nblk > chunk_threshold) {
    stride = chunk;
    hipLaunchKernelGGL(latent_reduce_chunks_kernel, dim3(gx, (nblk + stride - 1) / stride), dim3(256), 0, st, work, nblk, stride, nparam,
                       first, counts, ld);
    GODE_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(latent_reduce_kernel, dim3(gx), dim3(256), 0, st, work, grads, nblk, stride, nparam, first, grads_bias, accumulate,
                     counts, ld);
  GODE_LAUNCH_CHECK();
  return 0;
}

// rows of `work` (one per workgroup; the ops of a multi launch that share a grads pointer, in array order) -> grads
__global__ void __launch_bounds__(256) latent_rows_kernel(const RowsArgs A) {
  const int k = A.first + blockIdx.x * 256 + threadIdx.x;
  if (k >= A.nparam) return;
  float s = 0.f;
  for (int j = 0; j < A.count; ++j)
    for (int b = 0; b < A.rows[j]; ++b) s += A.work[j][(int64_t)b * A.nparam + k];
  A.grads[k] = A.accumulate[0] ? A.grads[k] + s : s;
}

int gode_launch_rows(const RowsArgs& A, hipStream_t st) {
  hipLaunchKernelGGL(latent_rows_kernel, dim3((A.nparam - A.first + 255) / 256), dim3(256), 0, st, A);
  GODE_LAUNCH_CHECK();
  return 0;
}
