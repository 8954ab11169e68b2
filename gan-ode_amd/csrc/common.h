// common.h -- launch helpers shared by the HIP translation units of libgode.so
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/gode.h"

#define GODE_LAUNCH_CHECK()                         \
  do {                                              \
    hipError_t e__ = hipGetLastError();             \
    if (e__ != hipSuccess) return (int)e__;         \
  } while (0)

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

// slope of the activation on the negative side (1: the identity); act(t) == fmaxf(t, t * slope), the slopes lie in [0, 1]
__host__ __device__ __forceinline__ float gode_act_neg_slope(int act) {
  return act == GODE_ACT_RELU ? 0.f : (act == GODE_ACT_LRELU ? 0.2f : (act == GODE_ACT_LRELU01 ? 0.1f : 1.f));
}
__device__ __forceinline__ float gode_act(float v, int act) {
  if (act == GODE_ACT_RELU) return v > 0.f ? v : 0.f;
  if (act == GODE_ACT_LRELU) return v > 0.f ? v : 0.2f * v;
  if (act == GODE_ACT_LRELU01) return v > 0.f ? v : 0.1f * v;
  return v;
}
// derivative of act evaluated at pre-activation z
__device__ __forceinline__ float gode_act_grad(float z, int act) {
  if (act == GODE_ACT_RELU) return z > 0.f ? 1.f : 0.f;
  if (act == GODE_ACT_LRELU) return z > 0.f ? 1.f : 0.2f;
  if (act == GODE_ACT_LRELU01) return z > 0.f ? 1.f : 0.1f;
  return 1.f;
}

// Raw-buffer view of an operand for the LDS-DMA loads (the resource type and its builtins exist in the device pass only; the
// host pass, which only needs the kernel's launch stub, sees empty shells).
struct BufRsrc {
#if defined(__HIP_DEVICE_COMPILE__)
  __amdgpu_buffer_rsrc_t r;
#endif
};
__device__ __forceinline__ BufRsrc make_buf_rsrc(const float* p, uint32_t bytes) {
  BufRsrc b;
#if defined(__HIP_DEVICE_COMPILE__)
  b.r = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p), 0, (int)bytes, 0x00020000);   // raw buffer, 32-bit words
#else
  (void)p; (void)bytes;
#endif
  return b;
}
// 16 bytes per lane, memory[voff + soff] -> LDS[lds + 16 * lane]: voff per lane (VGPR), soff wave-uniform (SGPR); a voff beyond
// the buffer's extent delivers zeros
__device__ __forceinline__ void buf_dma16(const BufRsrc& b, float* lds, int voff, int soff) {
#if defined(__HIP_DEVICE_COMPILE__)
  __builtin_amdgcn_raw_ptr_buffer_load_lds(b.r, (__attribute__((address_space(3))) void*)lds, 16, voff, soff, 0, 0);
#else
  (void)b; (void)lds; (void)voff; (void)soff;
#endif
}

// Division by a run-time invariant (Granlund-Montgomery, branch-free, exact for all 32-bit n): the host builds the
// magic once per launch, the kernels pay a v_mul_hi + 3 ALU ops instead of a ~30-instruction software divide.
struct FastDiv { uint32_t mul, sh1, sh2, d; };
static inline FastDiv make_fastdiv(uint32_t d) {
  FastDiv f; f.d = d;
  uint32_t l = 0; while ((1ull << l) < d) ++l;
  f.mul = (uint32_t)((((1ull << 32) * ((1ull << l) - d)) / d) + 1);
  f.sh1 = l < 1 ? l : 1; f.sh2 = l > 0 ? l - 1 : 0;
  return f;
}
__device__ __forceinline__ uint32_t fdiv(uint32_t n, const FastDiv& f) {
  const uint32_t t = __umulhi(f.mul, n);
  return (t + ((n - t) >> f.sh1)) >> f.sh2;
}


// ---- fixed-order sums of per-workgroup gradient rows (latent_reduce.hip) ---------------------------------------------
// grads[k - grads_bias] (+)= sum over the nblk rows of work[.][nparam], k in [first, nparam), rows in order.  More than
// chunk_threshold rows: chunks of `chunk` consecutive rows are first summed in place into their first row, then every
// chunk-th row is added (both levels in row order).  counts != NULL: nothing is touched when counts[0] < 0.  ld != 0: the rows
// are ld >= nparam floats apart (columns from nparam on are then neither read nor written).
int gode_reduce_rows(float* work, float* grads, int nblk, int nparam, int first, int grads_bias, int accumulate,
                     const int32_t* counts, int chunk_threshold, int chunk, hipStream_t st, int ld = 0);

// Multi-solve launches (up to GODE_MAX_JOBS ops): the ops that share a grads pointer form a group, in array order.
#define GODE_MAX_JOBS 8
struct RowsArgs {
  const float* work[GODE_MAX_JOBS]; int32_t rows[GODE_MAX_JOBS]; int32_t accumulate[GODE_MAX_JOBS];
  int32_t count, nparam, first; float* grads;
};
// grads[k] (+)= all rows of the group in order, k in [first, nparam), under the FIRST op's accumulate flag (the later ops of
// a group add by construction)
int gode_launch_rows(const RowsArgs& A, hipStream_t st);
// calls launch(A) once per group with work / rows / accumulate / count / grads filled in; stops at the first non-zero return
template <class Op, class Launch>
static inline int gode_for_each_grads_group(const Op* ops, const int32_t* nblk, int count, Launch launch) {
  bool done[GODE_MAX_JOBS] = {false};
  for (int k = 0; k < count; ++k) {
    if (done[k]) continue;
    RowsArgs A = {};
    A.grads = ops[k].grads;
    for (int j = k; j < count; ++j) {
      if (done[j] || ops[j].grads != A.grads) continue;
      A.work[A.count] = ops[j].work; A.rows[A.count] = nblk[j]; A.accumulate[A.count] = ops[j].accumulate ? 1 : 0;
      A.count += 1; done[j] = true;
    }
    const int rc = launch(A);
    if (rc) return rc;
  }
  return 0;
}
