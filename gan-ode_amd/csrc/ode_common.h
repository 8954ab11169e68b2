// ode_common.h -- device helpers shared by the motion-latent kernels: the transposed 16x16 mat-vec batch on
// v_mfma_f32_16x16x4_f32 (see the header comment of ode.hip for the lane mapping), the activations and the per-component
// f32x4 helpers of the error norms (sq4 / abs4 / max4), the layout of the gode_ode_params block and the content broadcast.
#pragma once
#include "common.h"

// parameter block in gode_ode_params order: the layout of `grads` and of a `work` row of gode_ode_bwd, and of the LDS copy
// the VALU kernels stage (valu_common.h:stage_ode_params)
#define OFF_WA 0
#define OFF_BA 1024
#define OFF_WB 1088
#define OFF_BB 2112
#define OFF_W1 2128
#define OFF_B1 2384
#define OFF_W2 2400
#define OFF_B2 2656
static_assert(OFF_B2 + 16 == GODE_ODE_NPARAM, "ODE parameter block");
// ODEFunc block alone (W1, b1, W2, b2): the theta state of the adaptive adjoints
#define TH_W1 0
#define TH_B1 256
#define TH_W2 272
#define TH_B2 528
#define TH_N 544
// gode_odernn_params order: the ODEFunc block, then the GRU cell
#define RO_W1 0
#define RO_B1 256
#define RO_W2 272
#define RO_B2 528
#define RO_WIH 544
#define RO_WHH 1312
#define RO_BIH 2080
#define RO_BHH 2128
static_assert(RO_BHH + 48 == GODE_ODERNN_NPARAM, "ODE-RNN parameter block");

#define MFMA16(a, b, c) __builtin_amdgcn_mfma_f32_16x16x4f32((a), (b), (c), 0, 0, 0)

__device__ __forceinline__ f32x4 ld4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
__device__ __forceinline__ f32x4 zero4() { return f32x4{0.f, 0.f, 0.f, 0.f}; }
__device__ __forceinline__ f32x4 matvec(const f32x4 w, const f32x4 x, f32x4 c) {
#pragma unroll
  for (int r = 0; r < 4; ++r) c = MFMA16(w[r], x[r], c);
  return c;
}
// tanh(x) = 1 - 2/(exp(2x)+1) on the hardware exp/rcp units (v_exp_f32, v_rcp_f32): absolute error ~1e-7, saturates
// correctly at +-inf; libm's tanhf costs ~10x more instructions and dominated the solve (4 tanh per lane per RHS).
__device__ __forceinline__ float fast_tanh(float x) {
  const float t = __expf(2.f * x);
  return 1.f - 2.f * __builtin_amdgcn_rcpf(t + 1.f);
}
__device__ __forceinline__ f32x4 tanh4(const f32x4 u) {
  return f32x4{fast_tanh(u[0]), fast_tanh(u[1]), fast_tanh(u[2]), fast_tanh(u[3])};
}
__device__ __forceinline__ float sq4(const f32x4 v) { return v[0] * v[0] + v[1] * v[1] + v[2] * v[2] + v[3] * v[3]; }
__device__ __forceinline__ f32x4 abs4(const f32x4 v) { return f32x4{fabsf(v[0]), fabsf(v[1]), fabsf(v[2]), fabsf(v[3])}; }
__device__ __forceinline__ f32x4 max4(const f32x4 a, const f32x4 b) {
  return f32x4{fmaxf(a[0], b[0]), fmaxf(a[1], b[1]), fmaxf(a[2], b[2]), fmaxf(a[3], b[3])};
}
__device__ __forceinline__ f32x4 lrelu4(const f32x4 u) {
  f32x4 o;
#pragma unroll
  for (int r = 0; r < 4; ++r) o[r] = u[r] > 0.f ? u[r] : 0.2f * u[r];
  return o;
}
__device__ __forceinline__ f32x4 lrelu_grad4(const f32x4 pre, const f32x4 gr) {
  f32x4 o;
#pragma unroll
  for (int r = 0; r < 4; ++r) o[r] = pre[r] > 0.f ? gr[r] : 0.2f * gr[r];
  return o;
}


#define LDT 20  // LDS row stride (floats) of a 16x16 transpose tile: conflict-free b128 writes / b32 reads

// sum over the 16 trajectories of a wave (lanes sharing g)
__device__ __forceinline__ f32x4 sum_over_samples(f32x4 v) {
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    v[r] += __shfl_xor(v[r], 1);
    v[r] += __shfl_xor(v[r], 2);
    v[r] += __shfl_xor(v[r], 4);
    v[r] += __shfl_xor(v[r], 8);
  }
  return v;
}


__device__ __forceinline__ float fast_sigmoid(float x) { return __builtin_amdgcn_rcpf(1.f + __expf(-x)); }
__device__ __forceinline__ f32x4 sigmoid4(const f32x4 u) {
  return f32x4{fast_sigmoid(u[0]), fast_sigmoid(u[1]), fast_sigmoid(u[2]), fast_sigmoid(u[3])};
}


// content columns 16..65 (the same 50 values on every row of a trajectory) + zero pad for the `ntraj` trajectories from n0
// on, one float4 per thread and turn; thread `tid` of `nthreads`.  Rows are 200 B in `content`, so the four values are
// gathered one by one (L1-resident).  Stores only: nothing in the caller waits for them.
__device__ __forceinline__ void broadcast_content(const float* content, float* z, const int32_t* sel_t, int N, int T, int zcols,
                                                  int n0, int ntraj, int tid, int nthreads) {
  const int rows_per = sel_t ? 1 : T;
  const int q4 = (zcols - 16) >> 2;      // float4 chunks of content + pad per latent row
  const int total4 = ntraj * rows_per * q4;
  for (int k = tid; k < total4; k += nthreads) {
    const int rr = k / q4, q = k - rr * q4;
    const int ns = rr / rows_per, tt = rr - ns * rows_per;
    if (n0 + ns < N) {
      const float* c = content + (int64_t)(n0 + ns) * 50 + 4 * q;
      f32x4 v = zero4();
      if (q < 12) v = f32x4{c[0], c[1], c[2], c[3]};
      else if (q == 12) v = f32x4{c[0], c[1], 0.f, 0.f};
      *reinterpret_cast<f32x4*>(z + ((int64_t)(n0 + ns) * rows_per + tt) * zcols + 16 + 4 * q) = v;
    }
  }
}
