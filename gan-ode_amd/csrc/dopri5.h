// dopri5.h -- what the adaptive solvers share: the Dormand-Prince tableau (torchdiffeq _DORMAND_PRINCE_SHAMPINE_TABLEAU),
// the scalar rules of the initial step and of the step-size controller, and the weights of the 4th-order interpolant.
// The scalar rules are stated once with the power function as their parameter: FastPow for the VALU kernels
// (odernn_valu.hip, cde_valu.hip), LibmPow for the MFMA kernels (odernn.hip, adj_adaptive.hip) -- which one a kernel uses
// is part of its bits.  The solvers themselves exist once per lane mapping: FwdV / AdjV (odernn_valu.hip), FwdM
// (odernn.hip), AdjSolver (adj_adaptive.hip).
#pragma once

#define DP5_A21 (1.f / 5.f)
#define DP5_A31 (3.f / 40.f)
#define DP5_A32 (9.f / 40.f)
#define DP5_A41 (44.f / 45.f)
#define DP5_A42 (-56.f / 15.f)
#define DP5_A43 (32.f / 9.f)
#define DP5_A51 (19372.f / 6561.f)
#define DP5_A52 (-25360.f / 2187.f)
#define DP5_A53 (64448.f / 6561.f)
#define DP5_A54 (-212.f / 729.f)
#define DP5_A61 (9017.f / 3168.f)
#define DP5_A62 (-355.f / 33.f)
#define DP5_A63 (46732.f / 5247.f)
#define DP5_A64 (49.f / 176.f)
#define DP5_A65 (-5103.f / 18656.f)
// 5th-order solution
#define DP5_B1 (35.f / 384.f)
#define DP5_B3 (500.f / 1113.f)
#define DP5_B4 (125.f / 192.f)
#define DP5_B5 (-2187.f / 6784.f)
#define DP5_B6 (11.f / 84.f)
// error estimate (5th - 4th order)
#define DP5_E1 (35.f / 384.f - 1951.f / 21600.f)
#define DP5_E3 (500.f / 1113.f - 22642.f / 50085.f)
#define DP5_E4 (125.f / 192.f - 451.f / 720.f)
#define DP5_E5 (-2187.f / 6784.f + 12231.f / 42400.f)
#define DP5_E6 (11.f / 84.f - 649.f / 6300.f)
#define DP5_E7 (-1.f / 60.f)
// mid-point of the step (dense output)
#define DP5_C1 (6025192743.f / 30085553152.f / 2.f)
#define DP5_C3 (51252292925.f / 65400821598.f / 2.f)
#define DP5_C4 (-2691868925.f / 45128329728.f / 2.f)
#define DP5_C5 (187940372067.f / 1594534317056.f / 2.f)
#define DP5_C6 (-1776094331.f / 19743644256.f / 2.f)
#define DP5_C7 (11237099.f / 235043384.f / 2.f)

// x^p through the hardware log2 / exp2 units (1 ulp each): the step-size controller needs 3-4 digits
__device__ __forceinline__ float fast_pow(float x, float p) { return __builtin_amdgcn_exp2f(p * __builtin_amdgcn_logf(x)); }

struct FastPow { __device__ __forceinline__ float operator()(float x, float p) const { return fast_pow(x, p); } };
struct LibmPow { __device__ __forceinline__ float operator()(float x, float p) const { return powf(x, p); } };

// torchdiffeq _select_initial_step (order 4), its scalar part.  d0, d1: norms of y0 / scale and f0 / scale;
// d2: norm of (f(y0 + h0 f0) - f0) / scale, divided by h0.
__device__ __forceinline__ float initial_h0(float d0, float d1) { return (d0 < 1e-5f || d1 < 1e-5f) ? 1e-6f : 0.01f * d0 / d1; }
template <class Pow = FastPow>
__device__ __forceinline__ float initial_step(float h0, float d1, float d2) {
  const float h1 = (d1 <= 1e-15f && d2 <= 1e-15f) ? fmaxf(1e-6f, h0 * 1e-3f) : Pow()(0.01f / fmaxf(d1, d2), 0.2f);
  return fminf(100.f * h0, h1);
}
// torchdiffeq _optimal_step_size (order 5): safety 0.9, ifactor 10, dfactor 0.2; a step with ratio < 1 never shrinks
template <class Pow = FastPow>
__device__ __forceinline__ float step_factor(float ratio) {
  if (ratio == 0.f) return 10.f;
  const float f = 0.9f * Pow()(ratio, -0.2f);
  return fminf(10.f, fmaxf(f, ratio < 1.f ? 1.f : 0.2f));
}
// weights of the 4th-order interpolant (torchdiffeq _interp_fit / _interp_eval) at abscissa x:
//   y(x) = y0 + wS (y1 - y0) + wM (ymid - y0) + dt (w1 f0 + w7 f1)
__device__ __forceinline__ void interp_weights(float x, float& wS, float& wM, float& w1c, float& w7c) {
  const float x2 = x * x, x3 = x2 * x, x4 = x3 * x;
  wS = -8.f * x4 + 14.f * x3 - 5.f * x2;
  wM = 16.f * x4 - 32.f * x3 + 16.f * x2;
  w1c = -2.f * x4 + 5.f * x3 - 4.f * x2 + x;
  w7c = 2.f * x4 - 3.f * x3 + x2;
}
