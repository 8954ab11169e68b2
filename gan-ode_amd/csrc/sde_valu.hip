// sde_valu.hip -- the Neural-SDE motion latent (models/mocogan_sde.py: sdeint_adjoint(SDEFunc, x, linspace(0, 1, T),
// method='euler', dt=2.5e-2); Ito, diagonal noise) and the exact gradient of its discrete forward.
//
// Mapping: that of ode_valu.hip -- one lane = one (trajectory, feature) pair, the 16 features of a trajectory in one DPP
// row, 16 trajectories per 256-thread workgroup, the 16x16 mat-vecs as mv16 over row rotations, all parameters staged in
// LDS once and the per-lane weight arrangements gathered from there.
//
// Forward, per Euler-Maruyama step k (schedule dt[k], sqrt_dt[k] from the host, torchsde's fixed-step loop in fp32):
//   y_{k+1} = y_k + dt_k f(y_k) + g(y_k) * sqrt_dt_k * xi_k,   f = Wf2 tanh(Wf1 y + bf1) + bf2,  g likewise with Wg*.
// Output j >= 1 is produced after step emit_at[j] as w0[j] y_k + w1[j] y_{k+1} (torchsde's linear_interp); output 0 is
// the pre-net output.  Every state is stored ([N][S+1][16]) for the backward.
//
// Backward (discretise-then-optimise, not torchsde's continuous adjoint): with a_k = dL/dy_k,
//   a_k = a_{k+1} + dt_k Jf^T a_{k+1} + Jg^T (a_{k+1} * dW_k)  + the interpolation weights' share of the upstream gradient,
// and the drift / diffusion parameter gradients accumulated per lane along the way (outer16), reduced over the
// trajectories of a workgroup once at the end, then over the workgroups in fixed order.  Bitwise deterministic.
#include "common.h"
#include "ode_common.h"
#include "valu_common.h"

// parameter block (gode_sde_params order; also the layout of `grads` with the pre-net): the pre-net's four tensors sit
// where gode_ode_params has them (prenet_fwd reads them there)
#define SP_WA OFF_WA
#define SP_BA OFF_BA
#define SP_WB OFF_WB
#define SP_BB OFF_BB
#define SP_WF1 2128
#define SP_BF1 2384
#define SP_WF2 2400
#define SP_BF2 2656
#define SP_WG1 2672
#define SP_BG1 2928
#define SP_WG2 2944
#define SP_BG2 3200
static_assert(SP_BG2 + 16 == GODE_SDE_NPARAM, "SDE parameter block");

__device__ __forceinline__ void sde_stage_params(const gode_sde_params& p, int prenet, float* lds) {
  const int t = threadIdx.x;
  if (prenet) {
    for (int k = t; k < 1024; k += 256) { lds[SP_WA + k] = p.Wa[k]; lds[SP_WB + k] = p.Wb[k]; }
    if (t < 64) lds[SP_BA + t] = p.ba[t];
    if (t < 16) lds[SP_BB + t] = p.bb[t];
  }
  lds[SP_WF1 + t] = p.Wf1[t];
  lds[SP_WF2 + t] = p.Wf2[t];
  lds[SP_WG1 + t] = p.Wg1[t];
  lds[SP_WG2 + t] = p.Wg2[t];
  if (t < 16) { lds[SP_BF1 + t] = p.bf1[t]; lds[SP_BF2 + t] = p.bf2[t]; lds[SP_BG1 + t] = p.bg1[t]; lds[SP_BG2 + t] = p.bg2[t]; }
  __syncthreads();
}

__global__ void __launch_bounds__(256) sde_fwd_kernel(const gode_sde_fwd_op a) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = lane & 15, tl = lane >> 4;
  const int n0 = blockIdx.x * 16, n = n0 + wave * 4 + tl;
  const bool valid = n < a.N;
  const int T = a.T, S = a.S;
  const int64_t xi_stride = (int64_t)a.N * 16;           // x = [1 + S][N][16]: x0, then xi_0 .. xi_{S-1}
  __shared__ float P[GODE_SDE_NPARAM];
  float y = valid ? a.x[(int64_t)n * 16 + i] : 0.f;
  sde_stage_params(a.p, a.prenet, P);
  if (a.content) broadcast_content(a.content, a.z, a.sel_t, a.N, T, a.zcols, n0, 16, threadIdx.x, 256);

  int src[16];
  probe_sources(i, src);
  if (a.prenet) y = prenet_fwd(P, y, i, src);
  W16 wf1, wf2, wg1, wg2;
  load_rows(wf1, P + SP_WF1, 16, 0, 0, i, src);
  load_rows(wf2, P + SP_WF2, 16, 0, 0, i, src);
  load_rows(wg1, P + SP_WG1, 16, 0, 0, i, src);
  load_rows(wg2, P + SP_WG2, 16, 0, 0, i, src);
  const float bf1 = P[SP_BF1 + i], bf2 = P[SP_BF2 + i], bg1 = P[SP_BG1 + i], bg2 = P[SP_BG2 + i];

  const int tsel = (a.sel_t && valid) ? a.sel_t[n] : -1;
  auto emit = [&](int t, float v) {
    if (!valid) return;
    if (a.sel_t == nullptr) a.z[((int64_t)n * T + t) * a.zcols + i] = v;
    else if (t == tsel) a.z[(int64_t)n * a.zcols + i] = v;
  };
  float* st = (a.states && valid) ? a.states + (int64_t)n * (S + 1) * 16 + i : nullptr;
  if (st) st[0] = y;
  emit(0, y);
  const float* xi = a.x + xi_stride + (int64_t)n * 16 + i;
  // the noise of the NEXT step is requested before the arithmetic of the current one
  float xn = (valid && S > 0) ? xi[0] : 0.f;
  int jo = 1;
  for (int k = 0; k < S; ++k) {
    const float xk = xn;
    if (k + 1 < S) xn = valid ? xi[(int64_t)(k + 1) * xi_stride] : 0.f;
    const float dt = a.dt[k], dw = a.sqrt_dt[k] * xk;
    const float fv = mv16(wf2, fast_tanh(mv16(wf1, y, bf1)), bf2);
    const float gv = mv16(wg2, fast_tanh(mv16(wg1, y, bg1)), bg2);
    const float y1 = y + fv * dt + gv * dw;
    if (st) st[(k + 1) * 16] = y1;
    while (jo < T && a.emit_at[jo] == k) {
      emit(jo, a.emit_w0[jo] * y + a.emit_w1[jo] * y1);
      ++jo;
    }
    y = y1;
  }
}

__global__ void __launch_bounds__(256) sde_bwd_kernel(const gode_sde_bwd_op a) {
  __shared__ float R[4][GODE_SDE_NPARAM];     // per-wave image of the gradient vector (combined once, at the end)
  __shared__ float P[GODE_SDE_NPARAM];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = lane & 15, tl = lane >> 4;
  const int n0 = blockIdx.x * 16, n = n0 + wave * 4 + tl;
  const bool valid = n < a.N;
  const int T = a.T, S = a.S;
  const int64_t xi_stride = (int64_t)a.N * 16;
  float* part = a.work + (int64_t)blockIdx.x * GODE_SDE_NPARAM;
  const float x = (valid && a.prenet) ? a.x[(int64_t)n * 16 + i] : 0.f;   // for the pre-net backward at the end

  sde_stage_params(a.p, a.prenet, P);
  int src[16];
  probe_sources(i, src);
  W16 wf1, wg1, wf1t, wf2t, wg1t, wg2t, gWf1, gWf2, gWg1, gWg2;
  load_rows(wf1, P + SP_WF1, 16, 0, 0, i, src);
  load_rows(wg1, P + SP_WG1, 16, 0, 0, i, src);
  load_cols(wf1t, P + SP_WF1, 16, 0, 0, i, src);
  load_cols(wf2t, P + SP_WF2, 16, 0, 0, i, src);
  load_cols(wg1t, P + SP_WG1, 16, 0, 0, i, src);
  load_cols(wg2t, P + SP_WG2, 16, 0, 0, i, src);
#pragma unroll
  for (int r = 0; r < 16; ++r) { gWf1.w[r] = 0.f; gWf2.w[r] = 0.f; gWg1.w[r] = 0.f; gWg2.w[r] = 0.f; }
  const float bf1 = P[SP_BF1 + i], bg1 = P[SP_BG1 + i];
  float gbf1 = 0.f, gbf2 = 0.f, gbg1 = 0.f, gbg2 = 0.f;

  const int tsel = (a.sel_t && valid) ? a.sel_t[n] : -1;
  auto upstream = [&](int t) -> float {
    if (!valid) return 0.f;
    if (a.sel_t == nullptr) return a.gz[((int64_t)n * T + t) * a.zcols + i];
    return t == tsel ? a.gz[(int64_t)n * a.zcols + i] : 0.f;
  };
  const float* stp = a.states + (int64_t)n * (S + 1) * 16 + i;
  const float* xi = a.x + xi_stride + (int64_t)n * 16 + i;
  float adj = 0.f;
  // outputs still to be folded in: jhi for the w1 share (state emit_at[j] + 1), jlo for the w0 share (state emit_at[j])
  int jhi = T - 1, jlo = T - 1;
  float y_next = (valid && S > 0) ? stp[(S - 1) * 16] : 0.f;
  float xi_next = (valid && S > 0) ? xi[(int64_t)(S - 1) * xi_stride] : 0.f;
  for (int k = S - 1; k >= 0; --k) {
    // adj holds a_{k+1} without the direct share of the outputs at state k+1: add it
    const float y = y_next, xk = xi_next;
    if (k > 0) {
      y_next = valid ? stp[(k - 1) * 16] : 0.f;
      xi_next = valid ? xi[(int64_t)(k - 1) * xi_stride] : 0.f;
    }
    while (jhi >= 1 && a.emit_at[jhi] == k) { adj += a.emit_w1[jhi] * upstream(jhi); --jhi; }
    while (jlo >= 1 && a.emit_at[jlo] == k + 1) { adj += a.emit_w0[jlo] * upstream(jlo); --jlo; }
    const float dt = a.dt[k], dw = a.sqrt_dt[k] * xk;
    const float hf = fast_tanh(mv16(wf1, y, bf1));
    const float hg = fast_tanh(mv16(wg1, y, bg1));
    const float uf = dt * adj, ug = dw * adj;
    const float vf = mv16(wf2t, uf, 0.f) * (1.f - hf * hf);
    const float vg = mv16(wg2t, ug, 0.f) * (1.f - hg * hg);
    gbf2 += uf; gbg2 += ug; gbf1 += vf; gbg1 += vg;
    outer16(gWf2, uf, hf);
    outer16(gWg2, ug, hg);
    outer16(gWf1, vf, y);
    outer16(gWg1, vg, y);
    adj = adj + (mv16(wf1t, vf, 0.f) + mv16(wg1t, vg, 0.f));
  }
  while (jlo >= 1 && a.emit_at[jlo] == 0) { adj += a.emit_w0[jlo] * upstream(jlo); --jlo; }
  adj += upstream(0);

  // ---- reduce over the 4 trajectories of a wave into the wave's LDS image (ode_valu.hip's scheme)
  auto put_matrix = [&](const W16& Gm, int off, int ld, int row0, int col0) {
    float t[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) t[r] = __shfl_xor(Gm.w[r], 16);
#pragma unroll
    for (int r = 0; r < 16; ++r) t[r] += Gm.w[r];
    float u[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) u[r] = __shfl_xor(t[r], 32);
    if (tl == 0) {
#pragma unroll
      for (int r = 0; r < 16; ++r) R[wave][off + (row0 + i) * ld + col0 + src[r]] = t[r] + u[r];
    }
  };
  auto put_vector = [&](float v, int off) {
    v += __shfl_xor(v, 16);
    v += __shfl_xor(v, 32);
    if (tl == 0) R[wave][off + i] = v;
  };
  put_matrix(gWf1, SP_WF1, 16, 0, 0);
  put_matrix(gWf2, SP_WF2, 16, 0, 0);
  put_matrix(gWg1, SP_WG1, 16, 0, 0);
  put_matrix(gWg2, SP_WG2, 16, 0, 0);
  put_vector(gbf1, SP_BF1);
  put_vector(gbf2, SP_BF2);
  put_vector(gbg1, SP_BG1);
  put_vector(gbg2, SP_BG2);

  // ---- pre-net backward; adj = dL/d(pre-net output)
  if (a.prenet) {
    float hpre[4];
    float acc = P[SP_BB + i];
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      W16 wa, wb;
      load_rows(wa, P + SP_WA, 16, 16 * m, 0, i, src);
      load_rows(wb, P + SP_WB, 64, 0, 16 * m, i, src);
      hpre[m] = mv16(wa, x, P[SP_BA + 16 * m + i]);
      acc = mv16(wb, lrelu1(hpre[m]), acc);
    }
    const float g0 = acc > 0.f ? adj : 0.2f * adj;
    put_vector(g0, SP_BB);
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      W16 G, wbt;
#pragma unroll
      for (int r = 0; r < 16; ++r) G.w[r] = 0.f;
      outer16(G, g0, lrelu1(hpre[m]));                       // dWb[i][16m + j] = sum g0_i * lrelu(hpre)_j
      put_matrix(G, SP_WB, 64, 0, 16 * m);
      load_cols(wbt, P + SP_WB, 64, 0, 16 * m, i, src);      // (Wb chunk)^T
      const float t = mv16(wbt, g0, 0.f);
      const float gh = hpre[m] > 0.f ? t : 0.2f * t;
      put_vector(gh, SP_BA + 16 * m);
#pragma unroll
      for (int r = 0; r < 16; ++r) G.w[r] = 0.f;
      outer16(G, gh, x);                                     // dWa[16m + i][j] = sum gh_i * x_j
      put_matrix(G, SP_WA, 16, 16 * m, 0);
    }
  }
  __syncthreads();
  // only the present tensors: without the pre-net the row's first 2128 entries are neither written nor read
  const int first = a.prenet ? 0 : SP_WF1;
  for (int k = first + threadIdx.x; k < GODE_SDE_NPARAM; k += 256)
    part[k] = (R[0][k] + R[1][k]) + (R[2][k] + R[3][k]);
}

static bool sde_params_ok(const gode_sde_params& p, int prenet) {
  if (!p.Wf1 || !p.bf1 || !p.Wf2 || !p.bf2 || !p.Wg1 || !p.bg1 || !p.Wg2 || !p.bg2) return false;
  return !prenet || (p.Wa && p.ba && p.Wb && p.bb);
}

extern "C" int64_t gode_sde_bwd_work_size(int32_t N) { return N > 0 ? (int64_t)((N + 15) / 16) * GODE_SDE_NPARAM : 0; }

extern "C" int gode_sde_fwd(const gode_sde_fwd_op* op, void* stream) {
  if (!op || !op->x || !op->z || op->N <= 0 || op->T < 1 || op->S < 0) return GODE_E_ARG;
  if (op->S > 0 && (!op->dt || !op->sqrt_dt)) return GODE_E_ARG;
  if (op->T > 1 && (!op->emit_at || !op->emit_w0 || !op->emit_w1)) return GODE_E_ARG;
  if (op->zcols < 16 || op->zcols % 4 != 0 || (op->content && op->zcols < 68)) return GODE_E_ARG;
  if (op->prenet != 0 && op->prenet != 1) return GODE_E_ARG;
  if (!sde_params_ok(op->p, op->prenet)) return GODE_E_ARG;
  hipLaunchKernelGGL(sde_fwd_kernel, dim3((op->N + 15) / 16), dim3(256), 0, (hipStream_t)stream, *op);
  GODE_LAUNCH_CHECK();
  return 0;
}

extern "C" int gode_sde_bwd(const gode_sde_bwd_op* op, void* stream) {
  if (!op || !op->x || !op->states || !op->gz || !op->work || !op->grads || op->N <= 0 || op->T < 1 || op->S < 0)
    return GODE_E_ARG;
  if (op->S > 0 && (!op->dt || !op->sqrt_dt)) return GODE_E_ARG;
  if (op->T > 1 && (!op->emit_at || !op->emit_w0 || !op->emit_w1)) return GODE_E_ARG;
  if (op->zcols < 16 || op->zcols % 4 != 0) return GODE_E_ARG;
  if (op->prenet != 0 && op->prenet != 1) return GODE_E_ARG;
  if (!sde_params_ok(op->p, op->prenet)) return GODE_E_ARG;
  hipStream_t st = (hipStream_t)stream;
  const int nblk = (op->N + 15) / 16;
  hipLaunchKernelGGL(sde_bwd_kernel, dim3(nblk), dim3(256), 0, st, *op);
  GODE_LAUNCH_CHECK();
  // without the pre-net `grads` holds the drift / diffusion block only; two levels above 128 rows
  const int first = op->prenet ? 0 : SP_WF1;
  return gode_reduce_rows(op->work, op->grads, nblk, GODE_SDE_NPARAM, first, first, op->accumulate, nullptr, 128, 64, st);
}
