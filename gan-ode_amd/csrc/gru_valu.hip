// gru_valu.hip -- the MoCoGAN GRU motion latent (models/mocogan.py:217-229) on the VECTOR ALU with DPP row rotations.
//
//   h_0 ~ N(0,1);  for t < T:  h_{t+1} = GRUCell(e_t, h_t),  e_t ~ N(0,1);  latent row t = h_{t+1}  (h_0 is not emitted).
//   GRUCell (torch, gate order r, z, n):  r = s(Wir e + bir + Whr h + bhr),  z = s(Wiz e + biz + Whz h + bhz),
//                                         n = tanh(Win e + bin + r (Whn h + bhn)),  h' = (1 - z) n + z h.
//
// Mapping: the one of ode_valu.hip / odernn_valu.hip -- one lane per (trajectory, feature), the 16 features of a
// trajectory in one DPP row, 4 trajectories per wave, the 16x16 mat-vecs on mv16 (valu_common.h) with the weight rows
// staged in LDS and gathered into registers in the order the rotations deliver the operand.  The trajectories never
// interact, so the forward is one wave per workgroup (4 trajectories; N = 32 spreads over 8 CUs).  Per step the input
// projections Wih e_t + bih do not depend on h and are formed one step ahead, off the dependent chain, which is then
// three independent Whh mat-vecs (4 accumulators each) plus the gate math.
//
// Backward (BPTT): 8 waves per workgroup (32 trajectories).  The gates are recomputed from the stored h_t and e_t -- they
// do not depend on the incoming gradient, so only the three transposed Whh mat-vecs sit on the reverse chain.  The
// weight-gradient outer products are summed over a wave's 4 trajectories by one v_mfma_f32_16x16x4_f32 per matrix and
// step (the per-lane values are the A / B operands for k = trajectory), accumulating over time in registers; the waves
// meet in LDS (wave order), the workgroups through one row of `work` each, added in row order by gru_bwd_rows_kernel:
// every sum has a fixed order, so results are bit-identical run to run for any N.
#include "valu_common.h"
#include "ode_common.h"

#define GF_TRAJ 4                    // forward: one wave, 4 trajectories per workgroup
#define GB_WAVES 8                   // backward: 8 waves, 32 trajectories per workgroup
#define GB_TRAJ (4 * GB_WAVES)
#define GB_THREADS (64 * GB_WAVES)
#define GR_MAX_JOBS GODE_MAX_JOBS
// parameter block == gradient block: Wih [48][16], Whh [48][16], bih [48], bhh [48]
#define GO_WIH 0
#define GO_WHH 768
#define GO_BIH 1536
#define GO_BHH 1584
#define GO_N GODE_GRU_NPARAM

__device__ __forceinline__ void stage_gru_params(const gode_gru_params& p, float* P, int nthreads) {
  for (int k = threadIdx.x; k < 768; k += nthreads) { P[GO_WIH + k] = p.Wih[k]; P[GO_WHH + k] = p.Whh[k]; }
  for (int k = threadIdx.x; k < 48; k += nthreads) { P[GO_BIH + k] = p.bih[k]; P[GO_BHH + k] = p.bhh[k]; }
  __syncthreads();
}

// ---- forward ----------------------------------------------------------------------------------------------------------
struct GruFwdJobs { gode_gru_fwd_op op[GR_MAX_JOBS]; int32_t nblk[GR_MAX_JOBS]; int32_t count; };

__global__ void __launch_bounds__(64) gru_fwd_kernel(const GruFwdJobs J) {
  __shared__ float P[GO_N];
  int job = 0, wg = blockIdx.x;
  while (job + 1 < J.count && wg >= J.nblk[job]) { wg -= J.nblk[job]; ++job; }
  const gode_gru_fwd_op& a = J.op[job];
  const int lane = threadIdx.x, i = lane & 15, tl = lane >> 4;
  const int N = a.N, T = a.T, zcols = a.zcols;
  const int n0 = wg * GF_TRAJ, n = n0 + tl;
  const bool valid = n < N;
  const float* noise = a.noise;
  // the first two noise rows are requested before the staging barrier
  float h = valid ? noise[(int64_t)n * 16 + i] : 0.f;
  float e = valid ? noise[((int64_t)N + n) * 16 + i] : 0.f;
  stage_gru_params(a.p, P, 64);
  if (a.content) broadcast_content(a.content, a.z, a.sel_t, N, T, zcols, n0, GF_TRAJ, lane, 64);      // stores only
  int src[16];
  probe_sources(i, src);
  W16 wih[3], whh[3];
  float bih[3], bhh[3];
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    load_rows(wih[q], P + GO_WIH, 16, 16 * q, 0, i, src);
    load_rows(whh[q], P + GO_WHH, 16, 16 * q, 0, i, src);
    bih[q] = P[GO_BIH + 16 * q + i];
    bhh[q] = P[GO_BHH + 16 * q + i];
  }
  const int tsel = (a.sel_t && valid) ? a.sel_t[n] : -1;
  float* hs = a.hs;
  if (valid && hs) hs[(int64_t)n * (T + 1) * 16 + i] = h;
  float gi0 = mv16(wih[0], e, bih[0]), gi1 = mv16(wih[1], e, bih[1]), gi2 = mv16(wih[2], e, bih[2]);
  for (int t = 0; t < T; ++t) {
    const float en = (valid && t + 1 < T) ? noise[((int64_t)(t + 2) * N + n) * 16 + i] : 0.f;
    const float hr = mv16(whh[0], h, bhh[0]);
    const float hz = mv16(whh[1], h, bhh[1]);
    const float hn = mv16(whh[2], h, bhh[2]);
    const float r = fast_sigmoid(gi0 + hr);
    const float zg = fast_sigmoid(gi1 + hz);
    const float nn = fast_tanh(gi2 + r * hn);
    h = (1.f - zg) * nn + zg * h;
    if (valid) {
      if (hs) hs[((int64_t)n * (T + 1) + t + 1) * 16 + i] = h;
      if (a.sel_t == nullptr) a.z[((int64_t)n * T + t) * zcols + i] = h;
      else if (t == tsel) a.z[(int64_t)n * zcols + i] = h;
    }
    if (t + 1 < T) {   // next step's input projections: independent of h, issued under this step's chain
      gi0 = mv16(wih[0], en, bih[0]); gi1 = mv16(wih[1], en, bih[1]); gi2 = mv16(wih[2], en, bih[2]);
    }
  }
}

static bool gru_fwd_args_ok(const gode_gru_fwd_op* op) {
  if (!op || !op->noise || !op->z || op->N <= 0 || op->T < 1) return false;
  if (!op->p.Wih || !op->p.Whh || !op->p.bih || !op->p.bhh) return false;
  if (op->content) return op->zcols >= 68 && op->zcols % 4 == 0;
  return op->zcols >= 16;
}

extern "C" int gode_gru_fwd_multi(const gode_gru_fwd_op* ops, int32_t count, void* stream) {
  if (!ops || count < 1 || count > GR_MAX_JOBS) return GODE_E_ARG;
  GruFwdJobs J;
  J.count = count;
  int grid = 0;
  for (int k = 0; k < count; ++k) {
    if (!gru_fwd_args_ok(&ops[k])) return GODE_E_ARG;
    J.op[k] = ops[k];
    J.nblk[k] = (ops[k].N + GF_TRAJ - 1) / GF_TRAJ;
    grid += J.nblk[k];
  }
  hipLaunchKernelGGL(gru_fwd_kernel, dim3(grid), dim3(64), 0, (hipStream_t)stream, J);
  GODE_LAUNCH_CHECK();
  return 0;
}

extern "C" int gode_gru_fwd(const gode_gru_fwd_op* op, void* stream) { return gode_gru_fwd_multi(op, 1, stream); }

// ---- backward (BPTT) --------------------------------------------------------------------------------------------------
struct GruBwdJobs { gode_gru_bwd_op op[GR_MAX_JOBS]; int32_t nblk[GR_MAX_JOBS]; int32_t count, direct; };

__global__ void __launch_bounds__(GB_THREADS) gru_bwd_kernel(const GruBwdJobs J) {
  __shared__ float P[GO_N];
  __shared__ float img[GB_WAVES][GO_N];       // per-wave gradient images, in the output order
  int job = 0, wg = blockIdx.x;
  while (job + 1 < J.count && wg >= J.nblk[job]) { wg -= J.nblk[job]; ++job; }
  const gode_gru_bwd_op& a = J.op[job];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = lane & 15, tl = lane >> 4;
  const int N = a.N, T = a.T, zcols = a.zcols;
  const int n = wg * GB_TRAJ + wave * 4 + tl;
  const bool valid = n < N;
  const int tsel = (a.sel_t && valid) ? a.sel_t[n] : -1;
  auto load_up = [&](int t) -> float {       // dL/dh_{t+1} from the decoder's input gradient
    if (!valid) return 0.f;
    if (a.sel_t == nullptr) return a.gz[((int64_t)n * T + t) * zcols + i];
    return t == tsel ? a.gz[(int64_t)n * zcols + i] : 0.f;
  };
  // this step's inputs are requested one step ahead (dependent HBM round trips otherwise)
  float up_n = load_up(T - 1);
  float e_n = valid ? a.noise[((int64_t)T * N + n) * 16 + i] : 0.f;
  float h_n = valid ? a.hs[((int64_t)n * (T + 1) + (T - 1)) * 16 + i] : 0.f;
  stage_gru_params(a.p, P, GB_THREADS);
  int src[16];
  probe_sources(i, src);
  W16 wih[3], whh[3], whht[3];
  float bih[3], bhh[3];
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    load_rows(wih[q], P + GO_WIH, 16, 16 * q, 0, i, src);
    load_rows(whh[q], P + GO_WHH, 16, 16 * q, 0, i, src);
    load_cols(whht[q], P + GO_WHH, 16, 16 * q, 0, i, src);     // (Whh_q)^T
    bih[q] = P[GO_BIH + 16 * q + i];
    bhh[q] = P[GO_BHH + 16 * q + i];
  }
  f32x4 gWih[3] = {zero4(), zero4(), zero4()}, gWhh[3] = {zero4(), zero4(), zero4()};
  float gb0 = 0.f, gb1 = 0.f, gbi2 = 0.f, gbh2 = 0.f;    // bias sums (gates r and z: d/dbih == d/dbhh)
  float carry = 0.f;                                      // dL/dh_{t+1} through the recurrence
  for (int t = T - 1; t >= 0; --t) {
    const float up = up_n, e = e_n, h = h_n;
    if (t > 0) {
      up_n = load_up(t - 1);
      e_n = valid ? a.noise[((int64_t)t * N + n) * 16 + i] : 0.f;
      h_n = valid ? a.hs[((int64_t)n * (T + 1) + (t - 1)) * 16 + i] : 0.f;
    }
    // gates of step t, recomputed from h_t and e_t (independent of the incoming gradient)
    const float gi0 = mv16(wih[0], e, bih[0]), gi1 = mv16(wih[1], e, bih[1]), gi2 = mv16(wih[2], e, bih[2]);
    const float hr = mv16(whh[0], h, bhh[0]), hz = mv16(whh[1], h, bhh[1]), hn = mv16(whh[2], h, bhh[2]);
    const float r = fast_sigmoid(gi0 + hr);
    const float zg = fast_sigmoid(gi1 + hz);
    const float nn = fast_tanh(gi2 + r * hn);
    const float gh = carry + up;
    const float dn = gh * (1.f - zg) * (1.f - nn * nn);
    const float dz = gh * (h - nn) * zg * (1.f - zg);
    const float dr = dn * hn * r * (1.f - r);
    const float dnh = dn * r;
    const float c0 = mv16(whht[0], dr, gh * zg);
    const float c1 = mv16(whht[1], dz, 0.f);
    const float c2 = mv16(whht[2], dnh, 0.f);
    carry = c0 + (c1 + c2);
    gWih[0] = MFMA16(dr, e, gWih[0]);  gWih[1] = MFMA16(dz, e, gWih[1]);  gWih[2] = MFMA16(dn, e, gWih[2]);
    gWhh[0] = MFMA16(dr, h, gWhh[0]);  gWhh[1] = MFMA16(dz, h, gWhh[1]);  gWhh[2] = MFMA16(dnh, h, gWhh[2]);
    gb0 += dr; gb1 += dz; gbi2 += dn; gbh2 += dnh;
  }
  // ---- the wave's totals (4 trajectories) -> LDS image; MFMA D layout: lane (tl, i) reg r = [4 tl + r][i]
  {
    float* im = img[wave];
#pragma unroll
    for (int q = 0; q < 3; ++q) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        im[GO_WIH + 256 * q + (4 * tl + r) * 16 + i] = gWih[q][r];
        im[GO_WHH + 256 * q + (4 * tl + r) * 16 + i] = gWhh[q][r];
      }
    }
    const float s0 = traj_sum(gb0), s1 = traj_sum(gb1), si2 = traj_sum(gbi2), sh2 = traj_sum(gbh2);
    if (tl == 0) {
      im[GO_BIH + i] = s0;       im[GO_BHH + i] = s0;
      im[GO_BIH + 16 + i] = s1;  im[GO_BHH + 16 + i] = s1;
      im[GO_BIH + 32 + i] = si2; im[GO_BHH + 32 + i] = sh2;
    }
  }
  __syncthreads();
  // ---- workgroup total (wave order) -> grads (a lone workgroup) or this workgroup's row of work
  float* out = J.direct ? a.grads : a.work + (int64_t)wg * GO_N;
  const bool acc = J.direct && a.accumulate;
  for (int k = threadIdx.x; k < GO_N; k += GB_THREADS) {
    float s = img[0][k];
#pragma unroll
    for (int w = 1; w < GB_WAVES; ++w) s += img[w][k];
    out[k] = acc ? out[k] + s : s;
  }
}

// rows of `work` -> grads, fixed order.  A group holds the ops of a launch that share a grads pointer, in array order;
// each op's rows are first summed into its own partial (row order), which is then stored or added under that op's own
// accumulate flag -- the arithmetic of the same ops launched one by one.
__global__ void __launch_bounds__(256) gru_bwd_rows_kernel(const RowsArgs A) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= GO_N) return;
  float v = A.accumulate[0] ? A.grads[k] : 0.f;
  for (int j = 0; j < A.count; ++j) {
    const float* w = A.work[j];
    float s = w[k];
    for (int b = 1; b < A.rows[j]; ++b) s += w[(int64_t)b * GO_N + k];
    v = A.accumulate[j] ? v + s : s;
  }
  A.grads[k] = v;
}

static bool gru_bwd_args_ok(const gode_gru_bwd_op* op) {
  if (!op || !op->noise || !op->hs || !op->gz || !op->work || !op->grads || op->N <= 0 || op->T < 1) return false;
  if (!op->p.Wih || !op->p.Whh || !op->p.bih || !op->p.bhh) return false;
  return op->zcols >= 16;
}

extern "C" int64_t gode_gru_bwd_work_size(int32_t N) { return N > 0 ? (int64_t)((N + GB_TRAJ - 1) / GB_TRAJ) * GO_N : 0; }

extern "C" int gode_gru_bwd_multi(const gode_gru_bwd_op* ops, int32_t count, void* stream) {
  if (!ops || count < 1 || count > GR_MAX_JOBS) return GODE_E_ARG;
  hipStream_t st = (hipStream_t)stream;
  GruBwdJobs J;
  J.count = count;
  int grid = 0;
  for (int k = 0; k < count; ++k) {
    if (!gru_bwd_args_ok(&ops[k])) return GODE_E_ARG;
    J.op[k] = ops[k];
    J.nblk[k] = (ops[k].N + GB_TRAJ - 1) / GB_TRAJ;
    grid += J.nblk[k];
  }
  J.direct = (count == 1 && grid == 1) ? 1 : 0;
  hipLaunchKernelGGL(gru_bwd_kernel, dim3(grid), dim3(GB_THREADS), 0, st, J);
  GODE_LAUNCH_CHECK();
  if (J.direct) return 0;
  return gode_for_each_grads_group(ops, J.nblk, count, [&](const RowsArgs& A) {
    hipLaunchKernelGGL(gru_bwd_rows_kernel, dim3((GO_N + 255) / 256), dim3(256), 0, st, A);
    GODE_LAUNCH_CHECK();
    return 0;
  });
}

extern "C" int gode_gru_bwd(const gode_gru_bwd_op* op, void* stream) { return gode_gru_bwd_multi(op, 1, stream); }
