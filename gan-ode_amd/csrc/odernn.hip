// odernn.hip -- the ODE-RNN motion latent (models/mocogan_ode_rnn.py:41-53):
//   h_0 ~ N(0,1);  per frame:  h' = odeint_adjoint(ODEFunc, h, [0,1])[-1]  (torchdiffeq default: dopri5, rtol 1e-7,
//   atol 1e-9),  h = GRUCell(e_t, h'),  e_t ~ N(0,1);  latent row t = h_{t+1}.
//
// These are the MFMA-chain kernels of rounds 1-2 (16 trajectories per wave, every 16x16 product a chained
// v_mfma_f32_16x16x4_f32 tile as in ode.hip).  Since round 3 the default kernels are odernn_valu.hip (VALU/DPP mapping,
// whole-batch error norm, several solves per launch); what remains in use from this file:
//   * odernn_fwd_kernel: the forward fallback above GODE_ODERNN_SYNC_MAX_N trajectories per launch (error norm per
//     64-trajectory workgroup instead of the whole batch: the one recorded deviation, unused by any configuration);
//   * odernn_bwd_kernel: the adjoint discretised with `substeps` FIXED reverse-time Kutta-3/8 steps per frame
//     (gode_odernn_bwd_op.substeps > 0; 32 steps agree with the adaptive adjoint to ~1e-6) -- an option, not the default:
//     the default (substeps == 0) integrates the adjoint adaptively with torchdiffeq's mixed norm, as odeint_adjoint does;
//   * ode_dopri5_fwd_kernel: dopri5 for the plain Neural-ODE generators (gode_ode_fwd_op.method == 1).
#include "ode_common.h"
#include "dopri5.h"

// trajectories per workgroup of the forward kernel (4 waves): keeps the kernel inside the register file -- a spilling
// build needed scratch memory, whose (re)allocation by the runtime stalled the queue for ~75 ms at a time
#define RNN_BLOCK_SAMPLES 64

// Workgroup sum, every thread gets the total (fixed order).  red[2][...] alternates per call, so ONE barrier per call
// suffices: a wave can write slot set p again only after passing the barrier of the call in between, which every wave
// reaches after its reads of p.
__device__ __forceinline__ float block_sum(float v, float (*red)[RNN_BLOCK_SAMPLES / 16], int nw, int& par) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  if ((threadIdx.x & 63) == 0) red[par][threadIdx.x >> 6] = v;
  __syncthreads();
  float s = 0.f;
  for (int w = 0; w < nw; ++w) s += red[par][w];
  par ^= 1;
  return s;
}

// The forward dopri5 stepper of this mapping (16 trajectories per wave, a lane holds 4 features of one trajectory as an f32x4;
// error norm: RMS over the workgroup's trajectories).  Both forward kernels drive it from their own outer loops (clock, trial
// limit, dense output, stores).  The scalar rules are the shared ones on powf (dopri5.h).
struct FwdM {
  f32x4 w1, w2, b1, b2;
  float rtol, atol, inv_count;       // (set by the kernel: ode_dopri5_fwd_kernel has to pin the tolerances to vector registers)
  int s, g, n, nw, red_par;          // lane = (trajectory s of the wave, feature group g); n: the trajectory; nw: waves
  bool valid;
  float (*red)[RNN_BLOCK_SAMPLES / 16];
  f32x4 y0, f0;                      // the accepted state and f(y0)
  double dtd;                        // step size (fp64, as torchdiffeq keeps it)
  float dt;                          // the last trial step: its size, stage derivatives and 5th-order solution
  f32x4 k3, k4, k5, k6, k7, y1;

  // lane mapping, the workgroup's share of the N trajectories, the ODEFunc weights as MFMA operands
  __device__ __forceinline__ void open(int N, const float* W1, const float* B1, const float* W2, const float* B2, float (*red_)[RNN_BLOCK_SAMPLES / 16]) {
    const int l = threadIdx.x & 63, wv = threadIdx.x >> 6;
    nw = blockDim.x >> 6; s = l & 15; g = l >> 4;
    n = blockIdx.x * RNN_BLOCK_SAMPLES + wv * 16 + s;
    valid = n < N;
    const int nblk = (N - blockIdx.x * RNN_BLOCK_SAMPLES) < RNN_BLOCK_SAMPLES ? (N - blockIdx.x * RNN_BLOCK_SAMPLES) : RNN_BLOCK_SAMPLES;
    inv_count = 1.f / (float)(nblk * 16);
    red = red_; red_par = 0;
    w1 = ld4(W1 + s * 16 + 4 * g); w2 = ld4(W2 + s * 16 + 4 * g);
    b1 = ld4(B1 + 4 * g); b2 = ld4(B2 + 4 * g);
  }
  __device__ __forceinline__ f32x4 f(const f32x4 yy) const { return matvec(w2, tanh4(matvec(w1, yy, b1)), b2); }
  __device__ __forceinline__ float rms(const f32x4 v) { return sqrtf(block_sum(valid ? sq4(v) : 0.f, red, nw, red_par) * inv_count); }
  // start a solve at y: the accepted state and torchdiffeq's _select_initial_step (order 4)
  __device__ __forceinline__ void start(const f32x4 y) {
    y0 = y; f0 = f(y);
    const f32x4 sc = atol + abs4(y0) * rtol;
    const float d0 = rms(y0 / sc), d1 = rms(f0 / sc);
    const float h0 = initial_h0(d0, d1);
    const f32x4 f1 = f(y0 + h0 * f0);
    const float d2 = rms((f1 - f0) / sc) / h0;
    dtd = (double)initial_step<LibmPow>(h0, d1, d2);
  }
  // one trial step of size dtd from the accepted state; returns the error ratio (accept when <= 1)
  __device__ __forceinline__ float trial() {
    dt = (float)dtd;
    const f32x4 k1 = f0;
    const f32x4 k2 = f(y0 + dt * (DP5_A21 * k1));
    k3 = f(y0 + dt * (DP5_A31 * k1 + DP5_A32 * k2));
    k4 = f(y0 + dt * (DP5_A41 * k1 + DP5_A42 * k2 + DP5_A43 * k3));
    k5 = f(y0 + dt * (DP5_A51 * k1 + DP5_A52 * k2 + DP5_A53 * k3 + DP5_A54 * k4));
    k6 = f(y0 + dt * (DP5_A61 * k1 + DP5_A62 * k2 + DP5_A63 * k3 + DP5_A64 * k4 + DP5_A65 * k5));
    y1 = y0 + dt * (DP5_B1 * k1 + DP5_B3 * k3 + DP5_B4 * k4 + DP5_B5 * k5 + DP5_B6 * k6);
    k7 = f(y1);
    const f32x4 err = dt * (DP5_E1 * k1 + DP5_E3 * k3 + DP5_E4 * k4 + DP5_E5 * k5 + DP5_E6 * k6 + DP5_E7 * k7);
    const f32x4 tol = atol + rtol * max4(abs4(y0), abs4(y1));
    return rms(err / tol);
  }
  // the 4th-order interpolant of the last trial (fit through the mid-point): y(x) = y0 + x (cd + x (cc + x (cb + x ca)))
  __device__ __forceinline__ void interp(f32x4& ca, f32x4& cb, f32x4& cc, f32x4& cd) const {
    const f32x4 k1 = f0;
    const f32x4 ymid = y0 + dt * (DP5_C1 * k1 + DP5_C3 * k3 + DP5_C4 * k4 + DP5_C5 * k5 + DP5_C6 * k6 + DP5_C7 * k7);
    ca = 2.f * dt * (k7 - k1) - 8.f * (y1 + y0) + 16.f * ymid;
    cb = dt * (5.f * k1 - 3.f * k7) + 18.f * y0 + 14.f * y1 - 32.f * ymid;
    cc = dt * (k7 - 4.f * k1) - 11.f * y0 - 5.f * y1 + 16.f * ymid;
    cd = dt * k1;
  }
  // the last trial becomes the accepted state
  __device__ __forceinline__ void accept() { y0 = y1; f0 = k7; }
};

__global__ void __launch_bounds__(RNN_BLOCK_SAMPLES * 4) odernn_fwd_kernel(const gode_odernn_fwd_op a) {
  __shared__ float red[2][RNN_BLOCK_SAMPLES / 16];
  FwdM S;
  S.open(a.N, a.p.W1, a.p.b1, a.p.W2, a.p.b2, red);
  S.rtol = a.rtol; S.atol = a.atol;
  const int s = S.s, g = S.g, n = S.n, T = a.T;
  const bool valid = S.valid;
  f32x4 wih[3], whh[3], bih[3], bhh[3];
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    wih[q] = ld4(a.p.Wih + (16 * q + s) * 16 + 4 * g); whh[q] = ld4(a.p.Whh + (16 * q + s) * 16 + 4 * g);
    bih[q] = ld4(a.p.bih + 16 * q + 4 * g); bhh[q] = ld4(a.p.bhh + 16 * q + 4 * g);
  }

  const int tsel = (a.sel_t && valid) ? a.sel_t[n] : -1;
  f32x4 h = valid ? ld4(a.noise + (int64_t)n * 16 + 4 * g) : zero4();
  if (valid && a.hs) *reinterpret_cast<f32x4*>(a.hs + ((int64_t)n * (T + 1)) * 16 + 4 * g) = h;

  for (int t = 0; t < T; ++t) {
    // ---- h' = y(1), y' = f(y), y(0) = h : dopri5 with torchdiffeq's controller
    // the clock and the step size are kept in fp64 (as torchdiffeq keeps them): near the tolerance floor dt can
    // shrink below the fp32 spacing of t, and an fp32 clock would then stop advancing
    S.start(h);
    f32x4 yend = h;
    double tcur = 0.0;
    int steps = 0;
    for (; steps < 100000; ++steps) {
      const float ratio = S.trial();
      if (ratio <= 1.f) {
        if (tcur + S.dtd >= 1.0) {   // dense output at t = 1
          f32x4 ca, cb, cc, cd;
          S.interp(ca, cb, cc, cd);
          const float x = (float)((1.0 - tcur) / S.dtd);
          yend = S.y0 + x * (cd + x * (cc + x * (cb + x * ca)));
          ++steps;
          break;
        }
        tcur += S.dtd; S.accept();
      }
      S.dtd *= (double)step_factor<LibmPow>(ratio);
    }
    if (a.nsteps && threadIdx.x == 0 && blockIdx.x == 0) a.nsteps[t] = steps;
    if (valid && a.hp) *reinterpret_cast<f32x4*>(a.hp + ((int64_t)n * T + t) * 16 + 4 * g) = yend;
    // ---- GRUCell(e_t, h')
    const f32x4 e = valid ? ld4(a.noise + ((int64_t)(t + 1) * a.N + n) * 16 + 4 * g) : zero4();
    const f32x4 r = sigmoid4(matvec(wih[0], e, bih[0]) + matvec(whh[0], yend, bhh[0]));
    const f32x4 zg = sigmoid4(matvec(wih[1], e, bih[1]) + matvec(whh[1], yend, bhh[1]));
    const f32x4 nn = tanh4(matvec(wih[2], e, bih[2]) + r * matvec(whh[2], yend, bhh[2]));
    h = (1.f - zg) * nn + zg * yend;
    if (valid) {
      if (a.hs) *reinterpret_cast<f32x4*>(a.hs + ((int64_t)n * (T + 1) + t + 1) * 16 + 4 * g) = h;
      if (a.sel_t == nullptr) *reinterpret_cast<f32x4*>(a.z + ((int64_t)n * T + t) * a.zcols + 4 * g) = h;
      else if (t == tsel) *reinterpret_cast<f32x4*>(a.z + (int64_t)n * a.zcols + 4 * g) = h;
    }
  }
}

// content columns 16..65 of the latent rows + zero pad (same layout as gode_ode_fwd writes)
__global__ void __launch_bounds__(256) latent_content_kernel(const float* content, float* z, int N, int rows_per, int zcols) {
  const int q4 = (zcols - 16) >> 2;
  const int64_t total4 = (int64_t)N * rows_per * q4;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total4; i += (int64_t)gridDim.x * 256) {
    const int64_t row = i / q4; const int q = (int)(i - row * q4);
    const int64_t nn = row / rows_per;
    f32x4 v = zero4();
    if (q < 12) v = f32x4{content[nn * 50 + 4 * q], content[nn * 50 + 4 * q + 1], content[nn * 50 + 4 * q + 2], content[nn * 50 + 4 * q + 3]};
    else if (q == 12) v = f32x4{content[nn * 50 + 48], content[nn * 50 + 49], 0.f, 0.f};
    *reinterpret_cast<f32x4*>(z + row * zcols + 16 + 4 * q) = v;
  }
}

// ---------------------------------------------------------------------------------------------------------------
// Plain Neural-ODE latent with torchdiffeq's dopri5 (gode_ode_fwd_op.method == 1): pre-net, then ONE adaptive solve over
// the T output times; every output is read off the 4th-order interpolant of the last accepted step, exactly the
// RKAdaptiveStepsizeODESolver flow (advance while target > t1, then evaluate).  Step control, error norm and clock as in
// odernn_fwd_kernel.  The interpolation abscissa is formed from the fp32-rounded times as torchdiffeq does.
__global__ void __launch_bounds__(RNN_BLOCK_SAMPLES * 4) ode_dopri5_fwd_kernel(const gode_ode_fwd_op a) {
  __shared__ float red[2][RNN_BLOCK_SAMPLES / 16];
  FwdM S;
  S.open(a.N, a.p.W1, a.p.b1, a.p.W2, a.p.b2, red);
  const int s = S.s, g = S.g, n = S.n, T = a.T;
  const bool valid = S.valid;
  // tolerances pinned to vector registers: with both in SGPRs hipcc (ROCm 7.2) emits a packed-fp32 VOP3P with two scalar
  // sources for `atol + rtol * max(...)` and the assembler rejects it ("violates constant bus restriction")
  float rtol = a.rtol, atol = a.atol;
  asm volatile("" : "+v"(rtol), "+v"(atol));
  S.rtol = rtol; S.atol = atol;

  f32x4 y0 = valid ? ld4(a.x + n * 16 + 4 * g) : zero4();
  if (a.prenet) {
    f32x4 acc = ld4(a.p.bb + 4 * g);
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      f32x4 hh = matvec(ld4(a.p.Wa + (16 * m + s) * 16 + 4 * g), y0, ld4(a.p.ba + 16 * m + 4 * g));
      acc = matvec(ld4(a.p.Wb + s * 64 + 16 * m + 4 * g), lrelu4(hh), acc);
    }
    y0 = lrelu4(acc);
  }
  const int tsel = (a.sel_t && valid) ? a.sel_t[n] : -1;
  auto emit = [&](int t, const f32x4 v) {
    if (!valid) return;
    if (a.traj) *reinterpret_cast<f32x4*>(a.traj + ((int64_t)n * T + t) * 16 + 4 * g) = v;
    if (a.sel_t == nullptr) *reinterpret_cast<f32x4*>(a.z + ((int64_t)n * T + t) * a.zcols + 4 * g) = v;
    else if (t == tsel) *reinterpret_cast<f32x4*>(a.z + (int64_t)n * a.zcols + 4 * g) = v;
  };
  emit(0, y0);

  S.start(y0);
  double tcur = (double)a.tout[0], seg0 = tcur, seg1 = tcur;
  f32x4 ca = y0, cb = y0, cc = y0, cd = y0, ce = y0;     // interp = (y, y, y, y, y) before the first accepted step
  int steps = 0;
  for (int j = 1; j < T; ++j) {
    const double target = (double)a.tout[j];
    while (target > seg1 && steps < 1000000) {
      const float ratio = S.trial();
      if (ratio <= 1.f) {
        S.interp(ca, cb, cc, cd);
        ce = S.y0;
        seg0 = tcur; seg1 = tcur + S.dtd;
        tcur = seg1; S.accept();
      }
      S.dtd *= (double)step_factor<LibmPow>(ratio);
      ++steps;
    }
    const float x = ((float)target - (float)seg0) / ((float)seg1 - (float)seg0);
    emit(j, ce + x * (cd + x * (cc + x * (cb + x * ca))));
  }
  if (a.nsteps && threadIdx.x == 0) a.nsteps[blockIdx.x] = steps;
}

// the content launch (if the op has content), then `kernel` with one workgroup per RNN_BLOCK_SAMPLES trajectories
template <class Op>
static int launch_fwd_mfma(void (*kernel)(const Op), const Op* op, hipStream_t st) {
  if (op->content) {
    const int rows_per = op->sel_t ? 1 : op->T;
    int64_t total4 = (int64_t)op->N * rows_per * ((op->zcols - 16) >> 2);
    int blocks = (int)((total4 + 255) / 256); if (blocks > 1024) blocks = 1024;
    hipLaunchKernelGGL(latent_content_kernel, dim3(blocks), dim3(256), 0, st, op->content, op->z, op->N, rows_per, op->zcols);
    GODE_LAUNCH_CHECK();
  }
  const int nblocks = (op->N + RNN_BLOCK_SAMPLES - 1) / RNN_BLOCK_SAMPLES;
  const int per = op->N < RNN_BLOCK_SAMPLES ? op->N : RNN_BLOCK_SAMPLES;
  const int threads = ((per + 15) / 16) * 64;     // every workgroup gets this many waves; trailing lanes are masked
  hipLaunchKernelGGL(kernel, dim3(nblocks), dim3(threads), 0, st, *op);
  GODE_LAUNCH_CHECK();
  return 0;
}
int gode_launch_ode_dopri5(const gode_ode_fwd_op* op, hipStream_t st) { return launch_fwd_mfma(ode_dopri5_fwd_kernel, op, st); }
int gode_launch_odernn_fwd_mfma(const gode_odernn_fwd_op* op, hipStream_t st) { return launch_fwd_mfma(odernn_fwd_kernel, op, st); }

// ---------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(64) odernn_bwd_kernel(const gode_odernn_bwd_op a) {
  __shared__ __attribute__((aligned(16))) float tile[2][16 * LDT];
  const int l = threadIdx.x, s = l & 15, g = l >> 4;
  const int n = blockIdx.x * 16 + s;
  const bool valid = n < a.N;
  const int T = a.T;
  float* part = a.work + (int64_t)blockIdx.x * GODE_ODERNN_NPARAM;

  const f32x4 w1 = ld4(a.p.W1 + s * 16 + 4 * g), w2 = ld4(a.p.W2 + s * 16 + 4 * g);
  const f32x4 b1 = ld4(a.p.b1 + 4 * g), b2 = ld4(a.p.b2 + 4 * g);
  f32x4 w1t, w2t, wih[3], whh[3], bih[3], bhh[3], whht[3];
#pragma unroll
  for (int r = 0; r < 4; ++r) { w1t[r] = a.p.W1[(4 * g + r) * 16 + s]; w2t[r] = a.p.W2[(4 * g + r) * 16 + s]; }
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    wih[q] = ld4(a.p.Wih + (16 * q + s) * 16 + 4 * g); whh[q] = ld4(a.p.Whh + (16 * q + s) * 16 + 4 * g);
    bih[q] = ld4(a.p.bih + 16 * q + 4 * g); bhh[q] = ld4(a.p.bhh + 16 * q + 4 * g);
#pragma unroll
    for (int r = 0; r < 4; ++r) whht[q][r] = a.p.Whh[(16 * q + 4 * g + r) * 16 + s];   // (Whh_q)^T operand
  }
  auto outer = [&](f32x4 dst, const f32x4 P, const f32x4 Q) {
    __syncthreads();
    *reinterpret_cast<f32x4*>(&tile[0][s * LDT + 4 * g]) = P;
    *reinterpret_cast<f32x4*>(&tile[1][s * LDT + 4 * g]) = Q;
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 4; ++r) dst = MFMA16(tile[0][(4 * g + r) * LDT + s], tile[1][(4 * g + r) * LDT + s], dst);
    return dst;
  };
  f32x4 gW1 = zero4(), gW2 = zero4(), gb1 = zero4(), gb2 = zero4();
  f32x4 gWih[3], gWhh[3], gbih[3], gbhh[3];
#pragma unroll
  for (int q = 0; q < 3; ++q) { gWih[q] = zero4(); gWhh[q] = zero4(); gbih[q] = zero4(); gbhh[q] = zero4(); }
  f32x4 ky, ka;
  auto stage = [&](const f32x4 ys, const f32x4 as, float c) {
    const f32x4 hh = tanh4(matvec(w1, ys, b1));
    const f32x4 fv = matvec(w2, hh, b2);
    const f32x4 du = matvec(w2t, as, zero4()) * (1.f - hh * hh);
    ka = matvec(w1t, du, zero4());
    ky = -fv;
    const f32x4 ca = c * as, cdu = c * du;
    gb2 += ca; gb1 += cdu;
    gW2 = outer(gW2, ca, hh);
    gW1 = outer(gW1, cdu, ys);
  };
  const int tsel = (a.sel_t && valid) ? a.sel_t[n] : -1;
  auto upstream = [&](int t) {
    if (!valid) return zero4();
    if (a.sel_t == nullptr) return ld4(a.gz + ((int64_t)n * T + t) * a.zcols + 4 * g);
    return t == tsel ? ld4(a.gz + (int64_t)n * a.zcols + 4 * g) : zero4();
  };
  const float third = 1.0f / 3.0f, dt = 1.f / (float)a.substeps;
  f32x4 carry = zero4();
  for (int t = T - 1; t >= 0; --t) {
    const f32x4 gh = carry + upstream(t);                                        // dL/dh_{t+1}
    const f32x4 e = valid ? ld4(a.noise + ((int64_t)(t + 1) * a.N + n) * 16 + 4 * g) : zero4();
    const f32x4 hp = valid ? ld4(a.hp + ((int64_t)n * T + t) * 16 + 4 * g) : zero4();
    // GRU recompute + backward
    const f32x4 r = sigmoid4(matvec(wih[0], e, bih[0]) + matvec(whh[0], hp, bhh[0]));
    const f32x4 zg = sigmoid4(matvec(wih[1], e, bih[1]) + matvec(whh[1], hp, bhh[1]));
    const f32x4 hn = matvec(whh[2], hp, bhh[2]);
    const f32x4 nn = tanh4(matvec(wih[2], e, bih[2]) + r * hn);
    const f32x4 dn_pre = gh * (1.f - zg) * (1.f - nn * nn);
    const f32x4 dz_pre = gh * (hp - nn) * zg * (1.f - zg);
    const f32x4 dr_pre = dn_pre * hn * r * (1.f - r);
    const f32x4 dgi[3] = {dr_pre, dz_pre, dn_pre};
    const f32x4 dgh[3] = {dr_pre, dz_pre, dn_pre * r};
    f32x4 adj = gh * zg;
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      gbih[q] += dgi[q]; gbhh[q] += dgh[q];
      gWih[q] = outer(gWih[q], dgi[q], e);
      gWhh[q] = outer(gWhh[q], dgh[q], hp);
      adj = matvec(whht[q], dgh[q], adj);
    }
    // continuous adjoint of h' = y(1), y(0) = h_t, reverse time, fixed Kutta-3/8 substeps
    f32x4 y = hp;
    for (int ss = 0; ss < a.substeps; ++ss) {
      stage(y, adj, dt * 0.125f);
      const f32x4 ky1 = ky, ka1 = ka;
      stage(y + dt * ky1 * third, adj + dt * ka1 * third, 3.f * dt * 0.125f);
      const f32x4 ky2 = ky, ka2 = ka;
      stage(y + dt * (ky2 - ky1 * third), adj + dt * (ka2 - ka1 * third), 3.f * dt * 0.125f);
      const f32x4 ky3 = ky, ka3 = ka;
      stage(y + dt * (ky1 - ky2 + ky3), adj + dt * (ka1 - ka2 + ka3), dt * 0.125f);
      y = y + (ky1 + 3.f * (ky2 + ky3) + ky) * dt * 0.125f;
      adj = adj + (ka1 + 3.f * (ka2 + ka3) + ka) * dt * 0.125f;
    }
    carry = adj;                                                                 // dL/dh_t
  }
  const f32x4 sb1 = sum_over_samples(gb1), sb2 = sum_over_samples(gb2);
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    part[RO_W1 + (4 * g + r) * 16 + s] = gW1[r];
    part[RO_W2 + (4 * g + r) * 16 + s] = gW2[r];
  }
  if (s == 0) { *reinterpret_cast<f32x4*>(part + RO_B1 + 4 * g) = sb1; *reinterpret_cast<f32x4*>(part + RO_B2 + 4 * g) = sb2; }
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    const f32x4 si = sum_over_samples(gbih[q]), sh = sum_over_samples(gbhh[q]);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      part[RO_WIH + (16 * q + 4 * g + r) * 16 + s] = gWih[q][r];
      part[RO_WHH + (16 * q + 4 * g + r) * 16 + s] = gWhh[q][r];
    }
    if (s == 0) { *reinterpret_cast<f32x4*>(part + RO_BIH + 16 * q + 4 * g) = si; *reinterpret_cast<f32x4*>(part + RO_BHH + 16 * q + 4 * g) = sh; }
  }
}

int gode_launch_odernn_bwd_adaptive(const gode_odernn_bwd_op* op, hipStream_t st);   // adj_adaptive.hip

// substeps > 0: fixed Kutta-3/8 substeps; substeps == 0: the MFMA adaptive adjoint (norm per 64-trajectory workgroup), only
// reached above the co-residency limit of odernn_valu.hip
int gode_launch_odernn_bwd_mfma(const gode_odernn_bwd_op* op, hipStream_t st) {
  const int nblk = (op->N + 15) / 16;
  if (op->substeps == 0) {
    const int rc = gode_launch_odernn_bwd_adaptive(op, st);
    if (rc) return rc;
  } else {
    hipLaunchKernelGGL(odernn_bwd_kernel, dim3(nblk), dim3(64), 0, st, *op);
    GODE_LAUNCH_CHECK();
  }
  return gode_reduce_rows(op->work, op->grads, nblk, GODE_ODERNN_NPARAM, 0, 0, op->accumulate, nullptr, INT32_MAX, 1, st);   // one level
}
