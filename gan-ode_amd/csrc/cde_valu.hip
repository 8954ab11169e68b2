// cde_valu.hip -- the Neural-CDE motion latent (models/mocogan_cde.py: torchcde.cdeint on the backward-difference Hermite
// cubic spline of [linspace(0, 1, T), x], torchdiffeq's dopri5) and the exact gradient of its discrete forward.
//
//   z0 = f([tt_0, x_0]),   dz/dt = F(z) dX/dt,   F(z) = tanh(W2 relu(W1 z + b1) + b2).view(16, 2)
//
// Mapping: that of ode_valu.hip / sde_valu.hip -- one lane = one (trajectory, feature) pair, the 16 features of a
// trajectory in one DPP row, 16 trajectories per 256-thread workgroup, every mat-vec a 16x16 block done as mv16 over row
// rotations.  The vector field is 16 -> 128 -> 32: 8 blocks of W1 and 16 of W2 per right-hand side (lane i owns hidden
// unit 16m + i of chunk m and the outputs 2i, 2i + 1), 24 blocks = 384 weights per lane, which do not fit the register
// file next to the solver state.  The blocks live in LDS instead, already in the per-lane order mv16 consumes (lane i,
// rotation r at [block][i][r], row stride 20 floats: four conflict-free ds_read_b128 per block), and are re-read for
// every right-hand side.  The backward adds the 24 transposed blocks.
//
// Forward: dopri5 with the controller of oracle/ode_ref.dopri5_solve (torchdiffeq's), fp64 clock and step size as the
// other adaptive kernels (odernn_valu.hip), stage times rounded to fp32 at the evaluation of dX/dt.  The error norm is the
// RMS over the whole batch: workgroups exchange partial sums through `sync` in fixed order, so every workgroup takes the
// same (bit-identical) accept / reject decisions and the accepted schedule is one for the whole batch.
//
// Backward (discretise-then-optimise): per accepted step in reverse, the 7 stages are recomputed from the stored state and
// back-propagated (step sizes constant).  The parameter gradients are outer products summed over trajectories and
// stages; per vector-Jacobian product the workgroup's 16 trajectories deposit their factors in LDS and every thread adds
// the sums for its own tile of the 6,304 CDEFunc entries (16 of W2, 8 of W1) in registers: fixed order, no atomics.
#include "common.h"
#include "ode_common.h"
#include "valu_common.h"
#include "dopri5.h"

// parameter block (gode_cde_params order; the layout of `grads`)
#define CP_WA 0
#define CP_BA 128
#define CP_WB 192
#define CP_BB 1216
#define CP_W1 1232
#define CP_B1 3280
#define CP_W2 3408
#define CP_B2 7504
static_assert(CP_B2 + 32 == GODE_CDE_NPARAM, "CDE parameter block");

#define CB_STRIDE 320      // one lane-ordered 16x16 block: 16 lanes x 20 floats
#define CB_W1 0            // W1 rows 16m..16m+15:            lane i, rot r -> W1[16m + i][src r]
#define CB_W2 8            // (c, m) = 8 + 8c + m:            lane i, rot r -> W2[2i + c][16m + src r]
#define CB_W2T 24          // (c, m) = 24 + 8c + m:           lane j, rot r -> W2[2 src r + c][16m + j]
#define CB_W1T 40          // m = 40 + m:                     lane j, rot r -> W1[16m + src r][j]
#define CDE_WG 16          // trajectories per workgroup
#define CDE_MAX_TRIALS 100000
#define XS_VALS 2           // floats per exchange slot

// ---- LDS image shared by both kernels ----------------------------------------------------------------------------------
struct CdeLds {
  float B1s[128], B2s[32];
  float Wa[128], Ba[64], Wb[1024], Bb[16];
  float ttab[16 * 3];               // time channel: per interval (b, 2c, 3d) of torchcde's derivative b + (2c + 3d s) s
  float xtab[CDE_WG][16 * 3];       // noise channel, per trajectory
  float xs[CDE_WG][16];             // noise knots
};

// per-lane-ordered weight blocks [0, nblk) from the global parameters
__device__ __forceinline__ void cde_stage_blocks(const gode_cde_params& p, float* Wp, int nblk, const int* src) {
  const int i = threadIdx.x & 15, q = threadIdx.x >> 4;
  for (int b = q; b < nblk; b += 16) {
    float* dst = Wp + b * CB_STRIDE + i * 20;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int j = src[r];
      float v;
      if (b < CB_W2) v = p.W1[(16 * b + i) * 16 + j];
      else if (b < CB_W2T) { const int c = (b - CB_W2) >> 3, m = (b - CB_W2) & 7; v = p.W2[(2 * i + c) * 128 + 16 * m + j]; }
      else if (b < CB_W1T) { const int c = (b - CB_W2T) >> 3, m = (b - CB_W2T) & 7; v = p.W2[(2 * j + c) * 128 + 16 * m + i]; }
      else { const int m = b - CB_W1T; v = p.W1[(16 * m + j) * 16 + i]; }
      dst[r] = v;
    }
  }
}

// biases, pre-net, the two spline tables and the knots of this workgroup's trajectories
__device__ __forceinline__ void cde_stage_small(const gode_cde_params& p, const float* x, const float* tslope, int N, int T,
                                                int n0, CdeLds& S) {
  const int t = threadIdx.x;
  if (t < 128) { S.B1s[t] = p.b1[t]; S.Wa[t] = p.Wa[t]; }
  if (t < 32) S.B2s[t] = p.b2[t];
  if (t < 64) S.Ba[t] = p.ba[t];
  if (t < 16) S.Bb[t] = p.bb[t];
  for (int k = t; k < 1024; k += 256) S.Wb[k] = p.Wb[k];
  {
    const int tr = t >> 4, k = t & 15;
    S.xs[tr][k] = (n0 + tr < N && k < T) ? x[(int64_t)(n0 + tr) * T + k] : 0.f;
  }
  __syncthreads();
  // torchcde hermite_cubic_coefficients_with_backward_differences (knots at 0, 1, ..., T-1, so t_diff = 1):
  //   b = d_{k-1} (d_{-1} = d_0),  2c = 2 (3 (d_k - b) - d_k + b),  3d = (d_k - b) - 2c
  {
    const int tr = t >> 4, k = t & 15;
    if (k < T - 1) {
      const float dk = S.xs[tr][k + 1] - S.xs[tr][k];
      const float b = k > 0 ? S.xs[tr][k] - S.xs[tr][k - 1] : dk;
      const float c2 = 2.f * (3.f * (dk - b) - dk + b);
      S.xtab[tr][3 * k] = b; S.xtab[tr][3 * k + 1] = c2; S.xtab[tr][3 * k + 2] = (dk - b) - c2;
    }
    if (tr == 0 && k < T - 1) {
      const float dk = tslope[k];
      const float b = k > 0 ? tslope[k - 1] : dk;
      const float c2 = 2.f * (3.f * (dk - b) - dk + b);
      S.ttab[3 * k] = b; S.ttab[3 * k + 1] = c2; S.ttab[3 * k + 2] = (dk - b) - c2;
    }
  }
  __syncthreads();
}

// dX/dt at fp32 time tf: torchcde's interval (bucketize(t, knots) - 1, clamped to [0, T-2]) and fractional part
__device__ __forceinline__ void cde_dxdt(const CdeLds& S, int tr, int T, float tf, float& D0, float& D1) {
  int k = (int)ceilf(tf) - 1;
  k = k < 0 ? 0 : (k > T - 2 ? T - 2 : k);
  const float s = tf - (float)k;
  D0 = S.ttab[3 * k] + (S.ttab[3 * k + 1] + S.ttab[3 * k + 2] * s) * s;
  D1 = S.xtab[tr][3 * k] + (S.xtab[tr][3 * k + 1] + S.xtab[tr][3 * k + 2] * s) * s;
}

__device__ __forceinline__ void cde_ldw(W16& W, const float* Wp, int b, int i) {
  const f32x4* q = reinterpret_cast<const f32x4*>(Wp + b * CB_STRIDE + i * 20);
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const f32x4 v = q[k];
    W.w[4 * k] = v[0]; W.w[4 * k + 1] = v[1]; W.w[4 * k + 2] = v[2]; W.w[4 * k + 3] = v[3];
  }
}

// F(z) dX/dt for this lane's feature; the block reads are re-issued per call (the compiler barrier keeps them from being
// merged across calls into 384 live registers)
__device__ __forceinline__ float cde_field(const float* Wp, const CdeLds& S, float z, int i, float D0, float D1) {
  asm volatile("" ::: "memory");
  float a0 = S.B2s[2 * i], a1 = S.B2s[2 * i + 1];
#pragma unroll
  for (int m = 0; m < 8; ++m) {
    W16 w;
    cde_ldw(w, Wp, CB_W1 + m, i);
    const float h = fmaxf(mv16(w, z, S.B1s[16 * m + i]), 0.f);
    cde_ldw(w, Wp, CB_W2 + m, i);
    a0 = mv16(w, h, a0);
    cde_ldw(w, Wp, CB_W2 + 8 + m, i);
    a1 = mv16(w, h, a1);
  }
  return fast_tanh(a0) * D0 + fast_tanh(a1) * D1;
}

// pre-net f([tt_0, x_0]) for this lane's feature (hp[c] = hidden unit 16c + i after the LeakyReLU)
__device__ __forceinline__ float cde_prenet(const CdeLds& S, float t0, float x0, int i, const int* src, float* hpre,
                                            float& acc_out) {
  float acc = S.Bb[i];
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const int u = 16 * c + i;
    hpre[c] = fmaf(S.Wa[2 * u + 1], x0, S.Wa[2 * u] * t0) + S.Ba[u];
    W16 wb;
    load_rows(wb, S.Wb, 64, 0, 16 * c, i, src);
    acc = mv16(wb, lrelu1(hpre[c]), acc);
  }
  acc_out = acc;
  return lrelu1(acc);
}

// whole-batch sums: 4 waves, the per-wave partials added pairwise
typedef RedLds<4, XS_VALS, true> CdeRed;

// =====================================================================================================================
__global__ void __launch_bounds__(256) cde_fwd_kernel(const gode_cde_fwd_op a) {
  __shared__ __attribute__((aligned(16))) float Wp[CB_W2T * CB_STRIDE];
  __shared__ CdeLds S;
  __shared__ CdeRed R;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = lane & 15, tl = lane >> 4, tr = wave * 4 + tl;
  const int wg = blockIdx.x, n0 = wg * CDE_WG, n = n0 + tr;
  const bool valid = n < a.N;
  const int T = a.T;
  const float inv_count = 1.f / ((float)a.N * 16.f);
  const float rtol = a.rtol, atol = a.atol;
  XSync X;
  X.nwg = gridDim.x; X.wg = wg; X.seq = 0; X.counter = a.sync;
  X.slots = a.sync ? reinterpret_cast<float*>(a.sync) + XS_HDR : nullptr;
  int par = 0;
  if (threadIdx.x == 0) R.dead = 0;

  int src[16];
  probe_sources(i, src);
  cde_stage_blocks(a.p, Wp, CB_W2T, src);
  cde_stage_small(a.p, a.x, a.tslope, a.N, T, n0, S);        // (ends with a barrier)
  if (a.content) broadcast_content(a.content, a.z, a.sel_t, a.N, T, a.zcols, n0, CDE_WG, threadIdx.x, 256);

  const int tsel = (a.sel_t && valid) ? a.sel_t[n] : -1;
  auto emit = [&](int t, float v) {
    if (!valid) return;
    if (a.sel_t == nullptr) a.z[((int64_t)n * T + t) * a.zcols + i] = v;
    else if (t == tsel) a.z[(int64_t)n * a.zcols + i] = v;
  };
  float* st = valid ? a.states + (int64_t)n * (a.S_cap + 1) * 16 + i : nullptr;
  auto f = [&](double tt, float z) {
    float D0, D1;
    cde_dxdt(S, tr, T, (float)tt, D0, D1);
    return cde_field(Wp, S, z, i, D0, D1);
  };

  float hpre[4], acc;
  float y0 = cde_prenet(S, 0.f, S.xs[tr][0], i, src, hpre, acc);
  if (!valid) y0 = 0.f;
  if (st) st[0] = y0;
  emit(0, y0);

  double tcur = 0.0;
  float k1 = f(tcur, y0);
  double dtd;
  {   // torchdiffeq _select_initial_step (order 4)
    const float sc = atol + fabsf(y0) * rtol;
    float v[2] = {valid ? (y0 / sc) * (y0 / sc) : 0.f, valid ? (k1 / sc) * (k1 / sc) : 0.f};
    batch_sum<2>(v, R, par, X);
    const float d0 = sqrtf(v[0] * inv_count), d1 = sqrtf(v[1] * inv_count);
    const float h0 = (d0 < 1e-5f || d1 < 1e-5f) ? 1e-6f : 0.01f * d0 / d1;
    const float f1 = f(tcur + (double)h0, fmaf(h0, k1, y0));
    const float df = (f1 - k1) / sc;
    float w[1] = {valid ? df * df : 0.f};
    batch_sum<1>(w, R, par, X);
    const float d2 = sqrtf(w[0] * inv_count) / h0;
    const float hh = (d1 <= 1e-15f && d2 <= 1e-15f) ? fmaxf(1e-6f, h0 * 1e-3f) : fast_pow(0.01f / fmaxf(d1, d2), 0.2f);
    dtd = (double)fminf(100.f * h0, hh);
  }

  int accepted = 0, trials = 0, jo = 1;
  bool failed = false;
  while (jo < T) {
    if (R.dead || trials >= CDE_MAX_TRIALS || !(tcur + dtd > tcur)) { failed = true; break; }
    const float dt = (float)dtd;
    const float k2 = f(tcur + 0.2 * dtd, fmaf(dt, DP5_A21 * k1, y0));
    const float k3 = f(tcur + 0.3 * dtd, fmaf(dt, DP5_A31 * k1 + DP5_A32 * k2, y0));
    const float k4 = f(tcur + 0.8 * dtd, fmaf(dt, DP5_A41 * k1 + DP5_A42 * k2 + DP5_A43 * k3, y0));
    const float k5 = f(tcur + (8.0 / 9.0) * dtd, fmaf(dt, DP5_A51 * k1 + DP5_A52 * k2 + DP5_A53 * k3 + DP5_A54 * k4, y0));
    const float k6 = f(tcur + dtd, fmaf(dt, DP5_A61 * k1 + DP5_A62 * k2 + DP5_A63 * k3 + DP5_A64 * k4 + DP5_A65 * k5, y0));
    const float y1 = fmaf(dt, DP5_B1 * k1 + DP5_B3 * k3 + DP5_B4 * k4 + DP5_B5 * k5 + DP5_B6 * k6, y0);
    const float k7 = f(tcur + dtd, y1);
    const float err = dt * (DP5_E1 * k1 + DP5_E3 * k3 + DP5_E4 * k4 + DP5_E5 * k5 + DP5_E6 * k6 + DP5_E7 * k7);
    const float tol = atol + rtol * fmaxf(fabsf(y0), fabsf(y1));
    const float rr = err / tol;
    float v[1] = {valid ? rr * rr : 0.f};
    batch_sum<1>(v, R, par, X);
    const float ratio = sqrtf(v[0] * inv_count);
    ++trials;
    if (ratio <= 1.f) {
      if (accepted >= a.S_cap) { failed = true; break; }      // capacity: stop before writing past the buffers
      const double t1 = tcur + dtd;
      if (wg == 0 && threadIdx.x == 0) { a.sched[accepted] = tcur; a.sched[a.S_cap + accepted] = dtd; }
      if (st) st[(int64_t)(accepted + 1) * 16] = y1;
      // dense output at every integer time in (tcur, t1] (the abscissa from the fp32-rounded times, as torchdiffeq)
      while (jo < T && (double)jo <= t1) {
        const float x = ((float)jo - (float)tcur) / ((float)t1 - (float)tcur);
        float wS, wM, w1c, w7c;
        interp_weights(x, wS, wM, w1c, w7c);
        const float ym = fmaf(dt, DP5_C1 * k1 + DP5_C3 * k3 + DP5_C4 * k4 + DP5_C5 * k5 + DP5_C6 * k6 + DP5_C7 * k7, y0);
        emit(jo, y0 + wS * (y1 - y0) + wM * (ym - y0) + dt * (w1c * k1 + w7c * k7));
        ++jo;
      }
      ++accepted;
      tcur = t1; y0 = y1; k1 = k7;
    }
    dtd *= (double)step_factor(ratio);
  }
  if (wg == 0 && threadIdx.x == 0) { a.counts[0] = failed ? -accepted - 1 : accepted; a.counts[1] = trials; }
}

// =====================================================================================================================
struct CdeBuf {                      // one vector-Jacobian product's factors of the parameter outer products
  float v2[CDE_WG][32];              // dL/d(W2 h + b2)
  float h[CDE_WG][128];              // relu(W1 z + b1)
  float g1[CDE_WG][128];             // dL/d(W1 z + b1)
  float z[CDE_WG][16];
};

__global__ void __launch_bounds__(256) cde_bwd_kernel(const gode_cde_bwd_op a) {
  __shared__ __attribute__((aligned(16))) float Wp[(CB_W1T + 8) * CB_STRIDE];
  __shared__ CdeLds S;
  __shared__ __attribute__((aligned(16))) CdeBuf Bf;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = lane & 15, tl = lane >> 4, tr = wave * 4 + tl;
  const int th = threadIdx.x;
  const int wg = blockIdx.x, n0 = wg * CDE_WG, n = n0 + tr;
  const bool valid = n < a.N;
  const int T = a.T;
  float* part = a.work + (int64_t)wg * GODE_CDE_NPARAM;
  const int S_acc = a.counts[0];
  if (S_acc < 0) return;             // failed forward: nothing is written (the host has raised)

  int src[16];
  probe_sources(i, src);
  cde_stage_blocks(a.p, Wp, CB_W1T + 8, src);
  cde_stage_small(a.p, a.x, a.tslope, a.N, T, n0, S);

  // this thread's tile of the CDEFunc gradient: W2[o][k0..k0+16), W1[m][j0..j0+8), b2[o], b1[m]
  const int o = th >> 3, k0 = (th & 7) * 16, m1 = th >> 1, j0 = (th & 1) * 8;
  float gW2[16], gW1[8], gb2 = 0.f, gb1 = 0.f;
#pragma unroll
  for (int q = 0; q < 16; ++q) gW2[q] = 0.f;
#pragma unroll
  for (int q = 0; q < 8; ++q) gW1[q] = 0.f;

  // vector-Jacobian product of F(z) dX/dt at (tt, z) with cotangent g: returns dL/dz, deposits the parameter factors
  // (uniform over the workgroup: every thread calls it the same number of times)
  auto vjp = [&](double tt, float z, float g) -> float {
    asm volatile("" ::: "memory");
    float D0, D1;
    cde_dxdt(S, tr, T, (float)tt, D0, D1);
    float u1[8];
    float a0 = S.B2s[2 * i], a1 = S.B2s[2 * i + 1];
#pragma unroll
    for (int m = 0; m < 8; ++m) {
      W16 w;
      cde_ldw(w, Wp, CB_W1 + m, i);
      u1[m] = mv16(w, z, S.B1s[16 * m + i]);
      const float h = fmaxf(u1[m], 0.f);
      Bf.h[tr][16 * m + i] = h;
      cde_ldw(w, Wp, CB_W2 + m, i);
      a0 = mv16(w, h, a0);
      cde_ldw(w, Wp, CB_W2 + 8 + m, i);
      a1 = mv16(w, h, a1);
    }
    const float F0 = fast_tanh(a0), F1 = fast_tanh(a1);
    const float v0 = g * D0 * (1.f - F0 * F0), v1 = g * D1 * (1.f - F1 * F1);
    Bf.v2[tr][2 * i] = v0;
    Bf.v2[tr][2 * i + 1] = v1;
    Bf.z[tr][i] = z;
    float gz = 0.f;
#pragma unroll
    for (int m = 0; m < 8; ++m) {
      W16 w;
      cde_ldw(w, Wp, CB_W2T + m, i);
      float gh = mv16(w, v0, 0.f);
      cde_ldw(w, Wp, CB_W2T + 8 + m, i);
      gh = mv16(w, v1, gh);
      const float g1 = u1[m] > 0.f ? gh : 0.f;
      Bf.g1[tr][16 * m + i] = g1;
      cde_ldw(w, Wp, CB_W1T + m, i);
      gz = mv16(w, g1, gz);
    }
    __syncthreads();
#pragma unroll 4
    for (int t = 0; t < CDE_WG; ++t) {
      const float vv = Bf.v2[t][o];
      const f32x4* hp = reinterpret_cast<const f32x4*>(&Bf.h[t][k0]);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const f32x4 hv = hp[q];
        gW2[4 * q] += vv * hv[0]; gW2[4 * q + 1] += vv * hv[1]; gW2[4 * q + 2] += vv * hv[2]; gW2[4 * q + 3] += vv * hv[3];
      }
      gb2 += vv;
      const float gg = Bf.g1[t][m1];
      const f32x4* zp = reinterpret_cast<const f32x4*>(&Bf.z[t][j0]);
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const f32x4 zv = zp[q];
        gW1[4 * q] += gg * zv[0]; gW1[4 * q + 1] += gg * zv[1]; gW1[4 * q + 2] += gg * zv[2]; gW1[4 * q + 3] += gg * zv[3];
      }
      gb1 += gg;
    }
    __syncthreads();
    return gz;
  };
  auto f = [&](double tt, float z) {
    float D0, D1;
    cde_dxdt(S, tr, T, (float)tt, D0, D1);
    return cde_field(Wp, S, z, i, D0, D1);
  };

  const int tsel = (a.sel_t && valid) ? a.sel_t[n] : -1;
  auto upstream = [&](int t) -> float {
    if (!valid) return 0.f;
    if (a.sel_t == nullptr) return a.gz[((int64_t)n * T + t) * a.zcols + i];
    return t == tsel ? a.gz[(int64_t)n * a.zcols + i] : 0.f;
  };
  const float* stp = valid ? a.states + (int64_t)n * (a.S_cap + 1) * 16 + i : nullptr;
  float adj = 0.f;                   // dL/d(state at the end of the current step)
  int jhi = T - 1;                   // the outputs not yet folded in: 1..jhi
  for (int s = S_acc - 1; s >= 0; --s) {
    const double t0 = a.sched[s], hd = a.sched[a.S_cap + s], t1 = t0 + hd;
    const float dt = (float)hd;
    const float y0 = stp ? stp[(int64_t)s * 16] : 0.f;
    // recompute the stages
    const float k1 = f(t0, y0);
    const float z2 = fmaf(dt, DP5_A21 * k1, y0);
    const float k2 = f(t0 + 0.2 * hd, z2);
    const float z3 = fmaf(dt, DP5_A31 * k1 + DP5_A32 * k2, y0);
    const float k3 = f(t0 + 0.3 * hd, z3);
    const float z4 = fmaf(dt, DP5_A41 * k1 + DP5_A42 * k2 + DP5_A43 * k3, y0);
    const float k4 = f(t0 + 0.8 * hd, z4);
    const float z5 = fmaf(dt, DP5_A51 * k1 + DP5_A52 * k2 + DP5_A53 * k3 + DP5_A54 * k4, y0);
    const float k5 = f(t0 + (8.0 / 9.0) * hd, z5);
    const float z6 = fmaf(dt, DP5_A61 * k1 + DP5_A62 * k2 + DP5_A63 * k3 + DP5_A64 * k4 + DP5_A65 * k5, y0);
    const float k6 = f(t0 + hd, z6);
    const float y1 = fmaf(dt, DP5_B1 * k1 + DP5_B3 * k3 + DP5_B4 * k4 + DP5_B5 * k5 + DP5_B6 * k6, y0);

    float gy0 = 0.f, gy1 = adj, gk1 = 0.f, gk3 = 0.f, gk4 = 0.f, gk5 = 0.f, gk6 = 0.f, gk7 = 0.f, gym = 0.f;
    bool outs = false;
    while (jhi >= 1 && (double)jhi > t0) {           // outputs read off this step's interpolant (t0 < j <= t1)
      const float x = ((float)jhi - (float)t0) / ((float)t1 - (float)t0);
      float wS, wM, w1c, w7c;
      interp_weights(x, wS, wM, w1c, w7c);
      const float g = upstream(jhi);
      gy0 += (1.f - wS - wM) * g;
      gy1 += wS * g;
      gym += wM * g;
      gk1 += dt * w1c * g;
      gk7 += dt * w7c * g;
      outs = true;
      --jhi;
    }
    if (outs) {                      // ym = y0 + dt (DP5_C1 k1 + DP5_C3 k3 + ... + DP5_C7 k7), k7 = f(t1, y1)
      gy0 += gym;
      const float dg = dt * gym;
      gk1 += DP5_C1 * dg; gk3 += DP5_C3 * dg; gk4 += DP5_C4 * dg; gk5 += DP5_C5 * dg; gk6 += DP5_C6 * dg; gk7 += DP5_C7 * dg;
      gy1 += vjp(t1, y1, gk7);
    }
    // y1 = y0 + dt (DP5_B1 k1 + DP5_B3 k3 + ... + DP5_B6 k6)
    gy0 += gy1;
    const float db = dt * gy1;
    gk1 += DP5_B1 * db; gk3 += DP5_B3 * db; gk4 += DP5_B4 * db; gk5 += DP5_B5 * db; gk6 += DP5_B6 * db;
    float gz = vjp(t0 + hd, z6, gk6);
    gy0 += gz; gz *= dt;
    gk1 += DP5_A61 * gz; float gk2 = DP5_A62 * gz; gk3 += DP5_A63 * gz; gk4 += DP5_A64 * gz; gk5 += DP5_A65 * gz;
    gz = vjp(t0 + (8.0 / 9.0) * hd, z5, gk5);
    gy0 += gz; gz *= dt;
    gk1 += DP5_A51 * gz; gk2 += DP5_A52 * gz; gk3 += DP5_A53 * gz; gk4 += DP5_A54 * gz;
    gz = vjp(t0 + 0.8 * hd, z4, gk4);
    gy0 += gz; gz *= dt;
    gk1 += DP5_A41 * gz; gk2 += DP5_A42 * gz; gk3 += DP5_A43 * gz;
    gz = vjp(t0 + 0.3 * hd, z3, gk3);
    gy0 += gz; gz *= dt;
    gk1 += DP5_A31 * gz; gk2 += DP5_A32 * gz;
    gz = vjp(t0 + 0.2 * hd, z2, gk2);
    gy0 += gz;
    gk1 += DP5_A21 * dt * gz;
    gy0 += vjp(t0, y0, gk1);
    adj = gy0;
  }
  adj += upstream(0);

  // ---- pre-net backward: z0 = lrelu(Wb lrelu(Wa [tt_0, x_0] + ba) + bb), tt_0 = 0
  {
    float hpre[4], acc;
    const float x0 = S.xs[tr][0];
    cde_prenet(S, 0.f, x0, i, src, hpre, acc);
    const float g0 = acc > 0.f ? adj : 0.2f * adj;
    Bf.z[tr][i] = g0;                                   // dL/dbb per trajectory
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      W16 wbt;
      load_cols(wbt, S.Wb, 64, 0, 16 * c, i, src);
      const float t = mv16(wbt, g0, 0.f);
      Bf.h[tr][16 * c + i] = lrelu1(hpre[c]);           // post-activation hidden
      Bf.g1[tr][16 * c + i] = hpre[c] > 0.f ? t : 0.2f * t;   // dL/d(hidden pre-activation)
    }
    __syncthreads();
    for (int k = th; k < 1232; k += 256) {
      float s = 0.f;
      if (k < CP_BA) {                                  // Wa[u][c]: sum g_u * [tt_0, x_0]_c
        const int u = k >> 1;
        if (k & 1) {
          for (int t = 0; t < CDE_WG; ++t) s += Bf.g1[t][u] * S.xs[t][0];
        } else {
          for (int t = 0; t < CDE_WG; ++t) s += Bf.g1[t][u] * 0.f;
        }
      } else if (k < CP_WB) {
        for (int t = 0; t < CDE_WG; ++t) s += Bf.g1[t][k - CP_BA];
      } else if (k < CP_BB) {
        const int r = (k - CP_WB) >> 6, c = (k - CP_WB) & 63;
        for (int t = 0; t < CDE_WG; ++t) s += Bf.z[t][r] * Bf.h[t][c];
      } else {
        for (int t = 0; t < CDE_WG; ++t) s += Bf.z[t][k - CP_BB];
      }
      part[k] = s;
    }
  }
#pragma unroll
  for (int q = 0; q < 16; ++q) part[CP_W2 + o * 128 + k0 + q] = gW2[q];
#pragma unroll
  for (int q = 0; q < 8; ++q) part[CP_W1 + m1 * 16 + j0 + q] = gW1[q];
  if ((th & 7) == 0) part[CP_B2 + o] = gb2;
  if ((th & 1) == 0) part[CP_B1 + m1] = gb1;
}

static bool cde_params_ok(const gode_cde_params& p) {
  return p.Wa && p.ba && p.Wb && p.bb && p.W1 && p.b1 && p.W2 && p.b2;
}

extern "C" int64_t gode_cde_sync_size(int32_t N) {
  const int64_t nwg = N > 0 ? (N + CDE_WG - 1) / CDE_WG : 0;
  return nwg > 1 ? XS_HDR + 2 * nwg * XS_VALS : 0;
}
extern "C" int64_t gode_cde_state_size(int32_t N, int32_t S_cap) {
  return (N > 0 && S_cap > 0) ? (int64_t)N * (S_cap + 1) * 16 : 0;
}
extern "C" int64_t gode_cde_bwd_work_size(int32_t N) {
  return N > 0 ? (int64_t)((N + CDE_WG - 1) / CDE_WG) * GODE_CDE_NPARAM : 0;
}

extern "C" int gode_cde_fwd(const gode_cde_fwd_op* op, void* stream) {
  if (!op || !op->x || !op->tslope || !op->z || !op->states || !op->sched || !op->counts) return GODE_E_ARG;
  if (op->N <= 0 || op->N > GODE_CDE_MAX_N || op->T < 2 || op->T > 16 || op->S_cap < 1) return GODE_E_ARG;
  if (!(op->rtol > 0.f) || !(op->atol >= 0.f)) return GODE_E_ARG;
  if (op->zcols < 16 || op->zcols % 4 != 0 || (op->content && op->zcols < 68)) return GODE_E_ARG;
  if (!cde_params_ok(op->p)) return GODE_E_ARG;
  const int nblk = (op->N + CDE_WG - 1) / CDE_WG;
  if (nblk > 1 && !op->sync) return GODE_E_ARG;
  hipStream_t st = (hipStream_t)stream;
  if (nblk > 1) {
    const hipError_t e = hipMemsetAsync(op->sync, 0, XS_HDR * sizeof(int32_t), st);
    if (e != hipSuccess) return (int)e;
  }
  hipLaunchKernelGGL(cde_fwd_kernel, dim3(nblk), dim3(256), 0, st, *op);
  GODE_LAUNCH_CHECK();
  return 0;
}

extern "C" int gode_cde_bwd(const gode_cde_bwd_op* op, void* stream) {
  if (!op || !op->x || !op->tslope || !op->states || !op->sched || !op->counts || !op->gz || !op->work || !op->grads)
    return GODE_E_ARG;
  if (op->N <= 0 || op->N > GODE_CDE_MAX_N || op->T < 2 || op->T > 16 || op->S_cap < 1) return GODE_E_ARG;
  if (op->zcols < 16 || op->zcols % 4 != 0) return GODE_E_ARG;
  if (!cde_params_ok(op->p)) return GODE_E_ARG;
  hipStream_t st = (hipStream_t)stream;
  const int nblk = (op->N + CDE_WG - 1) / CDE_WG;
  hipLaunchKernelGGL(cde_bwd_kernel, dim3(nblk), dim3(256), 0, st, *op);
  GODE_LAUNCH_CHECK();
  // two levels above 32 rows; a failed forward (counts[0] < 0) leaves grads alone
  return gode_reduce_rows(op->work, op->grads, nblk, GODE_CDE_NPARAM, 0, 0, op->accumulate, op->counts, 32, 16, st);
}
