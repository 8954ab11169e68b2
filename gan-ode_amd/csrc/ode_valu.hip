// ode_valu.hip -- the fixed-grid solve (rk4, euler, midpoint) and its adjoint on the VECTOR ALU with DPP row rotations (the
// default since round 2; the rk4-only MFMA-chain kernels of ode.hip remain selectable with GODE_ODE_MFMA=1 for the A/B in profiles/).
//
// Reference arithmetic: as ode.hip (models/mocogan_ode.py:6-17,123-148; torchdiffeq fixed-grid rk4 = Kutta 3/8 and its
// continuous adjoint, restated in oracle/ode_ref.py).
//
// Mapping: one lane = one (trajectory, feature) pair; the 16 features of a trajectory sit in one DPP row (16 lanes), a
// wave holds 4 trajectories, a 256-thread workgroup 16.  A 16x16 mat-vec is 16 v_fmac_f32 whose second operand is the
// state rotated within the row (`row_ror:r`, r = 0..15) and whose first operand is the weight the lane needs for that
// rotation, W[i][src(i, r)], held in 16 VGPRs per matrix; four independent accumulators keep the dependent chain at 4.
// Against the MFMA mapping of ode.hip (16 trajectories per wave, four chained v_mfma_f32_16x16x4_f32 of 40 cycles
// dependent latency each per mat-vec, 4 tanh per lane):
//   * latency per right-hand side: 2 x (16 FMA issue slots) + ONE tanh per lane instead of 2 x 160 cycles of dependent
//     MFMA + four tanh -- the config-size launch (N = 32: eight waves) is bound by exactly that chain;
//   * throughput: the same 1,024 useful FLOPs per trajectory and right-hand side on the same vector ALUs (fp32 MFMA and
//     fp32 VALU share one peak), without the accumulator-to-operand moves;
//   * adjoint: the parameter-gradient outer products sum_traj P_i Q_j become 16 more FMAs per matrix into PER-LANE
//     accumulators (lane i, rotation r holds dW[i][src(i, r)]) that live in registers for the whole solve and are
//     reduced over trajectories ONCE at the end -- no LDS transpose, no barrier inside the time loop (ode.hip: two
//     barriers + an LDS round trip per outer product, eight per RK4 step).
// Which lane a rotation delivers is read off the hardware once per kernel (the lane index is rotated the same way), so
// the weight arrangement cannot disagree with the DPP semantics.
//
// Both kernels are compiled once per fixed-grid method (the `method` codes of gode.h): METHOD_RK4 (torchdiffeq's rk4 =
// Kutta 3/8), METHOD_EULER, METHOD_MIDPOINT.  The method picks ONE step function per kernel (`step` below) at compile
// time; every grid mode -- output times with `substeps`, the grid_dt / emit_at / emit_w grid, the adjoint's bstep_off /
// bstep_dt -- calls that function, and nothing inside a time loop branches on the method.
//
// The right-hand side is a second compile-time axis (the `rhs` codes of gode.h, RHS_* of valu_common.h): RHS_MLP is
// f(y) = W2 tanh(W1 y + b1) + b2 (models/mocogan_ode.py:6-17); RHS_TANH is f(y) = tanh(W1 y + b1), the one-layer ODEFunc
// of models/mocogan_mnist.py:6-16, its weight in the block's W1 slot and its bias in the b1 slot.  An RHS_TANH kernel holds
// no W2 arrangement and no W2 / b2 accumulator, never dereferences p.W2 / p.b2, and its parameter block -- the LDS copy,
// the per-wave gradient images, the part of a `work` row it writes -- ends at OFF_W2.
#include <type_traits>
#include "common.h"
#include "ode_common.h"
#include "valu_common.h"

enum { METHOD_RK4 = 0, METHOD_EULER = 2, METHOD_MIDPOINT = 3 };
struct NoW16 {};                         // stands where an RHS_TANH kernel has no second matrix
template <int RHS> using W16If2 = std::conditional_t<RHS == RHS_MLP, W16, NoW16>;
template <int RHS> constexpr int rhs_nparam = RHS == RHS_MLP ? GODE_ODE_NPARAM : OFF_W2;

// y(t) -> y(t + dt) with right-hand side f: the ONE step function of a method, called by the forward kernel on every grid
// mode and by the discrete-backprop kernel's forward re-run
template <int METHOD, class F>
__device__ __forceinline__ float fixed_step(F&& f, float y0, float dt) {
  if constexpr (METHOD == METHOD_EULER) {
    return y0 + dt * f(y0);
  } else if constexpr (METHOD == METHOD_MIDPOINT) {
    return y0 + dt * f(y0 + (0.5f * dt) * f(y0));
  } else {
    const float third = 1.0f / 3.0f;
    const float k1 = f(y0);
    const float k2 = f(y0 + dt * k1 * third);
    const float k3 = f(y0 + dt * (k2 - k1 * third));
    const float k4 = f(y0 + dt * (k1 - k2 + k3));
    return y0 + (k1 + 3.f * (k2 + k3) + k4) * dt * 0.125f;
  }
}

template <int METHOD, int RHS>
__global__ void __launch_bounds__(256) ode_fwd_valu_kernel(const gode_ode_fwd_op a) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = lane & 15, tl = lane >> 4;
  const int n0 = blockIdx.x * 16, n = n0 + wave * 4 + tl;
  const bool valid = n < a.N;
  const int T = a.T;
  __shared__ float P[rhs_nparam<RHS>];
  float y = valid ? a.x[n * 16 + i] : 0.f;
  stage_ode_params<256, RHS>(a.p, a.prenet, P);
  if (a.content) broadcast_content(a.content, a.z, a.sel_t, a.N, T, a.zcols, n0, 16, threadIdx.x, 256);

  int src[16];
  probe_sources(i, src);
  if (a.prenet) y = prenet_fwd(P, y, i, src);
  W16 w1;
  W16If2<RHS> w2;
  load_rows(w1, P + OFF_W1, 16, 0, 0, i, src);
  if constexpr (RHS == RHS_MLP) load_rows(w2, P + OFF_W2, 16, 0, 0, i, src);
  const float b1 = P[OFF_B1 + i], b2 = RHS == RHS_MLP ? P[OFF_B2 + i] : 0.f;
  auto f = [&](float yy) {
    const float h = fast_tanh(mv16(w1, yy, b1));
    if constexpr (RHS == RHS_MLP) return mv16(w2, h, b2);
    else return h;
  };

  const int tsel = (a.sel_t && valid) ? a.sel_t[n] : -1;
  auto emit = [&](int t) {
    if (!valid) return;
    if (a.traj) a.traj[((int64_t)n * T + t) * 16 + i] = y;
    if (a.sel_t == nullptr) a.z[((int64_t)n * T + t) * a.zcols + i] = y;
    else if (t == tsel) a.z[(int64_t)n * a.zcols + i] = y;
  };
  emit(0);
  auto step = [&](float y0, float dt) -> float { return fixed_step<METHOD>(f, y0, dt); };
  if (a.grid_dt != nullptr) {
    int jo = 1;
    for (int s = 0; s < a.G; ++s) {
      const float y0 = y;
      const float y1 = step(y0, a.grid_dt[s]);
      while (jo < T && a.emit_at[jo] == s) {
        const float w = a.emit_w[jo];
        y = w == 1.f ? y1 : (w == 0.f ? y0 : y0 + w * (y1 - y0));
        emit(jo);
        ++jo;
      }
      y = y1;
    }
    return;
  }
  for (int j = 0; j + 1 < T; ++j) {
    const float dt = a.dt[j] / (float)a.substeps;
    for (int ss = 0; ss < a.substeps; ++ss) y = step(y, dt);
    emit(j + 1);
  }
}

// ---------------------------------------------------------------------------------------------------------------
// backward.  BACKPROP (the `backprop` codes of gode.h): BP_ADJOINT, torchdiffeq's continuous adjoint -- (y, adj, g_theta)
// re-integrated backwards in time with the method's own steps; BP_DISCRETE, the exact reverse-mode gradient of the forward
// kernel's steps (autograd through odeint), walked from each step's start state.  The two differ in the time loop only: the
// lane mapping, the six weight / accumulator arrangements, the upstream reads and everything behind the loop (reduction over
// trajectories, pre-net backward, the `work` row) are this one body.
enum { BP_ADJOINT = 0, BP_DISCRETE = 1 };
template <int METHOD, int RHS, int BACKPROP>
__global__ void __launch_bounds__(256) ode_bwd_valu_kernel(const gode_ode_bwd_op a) {
  constexpr int NPAR = rhs_nparam<RHS>;       // the block this kernel stages, accumulates and writes out
  __shared__ float R[4][NPAR];                // per-wave image of the gradient vector (combined once, at the end)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = lane & 15, tl = lane >> 4;
  const int n0 = blockIdx.x * 16, n = n0 + wave * 4 + tl;
  const bool valid = n < a.N;
  const int T = a.T;
  float* part = a.work + (int64_t)blockIdx.x * GODE_ODE_NPARAM;
  const float x = (valid && a.prenet) ? a.x[n * 16 + i] : 0.f;     // needed by the pre-net backward at the very end
#ifdef GODE_ODE_STAMPS   // diagnostic build only (scripts/exp/ode_stamps.sh): where the config-size launch spends its cycles
  const long long st0 = __builtin_amdgcn_s_memtime(), rt0 = __builtin_amdgcn_s_memrealtime();
  long long st1 = 0, st2 = 0, st3 = 0;
#endif

  __shared__ float P[NPAR];
  stage_ode_params<256, RHS>(a.p, a.prenet, P);
  int src[16];
  probe_sources(i, src);
  W16 w1, w1t, gW1;
  W16If2<RHS> w2, w2t, gW2;
  load_rows(w1, P + OFF_W1, 16, 0, 0, i, src);
  if constexpr (RHS == RHS_MLP) load_rows(w2, P + OFF_W2, 16, 0, 0, i, src);
  load_cols(w1t, P + OFF_W1, 16, 0, 0, i, src);
  if constexpr (RHS == RHS_MLP) load_cols(w2t, P + OFF_W2, 16, 0, 0, i, src);
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    gW1.w[r] = 0.f;
    if constexpr (RHS == RHS_MLP) gW2.w[r] = 0.f;
  }
  const float b1 = P[OFF_B1 + i], b2 = RHS == RHS_MLP ? P[OFF_B2 + i] : 0.f;
  float gb1 = 0.f, gb2 = 0.f;             // (gb2: RHS_MLP only)

  const int tsel = (a.sel_t && valid) ? a.sel_t[n] : -1;
  auto upstream = [&](int t) -> float {
    if (!valid) return 0.f;
    if (a.sel_t == nullptr) return a.gz[((int64_t)n * T + t) * a.zcols + i];
    return t == tsel ? a.gz[(int64_t)n * a.zcols + i] : 0.f;
  };
  float adj = 0.f;                        // dL/d(state): the adjoint, or discrete backprop's lambda
  if constexpr (BACKPROP == BP_ADJOINT) {
  adj = upstream(T - 1);
  float ky, ka;
  // one stage of the reversed augmented dynamics at (ys, as); c = the stage's b-weight * dt for the parameter integrals
  // (weighted = std::false_type: a stage of weight 0, whose outer products are not formed)
  auto stage = [&](float ys, float as, float c, auto weighted) {
    const float h = fast_tanh(mv16(w1, ys, b1));
    if constexpr (RHS == RHS_MLP) {
      const float fv = mv16(w2, h, b2);
      const float v = mv16(w2t, as, 0.f);
      const float du = v * (1.f - h * h);
      ka = mv16(w1t, du, 0.f);
      ky = -fv;
      if constexpr (decltype(weighted)::value) {
        const float ca = c * as, cdu = c * du;
        gb2 += ca; gb1 += cdu;
        outer16(gW2, ca, h);
        outer16(gW1, cdu, ys);
      }
    } else {
      // f = h: a^T df/dy = W1^T (a (1 - h^2)), a^T df/db1 = a (1 - h^2), a^T df/dW1 = (a (1 - h^2)) ys^T
      const float du = as * (1.f - h * h);
      ka = mv16(w1t, du, 0.f);
      ky = -h;
      if constexpr (decltype(weighted)::value) {
        const float cdu = c * du;
        gb1 += cdu;
        outer16(gW1, cdu, ys);
      }
    }
  };
  // (y, adj)(t) -> (y, adj)(t - dt); the parameter integrals advance with the same tableau's b-weights
  const std::true_type b_weighted;
  const std::false_type b_zero;
  auto step = [&](float& y, float& adj, float dt) {
    if constexpr (METHOD == METHOD_EULER) {
      stage(y, adj, dt, b_weighted);
      y = y + dt * ky;
      adj = adj + dt * ka;
    } else if constexpr (METHOD == METHOD_MIDPOINT) {
      const float half = 0.5f * dt;
      stage(y, adj, 0.f, b_zero);
      stage(y + half * ky, adj + half * ka, dt, b_weighted);
      y = y + dt * ky;
      adj = adj + dt * ka;
    } else {
      const float third = 1.0f / 3.0f;
      stage(y, adj, dt * 0.125f, b_weighted);
      const float ky1 = ky, ka1 = ka;
      stage(y + dt * ky1 * third, adj + dt * ka1 * third, 3.f * dt * 0.125f, b_weighted);
      const float ky2 = ky, ka2 = ka;
      stage(y + dt * (ky2 - ky1 * third), adj + dt * (ka2 - ka1 * third), 3.f * dt * 0.125f, b_weighted);
      const float ky3 = ky, ka3 = ka;
      stage(y + dt * (ky1 - ky2 + ky3), adj + dt * (ka1 - ka2 + ka3), dt * 0.125f, b_weighted);
      y = y + (ky1 + 3.f * (ky2 + ky3) + ky) * dt * 0.125f;
      adj = adj + (ka1 + 3.f * (ka2 + ka3) + ka) * dt * 0.125f;
    }
  };

#ifdef GODE_ODE_STAMPS
  st1 = __builtin_amdgcn_s_memtime();
#endif
  // the stored state and the upstream gradient of the NEXT interval are requested before the stages of the
  // current one, so the (dependent, ~1 us each at N = 32) loads land under the arithmetic (rk4: ~600 cycles)
  float y_next = (valid && T > 1) ? a.traj[((int64_t)n * T + (T - 1)) * 16 + i] : 0.f;
  for (int it = T - 1; it >= 1; --it) {
    float y = y_next;
    const float up = upstream(it - 1);
    if (it > 1) y_next = valid ? a.traj[((int64_t)n * T + (it - 1)) * 16 + i] : 0.f;
    const int s0 = a.bstep_off ? a.bstep_off[it - 1] : 0;
    const int ns = a.bstep_off ? a.bstep_off[it] - s0 : a.substeps;
    const float dt_eq = a.dt[it - 1] / (float)a.substeps;
    for (int ss = 0; ss < ns; ++ss) step(y, adj, a.bstep_off ? a.bstep_dt[s0 + ss] : dt_eq);
    adj = adj + up;
  }
  } else {
  // ---- discrete backprop: every solver step in reverse order, from its start state y0 and adj = dL/dy1.  The stage inputs
  // u_s and h_s = tanh(W1 u_s + b1) are recomputed and kept (at most 4 + 4 values per lane), then the stages are walked
  // backwards; vjp(g, u, h) = J^T g at u, and adds the stage's parameter VJP to the per-lane accumulators
  auto h_of = [&](float u) { return fast_tanh(mv16(w1, u, b1)); };
  auto k_of = [&](float h) {
    if constexpr (RHS == RHS_MLP) return mv16(w2, h, b2);
    else return h;
  };
  auto vjp = [&](float g, float u, float h) -> float {
    float du;
    if constexpr (RHS == RHS_MLP) {
      gb2 += g;
      outer16(gW2, g, h);
      du = mv16(w2t, g, 0.f) * (1.f - h * h);
    } else {
      du = g * (1.f - h * h);
    }
    gb1 += du;
    outer16(gW1, du, u);
    return mv16(w1t, du, 0.f);
  };
  auto rstep = [&](float y0, float dt) {
    if constexpr (METHOD == METHOD_EULER) {
      const float h1 = h_of(y0);
      adj = adj + vjp(dt * adj, y0, h1);
    } else if constexpr (METHOD == METHOD_MIDPOINT) {
      const float half = 0.5f * dt;
      const float h1 = h_of(y0);
      const float u2 = y0 + half * k_of(h1);
      const float h2 = h_of(u2);
      const float gu2 = vjp(dt * adj, u2, h2);
      const float gu1 = vjp(half * gu2, y0, h1);
      adj = adj + gu2 + gu1;
    } else {
      const float third = 1.0f / 3.0f;
      const float h1 = h_of(y0), k1 = k_of(h1);
      const float u2 = y0 + dt * k1 * third;
      const float h2 = h_of(u2), k2 = k_of(h2);
      const float u3 = y0 + dt * (k2 - k1 * third);
      const float h3 = h_of(u3), k3 = k_of(h3);
      const float u4 = y0 + dt * (k1 - k2 + k3);
      const float h4 = h_of(u4);
      const float l1 = dt * 0.125f * adj, l3 = 3.f * dt * 0.125f * adj;     // the b-weights' share of adj
      const float gu4 = vjp(l1, u4, h4);
      const float gu3 = vjp(l3 + dt * gu4, u3, h3);
      const float gu2 = vjp(l3 + dt * (gu3 - gu4), u2, h2);
      const float gu1 = vjp(l1 + dt * gu4 + dt * third * (gu2 - gu3), y0, h1);
      adj = adj + ((gu1 + gu2) + (gu3 + gu4));
    }
  };
#ifdef GODE_ODE_STAMPS
  st1 = __builtin_amdgcn_s_memtime();
#endif
  if (a.grid_dt == nullptr && a.substeps == 1) {
    // the grid is the output times: the step-start states are traj itself, read as the adjoint loop above reads it
    adj = upstream(T - 1);
    float y_next = (valid && T > 1) ? a.traj[((int64_t)n * T + (T - 2)) * 16 + i] : 0.f;
    for (int it = T - 1; it >= 1; --it) {
      const float y0 = y_next;
      const float up = upstream(it - 1);
      if (it > 1) y_next = valid ? a.traj[((int64_t)n * T + (it - 2)) * 16 + i] : 0.f;
      rstep(y0, a.dt[it - 1]);
      adj = adj + up;
    }
  } else {
    // substeps > 1 or a grid_dt grid: the forward is re-run from traj[n][0] (the pre-net output) with the forward kernel's
    // step, every step's start state goes to ysteps[n][s][:], and the steps are walked backwards.  A lane reads back only
    // what it wrote itself.
    const int S = a.grid_dt ? a.G : (T - 1) * a.substeps;
    float* ys = a.ysteps + (int64_t)n * S * 16 + i;          // (dereferenced by valid lanes only)
    auto dt_of = [&](int s) { return a.grid_dt ? a.grid_dt[s] : a.dt[s / a.substeps] / (float)a.substeps; };
    auto f = [&](float yy) { return k_of(h_of(yy)); };
    float y = valid ? a.traj[(int64_t)n * T * 16 + i] : 0.f;
    for (int s = 0; s < S; ++s) {
      if (valid) ys[(int64_t)s * 16] = y;
      y = fixed_step<METHOD>(f, y, dt_of(s));
    }
    int jo = T - 1;                                          // grid_dt: the next output to hand its gradient over
    float y_next = (valid && S > 0) ? ys[(int64_t)(S - 1) * 16] : 0.f;
    for (int s = S - 1; s >= 0; --s) {
      const float y0 = y_next;
      if (s > 0) y_next = valid ? ys[(int64_t)(s - 1) * 16] : 0.f;
      float after = 0.f;
      if (a.grid_dt) {
        // output jo = y0 + w (y1 - y0) of this step: w gz to dL/dy1 now, (1 - w) gz to dL/dy0 behind the reverse step
        while (jo >= 1 && a.emit_at[jo] == s) {
          const float w = a.emit_w[jo], g = upstream(jo);
          adj = adj + w * g;
          after = after + (1.f - w) * g;
          --jo;
        }
      } else if ((s + 1) % a.substeps == 0) {
        adj = adj + upstream((s + 1) / a.substeps);
      }
      rstep(y0, dt_of(s));
      adj = adj + after;
    }
    adj = adj + upstream(0);
  }
  }

#ifdef GODE_ODE_STAMPS
  st2 = __builtin_amdgcn_s_memtime();
#endif
  // ---- reduce over trajectories: 4 per wave by shuffles; every wave deposits its sums for ALL parameters in its own
  // LDS image of the gradient vector, ONE barrier at the very end, then the four images are added in fixed order and
  // written out coalesced.  (Writing each matrix to global memory as it was finished put a store drain -- the
  // s_waitcnt vmcnt(0) of the next barrier -- behind each of 17 pieces: 47k cycles.)
  auto put_matrix = [&](const W16& Gm, int off, int ld, int row0, int col0) {
    float t[16];      // the 16 shuffles of a level are independent: issue them all, then add (latency paid once per level)
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
    const float s = sum_traj(v);
    if (tl == 0) R[wave][off + i] = s;
  };
  put_matrix(gW1, OFF_W1, 16, 0, 0);
  if constexpr (RHS == RHS_MLP) put_matrix(gW2, OFF_W2, 16, 0, 0);
  put_vector(gb1, OFF_B1);
  if constexpr (RHS == RHS_MLP) put_vector(gb2, OFF_B2);

  // ---- pre-net backward; adj = dL/d(pre-net output)
  if (a.prenet) {
    float hpre[4];
    float acc = P[OFF_BB + i];
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      W16 wa, wb;
      load_rows(wa, P + OFF_WA, 16, 16 * m, 0, i, src);
      load_rows(wb, P + OFF_WB, 64, 0, 16 * m, i, src);
      hpre[m] = mv16(wa, x, P[OFF_BA + 16 * m + i]);
      acc = mv16(wb, lrelu1(hpre[m]), acc);
    }
    const float g0 = acc > 0.f ? adj : 0.2f * adj;
    put_vector(g0, OFF_BB);
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      W16 G, wbt;
#pragma unroll
      for (int r = 0; r < 16; ++r) G.w[r] = 0.f;
      outer16(G, g0, lrelu1(hpre[m]));                       // dWb[i][16m + j] = sum g0_i * lrelu(hpre)_j
      put_matrix(G, OFF_WB, 64, 0, 16 * m);
      load_cols(wbt, P + OFF_WB, 64, 0, 16 * m, i, src);      // (Wb chunk)^T
      const float t = mv16(wbt, g0, 0.f);
      const float gh = hpre[m] > 0.f ? t : 0.2f * t;
      put_vector(gh, OFF_BA + 16 * m);
#pragma unroll
      for (int r = 0; r < 16; ++r) G.w[r] = 0.f;
      outer16(G, gh, x);                                     // dWa[16m + i][j] = sum gh_i * x_j
      put_matrix(G, OFF_WA, 16, 16 * m, 0);
    }
  }
  __syncthreads();
  for (int k = threadIdx.x; k < NPAR; k += 256)     // (RHS_TANH: floats [OFF_W2, GODE_ODE_NPARAM) of the row stay unwritten)
    part[k] = (k < OFF_W1 && !a.prenet) ? 0.f : (R[0][k] + R[1][k]) + (R[2][k] + R[3][k]);
#ifdef GODE_ODE_STAMPS
  st3 = __builtin_amdgcn_s_memtime();
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    const long long rt1 = __builtin_amdgcn_s_memrealtime();
    printf("ode_bwd_valu stamps (cycles): setup %lld  time-loop %lld  epilogue %lld  total %lld | %.2f us, clock %.0f MHz (adj %g)\n",
           st1 - st0, st2 - st1, st3 - st2, st3 - st0, (double)(rt1 - rt0) / 100.0, (double)(st3 - st0) / ((double)(rt1 - rt0) / 100.0), (double)adj);
  }
#endif
}

// op->method picks the instantiation: 2 = euler, 3 = midpoint, anything else the rk4 kernels (0, and the adjoint's
// method 1 with substeps > 0: a dopri5 forward with a fixed Kutta-3/8 adjoint); op->rhs: 1 = RHS_TANH, else RHS_MLP.  The
// callers have checked both ranges.
template <int RHS>
static void launch_fwd(const gode_ode_fwd_op* op, dim3 grid, dim3 block, hipStream_t st) {
  if (op->method == METHOD_EULER) hipLaunchKernelGGL((ode_fwd_valu_kernel<METHOD_EULER, RHS>), grid, block, 0, st, *op);
  else if (op->method == METHOD_MIDPOINT) hipLaunchKernelGGL((ode_fwd_valu_kernel<METHOD_MIDPOINT, RHS>), grid, block, 0, st, *op);
  else hipLaunchKernelGGL((ode_fwd_valu_kernel<METHOD_RK4, RHS>), grid, block, 0, st, *op);
}
template <int RHS, int BACKPROP>
static void launch_bwd(const gode_ode_bwd_op* op, dim3 grid, dim3 block, hipStream_t st) {
  if (op->method == METHOD_EULER) hipLaunchKernelGGL((ode_bwd_valu_kernel<METHOD_EULER, RHS, BACKPROP>), grid, block, 0, st, *op);
  else if (op->method == METHOD_MIDPOINT) hipLaunchKernelGGL((ode_bwd_valu_kernel<METHOD_MIDPOINT, RHS, BACKPROP>), grid, block, 0, st, *op);
  else hipLaunchKernelGGL((ode_bwd_valu_kernel<METHOD_RK4, RHS, BACKPROP>), grid, block, 0, st, *op);
}
int gode_launch_ode_fwd_valu(const gode_ode_fwd_op* op, hipStream_t st) {
  const dim3 grid((op->N + 15) / 16), block(256);
  if (op->rhs == RHS_TANH) launch_fwd<RHS_TANH>(op, grid, block, st);
  else launch_fwd<RHS_MLP>(op, grid, block, st);
  GODE_LAUNCH_CHECK();
  return 0;
}
int gode_launch_ode_bwd_valu(const gode_ode_bwd_op* op, hipStream_t st) {
  const dim3 grid((op->N + 15) / 16), block(256);
  // op->backprop: 1 = discrete backprop (methods 0, 2, 3 only: the caller has refused method 1), else the adjoint
  if (op->backprop == BP_DISCRETE) {
    if (op->rhs == RHS_TANH) launch_bwd<RHS_TANH, BP_DISCRETE>(op, grid, block, st);
    else launch_bwd<RHS_MLP, BP_DISCRETE>(op, grid, block, st);
  } else if (op->rhs == RHS_TANH) launch_bwd<RHS_TANH, BP_ADJOINT>(op, grid, block, st);
  else launch_bwd<RHS_MLP, BP_ADJOINT>(op, grid, block, st);
  GODE_LAUNCH_CHECK();
  return 0;
}
