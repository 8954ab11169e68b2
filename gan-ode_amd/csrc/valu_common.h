// valu_common.h -- the VECTOR-ALU / DPP mapping of the 16-wide mat-vecs shared by the *_valu.hip kernels: one lane = one
// (trajectory, feature) pair, the 16 features of a trajectory in one DPP row (16 lanes), 4 trajectories per wave (see the
// header comment of ode_valu.hip); the staging of the gode_ode_params block, the pre-net on it, and the whole-batch sum
// with its cross-workgroup exchange.
#pragma once
#include "common.h"
#include "ode_common.h"

template <int R> __device__ __forceinline__ float row_ror(float v) {
  if (R == 0) return v;
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x120 + (R & 15), 0xf, 0xf, false));
}

struct W16 { float w[16]; };

// out_i = bias_i + sum_r W.w[r] * y[src(i, r)].  hipcc does not fold a DPP move into v_fmac (it emits v_mov_b32_dpp +
// v_fmac, or SLP-packs the FMAs into v_pk_fma_f32, which has no DPP form): the 16 instructions are written out.  The
// leading s_nop 1 covers the 2 wait states a DPP read needs after a VALU write of the same VGPR (the rotated operand
// is produced by compiler-scheduled code just before the block); accumulators are plain operands.
__device__ __forceinline__ float mv16(const W16& W, float y, float bias) {
  float a0, a1, a2, a3;
  asm("s_nop 1\n\t"
      "v_fma_f32 %0, %5, %4, %21\n\t"
      "v_mul_f32_dpp %1, %4, %6 row_ror:1 row_mask:0xf bank_mask:0xf\n\t"
      "v_mul_f32_dpp %2, %4, %7 row_ror:2 row_mask:0xf bank_mask:0xf\n\t"
      "v_mul_f32_dpp %3, %4, %8 row_ror:3 row_mask:0xf bank_mask:0xf\n\t"
      "v_fmac_f32_dpp %0, %4, %9 row_ror:4 row_mask:0xf bank_mask:0xf\n\t"
      "v_fmac_f32_dpp %1, %4, %10 row_ror:5 row_mask:0xf bank_mask:0xf\n\t"
      "v_fmac_f32_dpp %2, %4, %11 row_ror:6 row_mask:0xf bank_mask:0xf\n\t"
      "v_fmac_f32_dpp %3, %4, %12 row_ror:7 row_mask:0xf bank_mask:0xf\n\t"
      "v_fmac_f32_dpp %0, %4, %13 row_ror:8 row_mask:0xf bank_mask:0xf\n\t"
      "v_fmac_f32_dpp %1, %4, %14 row_ror:9 row_mask:0xf bank_mask:0xf\n\t"
      "v_fmac_f32_dpp %2, %4, %15 row_ror:10 row_mask:0xf bank_mask:0xf\n\t"
      "v_fmac_f32_dpp %3, %4, %16 row_ror:11 row_mask:0xf bank_mask:0xf\n\t"
      "v_fmac_f32_dpp %0, %4, %17 row_ror:12 row_mask:0xf bank_mask:0xf\n\t"
      "v_fmac_f32_dpp %1, %4, %18 row_ror:13 row_mask:0xf bank_mask:0xf\n\t"
      "v_fmac_f32_dpp %2, %4, %19 row_ror:14 row_mask:0xf bank_mask:0xf\n\t"
      "v_fmac_f32_dpp %3, %4, %20 row_ror:15 row_mask:0xf bank_mask:0xf"
      : "=&v"(a0), "=&v"(a1), "=&v"(a2), "=&v"(a3)
      : "v"(y), "v"(W.w[0]), "v"(W.w[1]), "v"(W.w[2]), "v"(W.w[3]), "v"(W.w[4]), "v"(W.w[5]), "v"(W.w[6]), "v"(W.w[7]), "v"(W.w[8]), "v"(W.w[9]), "v"(W.w[10]), "v"(W.w[11]), "v"(W.w[12]), "v"(W.w[13]), "v"(W.w[14]), "v"(W.w[15]), "v"(bias));
  return (a0 + a1) + (a2 + a3);
}
// The same product as ONE dependent chain (16 instructions instead of 19, no adds at the end): for kernels that run two
// waves per SIMD and are bound by vector-ALU issue, not by the length of the dependent chain (odernn_valu.hip).
__device__ __forceinline__ float mv16c(const W16& W, float y, float bias) {
  float a0;
  asm("s_nop 1\n\t"
      "v_fma_f32 %0, %2, %1, %18\n\t"
      "v_fmac_f32_dpp %0, %1, %3 row_ror:1 row_mask:0xf bank_mask:0xf\n\t"
      "v_fmac_f32_dpp %0, %1, %4 row_ror:2 row_mask:0xf bank_mask:0xf\n\t"
      "v_fmac_f32_dpp %0, %1, %5 row_ror:3 row_mask:0xf bank_mask:0xf\n\t"
      "v_fmac_f32_dpp %0, %1, %6 row_ror:4 row_mask:0xf bank_mask:0xf\n\t"
      "v_fmac_f32_dpp %0, %1, %7 row_ror:5 row_mask:0xf bank_mask:0xf\n\t"
      "v_fmac_f32_dpp %0, %1, %8 row_ror:6 row_mask:0xf bank_mask:0xf\n\t"
      "v_fmac_f32_dpp %0, %1, %9 row_ror:7 row_mask:0xf bank_mask:0xf\n\t"
      "v_fmac_f32_dpp %0, %1, %10 row_ror:8 row_mask:0xf bank_mask:0xf\n\t"
      "v_fmac_f32_dpp %0, %1, %11 row_ror:9 row_mask:0xf bank_mask:0xf\n\t"
      "v_fmac_f32_dpp %0, %1, %12 row_ror:10 row_mask:0xf bank_mask:0xf\n\t"
      "v_fmac_f32_dpp %0, %1, %13 row_ror:11 row_mask:0xf bank_mask:0xf\n\t"
      "v_fmac_f32_dpp %0, %1, %14 row_ror:12 row_mask:0xf bank_mask:0xf\n\t"
      "v_fmac_f32_dpp %0, %1, %15 row_ror:13 row_mask:0xf bank_mask:0xf\n\t"
      "v_fmac_f32_dpp %0, %1, %16 row_ror:14 row_mask:0xf bank_mask:0xf\n\t"
      "v_fmac_f32_dpp %0, %1, %17 row_ror:15 row_mask:0xf bank_mask:0xf"
      : "=&v"(a0)
      : "v"(y), "v"(W.w[0]), "v"(W.w[1]), "v"(W.w[2]), "v"(W.w[3]), "v"(W.w[4]), "v"(W.w[5]), "v"(W.w[6]), "v"(W.w[7]), "v"(W.w[8]), "v"(W.w[9]), "v"(W.w[10]), "v"(W.w[11]), "v"(W.w[12]), "v"(W.w[13]), "v"(W.w[14]), "v"(W.w[15]), "v"(bias));
  return a0;
}
// G.w[r] += p * q[src(i, r)]   (per-lane slice of the outer product p q^T)
__device__ __forceinline__ void outer16(W16& G, float p, float q) {
  asm("s_nop 1\n\t"
      "v_fmac_f32 %0, %17, %16\n\t"
      "v_fmac_f32_dpp %1, %17, %16 row_ror:1 row_mask:0xf bank_mask:0xf\n\t"
      "v_fmac_f32_dpp %2, %17, %16 row_ror:2 row_mask:0xf bank_mask:0xf\n\t"
      "v_fmac_f32_dpp %3, %17, %16 row_ror:3 row_mask:0xf bank_mask:0xf\n\t"
      "v_fmac_f32_dpp %4, %17, %16 row_ror:4 row_mask:0xf bank_mask:0xf\n\t"
      "v_fmac_f32_dpp %5, %17, %16 row_ror:5 row_mask:0xf bank_mask:0xf\n\t"
      "v_fmac_f32_dpp %6, %17, %16 row_ror:6 row_mask:0xf bank_mask:0xf\n\t"
      "v_fmac_f32_dpp %7, %17, %16 row_ror:7 row_mask:0xf bank_mask:0xf\n\t"
      "v_fmac_f32_dpp %8, %17, %16 row_ror:8 row_mask:0xf bank_mask:0xf\n\t"
      "v_fmac_f32_dpp %9, %17, %16 row_ror:9 row_mask:0xf bank_mask:0xf\n\t"
      "v_fmac_f32_dpp %10, %17, %16 row_ror:10 row_mask:0xf bank_mask:0xf\n\t"
      "v_fmac_f32_dpp %11, %17, %16 row_ror:11 row_mask:0xf bank_mask:0xf\n\t"
      "v_fmac_f32_dpp %12, %17, %16 row_ror:12 row_mask:0xf bank_mask:0xf\n\t"
      "v_fmac_f32_dpp %13, %17, %16 row_ror:13 row_mask:0xf bank_mask:0xf\n\t"
      "v_fmac_f32_dpp %14, %17, %16 row_ror:14 row_mask:0xf bank_mask:0xf\n\t"
      "v_fmac_f32_dpp %15, %17, %16 row_ror:15 row_mask:0xf bank_mask:0xf"
      : "+v"(G.w[0]), "+v"(G.w[1]), "+v"(G.w[2]), "+v"(G.w[3]), "+v"(G.w[4]), "+v"(G.w[5]), "+v"(G.w[6]), "+v"(G.w[7]), "+v"(G.w[8]), "+v"(G.w[9]), "+v"(G.w[10]), "+v"(G.w[11]), "+v"(G.w[12]), "+v"(G.w[13]), "+v"(G.w[14]), "+v"(G.w[15])
      : "v"(p), "v"(q));
}
// src[r] = the row-local lane whose value rotation r delivers to this lane
__device__ __forceinline__ void probe_sources(int i, int* src) {
  const float fi = (float)i;
  src[0] = i;
  src[1] = (int)row_ror<1>(fi);   src[2] = (int)row_ror<2>(fi);   src[3] = (int)row_ror<3>(fi);
  src[4] = (int)row_ror<4>(fi);   src[5] = (int)row_ror<5>(fi);   src[6] = (int)row_ror<6>(fi);
  src[7] = (int)row_ror<7>(fi);   src[8] = (int)row_ror<8>(fi);   src[9] = (int)row_ror<9>(fi);
  src[10] = (int)row_ror<10>(fi); src[11] = (int)row_ror<11>(fi); src[12] = (int)row_ror<12>(fi);
  src[13] = (int)row_ror<13>(fi); src[14] = (int)row_ror<14>(fi); src[15] = (int)row_ror<15>(fi);
}
// rows of a row-major [rows][ld] matrix: w[r] = M[(row0 + i) * ld + col0 + src[r]]
__device__ __forceinline__ void load_rows(W16& W, const float* M, int ld, int row0, int col0, int i, const int* src) {
#pragma unroll
  for (int r = 0; r < 16; ++r) W.w[r] = M[(row0 + i) * ld + col0 + src[r]];
}
// transposed: w[r] = M[(row0 + src[r]) * ld + col0 + i]  (so that mv16 computes M^T v)
__device__ __forceinline__ void load_cols(W16& W, const float* M, int ld, int row0, int col0, int i, const int* src) {
#pragma unroll
  for (int r = 0; r < 16; ++r) W.w[r] = M[(row0 + src[r]) * ld + col0 + i];
}
__device__ __forceinline__ float lrelu1(float u) { return u > 0.f ? u : 0.2f * u; }


// ---- reductions ---------------------------------------------------------------------------------------------------
// Sum over the 64 lanes of a wave, the same value in every lane, fixed order: four row rotations make every lane hold
// its row's sum, the four row sums are read out with v_readlane and added as (r0 + r1) + (r2 + r3).  ~10 VALU issue slots
// against six dependent ds_bpermute round trips (~100+ cycles each) for the __shfl_xor butterfly.
__device__ __forceinline__ float wave_sum(float v) {
  v += row_ror<8>(v);
  v += row_ror<4>(v);
  v += row_ror<2>(v);
  v += row_ror<1>(v);
  const int b = __builtin_bit_cast(int, v);
  const float r0 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 0));
  const float r1 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 16));
  const float r2 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 32));
  const float r3 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 48));
  return (r0 + r1) + (r2 + r3);
}
// sum over the 4 trajectories of a wave (lanes i, i+16, i+32, i+48), the result in every lane, fixed order
__device__ __forceinline__ float traj_sum(float v) {
  const int b = __builtin_bit_cast(int, v);
  const int i = threadIdx.x & 15;
  // four readlanes cannot take a per-lane index; the row partner values come through LDS-less cross-lane reads
  const float a = __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute((i) << 2, b));
  const float c = __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute((i + 16) << 2, b));
  const float d = __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute((i + 32) << 2, b));
  const float e = __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute((i + 48) << 2, b));
  return (a + c) + (d + e);
}
// the same sum, (a + c) + (d + e) in every lane, as two butterfly levels: ode_bwd_valu_kernel's form, kept beside traj_sum because swapping it changes that kernel's instructions
__device__ __forceinline__ float sum_traj(float v) {
  v += __shfl_xor(v, 16);
  v += __shfl_xor(v, 32);
  return v;
}


// ---- the gode_ode_params block in LDS ------------------------------------------------------------------------------
// All 2,672 parameters (10.7 KB) go to LDS with ONE round of coalesced loads before anything else: the per-lane weight
// arrangement is then gathered from LDS.  (Gathering it from global memory cost the config-size adjoint launch more
// than its whole time loop: twelve dependent batches of L2-missing loads in the pre-net backward, 60k of 126k cycles.)
// RHS: the `rhs` code of gode.h the calling kernel is compiled for.  RHS_TANH (f(y) = tanh(W1 y + b1)): p.W2 / p.b2 are not
// dereferenced and the block ends behind b1 (P holds OFF_W2 floats).
enum { RHS_MLP = 0, RHS_TANH = 1 };
template <int THREADS, int RHS = RHS_MLP>
__device__ __forceinline__ void stage_ode_params(const gode_ode_params& p, int prenet, float* P) {
  const int t = threadIdx.x;
  if (prenet) {
    for (int k = t; k < 1024; k += THREADS) { P[OFF_WA + k] = p.Wa[k]; P[OFF_WB + k] = p.Wb[k]; }
    if (t < 64) P[OFF_BA + t] = p.ba[t];
    if (t < 16) P[OFF_BB + t] = p.bb[t];
  }
  static_assert(THREADS >= 256, "one 16x16 matrix per round");
  if constexpr (RHS == RHS_TANH) {
    if (THREADS == 256 || t < 256) P[OFF_W1 + t] = p.W1[t];
    if (t < 16) P[OFF_B1 + t] = p.b1[t];
  } else {
    if (THREADS == 256 || t < 256) { P[OFF_W1 + t] = p.W1[t]; P[OFF_W2 + t] = p.W2[t]; }     // (256 threads: no guard)
    if (t < 16) { P[OFF_B1 + t] = p.b1[t]; P[OFF_B2 + t] = p.b2[t]; }
  }
  __syncthreads();
}
// pre-net Linear(16,64) -> LReLU -> Linear(64,16) -> LReLU on a staged block whose first four tensors are Wa, ba, Wb, bb:
// the 64 hidden units as four row-resident chunks (not unrolled: two weight arrangements live at a time)
__device__ __forceinline__ float prenet_fwd(const float* P, float y, int i, const int* src) {
  float acc = P[OFF_BB + i];
#pragma unroll 1
  for (int m = 0; m < 4; ++m) {
    W16 wa, wb;
    load_rows(wa, P + OFF_WA, 16, 16 * m, 0, i, src);
    load_rows(wb, P + OFF_WB, 64, 0, 16 * m, i, src);
    const float h = lrelu1(mv16(wa, y, P[OFF_BA + 16 * m + i]));
    acc = mv16(wb, h, acc);
  }
  return lrelu1(acc);
}


// ---- whole-batch sums ----------------------------------------------------------------------------------------------
// The workgroups of a call exchange partial sums through the caller's `sync` buffer: XS_HDR ints (sync[0] counts the
// arrivals over all exchanges of the launch; the host zeroes the header before every launch), then the slots.
#define XS_HDR 16
struct XSync {
  int* counter;     // sync[0]
  float* slots;     // sync + XS_HDR: [2][nwg][VALS] partial sums, double-buffered by exchange parity
  int nwg, wg, seq;
};
// WAVES waves per workgroup, VALS floats per slot; PAIRWISE: the 4 per-wave partials are added as (r0 + r1) + (r2 + r3)
// instead of one after the other (the order is part of each kernel's results: do not change it)
template <int WAVES, int VALS, bool PAIRWISE = false>
struct RedLds {
  float red[2][WAVES][VALS];         // per-wave partials, double-buffered: one barrier per sum
  float bc[2][VALS];                 // cross-workgroup totals broadcast to the workgroup
  int dead;                          // a spin timed out somewhere: every thread of the workgroup bails out
};
// ONE thread of the workgroup: publish what the workgroup stored (release), then wait until every workgroup of the call
// has arrived at exchange X.seq.  The spin is bounded; a workgroup that never arrives sets *dead instead of hanging us.
__device__ __forceinline__ void xs_arrive_and_wait(const XSync& X, int* dead) {
  __hip_atomic_fetch_add(X.counter, 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
  const int target = (X.seq + 1) * X.nwg;
  int spins = 0;
  while (__hip_atomic_load(X.counter, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) < target) {
    __builtin_amdgcn_s_sleep(2);
    if (++spins > (1 << 20)) { *dead = 1; break; }     // ~seconds: a workgroup of the call never arrived
  }
}
// v[0..K): per-thread values -> the sums over ALL threads of ALL workgroups of the call, in every thread, fixed order.
template <int K, int WAVES, int VALS, bool PAIRWISE>
__device__ __forceinline__ void batch_sum(float* v, RedLds<WAVES, VALS, PAIRWISE>& R, int& par, XSync& X) {
  static_assert(K <= VALS && (!PAIRWISE || WAVES == 4), "batch_sum");
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < K; ++k) v[k] = wave_sum(v[k]);
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < K; ++k) R.red[par][wave][k] = v[k];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < K; ++k) {
    if constexpr (PAIRWISE) {
      v[k] = (R.red[par][0][k] + R.red[par][1][k]) + (R.red[par][2][k] + R.red[par][3][k]);
    } else {
      float s = 0.f;
#pragma unroll
      for (int w = 0; w < WAVES; ++w) s += R.red[par][w][k];
      v[k] = s;
    }
  }
  if (X.nwg > 1) {
    float* slot = X.slots + (size_t)(X.seq & 1) * X.nwg * VALS;
    if (wave == 0) {
      if (lane == 0) {
#pragma unroll
        for (int k = 0; k < K; ++k) __hip_atomic_store(&slot[X.wg * VALS + k], v[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        xs_arrive_and_wait(X, &R.dead);
      }
      float t[K];
#pragma unroll
      for (int k = 0; k < K; ++k) t[k] = 0.f;
      for (int w = lane; w < X.nwg; w += 64) {
#pragma unroll
        for (int k = 0; k < K; ++k) t[k] += __hip_atomic_load(&slot[w * VALS + k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
#pragma unroll
      for (int k = 0; k < K; ++k) t[k] = wave_sum(t[k]);
      if (lane == 0) {
#pragma unroll
        for (int k = 0; k < K; ++k) R.bc[par][k] = t[k];
      }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = R.bc[par][k];
    X.seq += 1;
  }
  par ^= 1;
}
