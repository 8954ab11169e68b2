// dnoise.hip -- discriminator instance noise (Noise(use_noise=True, sigma), models/mocogan.py:20-29): the noisy copy of a
// convolution's input, x + sigma * N(0, 1), written in one HBM pass.  The stream is the counter-based Philox / Box-Muller
// of philox.h with the counter layout of gode.h (element index, forward call, tagged stream | layer), so the values do not
// depend on the grid, the vector width or how the batch is split into shards.
//
// Roofline: the apply mode moves 8 B per element (read y, write the copy) and issues one Philox call (~100 integer ops)
// plus two log / sqrt / sincospi pairs per float4; the gather mode (layer 0, 1-3 input channels) reads the caller's
// strided tensor element by element.
#include "common.h"
#include "philox.h"

static inline uint32_t dnoise_tag(int32_t stream, int32_t layer) {
  return 0x80000000u | ((uint32_t)stream << 8) | (uint32_t)layer;
}

__device__ __forceinline__ uint32_t dnoise_call(const gode_dnoise_op& a) {
  return (a.call_dev ? (uint32_t)a.call_dev[0] : 0u) + (uint32_t)a.call;
}

// layers >= 1: act(BN(y)) + noise, one float4 (one Philox quad) per thread and step
__global__ void __launch_bounds__(256) dnoise_apply_kernel(const gode_dnoise_op a, NoiseArgs na) {
  const int64_t n4 = a.M * a.C / 4;
  const int64_t n4_0 = a.M0 > 0 ? a.M0 * a.C / 4 : n4;          // float4s of the first group
  const float neg = gode_act_neg_slope(a.act);
  const uint32_t call0 = dnoise_call(a);
  const uint64_t q_off = (uint64_t)a.e_off >> 2;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
    const bool g1 = i >= n4_0;
    const int c = (int)((i * 4) % a.C) + (g1 ? a.C : 0);          // second image group: + C
    f32x4 v = *reinterpret_cast<const f32x4*>(a.x + i * 4);
    f32x4 sc = {1.f, 1.f, 1.f, 1.f}, sh = {0.f, 0.f, 0.f, 0.f};
    if (a.scale) { sc = *reinterpret_cast<const f32x4*>(a.scale + c); sh = *reinterpret_cast<const f32x4*>(a.shift + c); }
#pragma unroll
    for (int e = 0; e < 4; ++e) { const float t = v[e] * sc[e] + sh[e]; v[e] = fmaxf(t, t * neg); }   // = gode_bn_apply
    NoiseArgs nq = na;
    nq.step = call0 + (g1 ? 1u : 0u);
    uint32_t w[4];
    philox_quad(q_off + (uint64_t)(g1 ? i - n4_0 : i), nq, w);
    const f32x4 z = box_muller4(w);
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = noise_add(v[e], z[e], na.sigma);
    *reinterpret_cast<f32x4*>(a.out + i * 4) = v;
  }
}

// layer 0: the caller's tensor through its element strides (folds a transpose(1, 2) view), one Philox quad per thread and
// step; the four elements of a quad are consecutive in the channels-last output
__global__ void __launch_bounds__(256) dnoise_gather_kernel(const gode_dnoise_op a, NoiseArgs na, FastDiv dC, FastDiv dW,
                                                            FastDiv dH, FastDiv dD) {
  const uint32_t n = (uint32_t)(a.M * a.C);                       // (< 2^31: checked by the launcher)
  const uint64_t e_off = (uint64_t)a.e_off;
  const uint64_t q_lo = e_off >> 2, q_hi = (e_off + n - 1) >> 2;
  na.step = dnoise_call(a);
  for (uint64_t q = q_lo + (uint64_t)blockIdx.x * 256 + threadIdx.x; q <= q_hi; q += (uint64_t)gridDim.x * 256) {
    uint32_t w[4];
    philox_quad(q, na, w);
    const f32x4 z = box_muller4(w);
#pragma unroll
    for (int l = 0; l < 4; ++l) {
      const int64_t i = (int64_t)(q * 4 + l) - (int64_t)e_off;
      if (i < 0 || i >= (int64_t)n) continue;
      uint32_t t = (uint32_t)i;
      const uint32_t t1 = fdiv(t, dC), c = t - t1 * dC.d;
      const uint32_t t2 = fdiv(t1, dW), ww = t1 - t2 * dW.d;
      const uint32_t t3 = fdiv(t2, dH), hh = t2 - t3 * dH.d;
      const uint32_t nn = fdiv(t3, dD), dd = t3 - nn * dD.d;
      const float x = a.x[(int64_t)nn * a.xs[0] + (int64_t)dd * a.xs[1] + (int64_t)hh * a.xs[2] + (int64_t)ww * a.xs[3] +
                          (int64_t)c * a.xs[4]];
      a.out[i] = noise_add(x, z[l], na.sigma);
    }
  }
}

extern "C" int gode_dnoise(const gode_dnoise_op* op, void* stream) {
  if (!op || !op->x || !op->out || op->M <= 0 || op->C <= 0 || op->e_off < 0 || op->stream < 0 || op->stream >= (1 << 23) ||
      op->layer < 0 || op->layer > 255 || !(op->sigma >= 0.f))
    return GODE_E_ARG;
  const NoiseArgs na = make_noise_args((uint64_t)op->seed, dnoise_tag(op->stream, op->layer), 0u, op->sigma);
  if (op->N > 0) {
    if (op->D <= 0 || op->H <= 0 || op->W <= 0 || (int64_t)op->N * op->D * op->H * op->W != op->M || op->M0 != 0 ||
        op->M * op->C >= (1ll << 31) || op->scale || op->shift)
      return GODE_E_ARG;
    const int64_t quads = (((op->e_off + op->M * op->C - 1) >> 2) - (op->e_off >> 2)) + 1;
    int64_t b = (quads + 255) / 256; if (b > 8192) b = 8192;
    hipLaunchKernelGGL(dnoise_gather_kernel, dim3((int)b), dim3(256), 0, (hipStream_t)stream, *op, na,
                       make_fastdiv((uint32_t)op->C), make_fastdiv((uint32_t)op->W), make_fastdiv((uint32_t)op->H),
                       make_fastdiv((uint32_t)op->D));
    GODE_LAUNCH_CHECK();
    return 0;
  }
  if (op->C % 4 != 0 || op->e_off % 4 != 0 || op->M0 < 0 || op->M0 >= op->M || ((uintptr_t)op->x % 16) != 0 ||
      ((uintptr_t)op->out % 16) != 0 || (op->scale == nullptr) != (op->shift == nullptr))
    return GODE_E_ARG;
  const int64_t b = (op->M * op->C / 4 + 255) / 256;
  hipLaunchKernelGGL(dnoise_apply_kernel, dim3((int)(b > 8192 ? 8192 : b)), dim3(256), 0, (hipStream_t)stream, *op, na);
  GODE_LAUNCH_CHECK();
  return 0;
}

extern "C" int gode_dnoise_normals(float* out, int64_t n, uint64_t seed, uint32_t noise_stream, uint32_t layer,
                                   uint32_t call, int64_t e_off, int32_t raw, void* stream) {
  if (noise_stream >= (1u << 23) || layer > 255u) return GODE_E_ARG;
  // the same kernel as gode_param_noise (sigma 1: fp32(z * 1) == z), on the tagged stream word with `call` as the step
  return gode_param_noise(out, n, seed, dnoise_tag((int32_t)noise_stream, (int32_t)layer), call, e_off, 1.f, raw ? 2 : 0,
                          stream);
}
