// philox.h -- the counter-based normal stream shared by the parameter noise (elementwise.hip) and the
// discriminator instance noise (dnoise.hip): Philox4x32-10 keyed by the seed, one call per quad of
// elements, 23-bit uniforms and Box-Muller through sincospif.  See gode.h for the counter layouts.
#pragma once
#include "common.h"

struct NoiseArgs { uint32_t k0, k1, stream, step; float sigma; };

__device__ __forceinline__ void philox4x32_10(uint32_t c[4], uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = __umulhi(0xD2511F53u, c[0]), lo0 = 0xD2511F53u * c[0];
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, c[2]), lo1 = 0xCD9E8D57u * c[2];
    const uint32_t n0 = hi1 ^ c[1] ^ k0, n2 = hi0 ^ c[3] ^ k1;
    c[0] = n0; c[1] = lo1; c[2] = n2; c[3] = lo0;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
}
__device__ __forceinline__ void philox_quad(uint64_t quad, const NoiseArgs& a, uint32_t c[4]) {
  c[0] = (uint32_t)quad; c[1] = a.step; c[2] = a.stream; c[3] = (uint32_t)(quad >> 32);
  philox4x32_10(c, a.k0, a.k1);
}
// 23 bits per uniform: (k + 0.5) * 2^-23 is exact in fp32 and lies in (0, 1)
__device__ __forceinline__ float noise_uniform(uint32_t x) { return ((float)(x >> 9) + 0.5f) * 0x1p-23f; }
__device__ __forceinline__ f32x4 box_muller4(const uint32_t c[4]) {
  const float r0 = sqrtf(-2.f * logf(noise_uniform(c[0]))), r2 = sqrtf(-2.f * logf(noise_uniform(c[2])));
  float s1, c1, s3, c3;
  sincospif(2.f * noise_uniform(c[1]), &s1, &c1);      // sin / cos of 2 pi u: u in revolutions, no range reduction
  sincospif(2.f * noise_uniform(c[3]), &s3, &c3);
  f32x4 z;
  z[0] = r0 * c1; z[1] = r0 * s1; z[2] = r2 * c3; z[3] = r2 * s3;
  return z;
}
// p + fp32(z * sigma), each operation rounded on its own: the library builds with -ffp-contract=fast, which fuses across
// pragmas and __fmul_rn / __fadd_rn alike, and a fused multiply-add here would differ from the reference's
// randn_like(p) * sigma followed by add_.  The empty asm statement makes the product opaque to the combiner (no code).
__device__ __forceinline__ float noise_scale(float z, float sigma) {
  float t = z * sigma;
  __asm__("" : "+v"(t));
  return t;
}
__device__ __forceinline__ float noise_add(float p, float z, float sigma) { return p + noise_scale(z, sigma); }
__device__ __forceinline__ float noise_elem(uint64_t e, const NoiseArgs& a) {
  uint32_t c[4];
  philox_quad(e >> 2, a, c);
  const f32x4 z = box_muller4(c);
  const int l = (int)(e & 3);
  return l == 0 ? z[0] : l == 1 ? z[1] : l == 2 ? z[2] : z[3];
}
static inline NoiseArgs make_noise_args(uint64_t seed, uint32_t stream, uint32_t step, float sigma) {
  NoiseArgs a; a.k0 = (uint32_t)seed; a.k1 = (uint32_t)(seed >> 32); a.stream = stream; a.step = step; a.sigma = sigma;
  return a;
}
