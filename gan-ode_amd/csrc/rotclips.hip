// rotclips.hip -- Rotated-MNIST clips built on the device: every digit rotated through K angles with the cubic
// B-spline rotation of scipy.ndimage.rotate(image, angle, reshape=False, cval=...) and every frame normalised min-max, as
// utils/images.py:101-173 (rotate_data) builds rot-mnist_rand.mat.
#include "common.h"

// ---------------------------------------------------------------------------------------------------------------
// gode_rot_clips: one workgroup per digit.  The image goes to LDS once (rows ROT_STRIDE(W) words apart: an odd stride, so the H
// lanes that walk the rows in the second prefilter pass fall on different banks, as the W lanes that walk the columns in the
// first do by themselves), the two passes of the recursive prefilter run one lane per line, and the K frames then read the same
// coefficients: per pixel the source point (two fused multiply-adds), the 4 x 4 taps with mirrored indices, the frame's minimum
// and maximum over the workgroup (order-independent: bit-identical from run to run), the division and the store.
#define ROT_MIN 4
#define ROT_MAX 64
#define ROT_STRIDE(W) ((W) | 1)

// One line of n coefficients `step` words apart, in place: gain 6, pole z = sqrt(3) - 2, the causal pass started for a mirror
// boundary (the exact sum over the period 2n - 2), the anticausal one from z / (z^2 - 1) * (c[n-1] + z c[n-2]).
__device__ __forceinline__ void rot_prefilter_line(float* c, const int n, const int step) {
  const float z = -0.26794919243112270647f, gain = 6.f;
  float zn1 = 1.f;
  for (int i = 1; i < n; ++i) zn1 *= z;                       // z^(n-1)
  float acc = gain * (c[0] + zn1 * c[(n - 1) * step]), zi = z;
  for (int i = 1; i < n - 1; ++i) {
    acc = fmaf(zi, gain * (c[i * step] + zn1 * c[(n - 1 - i) * step]), acc);
    zi *= z;
  }
  float prev = acc / (1.f - zn1 * zn1);
  c[0] = prev;
  for (int i = 1; i < n; ++i) {
    prev = fmaf(z, prev, gain * c[i * step]);
    c[i * step] = prev;
  }
  prev = (z * c[(n - 2) * step] + prev) * (z / (z * z - 1.f));
  c[(n - 1) * step] = prev;
  for (int i = n - 2; i >= 0; --i) {
    prev = z * (prev - c[i * step]);
    c[i * step] = prev;
  }
}

__device__ __forceinline__ int rot_mirror(int i, const int n) {          // i in [-1, n + 1], n >= 3
  i = i < 0 ? -i : i;
  return i > n - 1 ? 2 * (n - 1) - i : i;
}
__device__ __forceinline__ void rot_weights(const float t, float* w) {
  const float u = 1.f - t, t2 = t * t, t3 = t2 * t;
  w[0] = u * u * u * (1.f / 6.f);
  w[1] = (3.f * t3 - 6.f * t2 + 4.f) * (1.f / 6.f);
  w[2] = (-3.f * t3 + 3.f * t2 + 3.f * t + 1.f) * (1.f / 6.f);
  w[3] = t3 * (1.f / 6.f);
}

__global__ void __launch_bounds__(256) rot_clips_kernel(const gode_rot_clips_op a, const FastDiv div_w) {
  extern __shared__ float lds[];             // coef [H][S] | frame [H * W] | wave partials [2][4][2]
  const int H = a.H, W = a.W, S = ROT_STRIDE(W), HW = H * W;
  float* coef = lds;
  float* frame = lds + H * S;
  float* part = frame + HW;
  const int tid = threadIdx.x;
  const int64_t d = blockIdx.x;

  if (a.in_u8) {
    const uint8_t* src = static_cast<const uint8_t*>(a.images) + d * HW;
    for (int p = tid; p < HW; p += 256) {
      const int y = (int)fdiv((uint32_t)p, div_w), x = p - y * W;
      coef[y * S + x] = fmaf(((float)src[p] - 127.5f) / 255.0f, a.in_scale, a.in_shift);
    }
  } else {
    const float* src = static_cast<const float*>(a.images) + d * HW;
    for (int p = tid; p < HW; p += 256) {
      const int y = (int)fdiv((uint32_t)p, div_w), x = p - y * W;
      coef[y * S + x] = fmaf(src[p], a.in_scale, a.in_shift);
    }
  }
  __syncthreads();
  if (tid < W) rot_prefilter_line(coef + tid, H, S);          // axis 0: lane = column
  __syncthreads();
  if (tid < H) rot_prefilter_line(coef + tid * S, W, 1);      // axis 1: lane = row
  __syncthreads();

  const float cy = 0.5f * (float)(H - 1), cx = 0.5f * (float)(W - 1), ymax = (float)(H - 1), xmax = (float)(W - 1);
  const float inf = __builtin_inff();
  for (int k = 0; k < a.K; ++k) {
    const float* cs = a.cs + (d * a.K + k) * 2;
    const float c = cs[0], s = cs[1];
    float mn = inf, mx = -inf;
    for (int p = tid; p < HW; p += 256) {
      const int y = (int)fdiv((uint32_t)p, div_w), x = p - y * W;
      const float dy = (float)y - cy, dx = (float)x - cx;
      const float py = fmaf(c, dy, fmaf(s, dx, cy));
      const float px = fmaf(c, dx, fmaf(-s, dy, cx));
      float v = a.cval;
      if (py >= 0.f && py <= ymax && px >= 0.f && px <= xmax) {           // a NaN coordinate takes cval too
        const float fy = floorf(py), fx = floorf(px);
        float wy[4], wx[4];
        rot_weights(py - fy, wy);
        rot_weights(px - fx, wx);
        const int iy = (int)fy - 1, ix = (int)fx - 1;
        int xs[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) xs[i] = rot_mirror(ix + i, W);
        v = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float* row = coef + rot_mirror(iy + j, H) * S;
          float r = wx[0] * row[xs[0]];
#pragma unroll
          for (int i = 1; i < 4; ++i) r = fmaf(wx[i], row[xs[i]], r);
          v = fmaf(wy[j], r, v);
        }
      }
      frame[p] = v;                          // read back by this thread only
      mn = fminf(mn, v);
      mx = fmaxf(mx, v);
    }
    const int64_t o = (d * a.K + k) * HW;
    if (a.raw)
      for (int p = tid; p < HW; p += 256) a.raw[o + p] = frame[p];
    if (a.out) {
#pragma unroll
      for (int m = 32; m >= 1; m >>= 1) {
        mn = fminf(mn, __shfl_xor(mn, m, 64));
        mx = fmaxf(mx, __shfl_xor(mx, m, 64));
      }
      float* slot = part + (k & 1) * 8;      // two slots in turn: one barrier per frame keeps writers off the readers' slot
      if ((tid & 63) == 0) { slot[(tid >> 6) * 2] = mn; slot[(tid >> 6) * 2 + 1] = mx; }
      __syncthreads();
      mn = fminf(fminf(slot[0], slot[2]), fminf(slot[4], slot[6]));
      mx = fmaxf(fmaxf(slot[1], slot[3]), fmaxf(slot[5], slot[7]));
      // X / (max - min), then minus the minimum of that quotient (utils/images.py:166-167); a constant frame divides by zero
      const float range = mx - mn, lo = mn / range;
      for (int p = tid; p < HW; p += 256) a.out[o + p] = frame[p] / range - lo;
    }
  }
}

extern "C" int gode_rot_clips(const gode_rot_clips_op* op, void* stream) {
  if (!op || !op->images || !op->cs || (!op->out && !op->raw) || op->n <= 0 || op->K <= 0 || (op->in_u8 != 0 && op->in_u8 != 1))
    return GODE_E_ARG;
  if (op->H < ROT_MIN || op->H > ROT_MAX || op->W < ROT_MIN || op->W > ROT_MAX) return GODE_E_SHAPE;
  const size_t lds = (size_t)(op->H * ROT_STRIDE(op->W) + op->H * op->W + 16) * sizeof(float);     // <= 33,088 bytes
  hipLaunchKernelGGL(rot_clips_kernel, dim3((uint32_t)op->n), dim3(256), lds, (hipStream_t)stream, *op,
                     make_fastdiv((uint32_t)op->W));
  GODE_LAUNCH_CHECK();
  return 0;
}
