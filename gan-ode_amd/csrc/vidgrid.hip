// vidgrid.hip -- gode_video_grid: a batch of fp32 videos, read in place through its strides, becomes the
// 8-bit frames of a sample grid (the drivers' genSamples: tile, (x + 1) / 2 * 255, clip, truncate) and their palette indices.
// Memory-bound: 4 to 12 bytes read and 1 to 4 written per pixel, no reuse, so no LDS and nothing shared between threads.
#include "common.h"

#define VG_MAX_SIDE 16384

// gw: the items of one grid row (pixels, or groups of four); h: H; w: the items of one tile row
struct VgDiv { FastDiv gw, h, w; };

// One value through the reference's float64 expression, clipped and truncated.  No contraction: every operation rounds once, as
// NumPy's does ((x + 1) / 2 * 255 holds no multiply-add to fuse; the pragma keeps that true whatever the flags).
__device__ __forceinline__ uint32_t vg_byte(const float x, const int mode) {
#pragma clang fp contract(off)
  double v = mode == 0 ? ((double)x + 1.0) / 2.0 * 255.0 : (double)x * 255.0;
  v = v < 0.0 ? 0.0 : v;
  v = v > 255.0 ? 255.0 : v;
  return (uint32_t)v;
}

// cell of the 6 x 7 x 6 cube: q = (v * (L - 1) + 127) / 255 per channel
__device__ __forceinline__ uint32_t vg_cube(const uint32_t r, const uint32_t g, const uint32_t b) {
  return (((r * 5u + 127u) / 255u) * 7u + (g * 6u + 127u) / 255u) * 6u + (b * 5u + 127u) / 255u;
}

__device__ __forceinline__ uint32_t vg_pack(const uint32_t b0, const uint32_t b1, const uint32_t b2, const uint32_t b3) {
  return b0 | (b1 << 8) | (b2 << 16) | (b3 << 24);
}

// Four consecutive pixels of a grid row per thread (W % 4 == 0, so the four lie in one tile): C floats4 in, one dword of
// indices and three dwords of colour bytes out.  The frames are walked by blockIdx.y.
template <int C>
__global__ void __launch_bounds__(256) vidgrid_vec4_kernel(const gode_video_grid_op a, const VgDiv d, const uint32_t items) {
  const uint32_t p = blockIdx.x * 256u + threadIdx.x;
  if (p >= items) return;
  const uint32_t W4 = (uint32_t)a.W >> 2, GW4 = (uint32_t)a.cols * W4;
  const uint32_t gy = fdiv(p, d.gw), g4 = p - gy * GW4;
  const uint32_t r = fdiv(gy, d.h), y = gy - r * (uint32_t)a.H;
  const uint32_t c = fdiv(g4, d.w), x = (g4 - c * W4) * 4u;
  const uint32_t b = r * (uint32_t)a.cols + c;
  const bool filled = b < (uint32_t)a.B;
  const int64_t GH = (int64_t)a.rows * a.H, GW = (int64_t)a.cols * a.W;
  const float* row = a.src + (int64_t)b * a.xs[0] + (int64_t)y * a.xs[3] + (int64_t)x * C;      // xs[4] == C on this path
  for (int t = blockIdx.y; t < a.T; t += gridDim.y) {
    uint32_t v[4 * C];
    if (filled) {
      const f32x4* s = reinterpret_cast<const f32x4*>(row + (int64_t)t * a.xs[2]);
#pragma unroll
      for (int k = 0; k < C; ++k) {
        const f32x4 q = s[k];
        v[4 * k] = vg_byte(q.x, a.mode); v[4 * k + 1] = vg_byte(q.y, a.mode);
        v[4 * k + 2] = vg_byte(q.z, a.mode); v[4 * k + 3] = vg_byte(q.w, a.mode);
      }
    } else {
      const uint32_t z = vg_byte(0.f, a.mode);
#pragma unroll
      for (int k = 0; k < 4 * C; ++k) v[k] = z;
    }
    const int64_t o = ((int64_t)t * GH + gy) * GW + (int64_t)g4 * 4;
    if (a.rgb) {
      uint32_t* dst = reinterpret_cast<uint32_t*>(a.rgb + o * 3);
      if constexpr (C == 3) {
        dst[0] = vg_pack(v[0], v[1], v[2], v[3]);
        dst[1] = vg_pack(v[4], v[5], v[6], v[7]);
        dst[2] = vg_pack(v[8], v[9], v[10], v[11]);
      } else {
        dst[0] = vg_pack(v[0], v[0], v[0], v[1]);
        dst[1] = vg_pack(v[1], v[1], v[2], v[2]);
        dst[2] = vg_pack(v[2], v[3], v[3], v[3]);
      }
    }
    if (a.idx) {
      uint32_t* dst = reinterpret_cast<uint32_t*>(a.idx + o);
      if constexpr (C == 3)
        dst[0] = vg_pack(vg_cube(v[0], v[1], v[2]), vg_cube(v[3], v[4], v[5]), vg_cube(v[6], v[7], v[8]),
                         vg_cube(v[9], v[10], v[11]));
      else
        dst[0] = vg_pack(v[0], v[1], v[2], v[3]);
    }
  }
}

// One pixel per thread through all five strides: whole-byte stores, each byte written by exactly one thread.
__global__ void __launch_bounds__(256) vidgrid_strided_kernel(const gode_video_grid_op a, const VgDiv d, const uint32_t items) {
  const uint32_t p = blockIdx.x * 256u + threadIdx.x;
  if (p >= items) return;
  const uint32_t GWp = (uint32_t)a.cols * (uint32_t)a.W;
  const uint32_t gy = fdiv(p, d.gw), gx = p - gy * GWp;
  const uint32_t r = fdiv(gy, d.h), y = gy - r * (uint32_t)a.H;
  const uint32_t c = fdiv(gx, d.w), x = gx - c * (uint32_t)a.W;
  const uint32_t b = r * (uint32_t)a.cols + c;
  const bool filled = b < (uint32_t)a.B;
  const int64_t GH = (int64_t)a.rows * a.H, GW = (int64_t)GWp;
  const float* px = a.src + (int64_t)b * a.xs[0] + (int64_t)y * a.xs[3] + (int64_t)x * a.xs[4];
  for (int t = blockIdx.y; t < a.T; t += gridDim.y) {
    uint32_t v0, v1, v2;
    if (filled) {
      const float* s = px + (int64_t)t * a.xs[2];
      v0 = vg_byte(s[0], a.mode);
      if (a.C == 3) { v1 = vg_byte(s[a.xs[1]], a.mode); v2 = vg_byte(s[2 * a.xs[1]], a.mode); }
      else v1 = v2 = v0;
    } else {
      v0 = v1 = v2 = vg_byte(0.f, a.mode);
    }
    const int64_t o = ((int64_t)t * GH + gy) * GW + gx;
    if (a.rgb) {
      uint8_t* dst = a.rgb + o * 3;
      dst[0] = (uint8_t)v0; dst[1] = (uint8_t)v1; dst[2] = (uint8_t)v2;
    }
    if (a.idx) a.idx[o] = (uint8_t)(a.C == 3 ? vg_cube(v0, v1, v2) : v0);
  }
}

// 0 and kind (1: four pixels per thread, 0: strided), or the refusal
static int vg_plan(const gode_video_grid_op* op, int32_t* kind) {
  if (!op || !op->src || (!op->rgb && !op->idx) || (op->C != 1 && op->C != 3) || (op->mode != 0 && op->mode != 1) || op->B < 1)
    return GODE_E_ARG;
  if (op->T < 1 || op->H < 1 || op->W < 1 || op->rows < 1 || op->cols < 1) return GODE_E_SHAPE;
  if ((int64_t)op->rows * op->H > VG_MAX_SIDE || (int64_t)op->cols * op->W > VG_MAX_SIDE) return GODE_E_SHAPE;
  if ((int64_t)op->B > (int64_t)op->rows * op->cols) return GODE_E_ARG;
  const bool layout = op->C == 1 ? op->xs[4] == 1 : (op->xs[1] == 1 && op->xs[4] == 3);
  const bool aligned = ((uintptr_t)op->src & 15) == 0 && op->xs[0] % 4 == 0 && op->xs[2] % 4 == 0 && op->xs[3] % 4 == 0 &&
                       ((uintptr_t)op->rgb & 3) == 0 && ((uintptr_t)op->idx & 3) == 0;
  *kind = (op->W % 4 == 0 && layout && aligned) ? 1 : 0;
  return 0;
}

extern "C" int gode_video_grid_launch_kind(const gode_video_grid_op* op, int32_t* kind) {
  if (!kind) return GODE_E_ARG;
  return vg_plan(op, kind);
}

extern "C" int gode_video_grid(const gode_video_grid_op* op, void* stream) {
  int32_t kind = 0;
  const int rc = vg_plan(op, &kind);
  if (rc) return rc;
  const uint32_t gh = (uint32_t)(op->rows * op->H);                         // <= 16384, so items <= 2^28
  const uint32_t tile_w = kind ? (uint32_t)op->W / 4u : (uint32_t)op->W, gw = (uint32_t)op->cols * tile_w;
  const uint32_t items = gh * gw;
  const VgDiv d = {make_fastdiv(gw), make_fastdiv((uint32_t)op->H), make_fastdiv(tile_w)};
  const dim3 grid((items + 255u) / 256u, (uint32_t)(op->T < 65535 ? op->T : 65535));
  if (kind && op->C == 1)
    hipLaunchKernelGGL(vidgrid_vec4_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, *op, d, items);
  else if (kind)
    hipLaunchKernelGGL(vidgrid_vec4_kernel<3>, grid, dim3(256), 0, (hipStream_t)stream, *op, d, items);
  else
    hipLaunchKernelGGL(vidgrid_strided_kernel, grid, dim3(256), 0, (hipStream_t)stream, *op, d, items);
  GODE_LAUNCH_CHECK();
  return 0;
}
