// clips.hip -- the device-resident UCF-101 feed: the once-per-dataset bicubic resize + crop + quantise of
// uint8 frames (dataset/ucf101new.py:73-78,162-167) and the per-step window gather + normalise ((x - 128) / 128, :95,:179).
#include "common.h"

// ---------------------------------------------------------------------------------------------------------------
// gode_resize_u8: one workgroup per (frame, band of RESIZE_BAND output rows).  The horizontal pass turns the input rows the
// band reads into fp32 partial rows [row][out_w * C] in LDS (one fused-multiply-add chain per value, taps ascending); the
// vertical pass combines them per output row (the same chain over LDS rows) and stores.  The LDS window [lo, hi) of input rows
// is refilled whenever an output row reads outside it, so any table is served: bicubic tables (first ascending) fill it once
// per band.  Every table row is checked where it is used; a bad one yields NaN / 0 and no read.
#define RESIZE_BAND 8
#define RESIZE_LDS_BYTES (48 * 1024)

__device__ __forceinline__ bool taps_ok(int first, int count, int k, int n_in) {
  return count >= 1 && count <= k && first >= 0 && first <= n_in - count;
}
__device__ __forceinline__ uint32_t quantise_u8(float v) {      // clamp, round half to even, cast; NaN -> 0
  return (uint32_t)__builtin_rintf(fminf(fmaxf(v, 0.f), 255.f));
}

template <bool VEC>
__global__ void __launch_bounds__(256) resize_u8_kernel(const gode_resize_u8_op a, const int rowlen, const int rcap,
                                                        const int bands, const FastDiv div_row, const FastDiv div_c) {
  extern __shared__ __attribute__((aligned(16))) float part[];      // [rcap][rowlen]
  const int tid = threadIdx.x;
  const int fr = (int)(blockIdx.x / (uint32_t)bands);
  const int r0 = ((int)blockIdx.x - fr * bands) * RESIZE_BAND;
  const int r1 = min(r0 + RESIZE_BAND, a.out_h);
  const uint8_t* src = a.src + (int64_t)fr * a.ss[0];
  const float nan = __builtin_nanf("");
  int lo = 0, hi = 0;
  for (int r = r0; r < r1; ++r) {
    const int f = __builtin_amdgcn_readfirstlane(a.y_first[r]), n = __builtin_amdgcn_readfirstlane(a.y_count[r]);
    const bool ok = taps_ok(f, n, a.ky, a.Hin);
    if (ok && (f < lo || f + n > hi)) {
      int end = f + n;          // ... and what the rest of the band reads from there on, as far as the window holds it
      for (int q = r + 1; q < r1; ++q) {
        const int fq = __builtin_amdgcn_readfirstlane(a.y_first[q]), nq = __builtin_amdgcn_readfirstlane(a.y_count[q]);
        if (taps_ok(fq, nq, a.ky, a.Hin) && fq >= f) end = max(end, fq + nq);
      }
      end = min(end, f + rcap);
      __syncthreads();          // the row before has read the old window
      lo = f; hi = end;
      const int items = (hi - lo) * rowlen;
      for (int i = tid; i < items; i += 256) {
        const int y = (int)fdiv((uint32_t)i, div_row), e = i - y * rowlen;
        const int ox = (int)fdiv((uint32_t)e, div_c), c = e - ox * a.C;
        const int xf = a.x_first[ox], xn = a.x_count[ox];
        float acc = nan;
        if (taps_ok(xf, xn, a.kx, a.Win)) {
          const uint8_t* p = src + (int64_t)(lo + y) * a.ss[1] + (int64_t)xf * a.ss[2] + (int64_t)c * a.ss[3];
          const float* w = a.x_w + (int64_t)ox * a.kx;
          acc = 0.f;
#pragma unroll 4      // four taps' loads in flight per step of the chain; the order of the additions is unchanged
          for (int j = 0; j < xn; ++j) acc = fmaf(w[j], (float)p[(int64_t)j * a.ss[2]], acc);
        }
        part[i] = acc;
      }
      __syncthreads();
    }
    const float* w = a.y_w + (int64_t)r * a.ky;
    const float* rows = part + (ok ? (f - lo) * rowlen : 0);
    const int64_t o = ((int64_t)fr * a.out_h + r) * rowlen;
    if (VEC) {
      for (int q = tid * 4; q < rowlen; q += 1024) {
        f32x4 v = {nan, nan, nan, nan};
        if (ok) {
          v = f32x4{0.f, 0.f, 0.f, 0.f};
          for (int k = 0; k < n; ++k) {
            const f32x4 p = *reinterpret_cast<const f32x4*>(rows + k * rowlen + q);
            const float wk = w[k];
            v.x = fmaf(wk, p.x, v.x); v.y = fmaf(wk, p.y, v.y); v.z = fmaf(wk, p.z, v.z); v.w = fmaf(wk, p.w, v.w);
          }
        }
        if (a.dst_f32) *reinterpret_cast<f32x4*>(a.dst_f32 + o + q) = v;
        if (a.dst)
          *reinterpret_cast<uint32_t*>(a.dst + o + q) =
              quantise_u8(v.x) | quantise_u8(v.y) << 8 | quantise_u8(v.z) << 16 | quantise_u8(v.w) << 24;
      }
    } else {
      for (int q = tid; q < rowlen; q += 256) {
        float v = nan;
        if (ok) {
          v = 0.f;
          for (int k = 0; k < n; ++k) v = fmaf(w[k], rows[k * rowlen + q], v);
        }
        if (a.dst_f32) a.dst_f32[o + q] = v;
        if (a.dst) a.dst[o + q] = (uint8_t)quantise_u8(v);
      }
    }
  }
}

extern "C" int gode_resize_u8(const gode_resize_u8_op* op, void* stream) {
  if (!op || !op->src || (!op->dst && !op->dst_f32) || !op->y_first || !op->y_count || !op->y_w || !op->x_first ||
      !op->x_count || !op->x_w || op->F <= 0 || op->Hin <= 0 || op->Win <= 0 || (op->C != 1 && op->C != 3) || op->out_h <= 0 ||
      op->out_w <= 0 || op->ky <= 0 || op->kx <= 0)
    return GODE_E_ARG;
  if (op->ky > GODE_RESIZE_MAX_TAPS || op->kx > GODE_RESIZE_MAX_TAPS) return GODE_E_SHAPE;
  const int64_t rowlen = (int64_t)op->out_w * op->C;
  const int64_t lds_rows = RESIZE_LDS_BYTES / 4 / rowlen;
  if (lds_rows < op->ky) return GODE_E_SHAPE;
  const int64_t bands = (op->out_h + RESIZE_BAND - 1) / RESIZE_BAND;
  if (bands * op->F >= (1ll << 31)) return GODE_E_SHAPE;
  // the input rows a band of a bicubic table reads: its RESIZE_BAND steps of Hin / out_h, one row's taps, and rounding
  int64_t rcap = ((int64_t)RESIZE_BAND * op->Hin + op->out_h - 1) / op->out_h + op->ky + 2;
  if (rcap > op->Hin) rcap = op->Hin;
  if (rcap < op->ky) rcap = op->ky;
  if (rcap > lds_rows) rcap = lds_rows;
  const bool vec = rowlen % 4 == 0 && ((uintptr_t)op->dst_f32 & 15) == 0 && ((uintptr_t)op->dst & 3) == 0;
  const dim3 grid((uint32_t)(bands * op->F));
  const size_t lds = (size_t)(rcap * rowlen * 4);
  const FastDiv div_row = make_fastdiv((uint32_t)rowlen), div_c = make_fastdiv((uint32_t)op->C);
  if (vec)
    hipLaunchKernelGGL(resize_u8_kernel<true>, grid, dim3(256), lds, (hipStream_t)stream, *op, (int)rowlen, (int)rcap, (int)bands,
                       div_row, div_c);
  else
    hipLaunchKernelGGL(resize_u8_kernel<false>, grid, dim3(256), lds, (hipStream_t)stream, *op, (int)rowlen, (int)rcap,
                       (int)bands, div_row, div_c);
  GODE_LAUNCH_CHECK();
  return 0;
}

// ---------------------------------------------------------------------------------------------------------------
// gode_clip_gather: the T frames of a clip are consecutive in the store, so clip b is ONE contiguous run of T * frame_elems
// bytes from frame first[b]; a thread converts 16 of them (VEC: one 16-byte load, four 16-byte stores) or one.
template <bool VEC>
__global__ void __launch_bounds__(256) clip_gather_kernel(const gode_clip_gather_op a, const uint32_t per_clip,
                                                          const uint32_t total, const FastDiv div_clip) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= total) return;
  const uint32_t b = fdiv(i, div_clip), u = i - b * per_clip;
  const int64_t f0 = a.first[b];
  const bool ok = f0 >= 0 && f0 <= a.n_frames - a.T;
  if (VEC) {
    f32x4* out = reinterpret_cast<f32x4*>(a.out) + (int64_t)i * 4;
    if (!ok) {
      const float nan = __builtin_nanf("");
      for (int k = 0; k < 4; ++k) out[k] = f32x4{nan, nan, nan, nan};
      return;
    }
    const uint4 q = *reinterpret_cast<const uint4*>(a.frames + f0 * a.frame_elems + (int64_t)u * 16);
    const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int k = 0; k < 4; ++k)
      out[k] = f32x4{((float)(w[k] & 255u) - a.sub) * a.inv, ((float)((w[k] >> 8) & 255u) - a.sub) * a.inv,
                     ((float)((w[k] >> 16) & 255u) - a.sub) * a.inv, ((float)(w[k] >> 24) - a.sub) * a.inv};
  } else {
    a.out[i] = ok ? ((float)a.frames[f0 * a.frame_elems + u] - a.sub) * a.inv : __builtin_nanf("");
  }
}

extern "C" int gode_clip_gather(const gode_clip_gather_op* op, void* stream) {
  if (!op || !op->frames || !op->first || !op->out || op->n_frames <= 0 || op->frame_elems <= 0 || op->B <= 0 || op->T <= 0)
    return GODE_E_ARG;
  const bool vec = op->frame_elems % 16 == 0 && ((uintptr_t)op->frames & 15) == 0 && ((uintptr_t)op->out & 15) == 0;
  if (op->frame_elems >= (1ll << 31) / op->T) return GODE_E_SHAPE;
  const int64_t per_clip = op->T * op->frame_elems / (vec ? 16 : 1);
  const int64_t total = per_clip * op->B;
  if (total >= (1ll << 31)) return GODE_E_SHAPE;
  const dim3 grid((uint32_t)((total + 255) / 256));
  const FastDiv div_clip = make_fastdiv((uint32_t)per_clip);
  if (vec)
    hipLaunchKernelGGL(clip_gather_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, *op, (uint32_t)per_clip,
                       (uint32_t)total, div_clip);
  else
    hipLaunchKernelGGL(clip_gather_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, *op, (uint32_t)per_clip,
                       (uint32_t)total, div_clip);
  GODE_LAUNCH_CHECK();
  return 0;
}
