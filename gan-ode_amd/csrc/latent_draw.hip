// latent_draw.hip -- the generators' latents drawn on the device (latent_rng = "device"): the four sub-blocks of a sampling
// plan's input block [x | content | sel | cls] written from the counter-based latent stream of gode.h -- Philox4x32-10 and
// Box-Muller of philox.h on the tag family 0x60000000 | stream << 8 | field.  Every value is a pure function of
// (seed, stream, call, trajectory), each takes its own lane of its own quad (the content block is 50 floats per trajectory,
// so quads straddle trajectories), and nothing depends on the grid.
//
// Select mode (sample_images): the B rows of the plan are chosen among R = n_all * T by Floyd's algorithm and sorted; every
// workgroup recomputes the selection into LDS (B <= 4096: 32 KiB), so the op stays ONE launch and the work O(B) -- up to 64
// rows in the registers of one wavefront (measured at sample_images(32): 14.8 us per launch with the block-wide form and
// its two barriers per pick), block-wide above.  At the configured sizes (2-10 k values) the launch itself is the cost.
#include "common.h"
#include "philox.h"

#define LATENT_SELECT_MAX 4096

static inline uint32_t latent_tag(int32_t stream, int field) {
  return 0x60000000u | ((uint32_t)stream << 8) | (uint32_t)field;
}

// the word of element e: lane e & 3 of quad e >> 2
__device__ __forceinline__ uint32_t latent_word(uint64_t e, const NoiseArgs& a) {
  uint32_t c[4];
  philox_quad(e >> 2, a, c);
  const int l = (int)(e & 3);
  return l == 0 ? c[0] : l == 1 ? c[1] : l == 2 ? c[2] : c[3];
}

// the normal of element e: box_muller4's arithmetic on the one pair of uniforms the lane needs
__device__ __forceinline__ float latent_normal(uint64_t e, const NoiseArgs& a) {
  uint32_t c[4];
  philox_quad(e >> 2, a, c);
  const int l = (int)(e & 3);
  const uint32_t w0 = l < 2 ? c[0] : c[2], w1 = l < 2 ? c[1] : c[3];
  const float r = sqrtf(-2.f * logf(noise_uniform(w0)));
  float s, co;
  sincospif(2.f * noise_uniform(w1), &s, &co);
  return (l & 1) ? r * s : r * co;
}

template <bool SELECT>
__global__ void __launch_bounds__(256) latent_draw_kernel(const gode_latent_draw_op a, NoiseArgs na) {
  __shared__ uint32_t s_taken[SELECT ? LATENT_SELECT_MAX : 1];     // Floyd's picks, in the order taken
  __shared__ uint32_t s_rows[SELECT ? LATENT_SELECT_MAX : 1];      // the words, then the sorted rows
  const int tid = threadIdx.x;
  const uint32_t n = (uint32_t)a.n;
  na.step = (a.call_dev ? (uint32_t)a.call_dev[0] : 0u) + (uint32_t)a.call;
  const uint32_t tag0 = na.stream;                                 // field 0; field f: tag0 + f
  if (SELECT) {
    const uint32_t R = (uint32_t)a.n_all * (uint32_t)a.T;
    NoiseArgs ns = na;
    ns.stream = tag0 + 3u;
    if (n <= 64u) {
      // the configured sizes (sample_images(32)): the first wavefront alone, pick k in a register of lane k -- no LDS
      // traffic and no barrier inside the dependent chain of n steps
      if (tid < 64) {
        const uint32_t w = (uint32_t)tid < n ? latent_word((uint64_t)tid, ns) : 0u;
        uint32_t mine = 0xFFFFFFFFu;                               // (no pick: every t and j is below 2^31)
        for (uint32_t m = 0; m < n; ++m) {
          const uint32_t j = R - n + m;
          const uint32_t t = __umulhi((uint32_t)__shfl((int)w, (int)m), j + 1u);
          const int hit = __any((uint32_t)tid < m && mine == t);
          if ((uint32_t)tid == m) mine = hit ? j : t;
        }
        if ((uint32_t)tid < n) s_taken[tid] = mine;
      }
      __syncthreads();
    } else {
      for (uint32_t m = tid; m < n; m += 256) s_rows[m] = latent_word(m, ns);
      __syncthreads();
      for (uint32_t m = 0; m < n; ++m) {
        const uint32_t j = R - n + m;
        const uint32_t t = __umulhi(s_rows[m], j + 1u);
        int hit = 0;
        for (uint32_t k = tid; k < m; k += 256) hit |= s_taken[k] == t;
        hit = __syncthreads_or(hit);
        if (tid == 0) s_taken[m] = hit ? j : t;
        __syncthreads();
      }
    }
    // the picks are distinct: the rank of each is its place in the sorted order
    for (uint32_t m = tid; m < n; m += 256) {
      const uint32_t v = s_taken[m];
      uint32_t rank = 0;
      for (uint32_t k = 0; k < n; ++k) rank += s_taken[k] < v;
      s_rows[rank] = v;
    }
    __syncthreads();
  }
  const uint32_t XW = (uint32_t)a.outer * (uint32_t)a.inner;
  const uint32_t n_x = n * XW, n_c = a.content ? n * 50u : 0u, n_k = (a.C > 0 && a.cls) ? n : 0u, n_s = SELECT ? n : 0u;
  const uint32_t total = n_x + n_c + n_k + n_s;                    // (< 2^31: checked by the launcher)
  for (uint32_t i = blockIdx.x * 256u + tid; i < total; i += gridDim.x * 256u) {
    uint32_t field, b, k;
    if (i < n_x) { field = 1u; b = i / XW; k = i - b * XW; }
    else if (i < n_x + n_c) { field = 0u; b = (i - n_x) / 50u; k = (i - n_x) - b * 50u; }
    else if (i < n_x + n_c + n_k) { field = 2u; b = i - n_x - n_c; k = 0u; }
    else { field = 3u; b = i - n_x - n_c - n_k; k = 0u; }
    uint64_t g = (uint64_t)a.traj0 + b;
    uint32_t t_sel = 0;
    if (SELECT) {
      const uint32_t r = s_rows[b], q = r / (uint32_t)a.T;
      g = (uint64_t)a.traj0 + q;
      t_sel = r - q * (uint32_t)a.T;
    }
    NoiseArgs nf = na;
    nf.stream = tag0 + field;
    if (field == 1u) {
      const uint32_t o = k / (uint32_t)a.inner, ii = k - o * (uint32_t)a.inner;
      a.x[((size_t)o * n + b) * (uint32_t)a.inner + ii] = latent_normal(g * XW + k, nf);
    } else if (field == 0u) {
      a.content[(size_t)b * 50u + k] = latent_normal(g * 50u + k, nf);
    } else if (field == 2u) {
      a.cls[b] = (int32_t)__umulhi(latent_word(g, nf), (uint32_t)a.C);
    } else {
      a.sel_t[b] = (int32_t)t_sel;
    }
  }
}

extern "C" int gode_latent_draw(const gode_latent_draw_op* op, void* stream) {
  if (!op || !op->x || op->n < 1 || op->outer < 1 || op->inner < 1 || op->T < 1 || op->C < 0 || op->n_all < 0 ||
      op->stream < 0 || op->stream >= (1 << 21) || op->traj0 < 0 || (op->n_all > 0 && !op->sel_t))
    return GODE_E_ARG;
  const int64_t total = (int64_t)op->n * ((int64_t)op->outer * op->inner + 52);
  if (total >= (1ll << 31)) return GODE_E_SHAPE;
  const NoiseArgs na = make_noise_args((uint64_t)op->seed, latent_tag(op->stream, 0), 0u, 1.f);
  if (op->n_all > 0) {
    const int64_t R = (int64_t)op->n_all * op->T;
    if (op->n > LATENT_SELECT_MAX || op->n > R || R >= (1ll << 31)) return GODE_E_SHAPE;
    // every workgroup repeats the selection: few of them, each striding over the values
    int64_t b = (total + 255) / 256; if (b > 64) b = 64;
    hipLaunchKernelGGL(latent_draw_kernel<true>, dim3((int)b), dim3(256), 0, (hipStream_t)stream, *op, na);
  } else {
    int64_t b = (total + 255) / 256; if (b > 4096) b = 4096;
    hipLaunchKernelGGL(latent_draw_kernel<false>, dim3((int)b), dim3(256), 0, (hipStream_t)stream, *op, na);
  }
  GODE_LAUNCH_CHECK();
  return 0;
}
