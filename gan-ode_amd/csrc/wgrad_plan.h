// wgrad_plan.h -- how one weight-gradient op (gode_wgrad_op) is launched, decided once: the path (LDS patch, thin, tiled
// GEMM), the tile, the position splits, the kernel family and its vector / LDS-DMA flags, the grid, and the kernel that sums
// the split slabs.  Plain host arithmetic on the op's geometry -- no pointer is dereferenced (x, y and work are read as
// integers, for their alignment), no HIP -- so it builds with g++ and is pinned on the CPU
// (tests/hostcheck/wgrad_plan_check.cpp against tests/golden/wgrad_plans.txt).  wgrad.hip turns a plan into two launches;
// gode_wgrad_work_size / gode_wgrad_auto_splits read the part of it that no pointer can reach (wgrad_plan_work).
#pragma once
#include <stdint.h>
#include <stdlib.h>
#include "conv_geom.h"

#define THIN_MAXKT 16      // weight columns (taps * Ci) the THIN kernel keeps in registers
#define WP_MAXB 4          // PATCH kernel: 32x32 output blocks per wave
#define WP_MAXE 16         // PATCH kernel: patch elements staged per thread and slab
#define RS_OUT 16          // small reduce: outputs per workgroup

// The tiles of the GEMM path, indexed by tile id: BI output channels x BJ weight columns per workgroup of WM x WN waves with
// TM x TN 32x32 MFMA tiles each (the kernels' template parameters).
//   0-2: four waves, by output channels (Co <= 32, <= 64, more).
//   3: 256 x 128, 8 waves (FAST kernel only): 25 % fewer operand bytes per MFMA than 128 x 128.  Measured: decoder layers
//      332 -> 310 and 313 -> 304 us, MNIST video-D layers 2 / 3 at N = 64 119 -> 112 and 144 -> 135 us; a 0.6-GFLOP problem
//      (image-D layer 2) loses 15 %, hence the size floor in wgrad_pick_tile.
//   4: 128 x 256, 8 waves (FAST kernel only): the decoder's last stride-2 layer (326 -> 321 us); with only two column tiles
//      (MNIST video-D layer 1, Kt = 512) it needs 128 position splits and loses 12 %.
enum { WG_TILE_32x128 = 0, WG_TILE_64x128 = 1, WG_TILE_128x128 = 2, WG_TILE_256x128 = 3, WG_TILE_128x256 = 4, WGRAD_TILE_IDS = 5 };
struct WgradTile { int BI, BJ, WM, WN, TM, TN, waves; };
constexpr WgradTile wgrad_tile(int WM, int WN, int TM, int TN) { return WgradTile{WM * TM * 32, WN * TN * 32, WM, WN, TM, TN, WM * WN}; }
static constexpr WgradTile WGRAD_TILES[WGRAD_TILE_IDS] = {wgrad_tile(1, 4, 1, 1), wgrad_tile(2, 2, 1, 2), wgrad_tile(2, 2, 2, 2),
                                                          wgrad_tile(4, 2, 2, 2), wgrad_tile(2, 4, 2, 2)};

// The tuning knobs, read once per process, here and nowhere else:
//   GODE_WGRAD_TILE=2/3/4 asks for that tile where the shape allows it (scripts/exp/sweep_wgrad.py);
//   GODE_WGRAD_GENERIC    (set to anything) forces the generic kernel;
//   GODE_WGRAD_GLDS=0     register staging instead of LDS-DMA in the FAST kernel, tiles 0-2.
struct WgradKnobs { int tile; bool generic, glds; };
static const WgradKnobs& wgrad_knobs() {
  static const WgradKnobs k = [] {
    const char* t = getenv("GODE_WGRAD_TILE");
    const char* gl = getenv("GODE_WGRAD_GLDS");
    return WgradKnobs{t ? atoi(t) : 0, getenv("GODE_WGRAD_GENERIC") != nullptr, gl ? atoi(gl) != 0 : true};
  }();
  return k;
}

static int wgrad_pick_tile(const gode_conv_geom& g, const WgradKnobs& knobs) {
  const int Kt = g.kd * g.kh * g.kw * g.Ci;
  const int64_t macs = (int64_t)g.N * g.Do * g.Ho * g.Wo * g.Co * Kt;
  const bool can3 = g.Co % 256 == 0 && g.Ci % 4 == 0, can4 = g.Co % 128 == 0 && g.Ci % 4 == 0 && Kt % 256 == 0;
  if (knobs.tile == 2 && g.Co > 64) return WG_TILE_128x128;
  if (knobs.tile == 3 && can3) return WG_TILE_256x128;
  if (knobs.tile == 4 && can4) return WG_TILE_128x256;
  if (can3 && macs >= (1ll << 31)) return WG_TILE_256x128;
  if (can4 && g.Co == 128 && Kt >= 1024 && macs >= (1ll << 31)) return WG_TILE_128x256;
  return g.Co <= 32 ? WG_TILE_32x128 : (g.Co <= 64 ? WG_TILE_64x128 : WG_TILE_128x128);
}

// Position splits of the weight-gradient GEMM.  All workgroups carry equal work, so the launch time is the busiest
// CU's share: the grid (tiles x splits) should be a multiple of the 256 CUs and give each CU >= 2 resident workgroups
// (measured on the decoder layers: 512 workgroups 96-105 TFLOP/s, 640 workgroups 84-88, 256 workgroups 90-99).  More
// splits also cost one more [Co][Kt] slab to write and reduce, ~114 positions' worth of GEMM time each.
static int wgrad_gemm_splits(const gode_conv_geom& g, int tile) {
  const int Kt = g.kd * g.kh * g.kw * g.Ci;
  const int64_t M = (int64_t)g.N * g.Do * g.Ho * g.Wo;
  const bool w8 = WGRAD_TILES[tile].waves == 8;   // one workgroup per CU (96 KB of LDS), its waves cover each other's barriers
  const int64_t tiles = (int64_t)gode_ceil_div(g.Co, WGRAD_TILES[tile].BI) * gode_ceil_div(Kt, WGRAD_TILES[tile].BJ);
  int64_t cap = (M + 63) / 64;
  if (cap > 256) cap = 256;
  if (cap < 1) cap = 1;
  int best = 1; double best_cost = 1e300;
  for (int64_t s = 1; s <= cap; ++s) {
    const double blocks = (double)(tiles * s);
    const double rounds = (double)((tiles * s + 255) / 256);
    const double balance = blocks / (rounds * 256.0);                 // busiest CU's share vs the mean
    const double overlap = (blocks >= 512.0 || w8) ? 1.0 : 0.92;      // a lone 4-wave workgroup per CU cannot hide its barriers
    const double cost = (1.0 + 114.0 * (double)s / (double)M) / (balance * overlap);
    if (cost < best_cost - 1e-12) { best_cost = cost; best = (int)s; }
  }
  return best;
}

// THIN path: Kt <= 16 weight columns, float4 channel lanes that divide the workgroup.  One slab per workgroup:
// ~4 positions per thread (the per-position gather chain is serial), up to 1024 workgroups.
static bool wgrad_thin_eligible(const gode_conv_geom& g) {
  const int Kt = g.kd * g.kh * g.kw * g.Ci;
  return Kt <= THIN_MAXKT && g.Co % 4 == 0 && (256 % ((g.Co / 4) < 64 ? (g.Co / 4) : 64)) == 0;
}
static int wgrad_thin_blocks(const gode_conv_geom& g) {
  const int64_t M = (int64_t)g.N * g.Do * g.Ho * g.Wo, b = (M + 63) / 64;
  return (int)(b > 1024 ? 1024 : (b < 1 ? 1 : b));
}

// PATCH path: eligibility and launch shape.  RB / CB: 32-row blocks of Co, 32-column blocks of Kt; PR patch rows (kd*kh), PL
// padded row length (floats), LW w positions per row ((32-1)*sw + kw); nseg 32-position segments per output row, segs of
// them in all, segs_per_wg per workgroup; nbw column blocks per wave (the kernel's NBW).
struct WgradPatch { int32_t RB, CB, PR, PL, LW, nseg, segs, segs_per_wg, nbw; };
static bool wgrad_patch_shape(const gode_conv_geom& g, bool requested_splits, bool xform_on_x, WgradPatch* P) {
  const int Kt = g.kd * g.kh * g.kw * g.Ci;
  // (Kt <= 16 stays on the THIN path: measured on the MNIST first layers, 33 / 36 us there against 44 / 84 us here)
  if (requested_splits || g.Ci > 4 || Kt <= THIN_MAXKT || (g.Co != 32 && g.Co != 64 && g.Co != 128) || g.Wo < 16) return false;
  if (xform_on_x) return false;
  const int RB = g.Co / 32, CB = (Kt + 31) / 32, nbw = (CB + 4 / RB - 1) / (4 / RB);
  if (nbw > WP_MAXB) return false;
  const int PR = g.kd * g.kh, LW = 31 * g.sw + g.kw;
  if (PR > 255 || LW > 32767 || PR * LW * g.Ci > 256 * WP_MAXE) return false;
  int PL = LW * g.Ci;
  while (PL % 32 != (g.kw * g.Ci) % 32) ++PL;
  if (2 * (PR * PL + 32 * g.Co + 4) * 4 > 64 * 1024 || 256 % (g.Co / 4) != 0 || PR > 30) return false;
  // the kernel packs tap-validity masks into one word: depth taps in bits 0..4, row taps from bit 5 (e_key's 5-bit fields)
  if (g.kd > 5 || g.kh > 27) return false;
  const int nseg = (g.Wo + 31) / 32;
  const int64_t segs = (int64_t)g.N * g.Do * g.Ho * nseg;
  if (segs >= (1ll << 31)) return false;
  int wgs = (int)(segs / 2 < 1 ? 1 : segs / 2);            // >= 2 segments per workgroup, two workgroups per CU at most
  if (wgs > 512) wgs = 512;
  *P = WgradPatch{RB, CB, PR, PL, LW, nseg, (int)segs, (int)((segs + wgs - 1) / wgs), nbw};
  return true;
}

// The part of the plan that sizes the workspace: which rule gives the split count, the tile it counts with, the count.  A
// function of the geometry, the requested splits, whether a transform is given and which side it is on -- it is handed no
// pointer, so gode_wgrad_work_size (called before `work` exists, and on probe ops) and the launch cannot disagree.
enum { WG_PATCH = 0, WG_THIN = 1, WG_GEMM = 2 };
struct WgradWork { int32_t rule, split_tile, splits; WgradPatch patch; };
static WgradWork wgrad_plan_work(const gode_conv_geom& g, int splits, bool has_scale, bool xform_on_y, const WgradKnobs& knobs) {
  WgradWork W = {WG_GEMM, wgrad_pick_tile(g, knobs), splits, {0, 0, 0, 0, 0, 0, 0, 0, 0}};
  if (wgrad_patch_shape(g, splits > 0, has_scale && !xform_on_y, &W.patch)) {
    W.rule = WG_PATCH; W.splits = (W.patch.segs + W.patch.segs_per_wg - 1) / W.patch.segs_per_wg;
  } else if (splits <= 0 && wgrad_thin_eligible(g)) {
    W.rule = WG_THIN; W.splits = wgrad_thin_blocks(g);
  } else if (splits <= 0) {
    W.splits = wgrad_gemm_splits(g, W.split_tile);
  }
  return W;
}
static int wgrad_auto_splits(const gode_conv_geom& g) { return wgrad_gemm_splits(g, wgrad_pick_tile(g, wgrad_knobs())); }
static int64_t wgrad_work_size(const gode_wgrad_op* op) {
  const WgradWork W = wgrad_plan_work(op->g, op->splits, op->scale != nullptr, op->xform_on_y != 0, wgrad_knobs());
  return (int64_t)W.splits * op->g.Co * op->g.kd * op->g.kh * op->g.kw * op->g.Ci;
}

enum { WG_FAST = 0, WG_GENERIC = 1 };
enum { WG_REDUCE_SMALL = 0, WG_REDUCE_VEC4 = 1, WG_REDUCE_SCALAR = 2 };

struct WgradPlan {
  WgradWork work;                              // rule of the split count, its tile, splits, the patch shape (path == WG_PATCH)
  int32_t path;                                // WG_PATCH / WG_THIN / WG_GEMM: the kernel launched
  int32_t tile, family;                        // WG_GEMM: the tile launched (index into WGRAD_TILES), WG_FAST / WG_GENERIC; else -1
  int32_t vx, vy, glds;                        // x / y rows read as float4; the FAST kernel stages by LDS-DMA (family WG_FAST only)
  int32_t M, taps, Kt, chunk, chunk_thin;      // positions, taps, weight columns; positions per split (whole slabs / THIN: exact)
  int32_t grid_x, grid_y, grid_z, block, lds_bytes;
  int32_t xs[5];                               // element strides of x {N, D, H, W, C}, resolved
  uint32_t x_bytes;                            // extent of x for the LDS-DMA kernels' raw buffers; 0: too large
  int32_t reduce, reduce_blocks;
  int64_t work_floats;
};

// The kernels of wgrad.hip a plan can name, one list per template, as X-macros: wgrad.hip expands them into the cases of its
// kernel switch and WGRAD_KERNEL_KEYS below into the keys the host check looks every plan's key up in, so the two cannot drift.
//   FAST(tile, glds)   wgrad_fast_kernel<tile..., glds>: both operands float4.  All five tiles, both staging forms.
//   GENERIC(tile, vx, vy)  wgrad_kernel<tile..., vx, vy>: tiles 0-2 (its loader assumes four waves); vx = vy = 1 only with
//                      GODE_WGRAD_GENERIC.
//   PATCH(nbw, Co)     wgrad_patch_kernel<nbw, Co>: every nbw <= WP_MAXB occurs for every Co.
#define WGRAD_FAST_KERNELS(X) X(0, 0) X(0, 1) X(1, 0) X(1, 1) X(2, 0) X(2, 1) X(3, 0) X(3, 1) X(4, 0) X(4, 1)
#define WGRAD_GENERIC_KERNELS(X) \
  X(0, 0, 0) X(0, 0, 1) X(0, 1, 0) X(0, 1, 1) X(1, 0, 0) X(1, 0, 1) X(1, 1, 0) X(1, 1, 1) X(2, 0, 0) X(2, 0, 1) X(2, 1, 0) X(2, 1, 1)
#define WGRAD_PATCH_KERNELS(X) \
  X(1, 32) X(2, 32) X(3, 32) X(4, 32) X(1, 64) X(2, 64) X(3, 64) X(4, 64) X(1, 128) X(2, 128) X(3, 128) X(4, 128)
constexpr uint32_t wgrad_key(int path, int family, int tile, int glds, int vx, int vy, int nbw, int Co) {
  return (uint32_t)path | (uint32_t)family << 2 | (uint32_t)tile << 3 | (uint32_t)glds << 6 | (uint32_t)vx << 7 | (uint32_t)vy << 8 |
         (uint32_t)nbw << 9 | (uint32_t)Co << 12;
}
constexpr uint32_t wgrad_fast_key(int tile, int glds) { return wgrad_key(WG_GEMM, WG_FAST, tile, glds, 1, 1, 0, 0); }
constexpr uint32_t wgrad_generic_key(int tile, int vx, int vy) { return wgrad_key(WG_GEMM, WG_GENERIC, tile, 0, vx, vy, 0, 0); }
constexpr uint32_t wgrad_patch_key(int nbw, int Co) { return wgrad_key(WG_PATCH, 0, 0, 0, 0, 0, nbw, Co); }
constexpr uint32_t wgrad_thin_key() { return wgrad_key(WG_THIN, 0, 0, 0, 0, 0, 0, 0); }
static uint32_t wgrad_kernel_key(const WgradPlan& P, int Co) {
  if (P.path == WG_PATCH) return wgrad_patch_key(P.work.patch.nbw, Co);
  if (P.path == WG_THIN) return wgrad_thin_key();
  return P.family == WG_FAST ? wgrad_fast_key(P.tile, P.glds) : wgrad_generic_key(P.tile, P.vx, P.vy);
}
static constexpr uint32_t WGRAD_KERNEL_KEYS[] = {
#define WG_KEY_FAST(t, gl) wgrad_fast_key(t, gl),
#define WG_KEY_GENERIC(t, vx, vy) wgrad_generic_key(t, vx, vy),
#define WG_KEY_PATCH(n, c) wgrad_patch_key(n, c),
    WGRAD_FAST_KERNELS(WG_KEY_FAST) WGRAD_GENERIC_KERNELS(WG_KEY_GENERIC) WGRAD_PATCH_KERNELS(WG_KEY_PATCH) wgrad_thin_key()};
#undef WG_KEY_FAST
#undef WG_KEY_GENERIC
#undef WG_KEY_PATCH

static int wgrad_make_plan_with(const gode_wgrad_op* op, const WgradKnobs& knobs, WgradPlan* P) {
  if (!op) return GODE_E_ARG;
  const gode_conv_geom& g = op->g;
  IgemmGeom chk;
  const int rc = gode_build_igemm_geom(g, GODE_FPROP, &chk);  // validates the conv relation
  if (rc) return rc;
  int64_t xs[5];
  if (gode_strides_are_channels_last(op->xs)) {
    xs[4] = 1; xs[3] = g.Ci; xs[2] = (int64_t)g.Wi * xs[3]; xs[1] = (int64_t)g.Hi * xs[2]; xs[0] = (int64_t)g.Di * xs[1];
  } else {
    for (int i = 0; i < 5; ++i) xs[i] = op->xs[i];
  }
  const int64_t span = 1 + (int64_t)(g.N - 1) * xs[0] + (int64_t)(g.Di - 1) * xs[1] + (int64_t)(g.Hi - 1) * xs[2] +
                       (int64_t)(g.Wi - 1) * xs[3] + (int64_t)(g.Ci - 1) * xs[4];
  const int64_t M = (int64_t)g.N * g.Do * g.Ho * g.Wo;
  if (span >= (1ll << 31) || M * g.Co >= (1ll << 31)) return GODE_E_SHAPE;
  for (int i = 0; i < 5; ++i) P->xs[i] = (int32_t)xs[i];
  P->x_bytes = (span * 4 < (1ll << 31) && M * g.Co * 4 < (1ll << 31)) ? (uint32_t)(span * 4) : 0u;
  P->M = (int)M; P->taps = g.kd * g.kh * g.kw; P->Kt = P->taps * g.Ci;

  const WgradWork& W = P->work = wgrad_plan_work(g, op->splits, op->scale != nullptr, op->xform_on_y != 0, knobs);
  const int splits = W.splits;
  P->chunk = (int)(((M + splits - 1) / splits + 31) / 32 * 32);
  P->chunk_thin = 0;
  P->vx =xs[4] == 1 && g.Ci % 4 == 0 && xs[0] % 4 == 0 && xs[1] % 4 == 0 && xs[2] % 4 == 0 && xs[3] % 4 == 0 && (uintptr_t)op->x % 16 == 0;
  P->vy = g.Co % 4 == 0 && (uintptr_t)op->y % 16 == 0;
  P->tile = -1; P->family = -1; P->glds = 0;
  P->grid_x = splits; P->grid_y = 1; P->grid_z = 1; P->block = 256; P->lds_bytes = 0;
  if (W.rule == WG_PATCH) {
    P->path = WG_PATCH;                        // (vy is the kernel's `yvec`: Co is 32, 64 or 128)
    P->lds_bytes = 2 * (W.patch.PR * W.patch.PL + 32 * g.Co + 4) * 4;
  } else if (W.rule == WG_THIN && P->vy) {
    P->path = WG_THIN;
    P->chunk_thin = (int)((M + splits - 1) / splits);
  } else {
    // known oddity, kept so that no plan changes: a thin-eligible op whose y is not 16-byte aligned comes here
    // with the THIN rule's split count (up to 1024) and runs the generic kernel of its tile
    P->path = WG_GEMM;
    const bool fast = P->vx && P->vy && !knobs.generic;
    P->family = fast ? WG_FAST : WG_GENERIC;
    // known oddity, kept so that no plan changes: the 8-wave tiles exist in the FAST kernel only, so without
    // it the launch is 128x128 with the split count that was chosen for the 8-wave tile ...
    // known oddity, kept so that no plan changes: ... and GODE_WGRAD_GENERIC thereby changes the tile too
    P->tile = WGRAD_TILES[W.split_tile].waves == 8 && !fast ? WG_TILE_128x128 : W.split_tile;
    // (GODE_WGRAD_GLDS does not reach the 8-wave tiles)
    const bool glds_on = WGRAD_TILES[P->tile].waves == 8 || knobs.glds;
    P->glds = fast && glds_on && op->scale == nullptr && op->act == GODE_ACT_NONE && P->x_bytes != 0;
    P->grid_x = gode_ceil_div(P->Kt, WGRAD_TILES[P->tile].BJ); P->grid_y = gode_ceil_div(g.Co, WGRAD_TILES[P->tile].BI); P->grid_z = splits;
    P->block = WGRAD_TILES[P->tile].waves * 64;
  }

  // the kernel that sums the slabs.  Small: few outputs, many slabs (patch path: hundreds of slabs of a [Co][Kt] of a few thousand)
  const int64_t total = (int64_t)g.Co * P->Kt;
  if ((total <= 8192 || (P->path == WG_PATCH && total <= 32768)) && splits >= 16) {
    P->reduce = WG_REDUCE_SMALL;
    P->reduce_blocks = (int)((total + RS_OUT - 1) / RS_OUT);
  } else {
    const bool v4 = P->Kt % 4 == 0 && (uintptr_t)op->work % 16 == 0;
    P->reduce = v4 ? WG_REDUCE_VEC4 : WG_REDUCE_SCALAR;
    const int64_t blocks = (total / (v4 ? 4 : 1) + 255) / 256;
    P->reduce_blocks = (int)(blocks > 4096 ? 4096 : (blocks < 1 ? 1 : blocks));
  }
  P->work_floats = (int64_t)splits * total;
  return 0;
}
static int wgrad_make_plan(const gode_wgrad_op* op, WgradPlan* P) { return wgrad_make_plan_with(op, wgrad_knobs(), P); }
