// igemm_plan.h -- how one implicit-GEMM op (gode_igemm_op) is launched, decided once: the phase table (plain, grouped or
// border-split), tile, K split, live-tap mode, workgroup->XCD order and the kernel family that serves it.  Plain host
// arithmetic on the op's geometry -- no pointer is dereferenced, no HIP -- so it builds with g++ and is pinned on the CPU
// (tests/hostcheck/plan_check.cpp against tests/golden/igemm_plans.txt).  igemm.hip turns a plan into launches; the
// queries of include/gode.h (gode_igemm_stats_rows / _rows0 / _stats_segments / _work_size / _model_cycles) read it.
#pragma once
#include <stdio.h>
#include <stdlib.h>
#include "conv_geom.h"

#define IGEMM_MAX_LIVE_TAPS 64   // MODE 3 tap table (+1 slot read past the end)
#define SPLITK_ROWS 16           // output positions per workgroup (and per statistics row) of the split-K finish
#define PW_MAXW 4096             // floats of weights the pointwise kernel keeps in LDS

// The tiles, indexed by tile id (gode_igemm_op.tile; 0 = auto, 5 is not a tile).  BM x BN outputs per workgroup of WM x WN
// waves with TM x TN 32x32 MFMA tiles each (the kernels' template parameters); for the cost model the MFMA cycles of one
// 32-deep K slab (64 per 32x32x2 instruction), the workgroups resident per CU, and the measured pipe efficiency with two
// or more of them resident (scripts/sweep_tiles.py; 64x64 re-measured with the round-3 loop: 0.62 before).
enum { TILE_128x128 = 1, TILE_128x64 = 2, TILE_128x32 = 3, TILE_64x64 = 4, TILE_256x128 = 6, IGEMM_TILE_IDS = 7 };
struct IgemmTile { int bm, bn, WM, WN, TM, TN; double cps; int resident; double eff2; };
constexpr IgemmTile igemm_tile(int WM, int WN, int TM, int TN, double cps, int resident, double eff2) {
  return IgemmTile{WM * TM * 32, WN * TN * 32, WM, WN, TM, TN, cps, resident, eff2};
}
static constexpr IgemmTile IGEMM_TILES[IGEMM_TILE_IDS] = {
    igemm_tile(0, 0, 0, 0, 0.0, 0, 0.0),
    igemm_tile(2, 2, 2, 2, 4096.0, 2, 0.76),      // 128x128
    igemm_tile(2, 2, 2, 1, 2048.0, 3, 0.76),      // 128x64
    igemm_tile(4, 1, 1, 1, 1024.0, 4, 0.62),      // 128x32
    igemm_tile(2, 2, 1, 1, 1024.0, 4, 0.70),      // 64x64
    igemm_tile(0, 0, 0, 0, 0.0, 0, 0.0),
    igemm_tile(4, 2, 2, 2, 8192.0, 1, 0.785)};    // 256x128, 8 waves

static bool tile_exists(int tile) { return tile > 0 && tile < IGEMM_TILE_IDS && IGEMM_TILES[tile].bm != 0; }
static int tile_bm(int tile) { return IGEMM_TILES[tile].bm; }
static int tile_bn(int tile) { return IGEMM_TILES[tile].bn; }
static int64_t count_tiles(const IgemmGeom& G, int tile) {      // workgroups of a launch of G with this tile
  int64_t n = 0;
  for (int i = 0; i < G.nphase; ++i) n += (int64_t)gode_ceil_div(G.ph[i].M, tile_bm(tile)) * gode_ceil_div(G.Ncols, tile_bn(tile));
  return n;
}

// split-K plan: purely a function of the geometry (so gode_igemm_stats_rows / gode_igemm_work_size agree with the
// launch).  Used when the FAST kernel applies and the natural grid would leave most of the 256 CUs idle.
struct SplitPlan { int ksplit, slabs_per_split, positions; };
static SplitPlan split_k(const gode_igemm_op* op, const IgemmGeom& G, int max_slabs, int k) {     // k <= 1: no split
  SplitPlan sp = {1, 0, op->g.N * G.Xd * G.Xh * G.Xw};
  if (k > 1) { sp.slabs_per_split = gode_ceil_div(max_slabs, k); sp.ksplit = gode_ceil_div(max_slabs, sp.slabs_per_split); }
  return sp;
}
static void slab_range(const IgemmGeom& G, int* min_slabs, int* max_slabs) {     // 32-deep K slabs of the shortest / longest phase
  *min_slabs = 1 << 30; *max_slabs = 0;
  for (int i = 0; i < G.nphase; ++i) {
    const int ns = G.ph[i].K >> 5;
    if (ns > *max_slabs) *max_slabs = ns;
    if (ns < *min_slabs) *min_slabs = ns;
  }
}

static bool fast_geometry(const IgemmGeom& G) {
  bool ok = G.Cg % 32 == 0;
  for (int i = 0; i < G.nphase; ++i) ok = ok && G.ph[i].K >= 32 && G.ph[i].K % 32 == 0 && G.ph[i].Kp == G.ph[i].K;
  return ok;
}

static bool strides_allow_vec(const gode_igemm_op* op, const IgemmGeom& G) {
  if (gode_strides_are_channels_last(op->gs)) return G.Cg % 4 == 0;
  return op->gs[4] == 1 && G.Cg % 4 == 0 && op->gs[0] % 4 == 0 && op->gs[1] % 4 == 0 && op->gs[2] % 4 == 0 &&
         op->gs[3] % 4 == 0;
}

static SplitPlan plan_split(const gode_igemm_op* op, const IgemmGeom& G, int tile) {
  const SplitPlan sp = split_k(op, G, 0, 1);
  if (!fast_geometry(G) || G.Ncols <= 4 || !strides_allow_vec(op, G)) return sp;
  // known oddity, kept so that no plan changes: a requested 256x128 tile has its grid counted in 128x64 blocks
  const int64_t blocks = count_tiles(G, tile == TILE_256x128 ? TILE_128x64 : tile);
  int max_slabs, min_slabs;
  slab_range(G, &min_slabs, &max_slabs);
  if (blocks >= 64 || min_slabs < 8) return sp;   // only grids that would leave >3/4 of the CUs idle
  int k = (int)((512 + blocks - 1) / blocks);
  if (k > min_slabs / 4) k = min_slabs / 4;
  if (k > 32) k = 32;
  return split_k(op, G, max_slabs, k);
}

// The tile off the modelled path: the requested one, or thresholds on the output columns and the grid.
static int pick_tile(const IgemmGeom& G, int requested) {
  if (requested != 0) return requested;
  if (G.Ncols <= 32) return TILE_128x32;
  if (G.Ncols <= 64) return TILE_128x64;
  const int64_t blocks = count_tiles(G, TILE_128x128);
  if (blocks >= 192) return TILE_128x128;
  // with split-K available a starved grid is better served by the big tile (unless there are very few rows)
  int maxM = 0;
  for (int i = 0; i < G.nphase; ++i) if (G.ph[i].M > maxM) maxM = G.ph[i].M;
  return fast_geometry(G) && maxM > tile_bm(TILE_64x64) && blocks < 64 ? TILE_128x128 : TILE_64x64;
}

// MODE 3 of the FAST kernel (live taps only) pays for its slower loop when the temporal taps that fall off the tensor's
// ends are > 15 % of the K loop (temporal stride 1: Do of the Di planes' taps are live)
static bool igemm_wants_tapskip(const gode_igemm_op* op, const IgemmGeom& G) {
  if (!(op->dir == GODE_DGRAD && op->groups != 2 && !G.fullk && op->g.sd == 1 && G.ph[0].Td > 1 && 100 * op->g.Do < 85 * op->g.Di))
    return false;
  for (int i = 0; i < G.nphase; ++i) if (G.ph[i].Td * G.ph[i].Th * G.ph[i].Tw >= IGEMM_MAX_LIVE_TAPS) return false;
  return true;
}

// Tile and K-split of a FAST-path GEMM from a small cost model instead of thresholds.  All workgroups of a launch
// carry equal work and the dispatcher deals them evenly, so the launch lasts as long as the busiest CU:
//   time = ceil(workgroups / 256) * (fixed + slabs * cycles_per_slab(tile) / efficiency) [+ split-K reduce]
// with the MFMA cycles of one 32-deep slab (64 per 32x32x2 instruction), the measured pipe efficiencies of the tiles
// (two or more resident workgroups per CU overlap each other's barriers; a lone one cannot) and ~4k cycles of
// prologue + epilogue.  Checked against measurements: ConvT 128->64 (4096 x 128x64) 314 us model / 297 us measured;
// UCF video-D layer-2 dgrad 128x128 578 / 514 us, for which the model prefers 128x64 (436 us).
static void choose_fast(const gode_igemm_op* op, const IgemmGeom& G, int* tile_out, SplitPlan* sp_out, double* cycles_out) {
  const gode_conv_geom& g = op->g;
  const int positions = g.N * G.Xd * G.Xh * G.Xw;
  const double out_bytes = 4.0 * positions * G.Ncols;
  int max_slabs, min_slabs;
  slab_range(G, &min_slabs, &max_slabs);
  bool even_phases = true;        // phases of unequal size leave early-exit workgroups in the grid: measured, a K split
  for (int i = 0; i < G.nphase; ++i)     // then gains nothing (video-D layer 3 dgrad: 101 us split 3 ways vs 64 us unsplit)
    even_phases = even_phases && G.ph[i].M == G.ph[0].M;
  // 256x128 (8 waves, one workgroup per CU, 25 % less operand traffic per MFMA) last: 2-3 % ahead of 128x128 on the full
  // decoder grids and 5 % on the MNIST video-D layer-2 input gradient (scripts/sweep_tiles.py), behind it on grids that
  // do not fill whole rounds of 256 such tiles
  static const int tiles[5] = {TILE_128x128, TILE_128x64, TILE_64x64, TILE_128x32, TILE_256x128};
  static const int ksplits[10] = {1, 2, 3, 4, 6, 8, 12, 16, 24, 32};
  const bool live_taps = igemm_wants_tapskip(op, G);
  double best = 1e300;
  int best_tile = G.Ncols <= 32 ? TILE_128x32 : TILE_128x64, best_k = 1;
  for (int ti = 0; ti < 5; ++ti) {
    const int t = tiles[ti], bn = tile_bn(t);
    if (bn >= 2 * G.Ncols && bn > 32) continue;              // more than half of every tile would be padding
    if (t == TILE_128x32 && G.Ncols > 32) continue;
    if (t == TILE_256x128 && (live_taps || op->groups == 2)) continue;     // (measured on plain launches only)
    const double cps = IGEMM_TILES[t].cps, eff2 = IGEMM_TILES[t].eff2;
    const int resident = IGEMM_TILES[t].resident;
    const int64_t tiles_n = count_tiles(G, t);
    if (t == TILE_256x128 && tiles_n < 192) continue;        // one workgroup per CU: needs a grid that covers the chip
    for (int ki = 0; ki < 10; ++ki) {
      const int k = ksplits[ki];
      // (uneven phases: no split once the unsplit grid already covers half the chip -- see above; tiny grids, e.g. the
      // image discriminator's 7x7 <- 3x3 input gradient with 25 tiles, still gain from one: 29.5 -> ~20 us)
      if (k > 1 && (min_slabs / k < 4 || out_bytes * k > 192e6 || min_slabs != max_slabs || (!even_phases && tiles_n >= 128))) break;
      // the 256x128 tile only unsplit (measured with K splits: never ahead); live-tap launches split only grids that do
      // not fill the chip (UCF video-D layer 2 input gradient at N = 16: 269 us unsplit, 318 us split 2 ways)
      if (k > 1 && (t == TILE_256x128 || (live_taps && tiles_n >= 256))) break;
      const int64_t blocks = tiles_n * k;
      // live-tap launches: tiles of the end planes are short, so the hardware's in-order dispatch evens the CUs out and
      // the whole-rounds quantisation does not apply to the big tile (measured, UCF video-D layer 2 input gradient at
      // N=32, 640 tiles of 128x128 vs 1280 of 128x64: 10 % apart although 640 is 2.5 rounds; at N=16 the smaller tile
      // with a K split stays ahead by 5 %)
      const double per_cu = (live_taps && t == TILE_128x128 && k == 1 && blocks >= 512) ? blocks / 256.0 : (double)((blocks + 255) / 256);
      const int slabs = gode_ceil_div(max_slabs, k);
      const double eff = ((per_cu >= 2 && resident >= 2) || t == TILE_256x128) ? eff2 : 0.8 * eff2;    // (8 waves cover their own barriers)
      double cyc = per_cu * (4000.0 + slabs * cps / eff);
      if (k > 1) cyc += 2.4e9 * (2.5e-6 + (k + 1) * out_bytes / 3e12);
      if (cyc < best * 0.97) { best = cyc; best_tile = t; best_k = k; }   // 3 % hysteresis toward the earlier (larger) choice
    }
  }
  *cycles_out = best;
  if (live_taps) {
    // Live-tap launches whose 128x128 grid does not cover the chip (UCF video-D layer 3 input gradient: 224 / 112 tiles): the
    // tiles of the end planes are a quarter as long as those of the middle planes and all of them are resident at once, so the
    // launch lasts as long as the CU that drew the long ones -- the estimate above (equal tiles) is 20-30 % off there.  Small
    // tiles even that out: 4-5 workgroups of 64x64 per CU (scripts/sweep_tiles.py, N = 32 / 16: 371 -> 288 us unsplit, 209 ->
    // 179 us split 3 ways; every other live-tap shape of the configs keeps the model's choice within 2 %).
    const int64_t t128 = count_tiles(G, TILE_128x128), t64 = count_tiles(G, TILE_64x64);
    if (t128 < 256 && G.Ncols >= 64 && min_slabs == max_slabs) {
      int k = (int)((1152 + t64 / 2) / t64);
      if (k < 1) k = 1;
      while (k > 1 && (min_slabs / k < 8 || out_bytes * k > 192e6)) --k;
      best_tile = TILE_64x64; best_k = k;
    }
  }
  *tile_out = best_tile;
  *sp_out = split_k(op, G, max_slabs, best_k);
}

// The border-split table of an op that asks for it (gode_igemm_op.border), or false: FPROP, fullk, image groups, live-tap
// (MODE 3) launches and shapes that do not split keep the plain table.
static bool border_table(const gode_igemm_op* op, const IgemmGeom& G, IgemmGeom* B) {
  if (!op->border || op->dir != GODE_DGRAD || op->groups == 2 || G.fullk || igemm_wants_tapskip(op, G)) return false;
  return gode_build_igemm_geom_border(op->g, op->dir, B) == 0 && B->border != 0;
}

// Cost of a FAST launch over a border-split table.  Its tiles differ in length (interior / edge / corner sub-phases: K, K/2,
// K/4 on a k4 s2 layer), the grid holds only live tiles and the longest come first, so the in-order dispatcher evens the
// CUs out and the launch lasts the summed work over the 256 CUs -- once there are clearly more tiles than workgroup slots
// and three or more workgroups per CU.  Measured on the three decoder layers at 512 rows (profiles/border_split_layers.md):
//   128x64 tiles (1024 / 2048 / 4096 of them on 768 slots): 0.826 / 0.929 / 1.004 of the plain launch with the same tile
//   where the summed work is 0.771 / 0.884 / 0.944 of it -- a loss of 1.071 / 1.050 / 1.064 against the sum: BORDER_LOSS;
//   a tail term (a share of one longest tile) fitted to the same launches came out at 0.01: the shortest tiles go last;
//   128x128 (512 tiles on 512 slots, 1024 on 512) and 256x128 (256 / 512 tiles on 256 slots): within 1 % of plain -- all
//   tiles are resident in one or two rounds and some CU draws only long ones.  Those tiles are not offered.
// Same per-tile constants as choose_fast.  Never a K split.
#define BORDER_LOSS 1.06
static void choose_border(const IgemmGeom& B, int* tile_out, double* cycles_out) {
  static const int tiles[2] = {TILE_128x64, TILE_64x64};     // (three or more workgroups per CU: see above)
  double best = 1e300; int best_tile = TILE_128x64;
  for (int ti = 0; ti < 2; ++ti) {
    const int t = tiles[ti], bm = tile_bm(t), bn = tile_bn(t);
    if (bn >= 2 * B.Ncols && bn > 32) continue;
    const double cps = IGEMM_TILES[t].cps, eff = IGEMM_TILES[t].eff2;
    const int resident = IGEMM_TILES[t].resident;
    if (3 * count_tiles(B, t) < 4 * 256 * (int64_t)resident) continue;     // (measured down to 4/3 tiles per slot)
    double work = 0;
    for (int i = 0; i < B.nphase; ++i)
      work += (double)gode_ceil_div(B.ph[i].M, bm) * gode_ceil_div(B.Ncols, bn) * (4000.0 + (B.ph[i].K >> 5) * cps / eff);
    const double cyc = BORDER_LOSS * work / 256.0;
    if (cyc < best) { best = cyc; best_tile = t; }
  }
  *tile_out = best_tile; *cycles_out = best;
}

// Which kernel of igemm.hip / conv_patch.hip serves the op.  The thin-output streaming kernels need aligned pointers besides
// (the patch kernel gathers scalars and does not): igemm_launch_cell below falls back to the tiled GEMM of the same plan when
// they are not, or when conv_patch.hip has no kernel for the shape (conv_patch_plan).
enum { IGEMM_GEMM = 0, IGEMM_PATCH_FPROP = 1, IGEMM_POINTWISE = 2, IGEMM_SMALLK = 3, IGEMM_DOT = 4 };

struct IgemmPlan {
  IgemmGeom G;                                 // the phase table in use (plain, two image groups, or border-split), row0 filled in
  int32_t family;
  int32_t tile;                                // index into IGEMM_TILES
  int32_t vec, fast;                           // strides allow float4 gathers; ... and the FAST kernel (every phase's K in whole slabs)
  int32_t ksplit, slabs_per_split, positions;  // split-K: ksplit copies of the grid, partial tiles of `positions` rows each
  int32_t max_mblk, stats_rows, rows0;         // rows of the partial statistics; those of image group 0
  int32_t tapskip, dmajor;                     // FAST kernel MODE 3; depth-major rows with this many images
  int32_t xcd_mode, MB, NB;                    // FAST kernel's 1-D grid order (igemm_block_id)
  int32_t ntab, tile0[GODE_MAX_PHASES + 1];    // border-split table: first workgroup of each entry, tile0[ntab] = grid
  int32_t interleave;                          // sub-phases per entry: 1 sub-phase after sub-phase, > 1 phase-interleaved, 0 no table
  double cycles;                               // the cost model's estimate, or -1 off the modelled path (and for image groups)
};

// The kernels beside the tiled GEMM (tile = 0 and no statistics only; image groups carry statistics).
static int thin_family(const gode_igemm_op* op, const IgemmGeom& G, bool vec) {
  if (op->tile != 0 || op->stats != nullptr || op->groups == 2) return IGEMM_GEMM;
  // first layers with 1-4 input channels: offered to conv_patch.hip (which takes 32 / 64 / 128 output channels and its own
  // list of tap shapes); none of the shapes below
  if (op->dir == GODE_FPROP && !op->scale && !op->shift && op->act == GODE_ACT_NONE && op->epilogue == GODE_EPI_RAW && op->g.Ci <= 4 &&
      op->g.Co >= 32 && G.ph[0].K >= 8)
    return IGEMM_PATCH_FPROP;
  int maxM = 0, minK = 1 << 30, maxK = 0; bool kp_ok = true;
  for (int i = 0; i < G.nphase; ++i) {
    if (G.ph[i].M > maxM) maxM = G.ph[i].M;
    if (G.ph[i].K < minK) minK = G.ph[i].K;
    if (G.ph[i].Kp > maxK) maxK = G.ph[i].Kp;
    kp_ok = kp_ok && G.ph[i].Kp == G.ph[i].K;
  }
  const int lpp = G.Cg / 4, nl = G.Ncols / 4;
  const bool one_tap = G.nphase == 1 && G.ph[0].K == G.Cg;
  // the multi-tap form needs many positions to beat the padded MFMA path (measured: M = 25 k slower, M >= 65 k faster)
  if (vec && kp_ok && G.Ncols <= 4 && G.Ncols * maxK <= PW_MAXW && maxM >= (one_tap ? 4096 : 65536) &&
      (lpp == 4 || lpp == 8 || lpp == 16 || lpp == 32 || lpp == 64))
    return IGEMM_POINTWISE;
  // K <= 4 only: at K = 8 / 16 (first discriminator layers) the per-lane gather chain made it no faster than the
  // padded MFMA path (24.9 vs 22 us, 15.7 vs 10 us); at K = 1 it is 27 us against 63 us
  if (G.nphase == 1 && G.ph[0].K <= 4 && G.Ncols % 4 == 0 && G.Ncols <= 128 && maxM >= 2048 && (nl == 4 || nl == 8 || nl == 16 || nl == 32))
    return IGEMM_SMALLK;
  if (vec && kp_ok && G.Ncols <= 4 && maxM <= 16384 && minK >= 512) return IGEMM_DOT;
  return IGEMM_GEMM;
}

// Workgroup `id` of a border-split launch -> (sub-phase, m-block, n-block); shared by the FAST kernel (igemm_block_id) and
// the host check that enumerates the whole map (tests/hostcheck/border_grid_check.cpp).  The 1-D grid holds exactly the live
// tiles, entry after entry (longest K first).  An entry is `np` consecutive sub-phases of the table with the same number
// of m-blocks and tile0[e] its first workgroup.  Inside an entry runs of 8 m-blocks go one to each XCD (workgroups are
// dealt round-robin to the 8 XCDs in id order) with all their (sub-phase, n-block) combos back to back, as xcd_mode 2 does:
// the gathered rows are fetched once per XCD; the last (< 8) m-blocks in the plain order.  A bijection of the entry's
// tiles whatever its m-block count.  np = 1: sub-phase after sub-phase.  np > 1 (gode_igemm_op.border == 2): the entry is
// one border class (interior, h-edge, w-edge, corner) of ALL stride phases, which gather the same input rows.
GODE_HD void igemm_border_block(int id, int ntab, const int32_t* tile0, int NB, int np, int& mblk, int& nblk, int& phase) {
  int e = 0;
  while (e + 1 < ntab && id >= tile0[e + 1]) ++e;     // (uniform scan of <= 16 entries)
  const int NC = NB * np, t = id - tile0[e], mb = (tile0[e + 1] - tile0[e]) / NC;
  const int grp = t / (8 * NC), r = t - grp * 8 * NC, rest = mb - grp * 8;
  int combo;
  if (rest >= 8) { mblk = grp * 8 + (r & 7); combo = r >> 3; }
  else { mblk = grp * 8 + r % rest; combo = r / rest; }
  nblk = combo % NB; phase = e * np + combo / NB;
}

// The border classes of a border-split table, for the phase-interleaved grid: sub-phases with the same extents and taps
// (hence the same K and the same number of m-blocks) form a class.  Writes the table order that lays the classes out one
// after the other (classes by first appearance, so K stays descending; members in table order) and returns the members per
// class -- or 0 when some class does not hold exactly one sub-phase of every stride phase (k3 s2 p1: the phases differ in
// taps and extents; temporal taps off both ends: two depth runs per phase), which keeps the order as it is.
static int border_classes(const IgemmGeom& B, int order[GODE_MAX_PHASES]) {
  const int nsp = B.OSd * B.OSh * B.OSw;       // stride phases
  if (!B.border || nsp < 2 || B.nphase % nsp != 0) return 0;
  const int ncls = B.nphase / nsp;
  int rep[GODE_MAX_PHASES], count[GODE_MAX_PHASES], seen[GODE_MAX_PHASES], nc = 0;
  for (int i = 0; i < B.nphase; ++i) {
    const PhaseGeom& s = B.ph[i];
    int c = 0;
    for (; c < nc; ++c) {
      const PhaseGeom& r = B.ph[rep[c]];
      if (r.Md == s.Md && r.Mh == s.Mh && r.Mw == s.Mw && r.Td == s.Td && r.Th == s.Th && r.Tw == s.Tw) break;
    }
    if (c == nc) { if (nc == ncls) return 0; rep[nc] = i; count[nc] = 0; seen[nc] = 0; ++nc; }
    const int residue = ((s.Pd % B.OSd) * B.OSh + s.Ph % B.OSh) * B.OSw + s.Pw % B.OSw;
    if (count[c] == nsp || (seen[c] >> residue & 1)) return 0;
    seen[c] |= 1 << residue;
    order[c * nsp + count[c]++] = i;
  }
  for (int c = 0; c < nc; ++c) if (count[c] != nsp) return 0;
  return nc == ncls ? nsp : 0;
}

// Order of the FAST kernel's 1-D grid over the 8 XCDs (igemm_block_id), and the tile table of a border-split launch.
static void plan_grid_order(const gode_igemm_op* op, IgemmPlan* P) {
  IgemmGeom& G = P->G;
  P->MB = 0; P->NB = 0; P->xcd_mode = 0; P->ntab = 0; P->interleave = 0;
  for (int i = 0; i <= GODE_MAX_PHASES; ++i) P->tile0[i] = 0;
  if (!P->fast) return;
  const int MB = P->max_mblk, NB = gode_ceil_div(G.Ncols, tile_bn(P->tile)), NC = NB * G.nphase;
  P->MB = MB; P->NB = NB;
  static const char* xenv = getenv("GODE_IGEMM_XCD");
  const int force = xenv ? atoi(xenv) : -1;
  const int64_t wbytes = gode_pack_floats(G) * 4;
  const bool ok1 = (NC % 8 == 0) || (NC < 8 && 8 % NC == 0 && MB % (8 / NC) == 0);
  const bool ok2 = MB % 8 == 0;
  // measured L2-miss (fabric) fetch per launch on the three decoder layers, forward / backward-data, raw FETCH_SIZE MB:
  // mode 0: 45/95/411, 76/139/161;  mode 1: 203/230/338, 197/222/161;  mode 2: 68/73/46, 76/93/161;
  // mode 3: 68/33/36, 60/89/154 -- at equal launch times (+-1.5 %), so the choice is made on traffic alone
  // Mode 3 makes every XCD read the whole weight pack once; when 8 copies of it outweigh the gathered tensor 3:1
  // (ConvT 512->256 forward: 8 x 8.4 MB vs 16.8 MB) the plain order, which spreads the panels, fetches less.
  const int64_t in_bytes = (int64_t)op->g.N * G.Gd * G.Gh * G.Gw * G.Cg * 4;
  int mode = ok2 ? (wbytes * 8 < 3 * in_bytes ? 3 : 0) : 0;
  // depth-major rows with dead-tap skipping: the tiles of the end planes are light, so a contiguous run per XCD would
  // leave the XCDs that own them idle -- interleave the m-blocks over the XCDs instead
  // -- and NOT the plain order either: it hands an XCD m-blocks 8 apart, i.e. (at 16 tiles per depth plane) only
  // planes of one weight: UCF video-D layer 2 at N = 32 runs 600 us in the plain order, 845 us with contiguous runs,
  // 470 us interleaved (scripts/exp/xcd_sweep.py; no other shape of either config moves by more than 2 %)
  if (P->dmajor > 0) mode = ok2 ? 2 : (ok1 ? 1 : 0);
  if (force == 0) mode = 0;
  if (force == 1 && ok1) mode = 1;
  if (force == 2 && ok2) mode = 2;
  if (force == 3 && ok2) mode = 3;
  P->xcd_mode = mode;
  if (G.border) {       // (never with a K split or live taps: see igemm_make_plan and border_table)
    int order[GODE_MAX_PHASES];
    static const char* oenv = getenv("GODE_IGEMM_BORDER_ORDER");      // calibration runs: 0 keeps sub-phase after sub-phase
    const int np = op->border == 2 && !(oenv && atoi(oenv) == 0) ? border_classes(G, order) : 0;
    if (np > 0) {
      // phase-interleaved: the table is re-laid class by class.  row0 was given in the table's own order and travels with
      // the sub-phase, so the launch writes the statistics rows of the op with border == 1
      const IgemmGeom T = G;
      for (int i = 0; i < G.nphase; ++i) G.ph[i] = T.ph[order[i]];
    }
    P->interleave = np > 0 ? np : 1;
    P->ntab = G.nphase / P->interleave;
    for (int e = 0; e < P->ntab; ++e)
      P->tile0[e + 1] = P->tile0[e] + gode_ceil_div(G.ph[e * P->interleave].M, tile_bm(P->tile)) * NB * P->interleave;
    for (int i = P->ntab + 1; i <= GODE_MAX_PHASES; ++i) P->tile0[i] = P->tile0[P->ntab];
  }
}

static int igemm_make_plan(const gode_igemm_op* op, IgemmPlan* P) {
  if (!op || (op->tile != 0 && !tile_exists(op->tile))) return GODE_E_ARG;
  IgemmGeom& G = P->G;
  int rc = gode_build_igemm_geom(op->g, op->dir, &G);
  if (rc) return rc;
  // input gradient of a convolution with temporal taps: depth-major tiles, so that the taps falling off the tensor's ends
  // are dead for whole tiles (skipped in the FAST kernel's K loop).  Every tile sees one or two planes (a small plane) or
  // a slice of one (a plane of >= 128 rows, which would fill tiles by itself in image-major order too -- but depth-major
  // with the interleaved XCD order is 4-6 % faster there as well: UCF video-D layer 1 input gradient 833 -> 800 us at
  // N = 32, 405 -> 381 at N = 16).
  P->tapskip = igemm_wants_tapskip(op, G);
  P->dmajor = P->tapskip ? op->g.N : 0;
  IgemmGeom B;
  const bool can_border = border_table(op, G, &B);
  const bool grouped = op->groups == 2;
  if (grouped) {
    // two image groups with SEPARATE BatchNorm partial statistics (one discriminator pass over [real; fake]): the
    // single FPROP phase becomes two phases over the two halves of the batch, so no tile straddles the groups and
    // each group's partial-statistics rows are contiguous
    if (op->dir != GODE_FPROP || op->g.N % 2 != 0 || G.nphase != 1) return GODE_E_ARG;
    G.ph[1] = G.ph[0];
    G.ph[0].M /= 2; G.ph[1].M = G.ph[0].M; G.ph[1].img0 = op->g.N / 2;
    G.nphase = 2;
  } else if (op->groups != 0 && op->groups != 1) return GODE_E_ARG;
  P->vec = strides_allow_vec(op, G);
  int tile; SplitPlan sp; double cyc = -1.0;
  bool take_border = false;
  if (op->tile == 0 && fast_geometry(G) && G.Ncols > 4 && P->vec) {
    choose_fast(op, G, &tile, &sp, &cyc);
    if (can_border && fast_geometry(B) && sp.ksplit == 1) {
      // per layer: the border form only where the model prices it below the plain launch (3 % hysteresis toward plain).
      // A launch that splits K keeps doing so: a K split adds its partial sums in another order, and an op with the flag
      // must give the raw outputs of the op without it bit for bit
      // border == 2: the caller decides per layer, from measurements -- taken whenever choose_border offers a tile
      int tb; double cb;
      choose_border(B, &tb, &cb);
      if (op->border == 2 ? cb < 1e300 : cb < 0.97 * cyc) { take_border = true; tile = tb; cyc = cb; }
    }
    // calibration runs (scripts/sweep_tiles.py): GODE_IGEMM_SWEEP enables GODE_IGEMM_FORCE="tile,k", re-read per call
    static const bool sweeping = getenv("GODE_IGEMM_SWEEP") != nullptr;
    const char* fenv = sweeping ? getenv("GODE_IGEMM_FORCE") : nullptr;
    int fk = 0, min_slabs, max_slabs;
    if (fenv && sscanf(fenv, "%d,%d", &tile, &fk) == 2) {
      if (!tile_exists(tile)) return GODE_E_ARG;
      slab_range(G, &min_slabs, &max_slabs);
      sp = split_k(op, G, max_slabs, fk);
      take_border = can_border && fk <= 1;     // (they time the border form with the forced tile)
    }
  } else {
    tile = pick_tile(G, op->tile);
    sp = plan_split(op, G, tile);
    // a REQUESTED tile takes the border form unless a plan splits K; tile = 0 off the modelled path (generic kernel, odd
    // channel counts) stays plain: nothing measured says it would pay there
    // (border == 2: on the FAST kernel only -- its grid order is what the value asks for)
    if (can_border && sp.ksplit == 1 && op->tile != 0 && (op->border != 2 || (P->vec && fast_geometry(G) && fast_geometry(B)))) {
      const int tb = pick_tile(B, op->tile);
      const SplitPlan sb = plan_split(op, B, tb);
      if (sb.ksplit == 1) { take_border = true; tile = tb; sp = sb; }
    }
  }
  if (take_border) G = B;
  if (grouped && sp.ksplit > 1 && (sp.positions / 2) % SPLITK_ROWS != 0) {
    // the split-K finish emits one statistics row per SPLITK_ROWS output positions: the groups must not share a row
    sp.ksplit = 1; sp.slabs_per_split = 0;
  }
  const int bm = tile_bm(tile);
  int r0 = 0, mx = 0;
  for (int i = 0; i < G.nphase; ++i) {
    G.ph[i].row0 = r0;
    const int mb = gode_ceil_div(G.ph[i].M, bm);
    r0 += mb;
    if (mb > mx) mx = mb;
  }
  P->tile = tile; P->ksplit = sp.ksplit; P->slabs_per_split = sp.slabs_per_split; P->positions = sp.positions;
  P->max_mblk = mx;
  P->stats_rows = sp.ksplit > 1 ? gode_ceil_div(sp.positions, SPLITK_ROWS) : r0;
  P->rows0 = !grouped ? P->stats_rows : (sp.ksplit > 1 ? P->stats_rows / 2 : G.ph[1].row0);
  P->cycles = grouped ? -1.0 : cyc;        // (its reader splits a batch into two launches; a grouped pass is never split)
  P->fast = P->vec && fast_geometry(G);
  P->family = thin_family(op, G, P->vec);
  plan_grid_order(op, P);
  return 0;
}

// ---------------------------------------------------------------------------------------------------------------
// The launch cell: what gode_igemm actually launches for an op -- the plan plus what the plan cannot see (the pointers'
// alignment, the fused operand transform, the operands' size, what conv_patch.hip has a kernel for).  gode_igemm and
// launch<TILE> (igemm.hip) dispatch on it and gode_igemm_launch_cell reports it, so a test that asserts a cell asserts the
// launch.  Still plain host arithmetic: the pointers are looked at, never through.

#define CP_MAXCOL 2         // conv_patch.hip: patch columns staged per thread and row

// conv_patch.hip's launch of an op, or false when it has no kernel for the shape (the op then runs the tiled GEMM of its plan)
struct ConvPatchPlan { int32_t Kp, CB, SPI, LWC, PR, nseg, segs, iters_per_wg, wgs, variant; int64_t lds; };
enum { CP_K3D_C3 = 1, CP_K2D_C3 = 2, CP_K3D_C1 = 3, CP_K2D_C1 = 4 };     // ConvPatchPlan.variant: the kernel instantiations
static bool conv_patch_plan(const gode_igemm_op* op, ConvPatchPlan* C) {
  const gode_conv_geom& g = op->g;
  if (op->dir != GODE_FPROP || op->groups == 2 || op->stats || op->scale || op->shift || op->act != GODE_ACT_NONE ||
      op->epilogue != GODE_EPI_RAW || op->tile != 0)
    return false;
  const int KC = g.kw * g.Ci, Kt = g.kd * g.kh * KC;
  if (g.Ci > 4 || (g.Co != 32 && g.Co != 64 && g.Co != 128) || KC % 2 != 0 || Kt < 8 || g.Wo < 16) return false;
  C->Kp = (Kt + 3) & ~3;
  C->CB = g.Co / 32; C->SPI = 4 / C->CB;
  C->LWC = (31 * g.sw + g.kw) * g.Ci;
  if (C->LWC > CP_MAXCOL * (256 / C->SPI)) return false;
  C->PR = g.kd * g.kh;
  C->lds = (int64_t)2 * C->SPI * C->PR * C->LWC * (int64_t)sizeof(float);
  if (C->lds > 60 * 1024) return false;
  C->nseg = (g.Wo + 31) / 32;
  const int64_t segs = (int64_t)g.N * g.Do * g.Ho * C->nseg;
  if (segs >= (1ll << 31) || (int64_t)g.N * g.Do * g.Ho * g.Wo * g.Co >= (1ll << 31)) return false;
  C->segs = (int)segs;
  const int nit = (C->segs + C->SPI - 1) / C->SPI;
  int wgs = nit / 4 < 1 ? 1 : nit / 4;               // >= 4 iterations per workgroup, two workgroups per CU at most
  if (wgs > 512) wgs = 512;
  C->iters_per_wg = (nit + wgs - 1) / wgs;
  C->wgs = (nit + C->iters_per_wg - 1) / C->iters_per_wg;
  const int KC2 = KC / 2;
  C->variant = 0;
  // Keyed on (kd, kh, kw * Ci / 2), not on (kw, Ci): CP_K2D_C3 also serves Ci = 4 with kw = 3, CP_K2D_C1 also Ci = 2 with kw = 2.
  // The two one-channel kernels take the tap shapes of the MNIST discriminators' first layers, but those layers have output
  // rows of 15 and 14 positions, are declined above (Wo < 16) and run the tiled GEMM; what reaches CP_K3D_C1 / CP_K2D_C1 is
  // a one-channel input with Wo >= 16, from a caller of the C ABI (tests/patch_cells.py runs all four at every Co).
  if (g.kd == 4 && g.kh == 4 && KC2 == 6) C->variant = CP_K3D_C3;      // Conv3d(3, ., 4): UCF video discriminator
  if (g.kd == 1 && g.kh == 4 && KC2 == 6) C->variant = CP_K2D_C3;      // Conv2d(3, ., 4): UCF image discriminator
  if (g.kd == 2 && g.kh == 2 && KC2 == 1) C->variant = CP_K3D_C1;      // Conv3d(1, ., 2) with Wo >= 16 (no config has one)
  if (g.kd == 1 && g.kh == 4 && KC2 == 2) C->variant = CP_K2D_C1;      // Conv2d(1, ., 4) with Wo >= 16 (no config has one)
  return C->variant != 0;
}

enum { IGEMM_K_NONE = -1,             // nothing to launch (an empty op)
       IGEMM_K_FAST_DMA = 0,          // igemm_fast_kernel MODE 2: LDS-DMA staging
       IGEMM_K_FAST_DMA_LIVE = 1,     //                   MODE 3: LDS-DMA over the live taps
       IGEMM_K_FAST_REG_XF = 2,       //                   MODE 0 with the transform on load
       IGEMM_K_FAST_REG = 3,          //                   MODE 0 plain (an operand beyond 2 GiB)
       IGEMM_K_GENERIC_VEC = 4, IGEMM_K_GENERIC_SCALAR = 5,      // igemm_kernel, float4 / scalar gathers
       IGEMM_K_POINTWISE1 = 6,        // conv_pointwise1_kernel (one tap, one column)
       IGEMM_K_POINTWISE_TAP1 = 7, IGEMM_K_POINTWISE_TAPS = 8,   // conv_pointwise_kernel<true / false>
       IGEMM_K_SMALLK = 9, IGEMM_K_DOT = 10, IGEMM_K_PATCH = 11 };
enum { IGEMM_REDUCE_NONE = 0, IGEMM_REDUCE_VEC = 1, IGEMM_REDUCE_SCALAR = 2 };           // the split-K finish
enum { IGEMM_TABLE_PLAIN = 0, IGEMM_TABLE_BORDER = 1, IGEMM_TABLE_INTERLEAVED = 2 };     // the phase table of a tiled launch

struct IgemmLaunchCell {
  int32_t rc;                         // what gode_igemm returns before it launches anything (0: it launches `kernel`)
  int32_t kernel, tile, reduce;       // tile: 0 off the tiled GEMM
  int32_t ksplit, xcd_mode, table, interleave, tapskip;    // of the tiled GEMM (xcd_mode: the FAST kernels only); ksplit 1
                                      // with a reduce: a plan that splits K served unsplit by the generic kernel
  int32_t vec;                        // pointers and strides allow float4 gathers
  uint32_t src_bytes, w_bytes;        // extents of the operands as raw buffers, 0 beyond 2 GiB
  ConvPatchPlan patch;                // kernel == IGEMM_K_PATCH
};
#define IGEMM_CELL_INTS 8             // gode_igemm_launch_cell: kernel, tile, reduce, ksplit, xcd_mode, table, interleave, tapskip

static bool igemm_ptr16(const void* p) { return ((uintptr_t)p % 16) == 0; }

// Element strides of the gathered operand and the span they cover, in elements; -1 with a negative stride.
static int64_t igemm_gather_span(const gode_igemm_op* op, const IgemmGeom& G, int64_t gs[5]) {
  if (gode_strides_are_channels_last(op->gs)) {
    gs[4] = 1; gs[3] = G.Cg; gs[2] = (int64_t)G.Gw * gs[3]; gs[1] = (int64_t)G.Gh * gs[2]; gs[0] = (int64_t)G.Gd * gs[1];
  } else {
    for (int i = 0; i < 5; ++i) gs[i] = op->gs[i];
  }
  for (int i = 0; i < 5; ++i) if (gs[i] < 0) return -1;
  return 1 + (int64_t)(op->g.N - 1) * gs[0] + (int64_t)(G.Gd - 1) * gs[1] + (int64_t)(G.Gh - 1) * gs[2] + (int64_t)(G.Gw - 1) * gs[3] +
         (int64_t)(G.Cg - 1) * gs[4];
}

static IgemmLaunchCell igemm_launch_cell(const gode_igemm_op* op, const IgemmPlan& P, int64_t span) {
  const IgemmGeom& G = P.G;
  IgemmLaunchCell c;
  c.rc = 0; c.kernel = IGEMM_K_NONE; c.tile = 0; c.reduce = IGEMM_REDUCE_NONE;
  c.ksplit = 1; c.xcd_mode = 0; c.table = IGEMM_TABLE_PLAIN; c.interleave = 0; c.tapskip = 0; c.vec = 0; c.src_bytes = 0; c.w_bytes = 0;
  if (P.max_mblk == 0) return c;
  // 32-bit offset arithmetic inside the kernels: the gathered span and the output must stay below 2^31 elements
  const int64_t outn = (int64_t)op->g.N * G.Xd * G.Xh * G.Xw * G.Ncols;
  if (span < 0) { c.rc = GODE_E_ARG; return c; }
  if (span >= (1ll << 31) || outn >= (1ll << 31)) { c.rc = GODE_E_SHAPE; return c; }
  if (!igemm_ptr16(op->wpack) || (op->scale == nullptr) != (op->shift == nullptr)) { c.rc = GODE_E_ARG; return c; }
  if (P.family == IGEMM_PATCH_FPROP && conv_patch_plan(op, &c.patch)) { c.kernel = IGEMM_K_PATCH; return c; }
  c.src_bytes = span * 4 < (1ll << 31) ? (uint32_t)(span * 4) : 0u;
  c.w_bytes = gode_pack_floats(G) * 4 < (1ll << 31) ? (uint32_t)(gode_pack_floats(G) * 4) : 0u;
  // what the plan could not see: the pointers' alignment.  It only ever takes the op from its family to the tiled GEMM, and
  // there from the vector kernels to the generic one -- tile and K split stay the plan's
  const bool vec = P.vec && igemm_ptr16(op->src) && (op->scale == nullptr || (igemm_ptr16(op->scale) && igemm_ptr16(op->shift)));
  c.vec = vec;
  if (P.family == IGEMM_POINTWISE && vec) {
    const bool one_tap = G.nphase == 1 && G.ph[0].K == G.Cg;
    c.kernel = one_tap && G.Ncols == 1 && G.Cg / 4 <= 16 ? IGEMM_K_POINTWISE1 : (one_tap ? IGEMM_K_POINTWISE_TAP1 : IGEMM_K_POINTWISE_TAPS);
    return c;
  }
  if (P.family == IGEMM_SMALLK && igemm_ptr16(op->out)) { c.kernel = IGEMM_K_SMALLK; return c; }
  if (P.family == IGEMM_DOT && vec) { c.kernel = IGEMM_K_DOT; return c; }
  // the tiled GEMM
  c.tile = P.tile; c.ksplit = P.ksplit; c.tapskip = P.tapskip; c.interleave = P.interleave;
  c.table = !G.border ? IGEMM_TABLE_PLAIN : (P.interleave > 1 ? IGEMM_TABLE_INTERLEAVED : IGEMM_TABLE_BORDER);
  const bool fast = vec && P.fast;
  if (!fast || (P.ksplit > 1 && op->work == nullptr)) {
    c.kernel = vec ? IGEMM_K_GENERIC_VEC : IGEMM_K_GENERIC_SCALAR;
    if (P.ksplit > 1) {
      // A plan that splits K, without its workspace or off the FAST path.  The statistics rows were sized from the plan (one
      // per SPLITK_ROWS positions), so the launch keeps that layout: the generic kernel writes the raw, unsplit result as the
      // one slab -- into work, or into out itself -- and the split-K finish runs over that slab (in place: every element is
      // read and written by the same thread), applying the epilogue and the statistics.
      const float* slab = op->work ? op->work : op->out;
      c.ksplit = 1;
      c.reduce = G.Ncols % 4 == 0 && igemm_ptr16(slab) && igemm_ptr16(op->out) ? IGEMM_REDUCE_VEC : IGEMM_REDUCE_SCALAR;
    }
    return c;
  }
  c.xcd_mode = P.xcd_mode;
  // LDS-DMA staging unless the previous layer's BatchNorm/activation is fused into the load or an operand is beyond the
  // 2 GiB a raw buffer's offsets span: then register staging (MODE 0)
  const bool has_xf = op->scale != nullptr || op->act != GODE_ACT_NONE;
  const bool glds = !has_xf && c.src_bytes != 0 && c.w_bytes != 0;
  c.kernel = glds ? (P.tapskip ? IGEMM_K_FAST_DMA_LIVE : IGEMM_K_FAST_DMA) : (has_xf ? IGEMM_K_FAST_REG_XF : IGEMM_K_FAST_REG);
  if (P.ksplit > 1) c.reduce = G.Ncols % 4 == 0 && igemm_ptr16(op->work) && igemm_ptr16(op->out) ? IGEMM_REDUCE_VEC : IGEMM_REDUCE_SCALAR;
  return c;
}

// Plan and cell of an op as gode_igemm sees it (the argument checks in its order); gs: the gathered operand's strides.
static int igemm_plan_launch(const gode_igemm_op* op, IgemmPlan* P, int64_t gs[5], IgemmLaunchCell* cell) {
  if (!op || !op->src || !op->wpack || !op->out) return GODE_E_ARG;
  const int rc = igemm_make_plan(op, P);
  if (rc) return rc;
  *cell = igemm_launch_cell(op, *P, igemm_gather_span(op, P->G, gs));
  return cell->rc;
}
