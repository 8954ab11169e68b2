// Stand-alone host check (own main, built with -fsanitize=address,undefined by tests/test_host_border_grid.py) of
// gode_igemm_op.border == 2 in gan-ode_amd/csrc/igemm_plan.h: when such an op takes the border-split table, and the map from
// workgroup id to (sub-phase, m-block, n-block) that the FAST kernel shares with this program (igemm_border_block), in both
// grid orders.  Every DGRAD op of plan_check.cpp's corpus (the same shape lists; the k4 s2 p1 shapes of the GPU test
// besides), tile 0 and the requested tiles 2 and 4.  No randomness, no GPU.
//   1. the border table is used exactly when border_table() has one, the geometry is FAST, K is not split and a tile is
//      offered (tile 0: choose_border; a requested tile: that tile);
//   2. the decode maps [0, grid) onto every live (sub-phase, m-block, n-block) exactly once;
//   3. K never grows along the grid;
//   4. border == 1 and border == 2 give the same statistics rows to the same sub-phases at equal tile, and an interleaved
//      entry holds one sub-phase of every stride phase, all of one extent;
//   5. plans of border 0 / 1 do not depend on anything this value added (the same op planned twice, around a flagged one).
#include <cstdio>
#include <cstring>
#include <set>
#include <string>
#include <vector>
#include "../../gan-ode_amd/csrc/igemm_plan.h"

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { ++failures; std::printf("FAIL: " __VA_ARGS__); std::printf("\n"); } } while (0)

struct Base { std::string name; gode_conv_geom g; };
static std::vector<Base> corpus;
static std::set<std::string> seen;

static int conv_out(int i, int k, int s, int p) { return (i + 2 * p - k) / s + 1; }

static void add(const std::string& name, int N, int Ci, int Co, int Di, int Hi, int Wi, int kd, int kh, int kw, int sd, int sh, int sw,
                int pd, int ph, int pw) {
  const gode_conv_geom g = {N, Ci, Co, Di, Hi, Wi, conv_out(Di, kd, sd, pd), conv_out(Hi, kh, sh, ph), conv_out(Wi, kw, sw, pw),
                            kd, kh, kw, sd, sh, sw, pd, ph, pw};
  char key[160];
  std::snprintf(key, sizeof key, "%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d", N, Ci, Co, Di, Hi, Wi, kd, kh, kw, sd, sh, sw, pd, ph, pw);
  if (seen.insert(key).second) corpus.push_back(Base{name, g});
}

static void add_generator(const char* cfg, int rows, bool mnist) {
  const std::string n = std::string(cfg) + ".G" + std::to_string(rows) + ".L";
  add(n + "0", rows, 512, 96, 1, 4, 4, 1, 4, 4, 1, 1, 1, 0, 0, 0);
  const int ci[3] = {256, 128, 64};
  for (int l = 0, hw = 4; l < 3; ++l, hw *= 2) add(n + std::to_string(l + 1), rows, ci[l], 2 * ci[l], 1, 2 * hw, 2 * hw, 1, 4, 4, 1, 2, 2, 0, 1, 1);
  if (mnist) add(n + "4", rows, 1, 64, 1, 28, 28, 1, 1, 1, 1, 1, 1, 0, 2, 2);
  else add(n + "4", rows, 3, 64, 1, 64, 64, 1, 4, 4, 1, 2, 2, 0, 1, 1);
}

static void add_video_d(const char* cfg, int B, int C, int D, int HW, int k) {
  const std::string n = std::string(cfg) + ".V" + std::to_string(B) + ".L";
  const int ch[5] = {C, 64, 128, 256, 512};
  int H = HW;
  for (int l = 0; l < 4; ++l) {
    add(n + std::to_string(l), B, ch[l], ch[l + 1], D, H, H, k, k, k, 1, 2, 2, 0, 1, 1);
    D = conv_out(D, k, 1, 0); H = conv_out(H, k, 2, 1);
  }
  add(n + "4", B, 512, 1, D, H, H, k, k, k, 1, 1, 1, 0, 0, 0);
}

static void add_image_d(const char* cfg, int B, int C, int HW) {
  const std::string n = std::string(cfg) + ".I" + std::to_string(B) + ".L";
  const int ch[5] = {C, 64, 128, 256, 1};
  for (int l = 0, H = HW; l < 4; ++l, H = conv_out(H, 4, 2, 1)) add(n + std::to_string(l), B, ch[l], ch[l + 1], 1, H, H, 1, 4, 4, 1, 2, 2, 0, 1, 1);
}

static void build_corpus() {
  static const int mnist_rows[3] = {512, 32, 544}, mnist_batch[2] = {32, 64};
  for (int r : mnist_rows) add_generator("mnist", r, true);
  for (int b : mnist_batch) { add_video_d("mnist", b, 1, 16, 28, 2); add_image_d("mnist", b, 1, 28); }
  static const int ucf_rows[6] = {256, 16, 272, 512, 32, 544}, ucf_batch[3] = {16, 32, 64};
  for (int r : ucf_rows) add_generator("ucf", r, false);
  for (int b : ucf_batch) { add_video_d("ucf", b, 3, 16, 64, 4); add_image_d("ucf", b, 3, 64); }
  // tests/test_gpu_kernels.py CASES: (Ci, Co, (Di,Hi,Wi), k, s, p, N)
  static const int cases[][15] = {
      {1, 8, 16, 28, 28, 2, 2, 2, 1, 2, 2, 0, 1, 1, 3},       {8, 16, 15, 15, 15, 2, 2, 2, 1, 2, 2, 0, 1, 1, 3},
      {64, 128, 15, 15, 15, 2, 2, 2, 1, 2, 2, 0, 1, 1, 2},    {16, 1, 12, 3, 3, 2, 2, 2, 1, 1, 1, 0, 0, 0, 5},
      {3, 8, 6, 16, 16, 4, 4, 4, 1, 2, 2, 0, 1, 1, 2},        {32, 64, 1, 8, 8, 1, 4, 4, 1, 2, 2, 0, 1, 1, 9},
      {128, 256, 1, 8, 8, 1, 4, 4, 1, 2, 2, 0, 1, 1, 40},     {1, 8, 1, 28, 28, 1, 1, 1, 1, 1, 1, 0, 2, 2, 4},
      {12, 1, 1, 3, 3, 1, 4, 4, 1, 2, 2, 0, 1, 1, 7},         {5, 7, 3, 7, 9, 3, 2, 2, 1, 3, 2, 1, 1, 0, 2},
      {64, 128, 1, 32, 32, 1, 4, 4, 1, 2, 2, 0, 1, 1, 6},     {256, 512, 1, 8, 8, 1, 4, 4, 1, 2, 2, 0, 1, 1, 70},
      {256, 512, 13, 5, 5, 2, 2, 2, 1, 2, 2, 0, 1, 1, 8},     {1, 64, 1, 28, 28, 1, 1, 1, 1, 1, 1, 0, 2, 2, 8},
      {2, 32, 1, 28, 28, 1, 1, 1, 1, 1, 1, 0, 2, 2, 9},       {1, 64, 16, 28, 28, 2, 2, 2, 1, 2, 2, 0, 1, 1, 3},
      {1, 64, 1, 28, 28, 1, 4, 4, 1, 2, 2, 0, 1, 1, 12},      {2, 16, 1, 30, 30, 1, 3, 3, 1, 1, 1, 0, 1, 1, 3},
      {3, 64, 1, 64, 64, 1, 4, 4, 1, 2, 2, 0, 1, 1, 5},       {64, 3, 1, 32, 32, 1, 4, 4, 1, 2, 2, 0, 1, 1, 20},
      {1, 32, 6, 28, 28, 2, 2, 2, 1, 2, 2, 0, 1, 1, 4},       {3, 64, 16, 64, 64, 4, 4, 4, 1, 2, 2, 0, 1, 1, 16},
      {64, 128, 13, 32, 32, 4, 4, 4, 1, 2, 2, 0, 1, 1, 16},   {128, 256, 10, 16, 16, 4, 4, 4, 1, 2, 2, 0, 1, 1, 16},
      {256, 512, 7, 8, 8, 4, 4, 4, 1, 2, 2, 0, 1, 1, 16},     {512, 1, 4, 4, 4, 4, 4, 4, 1, 1, 1, 0, 0, 0, 16},
      {256, 512, 7, 8, 8, 4, 4, 4, 1, 2, 2, 0, 1, 1, 2},      {64, 128, 13, 32, 32, 4, 4, 4, 1, 2, 2, 0, 1, 1, 1},
      {128, 256, 10, 16, 16, 4, 4, 4, 1, 2, 2, 0, 1, 1, 3},   {3, 32, 1, 40, 40, 1, 4, 4, 1, 2, 2, 0, 1, 1, 3},
      {2, 128, 2, 20, 96, 2, 3, 3, 1, 1, 2, 0, 1, 1, 2},      {4, 32, 5, 18, 66, 3, 3, 3, 1, 2, 2, 1, 0, 1, 2},
      {3, 32, 7, 12, 40, 5, 2, 2, 1, 1, 1, 2, 1, 0, 2},       {3, 32, 8, 12, 40, 6, 2, 2, 1, 1, 1, 2, 1, 0, 2}};
  int i = 0;
  for (const auto& c : cases)
    add("case" + std::to_string(i++), c[14], c[0], c[1], c[2], c[3], c[4], c[5], c[6], c[7], c[8], c[9], c[10], c[11], c[12], c[13]);
  static const int convt[][4] = {{512, 64, 96, 4}, {2, 512, 256, 16}, {512, 512, 256, 4}, {512, 256, 128, 8}, {512, 128, 64, 16}, {4, 64, 96, 4}};
  for (const auto& c : convt) add("convt" + std::to_string(c[0]) + "x" + std::to_string(c[1]) + "x" + std::to_string(c[3]), c[0], c[2], c[1], 1, 2 * c[3], 2 * c[3], 1, 4, 4, 1, 2, 2, 0, 1, 1);
  add("fullk4", 4, 32, 64, 1, 4, 4, 1, 4, 4, 1, 1, 1, 0, 0, 0);
  static const int hs[6] = {1, 2, 3, 4, 8, 16};
  for (int h : hs) add("bc.k4s2p1." + std::to_string(h), 2, 3, 8, 1, 2 * h, 2 * h, 1, 4, 4, 1, 2, 2, 0, 1, 1);
  add("bc.k4s2p1.2x5", 2, 3, 8, 1, 4, 10, 1, 4, 4, 1, 2, 2, 0, 1, 1);
  add("bc.k3s2p1.7", 2, 3, 8, 1, 7, 7, 1, 3, 3, 1, 2, 2, 0, 1, 1);
  add("bc.k3s2p1.8", 2, 3, 8, 1, 8, 8, 1, 3, 3, 1, 2, 2, 0, 1, 1);
  add("bc.3d.k144", 2, 3, 8, 3, 8, 8, 1, 4, 4, 1, 2, 2, 0, 1, 1);
  add("bc.3d.k344.2x1x1", 2, 3, 8, 2, 2, 2, 3, 4, 4, 1, 2, 2, 1, 1, 1);
  add("bc.3d.k344.2x2x2", 2, 3, 8, 2, 4, 4, 3, 4, 4, 1, 2, 2, 1, 1, 1);
  add("extra.n32", 64, 32, 32, 1, 16, 16, 1, 3, 3, 1, 1, 1, 0, 1, 1);
  // the shapes of tests/test_gpu_border_grid.py: ConvTranspose 32 -> 64 (conv orientation: Ci = 64, Co = 32)
  static const int gt[][3] = {{24, 4, 4}, {40, 4, 4}, {24, 8, 8}, {40, 8, 8}, {24, 3, 3}, {24, 4, 10}};
  for (const auto& c : gt) add("gt.k4s2p1." + std::to_string(c[0]) + "x" + std::to_string(c[1]) + "x" + std::to_string(c[2]), c[0], 64, 32, 1, 2 * c[1], 2 * c[2], 1, 4, 4, 1, 2, 2, 0, 1, 1);
  add("gt.k3s2p1.7", 24, 64, 32, 1, 7, 7, 1, 3, 3, 1, 2, 2, 0, 1, 1);
  // (12 slabs of K: 1040 images give the >= 64 tiles below which such a launch splits K and stays plain)
  add("gt.3d.k344.2x1x1", 1040, 64, 32, 2, 2, 2, 3, 4, 4, 1, 2, 2, 1, 1, 1);
}

static bool same_plan(const IgemmPlan& a, const IgemmPlan& b) {
  bool eq = a.family == b.family && a.tile == b.tile && a.vec == b.vec && a.fast == b.fast && a.ksplit == b.ksplit &&
            a.slabs_per_split == b.slabs_per_split && a.positions == b.positions && a.max_mblk == b.max_mblk && a.stats_rows == b.stats_rows &&
            a.rows0 == b.rows0 && a.tapskip == b.tapskip && a.dmajor == b.dmajor && a.xcd_mode == b.xcd_mode && a.MB == b.MB && a.NB == b.NB &&
            a.ntab == b.ntab && a.interleave == b.interleave && std::memcmp(&a.cycles, &b.cycles, sizeof a.cycles) == 0 &&
            a.G.nphase == b.G.nphase && a.G.border == b.G.border;
  for (int i = 0; i <= GODE_MAX_PHASES; ++i) eq = eq && a.tile0[i] == b.tile0[i];
  for (int i = 0; eq && i < a.G.nphase; ++i) {
    const PhaseGeom &p = a.G.ph[i], &q = b.G.ph[i];
    eq = p.M == q.M && p.Md == q.Md && p.Mh == q.Mh && p.Mw == q.Mw && p.K == q.K && p.Kp == q.Kp && p.Td == q.Td && p.Th == q.Th && p.Tw == q.Tw &&
         p.Od == q.Od && p.Oh == q.Oh && p.Ow == q.Ow && p.Pd == q.Pd && p.Ph == q.Ph && p.Pw == q.Pw && p.kd0 == q.kd0 && p.kh0 == q.kh0 &&
         p.kw0 == q.kw0 && p.row0 == q.row0 && p.img0 == q.img0 && p.w_off == q.w_off;
  }
  return eq;
}

// the whole grid of a border-split FAST plan through the kernel's decode
static void check_grid(const char* what, const IgemmPlan& P) {
  const int bm = tile_bm(P.tile), NB = gode_ceil_div(P.G.Ncols, tile_bn(P.tile)), np = P.interleave;
  CHECK(P.ntab > 0 && np >= 1 && P.ntab * np == P.G.nphase && P.NB == NB && P.tile0[0] == 0, "%s: table of %d entries x %d for %d sub-phases", what, P.ntab, np,
        P.G.nphase);
  if (!(P.ntab > 0 && np >= 1 && P.ntab * np == P.G.nphase)) return;
  int64_t live = 0;
  std::vector<int> first(P.G.nphase + 1, 0);      // index of (phase, 0, 0) in the visited bitmap
  for (int i = 0; i < P.G.nphase; ++i) { first[i + 1] = first[i] + gode_ceil_div(P.G.ph[i].M, bm) * NB; }
  live = first[P.G.nphase];
  const int grid = P.tile0[P.ntab];
  CHECK(grid == live, "%s: grid %d, live tiles %lld", what, grid, (long long)live);
  for (int e = 0; e < P.ntab; ++e)
    for (int j = 0; j < np; ++j)
      CHECK(gode_ceil_div(P.G.ph[e * np + j].M, bm) == gode_ceil_div(P.G.ph[e * np].M, bm) && P.G.ph[e * np + j].K == P.G.ph[e * np].K,
            "%s: entry %d mixes sub-phases of different length", what, e);
  std::vector<char> hit(live, 0);
  int prev_K = 1 << 30;
  for (int id = 0; id < grid; ++id) {
    int mblk = -1, nblk = -1, phase = -1;
    igemm_border_block(id, P.ntab, P.tile0, P.NB, np, mblk, nblk, phase);
    const bool in = phase >= 0 && phase < P.G.nphase && nblk >= 0 && nblk < NB && mblk >= 0 && mblk * bm < P.G.ph[phase < 0 || phase >= P.G.nphase ? 0 : phase].M;
    CHECK(in, "%s: workgroup %d -> (%d, %d, %d) is no live tile", what, id, phase, mblk, nblk);
    if (!in) return;
    char& h = hit[first[phase] + mblk * NB + nblk];
    CHECK(!h, "%s: tile (%d, %d, %d) visited twice", what, phase, mblk, nblk);
    h = 1;
    CHECK(P.G.ph[phase].K <= prev_K, "%s: K grows at workgroup %d", what, id);
    prev_K = P.G.ph[phase].K;
  }
  for (int64_t i = 0; i < live; ++i) if (!hit[i]) { CHECK(false, "%s: a live tile is never visited", what); break; }
}

int main(int argc, char** argv) {
  const bool verbose = argc > 1 && std::strcmp(argv[1], "-v") == 0;      // one line per plan that takes the table
  build_corpus();
  static const int tiles[3] = {0, TILE_128x64, TILE_64x64};
  int taken = 0, interleaved = 0, kept_order = 0, declined = 0;
  for (const Base& b : corpus)
    for (int tile : tiles) {
      gode_igemm_op op;
      std::memset(&op, 0, sizeof op);
      op.g = b.g; op.dir = GODE_DGRAD; op.tile = tile; op.groups = 1;
      char what[96];
      std::snprintf(what, sizeof what, "%s t%d", b.name.c_str(), tile);
      IgemmPlan P0, P1, P2, Q0, Q1;
      op.border = 0; const int r0 = igemm_make_plan(&op, &P0);
      op.border = 1; const int r1 = igemm_make_plan(&op, &P1);
      op.border = 2; const int r2 = igemm_make_plan(&op, &P2);
      op.border = 1; const int q1 = igemm_make_plan(&op, &Q1);
      op.border = 0; const int q0 = igemm_make_plan(&op, &Q0);
      CHECK(r0 == q0 && r1 == q1 && r0 == r2, "%s: return codes %d %d %d", what, r0, r1, r2);
      if (r0 || r1 || r2) continue;
      // 5. (the golden of tests/test_host_igemm_plan.py pins their text; here: no state leaks from the flagged plan)
      CHECK(same_plan(P0, Q0) && same_plan(P1, Q1) && P0.interleave == 0 && P1.interleave == (P1.ntab > 0 ? 1 : 0) && P0.G.border == 0,
            "%s: a plan without the new value changed", what);
      // 1. when the table is used
      IgemmGeom G, B;
      gode_build_igemm_geom(op.g, GODE_DGRAD, &G);
      op.border = 2;
      const bool table = border_table(&op, G, &B);
      const bool fast = strides_allow_vec(&op, G) && fast_geometry(G) && table && fast_geometry(B);
      bool offered = false; int want_tile = tile;
      if (fast && tile == 0) { double c; choose_border(B, &want_tile, &c); offered = c < 1e300 && G.Ncols > 4; }
      else if (fast) offered = true;
      const bool unsplit = P0.ksplit == 1 && (tile == 0 || plan_split(&op, B, tile).ksplit == 1);
      const bool expect = table && fast && unsplit && offered;
      CHECK((P2.G.border != 0) == expect, "%s: border table %s, expected %s (table %d fast %d unsplit %d offered %d)", what, P2.G.border ? "used" : "not used",
            expect ? "used" : "not used", table, fast, unsplit, offered);
      if (!P2.G.border) {
        CHECK(same_plan(P2, P0), "%s: a declined border = 2 plan is not the plain plan", what);
        ++declined;
        continue;
      }
      ++taken;
      if (verbose) {
        std::printf("%s: tile %d, %d entries x %d sub-phases [", what, P2.tile, P2.ntab, P2.interleave);
        for (int e = 0; e <= P2.ntab; ++e) std::printf("%s%d", e ? "," : "", P2.tile0[e]);
        std::printf("] %.0f cycles (plain %.0f)\n", P2.cycles, P0.cycles);
      }
      CHECK(P2.tile == want_tile && P2.ksplit == 1 && P2.fast == 1 && P2.ntab > 0, "%s: tile %d (expected %d), ksplit %d, fast %d", what, P2.tile, want_tile, P2.ksplit, P2.fast);
      check_grid(what, P2);
      if (P2.interleave > 1) ++interleaved; else ++kept_order;
      // 4. an interleaved entry: one sub-phase of every stride phase, equal extents
      const int nsp = G.nphase;
      if (P2.interleave > 1) {
        CHECK(P2.interleave == nsp, "%s: %d sub-phases per entry, %d stride phases", what, P2.interleave, nsp);
        for (int e = 0; e < P2.ntab; ++e) {
          unsigned mask = 0;
          for (int j = 0; j < P2.interleave; ++j) {
            const PhaseGeom &s = P2.G.ph[e * P2.interleave + j], &f = P2.G.ph[e * P2.interleave];
            mask |= 1u << (((s.Pd % G.OSd) * G.OSh + s.Ph % G.OSh) * G.OSw + s.Pw % G.OSw);
            CHECK(s.Md == f.Md && s.Mh == f.Mh && s.Mw == f.Mw && s.Td == f.Td && s.Th == f.Th && s.Tw == f.Tw, "%s: entry %d mixes classes", what, e);
          }
          CHECK(mask == (1u << nsp) - 1, "%s: entry %d does not hold every stride phase once", what, e);
        }
      }
      // 4. the same statistics rows as border == 1 with this tile (tile 0: border == 1 may have stayed plain)
      op.border = 1; op.tile = P2.tile;
      IgemmPlan R;
      CHECK(igemm_make_plan(&op, &R) == 0 && R.G.border && R.tile == P2.tile && R.stats_rows == P2.stats_rows && R.interleave == 1, "%s: no border = 1 plan with tile %d", what, P2.tile);
      check_grid(what, R);
      for (int i = 0; i < P2.G.nphase; ++i) {
        const PhaseGeom& s = P2.G.ph[i];
        int hits = 0;
        for (int j = 0; j < R.G.nphase; ++j) {
          const PhaseGeom& r = R.G.ph[j];
          hits += r.row0 == s.row0 && r.M == s.M && r.K == s.K && r.w_off == s.w_off && r.Pd == s.Pd && r.Ph == s.Ph && r.Pw == s.Pw && r.Od == s.Od &&
                  r.Oh == s.Oh && r.Ow == s.Ow && r.kd0 == s.kd0 && r.kh0 == s.kh0 && r.kw0 == s.kw0 && r.Md == s.Md && r.Mh == s.Mh && r.Mw == s.Mw;
        }
        CHECK(hits == 1, "%s: sub-phase %d is not a sub-phase of the border = 1 plan with its rows", what, i);
      }
    }
  std::printf("%zu ops x 3 tiles: border table taken %d (phase-interleaved %d, order kept %d), declined %d\n", corpus.size(), taken, interleaved, kept_order, declined);
  // the cases the rule is about must be in the walk
  CHECK(interleaved > 0 && kept_order > 0 && declined > 0, "the corpus does not reach every case");
  std::printf("%s (%d failures)\n", failures ? "FAILED" : "OK", failures);
  return failures ? 1 : 0;
}
