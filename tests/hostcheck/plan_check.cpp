// Stand-alone host check (own main, built with -fsanitize=address,undefined by tests/test_host_igemm_plan.py) of the launch
// plans of gan-ode_amd/csrc/igemm_plan.h.  Plans every op of a fixed corpus and writes each plan as one line with every field
// of its IgemmPlan (the phase table as kind, phase count and an FNV-1a hash over all of its fields): the plans the configs
// get are printed, the other variants are hashed per op (see main).  The test compares the output with
// tests/golden/igemm_plans.txt line by line.  No randomness, no GPU.
//
// Corpus: every layer, both directions, of build_mnist() (generator rows 512 / 32 / 544, discriminator batch 32 / 64) and of
// build_ucf() at batch 16 and 32; the CASES of tests/test_gpu_kernels.py; the shapes of tests/test_host_border_geometry.py
// and tests/hostcheck/border_check.cpp; a few shapes added for plan fields the rest does not reach.  Each op with border 0 / 1,
// groups 1 / 2 (FPROP, even batch), tile 0 / 1 / 2 / 3 / 4 / 6, channels-last strides and (first layers: FPROP with up to 4 input
// channels) the source read in place as [N, C, D, H, W].
// Line: name s<strided> g<groups> b<border> t<tile>: family tile vec fast ksplit/slabs_per_split positions max_mblk
//       stats_rows/rows0 tapskip dmajor xcd_mode MB NB ntab[tile0...] cycles(%a, or -1) table/nphase/hash
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <set>
#include <string>
#include <vector>
#include "../../gan-ode_amd/csrc/igemm_plan.h"

struct Base { std::string name; gode_conv_geom g; int dir; };
static std::vector<Base> corpus;
static std::set<std::string> seen;

static int conv_out(int i, int k, int s, int p) { return (i + 2 * p - k) / s + 1; }

// (N, Ci, Co, x extent, k, s, p) in conv orientation, both directions; a geometry already in the corpus is not repeated
static void add(const std::string& name, int N, int Ci, int Co, int Di, int Hi, int Wi, int kd, int kh, int kw, int sd, int sh, int sw,
                int pd, int ph, int pw) {
  const gode_conv_geom g = {N, Ci, Co, Di, Hi, Wi, conv_out(Di, kd, sd, pd), conv_out(Hi, kh, sh, ph), conv_out(Wi, kw, sw, pw),
                            kd, kh, kw, sd, sh, sw, pd, ph, pw};
  char key[160];
  std::snprintf(key, sizeof key, "%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d", N, Ci, Co, Di, Hi, Wi, kd, kh, kw, sd, sh, sw, pd, ph, pw);
  if (!seen.insert(key).second) return;
  corpus.push_back(Base{name + ".f", g, GODE_FPROP});
  corpus.push_back(Base{name + ".d", g, GODE_DGRAD});
}

// the decoder (modules.py, _decoder_specs): ConvTranspose2d layers as the input gradients of their convolutions
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
  // UCF at batch 16 and 32: 16 frames per video -> video rows, image rows, the joint pass; the discriminators also paired
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
  // tests/test_host_border_geometry.py: ConvTranspose2d(cin, cout, 4, 2, 1) on h x h as (n, cin, cout, h)
  static const int convt[][4] = {{512, 64, 96, 4}, {2, 512, 256, 16}, {512, 512, 256, 4}, {512, 256, 128, 8}, {512, 128, 64, 16}, {4, 64, 96, 4}};
  for (const auto& c : convt) add("convt" + std::to_string(c[0]) + "x" + std::to_string(c[1]) + "x" + std::to_string(c[3]), c[0], c[2], c[1], 1, 2 * c[3], 2 * c[3], 1, 4, 4, 1, 2, 2, 0, 1, 1);
  add("fullk4", 4, 32, 64, 1, 4, 4, 1, 4, 4, 1, 1, 1, 0, 0, 0);
  // tests/hostcheck/border_check.cpp (N = 2, Ci = 3, Co = 8)
  static const int hs[6] = {1, 2, 3, 4, 8, 16};
  for (int h : hs) add("bc.k4s2p1." + std::to_string(h), 2, 3, 8, 1, 2 * h, 2 * h, 1, 4, 4, 1, 2, 2, 0, 1, 1);
  add("bc.k4s2p1.2x5", 2, 3, 8, 1, 4, 10, 1, 4, 4, 1, 2, 2, 0, 1, 1);
  add("bc.k3s2p1.7", 2, 3, 8, 1, 7, 7, 1, 3, 3, 1, 2, 2, 0, 1, 1);
  add("bc.k3s2p1.8", 2, 3, 8, 1, 8, 8, 1, 3, 3, 1, 2, 2, 0, 1, 1);
  add("bc.3d.k144", 2, 3, 8, 3, 8, 8, 1, 4, 4, 1, 2, 2, 0, 1, 1);
  add("bc.3d.k344.2x1x1", 2, 3, 8, 2, 2, 2, 3, 4, 4, 1, 2, 2, 1, 1, 1);
  add("bc.3d.k344.2x2x2", 2, 3, 8, 2, 4, 4, 3, 4, 4, 1, 2, 2, 1, 1, 1);
  // added for plan fields the lists above do not reach: 32 output columns on the modelled path (the 128x32 tile)
  add("extra.n32", 64, 32, 32, 1, 16, 16, 1, 3, 3, 1, 1, 1, 0, 1, 1);
}

static uint64_t fnv(uint64_t h, const void* p, size_t n) {
  const unsigned char* b = static_cast<const unsigned char*>(p);
  for (size_t i = 0; i < n; ++i) { h ^= b[i]; h *= 1099511628211ull; }
  return h;
}

// every field of the phase table in use, field by field (no padding bytes)
static uint64_t table_hash(const IgemmGeom& G) {
  uint64_t h = 14695981039346656037ull;
  const int32_t head[] = {G.nphase, G.Cg, G.Ncols, G.Sd, G.Sh, G.Sw, G.J, G.Gd, G.Gh, G.Gw, G.OSd, G.OSh, G.OSw, G.Xd, G.Xh, G.Xw,
                          G.kstep_d, G.kstep_h, G.kstep_w, G.border, G.fullk};
  h = fnv(h, head, sizeof head);
  for (int i = 0; i < G.nphase; ++i) {
    const PhaseGeom& p = G.ph[i];
    const int32_t f[] = {p.Md, p.Mh, p.Mw, p.M, p.Td, p.Th, p.Tw, p.K, p.Kp, p.Od, p.Oh, p.Ow, p.Pd, p.Ph, p.Pw, p.kd0, p.kh0, p.kw0, p.row0, p.img0};
    h = fnv(h, f, sizeof f);
    h = fnv(h, &p.w_off, sizeof p.w_off);
  }
  return h;
}

static const char* const FAMILY[] = {"gemm", "patch", "pointwise", "smallk", "dot"};

// one plan as text: every field of IgemmPlan
static std::string plan_line(const IgemmPlan& P, int groups) {
  char buf[512];
  int n = std::snprintf(buf, sizeof buf, " %s %d %d %d %d/%d %d %d %d/%d %d %d %d %d %d %d", FAMILY[P.family], P.tile, P.vec, P.fast, P.ksplit,
                        P.slabs_per_split, P.positions, P.max_mblk, P.stats_rows, P.rows0, P.tapskip, P.dmajor, P.xcd_mode, P.MB, P.NB, P.ntab);
  for (int i = 0; i <= P.ntab && P.ntab > 0; ++i) n += std::snprintf(buf + n, sizeof buf - n, "%c%d", i ? ',' : '[', P.tile0[i]);
  if (P.ntab > 0) n += std::snprintf(buf + n, sizeof buf - n, "]");
  n += P.cycles < 0 ? std::snprintf(buf + n, sizeof buf - n, " %g", P.cycles) : std::snprintf(buf + n, sizeof buf - n, " %a", P.cycles);
  std::snprintf(buf + n, sizeof buf - n, " %s/%d/%016" PRIx64, P.G.border ? "border" : (groups == 2 ? "grouped" : "plain"), P.G.nphase, table_hash(P.G));
  return buf;
}

// Printed in full: the plans the configs actually get (tile 0, channels-last; the border flag where it can matter, on DGRAD) of
// the config / border-test / extra ops.  Every other variant of every op goes, as the same text, into one FNV-1a hash per op
// ("<name> rest: <count> <hash>"); `plan_check -v` prints them all in full, to see which one moved.
int main(int argc, char** argv) {
  const bool verbose = argc > 1 && std::strcmp(argv[1], "-v") == 0;
  build_corpus();
  static const int tiles[6] = {0, 1, 2, 3, 4, 6};
  size_t plans = 0;
  for (const Base& b : corpus) {
    uint64_t rest = 14695981039346656037ull; int nrest = 0;
    const bool listed = b.name.compare(0, 4, "case") != 0 && b.name.compare(0, 3, "bc.") != 0;
    for (int strided = 0; strided < 2; ++strided)
      for (int groups = 1; groups <= 2; ++groups)
        for (int border = 0; border < 2; ++border)
          for (int tile : tiles) {
            if (strided && (b.dir != GODE_FPROP || b.g.Ci > 4)) continue;              // the first-layer form reads x in place
            if (groups == 2 && (b.dir != GODE_FPROP || b.g.N % 2 != 0)) continue;      // image groups: FPROP, even batch
            gode_igemm_op op;
            std::memset(&op, 0, sizeof op);
            op.g = b.g; op.dir = b.dir; op.tile = tile; op.groups = groups; op.border = border;
            if (strided) {      // {N, D, H, W, C} element strides of a contiguous [N, C, D, H, W] tensor
              op.gs[3] = 1; op.gs[2] = b.g.Wi; op.gs[1] = (int64_t)b.g.Hi * b.g.Wi; op.gs[4] = b.g.Di * op.gs[1]; op.gs[0] = b.g.Ci * op.gs[4];
            }
            IgemmPlan P;
            const int rc = igemm_make_plan(&op, &P);
            char key[96];
            std::snprintf(key, sizeof key, "%s s%d g%d b%d t%d:", b.name.c_str(), strided, groups, border, tile);
            const std::string line = key + (rc ? " rc=" + std::to_string(rc) : plan_line(P, groups));
            ++plans;
            if (verbose || (listed && tile == 0 && !strided && (border == 0 || b.dir == GODE_DGRAD))) std::printf("%s\n", line.c_str());
            else { rest = fnv(rest, line.data(), line.size()); ++nrest; }
          }
    if (!verbose) std::printf("%s rest: %d %016" PRIx64 "\n", b.name.c_str(), nrest, rest);
  }
  std::fprintf(stderr, "%zu ops, %zu plans\n", corpus.size(), plans);
  return 0;
}
