// Stand-alone host check (own main, built with -fsanitize=address,undefined by tests/test_host_wgrad_plan.py) of the launch
// plans of gan-ode_amd/csrc/wgrad_plan.h.  Plans every op of a fixed corpus and writes each plan as one line with every field
// of its WgradPlan; the test compares the output with tests/golden/wgrad_plans.txt line by line.  No randomness, no GPU; the
// pointers of an op are made-up integers (the plan reads only their alignment).
//
// Corpus: the geometries of corpus.h (config layers, the CASES of tests/test_gpu_kernels.py, the border shapes), the 1x1x1
// products of fcgan.py at batch 1 / 64 / 128, the layers of dcgan.py at batch 64, the three convolutions of a GResBlock(64, 32)
// on 8x8 at N = 4, and the shapes of tests/test_gpu_wgrad_paths.py.  Each geometry with splits 0 / 3, the transform on x or
// on y, with and without a scale, act NONE / RELU, channels-last strides and (Ci <= 4) x read in place as [N, C, D, H, W], and
// x, y and work each 16-byte aligned and 4 bytes off.  The plan reads neither accumulate nor co_perm.  Then, channels-last,
// aligned and without a transform, under each tuning knob (wgrad_make_plan_with): tile 2 / 3 / 4, generic, no LDS-DMA.
// Line: name sp<splits> xf<xform_on_y> sc<scale> a<act> st<strided> x<off> y<off> w<off>  (or: name k:<knob>):
//       rule/split_tile/splits path tile family vx vy glds M taps Kt chunk/chunk_thin grid block lds xs x_bytes reduce/blocks
//       work_floats patch[RB,CB,PR,PL,LW,nseg,segs,segs_per_wg,nbw]
//
// Checked here, for every plan (a failure is a message on stderr and exit status 1, whatever the golden says):
//   the workspace part (WgradPlan.work) of an op (geometry, splits, scale, xform_on_y) is the same for every act, stride
//   form and pointer alignment and is what wgrad_work_size / wgrad_auto_splits return; splits * chunk >= M; grid z == splits
//   on the GEMM path; the patch kernel's LDS <= 64 KB; the plan's kernel is one wgrad.hip has a case for (WGRAD_KERNEL_KEYS).
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <string>
#include "../../gan-ode_amd/csrc/wgrad_plan.h"
#include "corpus.h"

static uint64_t fnv(uint64_t h, const void* p, size_t n) {
  const unsigned char* b = static_cast<const unsigned char*>(p);
  for (size_t i = 0; i < n; ++i) { h ^= b[i]; h *= 1099511628211ull; }
  return h;
}

static void add_wgrad_shapes() {
  static const int fc[8][2] = {{100, 256}, {256, 512}, {512, 1024}, {1024, 784}, {784, 1024}, {1024, 512}, {512, 256}, {256, 1}};
  static const int fc_batch[3] = {1, 64, 128};
  for (int b : fc_batch)
    for (const auto& l : fc) add("fc" + std::to_string(b) + "." + std::to_string(l[0]) + "x" + std::to_string(l[1]), b, l[0], l[1], 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0);
  // dcgan.py at batch 64 (nz 128, ngf = ndf = 64, nc 3): generator, then discriminator
  add("dcgan.G.L0", 64, 128, 8192, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0);
  for (int l = 0, c = 512, hw = 4; l < 3; ++l, c /= 2, hw *= 2) add("dcgan.G.L" + std::to_string(l + 1), 64, c / 2, c, 1, 2 * hw, 2 * hw, 1, 4, 4, 1, 2, 2, 0, 1, 1);
  add("dcgan.G.L4", 64, 64, 3, 1, 32, 32, 1, 3, 3, 1, 1, 1, 0, 1, 1);
  static const int dch[8] = {3, 64, 64, 128, 128, 256, 256, 512};
  for (int l = 0, hw = 32; l < 7; ++l) {
    const int k = l % 2 ? 4 : 3, s = l % 2 ? 2 : 1;
    add("dcgan.D.L" + std::to_string(l), 64, dch[l], dch[l + 1], 1, hw, hw, 1, k, k, 1, s, s, 0, 1, 1);
    hw = conv_out(hw, k, s, 1);
  }
  add("dcgan.D.L7", 64, 512, 1, 1, 4, 4, 1, 4, 4, 1, 1, 1, 0, 0, 0);
  // GResBlock(64, 32) on 8x8 at N = 4: conv0, conv1, the 1x1 shortcut
  add("gres.conv0", 4, 64, 32, 1, 8, 8, 1, 3, 3, 1, 1, 1, 0, 1, 1);
  add("gres.conv1", 4, 32, 32, 1, 8, 8, 1, 3, 3, 1, 1, 1, 0, 1, 1);
  add("gres.sc", 4, 64, 32, 1, 8, 8, 1, 1, 1, 1, 1, 1, 0, 0, 0);
  // tests/test_gpu_wgrad_paths.py: the floors of the 8-wave tiles, a thin op, a patch op whose 16 slabs of 12288 sums take the
  // small reduce, 27 weight columns (scalar reduce), and small ops of the 64- and 128-row tiles
  add("paths.t256x128", 8, 64, 256, 1, 64, 64, 1, 4, 4, 1, 2, 2, 0, 1, 1);
  add("paths.t128x256", 16, 64, 128, 1, 64, 64, 1, 4, 4, 1, 2, 2, 0, 1, 1);
  add("paths.thin", 2, 1, 8, 1, 28, 28, 1, 4, 4, 1, 2, 2, 0, 1, 1);
  add("paths.patch", 2, 3, 64, 4, 32, 32, 4, 4, 4, 1, 2, 2, 0, 1, 1);
  add("paths.kt27", 2, 3, 16, 1, 8, 8, 1, 3, 3, 1, 1, 1, 0, 1, 1);
  add("paths.t64", 4, 8, 64, 1, 8, 8, 1, 3, 3, 1, 1, 1, 0, 1, 1);
  add("paths.t128", 4, 8, 128, 1, 8, 8, 1, 3, 3, 1, 1, 1, 0, 1, 1);
}

static const char* const PATH[] = {"patch", "thin", "gemm"};
static const char* const FAMILY[] = {"-", "fast", "generic"};
static const char* const REDUCE[] = {"small", "vec4", "scalar"};

// one plan as text: every field of WgradPlan
static std::string plan_line(const WgradPlan& P) {
  char buf[512];
  const WgradPatch& w = P.work.patch;
  std::snprintf(buf, sizeof buf, " %s/%d/%d %s %d %s %d %d %d %d %d %d %d/%d %d,%d,%d %d %d %d,%d,%d,%d,%d %u %s/%d %" PRId64 " [%d,%d,%d,%d,%d,%d,%d,%d,%d]",
                PATH[P.work.rule], P.work.split_tile, P.work.splits, PATH[P.path], P.tile, FAMILY[P.family + 1], P.vx, P.vy, P.glds, P.M, P.taps,
                P.Kt, P.chunk, P.chunk_thin, P.grid_x, P.grid_y, P.grid_z, P.block, P.lds_bytes, P.xs[0], P.xs[1], P.xs[2], P.xs[3], P.xs[4],
                P.x_bytes, REDUCE[P.reduce], P.reduce_blocks, P.work_floats, w.RB, w.CB, w.PR, w.PL, w.LW, w.nseg, w.segs, w.segs_per_wg, w.nbw);
  return buf;
}

static int failures = 0;
static void fail(const std::string& key, const char* what) {
  std::fprintf(stderr, "FAILED %s %s\n", key.c_str(), what);
  ++failures;
}

static void check_plan(const std::string& key, const gode_wgrad_op& op, const WgradPlan& P) {
  if ((int64_t)P.work.splits * P.chunk < P.M) fail(key, "splits * chunk < M");
  if (P.path == WG_GEMM && P.grid_z != P.work.splits) fail(key, "grid z != splits on the GEMM path");
  if (P.path == WG_PATCH && P.lds_bytes > 64 * 1024) fail(key, "patch LDS > 64 KB");
  const uint32_t kk = wgrad_kernel_key(P, op.g.Co);
  bool known = false;
  for (uint32_t k : WGRAD_KERNEL_KEYS) known = known || k == kk;
  if (!known) fail(key, "no kernel case for this plan");
}

static const uintptr_t FAKE_X = 0x100000, FAKE_Y = 0x200000, FAKE_WORK = 0x300000, FAKE_DW = 0x400000;
static float fake_scale;

// Printed in full: what the configs get (splits 0, channels-last, aligned; no transform, BN+ReLU on x, BN+ReLU on y), the same
// op with x, y or work alone 4 bytes off, and a knob's plan where it differs from the plain one -- of every geometry that is
// not a kernel-test ("case") or border ("bc.") shape.  Every other plan goes, as the same text, into one FNV-1a hash per
// geometry ("<name> rest: <count> <hash>"); `wgrad_plan_check -v` prints them all in full, to see which one moved.
int main(int argc, char** argv) {
  const bool verbose = argc > 1 && std::strcmp(argv[1], "-v") == 0;
  build_corpus();
  add_wgrad_shapes();
  static const struct { const char* name; WgradKnobs k; } knobs[5] = {
      {"tile2", {2, false, true}}, {"tile3", {3, false, true}}, {"tile4", {4, false, true}}, {"generic", {0, true, true}}, {"noglds", {0, false, false}}};
  if (wgrad_knobs().tile != 0 || wgrad_knobs().generic || !wgrad_knobs().glds) { std::fprintf(stderr, "run without GODE_WGRAD_* set\n"); return 2; }
  size_t plans = 0, geoms = 0;
  for (const Base& b : corpus) {
    if (b.dir != GODE_FPROP) continue;
    ++geoms;
    const std::string name = b.name.substr(0, b.name.size() - 2);
    const bool listed = name.compare(0, 4, "case") != 0 && name.compare(0, 3, "bc.") != 0;
    uint64_t rest = 14695981039346656037ull; int nrest = 0;
    std::string plain_line;
    auto emit = [&](const std::string& line, bool full) {
      ++plans;
      if (verbose || (listed && full)) std::printf("%s\n", line.c_str());
      else { rest = fnv(rest, line.data(), line.size()); ++nrest; }
    };
    gode_wgrad_op op;
    for (int splits : {0, 3})
      for (int xf = 0; xf < 2; ++xf)
        for (int sc = 0; sc < 2; ++sc) {
          bool have_work = false; WgradWork first = {};
          for (int act : {(int)GODE_ACT_NONE, (int)GODE_ACT_RELU})
            for (int strided = 0; strided < (b.g.Ci <= 4 ? 2 : 1); ++strided)
              for (int xo = 0; xo < 2; ++xo)
                for (int yo = 0; yo < 2; ++yo)
                  for (int wo = 0; wo < 2; ++wo) {
                    std::memset(&op, 0, sizeof op);
                    op.g = b.g; op.act = act; op.xform_on_y = xf; op.splits = splits;
                    op.x = reinterpret_cast<const float*>(FAKE_X + 4 * xo); op.y = reinterpret_cast<const float*>(FAKE_Y + 4 * yo);
                    op.work = reinterpret_cast<float*>(FAKE_WORK + 4 * wo); op.dw = reinterpret_cast<float*>(FAKE_DW);
                    if (sc) { op.scale = &fake_scale; op.shift = &fake_scale; }
                    if (strided) {      // {N, D, H, W, C} element strides of a contiguous [N, C, D, H, W] tensor
                      op.xs[3] = 1; op.xs[2] = b.g.Wi; op.xs[1] = (int64_t)b.g.Hi * b.g.Wi; op.xs[4] = b.g.Di * op.xs[1]; op.xs[0] = b.g.Ci * op.xs[4];
                    }
                    char key[128];
                    std::snprintf(key, sizeof key, "%s sp%d xf%d sc%d a%d st%d x%d y%d w%d:", name.c_str(), splits, xf, sc, act, strided, 4 * xo, 4 * yo, 4 * wo);
                    WgradPlan P;
                    const int rc = wgrad_make_plan(&op, &P);
                    const std::string line = key + (rc ? " rc=" + std::to_string(rc) : plan_line(P));
                    const bool config = splits == 0 && !strided && ((!xf && !sc && act == GODE_ACT_NONE) || (sc && act == GODE_ACT_RELU));
                    const bool plain_op = splits == 0 && !strided && !xf && !sc && act == GODE_ACT_NONE;
                    emit(line, (config && xo + yo + wo == 0) || (plain_op && xo + yo + wo == 1));
                    if (plain_op && xo + yo + wo == 0) plain_line = line.substr(std::strlen(key));
                    if (rc) continue;
                    check_plan(key, op, P);
                    if (!have_work) { first = P.work; have_work = true; }
                    if (std::memcmp(&first, &P.work, sizeof first) != 0) fail(key, "the workspace part moved with act, strides or a pointer");
                    if (P.work_floats != wgrad_work_size(&op)) fail(key, "work_floats != wgrad_work_size");
                    if (splits == 0 && P.work.rule == WG_GEMM && P.work.splits != wgrad_auto_splits(op.g)) fail(key, "splits != wgrad_auto_splits");
                  }
        }
    for (const auto& kn : knobs) {
      std::memset(&op, 0, sizeof op);
      op.g = b.g; op.act = GODE_ACT_NONE;
      op.x = reinterpret_cast<const float*>(FAKE_X); op.y = reinterpret_cast<const float*>(FAKE_Y);
      op.work = reinterpret_cast<float*>(FAKE_WORK); op.dw = reinterpret_cast<float*>(FAKE_DW);
      WgradPlan P;
      const int rc = wgrad_make_plan_with(&op, kn.k, &P);
      const std::string key = name + " k:" + kn.name + ":", body = rc ? " rc=" + std::to_string(rc) : plan_line(P);
      emit(key + body, body != plain_line);
      if (!rc) check_plan(key, op, P);
    }
    if (!verbose) std::printf("%s rest: %d %016" PRIx64 "\n", name.c_str(), nrest, rest);
  }
  std::fprintf(stderr, "%zu geometries, %zu plans, %d failed checks\n", geoms, plans, failures);
  return failures ? 1 : 0;
}
