// Stand-alone host check (own main, built with -fsanitize=address,undefined by tests/test_host_igemm_plan.py) of the launch
// plans of gan-ode_amd/csrc/igemm_plan.h.  Plans every op of a fixed corpus and writes each plan as one line with every field
// of its IgemmPlan (the phase table as kind, phase count and an FNV-1a hash over all of its fields): the plans the configs
// get are printed, the other variants are hashed per op (see main).  The test compares the output with
// tests/golden/igemm_plans.txt line by line.  No randomness, no GPU.
//
// Corpus (corpus.h): every layer, both directions, of build_mnist() (generator rows 512 / 32 / 544, discriminator batch 32 / 64) and of
// build_ucf() at batch 16 and 32; the CASES of tests/test_gpu_kernels.py; the shapes of tests/test_host_border_geometry.py
// and tests/hostcheck/border_check.cpp; a few shapes added for plan fields the rest does not reach.  Each op with border 0 / 1,
// groups 1 / 2 (FPROP, even batch), tile 0 / 1 / 2 / 3 / 4 / 6, channels-last strides and (first layers: FPROP with up to 4 input
// channels) the source read in place as [N, C, D, H, W].
// Line: name s<strided> g<groups> b<border> t<tile>: family tile vec fast ksplit/slabs_per_split positions max_mblk
//       stats_rows/rows0 tapskip dmajor xcd_mode MB NB ntab[tile0...] cycles(%a, or -1) table/nphase/hash
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <string>
#include "../../gan-ode_amd/csrc/igemm_plan.h"
#include "corpus.h"

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
