// Stand-alone host check (own main, built with -fsanitize=address,undefined by tests/test_host_patch_cells.py) of the two
// LDS-patch planners: conv_patch_plan (gan-ode_amd/csrc/igemm_plan.h, forward) and wgrad_patch_shape as wgrad_make_plan uses it
// (gan-ode_amd/csrc/wgrad_plan.h, weight gradient).  It has no corpus of its own: it reads one op per line from stdin -- the
// rows of tests/patch_cells.py, written out by the test -- and prints that op's plan with every field, or "no" when the
// planner declines.  No GPU; the pointers of an op are made-up integers of the stated alignment (the planners read nothing
// through them).
//
// Input line (blank-separated):
//   name kind N Ci Co Di Hi Wi kd kh kw sd sh sw pd ph pw  s0 s1 s2 s3 s4  xoff yoff woff  xform scoff  stats act tile
//   kind: f (gode_igemm_op, FPROP) or w (gode_wgrad_op).  s0..s4: element strides {N, D, H, W, C} of x, all zero for
//   channels-last.  xoff / yoff / woff / scoff: floats past a 16-byte boundary of x (src), y, work, scale and shift.
//   xform: 0 none, 1 scale / shift given (w: applied to y), 2 (w only) applied to x.  stats: a statistics pointer is given (f).
//   act: the op's act.  tile: the requested tile (f).
// Output line:
//   name fprop: cell=<kernel>/<tile> variant= CB= SPI= LWC= PR= nseg= segs= iters_per_wg= wgs= Kp= lds=       (or "... no")
//   name wgrad: path=<0 patch, 1 thin, 2 gemm> nbw= RB= CB= PR= PL= LW= nseg= segs= segs_per_wg= splits= lds_bytes= reduce= vy=
//               work_floats= work_size=                                                                       (or "... no")
//   cell: what gode_igemm would launch (igemm_plan_launch: IGEMM_K_*, tile id), or rc=<code> when it refuses the op.
//   "no" for w: the plan's path is not the patch kernel.  work_size: wgrad_work_size, the value behind gode_wgrad_work_size.
// Exit status 1 with a message on stderr for a line it cannot parse or a geometry a planner rejects outright.
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include "../../gan-ode_amd/csrc/igemm_plan.h"
#include "../../gan-ode_amd/csrc/wgrad_plan.h"

static int conv_out(int i, int k, int s, int p) { return (i + 2 * p - k) / s + 1; }

static const uintptr_t FAKE_X = 0x100000, FAKE_Y = 0x200000, FAKE_WORK = 0x300000, FAKE_DW = 0x400000, FAKE_W = 0x500000,
                       FAKE_SCALE = 0x600000, FAKE_SHIFT = 0x700000, FAKE_STATS = 0x800000;
template <class T> static T* fake(uintptr_t base, int off) { return reinterpret_cast<T*>(base + 4 * (uintptr_t)off); }

int main() {
  if (wgrad_knobs().tile != 0 || wgrad_knobs().generic || !wgrad_knobs().glds) { std::fprintf(stderr, "run without GODE_WGRAD_* set\n"); return 2; }
  std::string line;
  int lines = 0;
  while (std::getline(std::cin, line)) {
    if (line.empty()) continue;
    std::istringstream in(line);
    std::string name, kind;
    int N, Ci, Co, Di, Hi, Wi, kd, kh, kw, sd, sh, sw, pd, ph, pw, xoff, yoff, woff, xform, scoff, stats, act, tile;
    int64_t s[5];
    in >> name >> kind >> N >> Ci >> Co >> Di >> Hi >> Wi >> kd >> kh >> kw >> sd >> sh >> sw >> pd >> ph >> pw >> s[0] >> s[1] >> s[2] >> s[3] >>
        s[4] >> xoff >> yoff >> woff >> xform >> scoff >> stats >> act >> tile;
    if (!in || (kind != "f" && kind != "w")) { std::fprintf(stderr, "cannot parse: %s\n", line.c_str()); return 1; }
    ++lines;
    const gode_conv_geom g = {N, Ci, Co, Di, Hi, Wi, conv_out(Di, kd, sd, pd), conv_out(Hi, kh, sh, ph), conv_out(Wi, kw, sw, pw),
                              kd, kh, kw, sd, sh, sw, pd, ph, pw};
    if (kind == "f") {
      gode_igemm_op op;
      std::memset(&op, 0, sizeof op);
      op.g = g; op.dir = GODE_FPROP; op.act = act; op.epilogue = GODE_EPI_RAW; op.tile = tile; op.groups = 1;
      op.src = fake<const float>(FAKE_X, xoff); op.wpack = fake<const float>(FAKE_W, 0); op.out = fake<float>(FAKE_Y, yoff);
      op.work = fake<float>(FAKE_WORK, woff);
      if (xform) { op.scale = fake<const float>(FAKE_SCALE, scoff); op.shift = fake<const float>(FAKE_SHIFT, scoff); }
      if (stats) op.stats = fake<float>(FAKE_STATS, 0);
      for (int i = 0; i < 5; ++i) op.gs[i] = s[i];
      IgemmPlan P;
      IgemmLaunchCell cell;
      int64_t gs[5];
      const int rc = igemm_plan_launch(&op, &P, gs, &cell);
      std::printf("%s fprop:", name.c_str());
      if (rc) std::printf(" cell=rc=%d", rc); else std::printf(" cell=%d/%d", cell.kernel, cell.tile);
      ConvPatchPlan C;
      if (!conv_patch_plan(&op, &C)) { std::printf(" no\n"); continue; }
      std::printf(" variant=%d CB=%d SPI=%d LWC=%d PR=%d nseg=%d segs=%d iters_per_wg=%d wgs=%d Kp=%d lds=%" PRId64 "\n", C.variant, C.CB, C.SPI,
                  C.LWC, C.PR, C.nseg, C.segs, C.iters_per_wg, C.wgs, C.Kp, C.lds);
    } else {
      gode_wgrad_op op;
      std::memset(&op, 0, sizeof op);
      op.g = g; op.act = act; op.xform_on_y = xform == 1; op.splits = 0;
      op.x = fake<const float>(FAKE_X, xoff); op.y = fake<const float>(FAKE_Y, yoff); op.work = fake<float>(FAKE_WORK, woff);
      op.dw = fake<float>(FAKE_DW, 0);
      if (xform) { op.scale = fake<const float>(FAKE_SCALE, scoff); op.shift = fake<const float>(FAKE_SHIFT, scoff); }
      for (int i = 0; i < 5; ++i) op.xs[i] = s[i];
      WgradPlan P;
      const int rc = wgrad_make_plan(&op, &P);
      if (rc) { std::fprintf(stderr, "%s: wgrad_make_plan returned %d\n", name.c_str(), rc); return 1; }
      std::printf("%s wgrad: path=%d", name.c_str(), P.path);
      if (P.path != WG_PATCH) { std::printf(" no\n"); continue; }
      const WgradPatch& w = P.work.patch;
      std::printf(" nbw=%d RB=%d CB=%d PR=%d PL=%d LW=%d nseg=%d segs=%d segs_per_wg=%d splits=%d lds_bytes=%d reduce=%d vy=%d work_floats=%" PRId64
                  " work_size=%" PRId64 "\n", w.nbw, w.RB, w.CB, w.PR, w.PL, w.LW, w.nseg, w.segs, w.segs_per_wg, P.work.splits, P.lds_bytes, P.reduce,
                  P.vy, P.work_floats, wgrad_work_size(&op));
    }
  }
  std::fprintf(stderr, "%d ops\n", lines);
  return 0;
}
