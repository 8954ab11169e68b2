// Stand-alone host check (own main, built with -fsanitize=address,undefined by tests/test_host_border_geometry.py) of the
// border-split DGRAD phase table in gan-ode_amd/csrc/conv_geom.h against the plain table: the sub-phases tile the output
// exactly once, gather the same (output position, canonical tap, input position) triples as the plain table's in-range
// taps and nothing out of range, keep the plain tap order per output position, and their packed panels hold the same
// canonical weights as the plain panels.  Prints one line per shape; exit status 0 only if every assertion held.
#include <algorithm>
#include <array>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <vector>
#include "../../gan-ode_amd/csrc/conv_geom.h"

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { ++failures; std::printf("  FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

struct Shape {
  const char* name;
  int Di, Hi, Wi;      // the transposed convolution's OUTPUT (the conv's x)
  int Do, Ho, Wo;      // its input (the conv's y, the gathered tensor)
  int kd, kh, kw, sd, sh, sw, pd, ph, pw;
  int expect_border, expect_phases;    // expect_phases < 0: not checked
};

typedef std::array<int, 9> Triple;   // out (d,h,w), canonical tap (kd,kh,kw), gathered (d,h,w)

// every (position, tap) of a table for image 0; taps out of range go to `dead`
static void walk(const IgemmGeom& G, std::vector<Triple>* live, int* dead, std::map<std::array<int, 3>, std::vector<std::array<int, 3>>>* order,
                 std::map<std::array<int, 3>, int>* cover) {
  *dead = 0;
  for (int p = 0; p < G.nphase; ++p) {
    const PhaseGeom& P = G.ph[p];
    for (int qd = 0; qd < P.Md; ++qd)
      for (int qh = 0; qh < P.Mh; ++qh)
        for (int qw = 0; qw < P.Mw; ++qw) {
          const std::array<int, 3> o = {qd * G.OSd + P.Pd, qh * G.OSh + P.Ph, qw * G.OSw + P.Pw};
          ++(*cover)[o];
          (*order)[o];
          for (int jd = 0; jd < P.Td; ++jd)
            for (int jh = 0; jh < P.Th; ++jh)
              for (int jw = 0; jw < P.Tw; ++jw) {
                const int id = gode_gather_coord(qd, G.Sd, P.Od, G.J, jd), ih = gode_gather_coord(qh, G.Sh, P.Oh, G.J, jh),
                          iw = gode_gather_coord(qw, G.Sw, P.Ow, G.J, jw);
                const std::array<int, 3> tap = {P.kd0 + jd * G.kstep_d, P.kh0 + jh * G.kstep_h, P.kw0 + jw * G.kstep_w};
                if (id < 0 || id >= G.Gd || ih < 0 || ih >= G.Gh || iw < 0 || iw >= G.Gw) { ++*dead; continue; }
                live->push_back(Triple{o[0], o[1], o[2], tap[0], tap[1], tap[2], id, ih, iw});
                (*order)[o].push_back(tap);
              }
        }
  }
}

static void check_shape(const Shape& s) {
  gode_conv_geom g;
  g.N = 2; g.Ci = 3; g.Co = 8;
  g.Di = s.Di; g.Hi = s.Hi; g.Wi = s.Wi; g.Do = s.Do; g.Ho = s.Ho; g.Wo = s.Wo;
  g.kd = s.kd; g.kh = s.kh; g.kw = s.kw; g.sd = s.sd; g.sh = s.sh; g.sw = s.sw; g.pd = s.pd; g.ph = s.ph; g.pw = s.pw;
  IgemmGeom P, B;
  const int rp = gode_build_igemm_geom(g, GODE_DGRAD, &P), rb = gode_build_igemm_geom_border(g, GODE_DGRAD, &B);
  CHECK(rp == 0 && rb == 0, "%s: builders returned %d / %d", s.name, rp, rb);
  if (rp || rb) return;
  std::printf("%-28s plain %2d phases, border=%d with %2d phases, pack %lld -> %lld floats\n", s.name, P.nphase, B.border, B.nphase,
              (long long)gode_pack_floats(P), (long long)gode_pack_floats(B));
  CHECK(B.border == s.expect_border, "%s: border = %d, expected %d", s.name, B.border, s.expect_border);
  if (s.expect_phases >= 0) CHECK(B.nphase == s.expect_phases, "%s: %d sub-phases, expected %d", s.name, B.nphase, s.expect_phases);
  CHECK(B.nphase <= GODE_MAX_PHASES, "%s: too many sub-phases", s.name);

  std::vector<Triple> lp, lb;
  int dp = 0, db = 0;
  std::map<std::array<int, 3>, std::vector<std::array<int, 3>>> op, ob;
  std::map<std::array<int, 3>, int> cp, cb;
  walk(P, &lp, &dp, &op, &cp);
  walk(B, &lb, &db, &ob, &cb);
  // every output position in exactly one (sub-)phase
  CHECK((int)cb.size() == s.Di * s.Hi * s.Wi, "%s: %zu of %d output positions covered", s.name, cb.size(), s.Di * s.Hi * s.Wi);
  for (const auto& kv : cb) {
    CHECK(kv.second == 1, "%s: output (%d,%d,%d) lies in %d sub-phases", s.name, kv.first[0], kv.first[1], kv.first[2], kv.second);
    CHECK(kv.first[0] >= 0 && kv.first[0] < s.Di && kv.first[1] >= 0 && kv.first[1] < s.Hi && kv.first[2] >= 0 && kv.first[2] < s.Wi,
          "%s: output position out of range", s.name);
  }
  CHECK(cp.size() == cb.size(), "%s: plain covers %zu positions, border %zu", s.name, cp.size(), cb.size());
  // no sub-phase gathers out of range (a fallen-back table is the plain one and may)
  if (B.border) CHECK(db == 0, "%s: %d taps of the border-split table gather out of range", s.name, db);
  else CHECK(db == dp, "%s: fallback differs from the plain table", s.name);
  // the same multiset of live triples
  std::sort(lp.begin(), lp.end());
  std::sort(lb.begin(), lb.end());
  CHECK(lp == lb, "%s: live (position, tap, input) triples differ (%zu plain, %zu border)", s.name, lp.size(), lb.size());
  // per output position: the plain tap order restricted to the live taps
  CHECK(op == ob, "%s: the tap order of some output position differs", s.name);

  int64_t plain_floats = gode_pack_floats(P), prev_K = 1 << 30;
  std::vector<std::pair<int64_t, int64_t>> own;
  for (int i = 0; i < B.nphase; ++i) {
    const PhaseGeom& S = B.ph[i];
    CHECK(S.M > 0 && S.K > 0, "%s: empty sub-phase %d", s.name, i);
    CHECK(S.M == g.N * S.Md * S.Mh * S.Mw && S.K == S.Td * S.Th * S.Tw * B.Cg, "%s: sub-phase %d extents", s.name, i);
    if (B.border) CHECK(S.K <= prev_K, "%s: sub-phases are not sorted by descending K", s.name);
    prev_K = S.K;
    // the plain phase of the same stride residue
    int par = -1;
    for (int p = 0; p < P.nphase; ++p)
      if (P.ph[p].Pd == S.Pd % B.OSd && P.ph[p].Ph == S.Ph % B.OSh && P.ph[p].Pw == S.Pw % B.OSw) par = p;
    CHECK(par >= 0, "%s: sub-phase %d has no parent", s.name, i);
    if (par < 0) continue;
    const PhaseGeom& Q = P.ph[par];
    const int64_t end = S.w_off + (int64_t)B.Ncols * S.Kp;
    CHECK(S.w_off >= 0 && end <= gode_pack_floats(B), "%s: panel %d outside the pack", s.name, i);
    if (S.w_off >= plain_floats) own.push_back({S.w_off, end});
    else CHECK(S.w_off == Q.w_off && S.K == Q.K && S.Kp == Q.Kp, "%s: sub-phase %d shares a plain panel it does not equal", s.name, i);
    for (int n = 0; n < B.Ncols; ++n)
      for (int k = 0; k < S.Kp; ++k) {
        const int64_t src = gode_pack_source(g, GODE_DGRAD, B, S, n, k, nullptr);
        if (k >= S.K) { CHECK(src == -1, "%s: padding column maps to a weight", s.name); continue; }
        const int tap = k / B.Cg, c = k - tap * B.Cg;
        const int jw = tap % S.Tw, jh = (tap / S.Tw) % S.Th, jd = tap / (S.Tw * S.Th);
        const int kd = S.kd0 + jd * B.kstep_d, kh = S.kh0 + jh * B.kstep_h, kw = S.kw0 + jw * B.kstep_w;
        // the plain panel's element for that (tap, channel)
        const int pd_ = (kd - Q.kd0) / P.kstep_d, ph_ = (kh - Q.kh0) / P.kstep_h, pw_ = (kw - Q.kw0) / P.kstep_w;
        CHECK((kd - Q.kd0) % P.kstep_d == 0 && (kh - Q.kh0) % P.kstep_h == 0 && (kw - Q.kw0) % P.kstep_w == 0 && pd_ >= 0 && pd_ < Q.Td &&
              ph_ >= 0 && ph_ < Q.Th && pw_ >= 0 && pw_ < Q.Tw, "%s: sub-phase %d tap (%d,%d,%d) is no tap of its parent", s.name, i, kd, kh, kw);
        const int kq = ((pd_ * Q.Th + ph_) * Q.Tw + pw_) * P.Cg + c;
        const int64_t want = gode_pack_source(g, GODE_DGRAD, P, Q, n, kq, nullptr);
        CHECK(src == want && src >= 0 && src == gode_w_index(g, c, n, kd, kh, kw), "%s: sub-phase %d panel (%d,%d) -> %lld, plain -> %lld",
              s.name, i, n, k, (long long)src, (long long)want);
      }
  }
  std::sort(own.begin(), own.end());
  for (size_t i = 1; i < own.size(); ++i) CHECK(own[i - 1].second <= own[i].first, "%s: panels overlap", s.name);
}

int main() {
  std::vector<Shape> shapes;
  static const int hs[6] = {1, 2, 3, 4, 8, 16};
  static char names[6][32];
  for (int i = 0; i < 6; ++i) {      // ConvTranspose2d k4 s2 p1, H x H -> 2H x 2H
    const int h = hs[i];
    std::snprintf(names[i], sizeof names[i], "k4s2p1 %dx%d", h, h);
    shapes.push_back(Shape{names[i], 1, 2 * h, 2 * h, 1, h, h, 1, 4, 4, 1, 2, 2, 0, 1, 1, 1, h == 1 ? 4 : 16});
  }
  shapes.push_back(Shape{"k4s2p1 2x5", 1, 4, 10, 1, 2, 5, 1, 4, 4, 1, 2, 2, 0, 1, 1, 1, 16});
  // k3 s2 p1 without output padding: 4x4 -> 7x7 (phases of 1 and 2 taps per dim, unequal extents)
  shapes.push_back(Shape{"k3s2p1 4x4 -> 7x7", 1, 7, 7, 1, 4, 4, 1, 3, 3, 1, 2, 2, 0, 1, 1, 1, -1});
  // (and with output padding 1, 4x4 -> 8x8: the last row / column of the odd phase loses a tap)
  shapes.push_back(Shape{"k3s2p1 4x4 -> 8x8", 1, 8, 8, 1, 4, 4, 1, 3, 3, 1, 2, 2, 0, 1, 1, 1, 9});
  // 3-D, stride (1,2,2): one temporal tap, 3 planes
  shapes.push_back(Shape{"3-D k(1,4,4) s(1,2,2) 3x4x4", 3, 8, 8, 3, 4, 4, 1, 4, 4, 1, 2, 2, 0, 1, 1, 1, 16});
  // 3-D with temporal taps that run off both ends, 1x1 planes: 2 runs in depth x 4 phases
  shapes.push_back(Shape{"3-D k(3,4,4) s(1,2,2) 2x1x1", 2, 2, 2, 2, 1, 1, 3, 4, 4, 1, 2, 2, 1, 1, 1, 1, 8});
  // the same on 2x2 planes: 2 x 2 x 2 runs x 4 phases = 32 sub-phases -> falls back to the plain table
  shapes.push_back(Shape{"3-D k(3,4,4) 2x2x2 fallback", 2, 4, 4, 2, 2, 2, 3, 4, 4, 1, 2, 2, 1, 1, 1, 0, 4});
  for (const Shape& s : shapes) check_shape(s);
  // FPROP and fullk never split
  {
    gode_conv_geom g = {2, 3, 8, 1, 8, 8, 1, 4, 4, 1, 4, 4, 1, 2, 2, 0, 1, 1};
    IgemmGeom B;
    CHECK(gode_build_igemm_geom_border(g, GODE_FPROP, &B) == 0 && B.border == 0 && B.nphase == 1, "FPROP must stay plain");
    gode_conv_geom f = {2, 3, 8, 1, 4, 4, 1, 1, 1, 1, 4, 4, 1, 1, 1, 0, 0, 0};
    CHECK(gode_build_igemm_geom_border(f, GODE_DGRAD, &B) == 0 && B.border == 0 && B.fullk == 1, "fullk must stay plain");
  }
  std::printf("%s (%d failures)\n", failures ? "FAILED" : "OK", failures);
  return failures ? 1 : 0;
}
