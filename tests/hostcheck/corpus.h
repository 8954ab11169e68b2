// The geometry corpus of the stand-alone plan checks (plan_check.cpp, wgrad_plan_check.cpp): every layer, both directions, of
// build_mnist() and build_ucf() at the configs' batch sizes, the CASES of tests/test_gpu_kernels.py and the border shapes.
// A geometry enters once, as <name>.f (GODE_FPROP) and <name>.d (GODE_DGRAD); add() skips one that is already there.
#pragma once
#include <cstdio>
#include <set>
#include <string>
#include <vector>
#include "../../gan-ode_amd/csrc/conv_geom.h"

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
