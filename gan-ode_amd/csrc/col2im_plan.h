// col2im_plan.h -- how one overlap-add op (gode_col2im_op) is launched, decided once: which of the four kernels of
// elementwise.hip, why a 2-D op left the row-group kernel (or a 3-D op the fixed one), the grid, and the row-group kernel's
// R, nq and LDS bytes.  Plain host arithmetic on the op -- no pointer is dereferenced (cols is read as an integer, for its
// alignment), no HIP.  gode_col2im dispatches on the plan and on nothing else; gode_col2im_launch_kind reports it, so a test
// that asserts a kind asserts the launch.
#pragma once
#include <stdint.h>
#include "../../include/gode.h"

enum { C2I_ROWS = 0, C2I_PIXEL = 1, C2I_3D_FIXED = 2, C2I_3D = 3 };
// `why` of a 2-D op that is not C2I_ROWS
enum { C2I_WHY_ROWLEN = 1, C2I_WHY_COLS_ALIGN = 2, C2I_WHY_LDS = 4, C2I_WHY_GRID = 8 };
// `why` of a 3-D op that is not C2I_3D_FIXED
enum { C2I_WHY_TAPS = 1, C2I_WHY_CHANNELS = 2, C2I_WHY_VOXELS = 4 };

#define C2I_LDS_MAX (48 * 1024)      // bytes of LDS the row-group kernel may ask for
#define C2I_PIXEL_BLOCKS 8192        // grid caps of the per-pixel kernels (they stride beyond)
#define C2I_3D_BLOCKS 16384

struct Col2imPlan {
  int kind, why;
  int grid;          // workgroups of 256 threads
  int R, nq;         // C2I_ROWS: input rows a row group draws on, row groups per image
  int64_t lds;       // C2I_ROWS: bytes of dynamic LDS
};

// 0 and *P, or the error gode_col2im returns before launching anything
static int col2im_plan(const gode_col2im_op* op, Col2imPlan* P) {
  if (!op || !op->cols || !op->out || op->N <= 0 || op->C <= 0 || op->C > 4 || op->kh <= 0 || op->kw <= 0 || op->sh <= 0 ||
      op->sw <= 0 || op->ph < 0 || op->pw < 0 || op->Hi <= 0 || op->Wi <= 0)
    return GODE_E_ARG;
  if (op->Ho != (op->Hi - 1) * op->sh - 2 * op->ph + op->kh || op->Wo != (op->Wi - 1) * op->sw - 2 * op->pw + op->kw) return GODE_E_SHAPE;
  if (op->epilogue != GODE_EPI_RAW && op->epilogue != GODE_EPI_TANH) return GODE_E_ARG;
  Col2imPlan p = {};
  if (op->kd > 0) {
    if (op->sd <= 0 || op->pd < 0 || op->Di <= 0 || op->Do != (op->Di - 1) * op->sd - 2 * op->pd + op->kd) return GODE_E_SHAPE;
    const int64_t voxels = (int64_t)op->N * op->Do * op->Ho * op->Wo;
    int64_t nb = (voxels + 255) / 256; if (nb > C2I_3D_BLOCKS) nb = C2I_3D_BLOCKS;
    p.grid = (int)nb;
    if (!(op->kd == 4 && op->kh == 4 && op->kw == 4 && op->sd == 1 && op->sh == 2 && op->sw == 2)) p.why |= C2I_WHY_TAPS;
    if (op->C != 3) p.why |= C2I_WHY_CHANNELS;
    if (voxels >= (1ll << 31)) p.why |= C2I_WHY_VOXELS;       // (the fixed kernel counts voxels in 32 bits)
    p.kind = p.why ? C2I_3D : C2I_3D_FIXED;
    *P = p;
    return 0;
  }
  const int KC = op->kh * op->kw * op->C;
  p.R = (op->kh + op->sh - 1) / op->sh;
  p.nq = (op->Ho - 1 + op->ph) / op->sh + 1;                    // row groups that contain an output row
  p.lds = (int64_t)p.R * op->Wi * KC * (int64_t)sizeof(float);
  if ((op->Wi * KC) % 4 != 0) p.why |= C2I_WHY_ROWLEN;
  if (((uintptr_t)op->cols % 16) != 0) p.why |= C2I_WHY_COLS_ALIGN;
  if (p.lds > C2I_LDS_MAX) p.why |= C2I_WHY_LDS;
  if ((int64_t)op->N * p.nq >= (1ll << 31)) p.why |= C2I_WHY_GRID;
  if (!p.why) {
    p.kind = C2I_ROWS;
    p.grid = op->N * p.nq;
  } else {
    p.kind = C2I_PIXEL;
    int64_t nb = ((int64_t)op->N * op->Ho * op->Wo + 255) / 256; if (nb > C2I_PIXEL_BLOCKS) nb = C2I_PIXEL_BLOCKS;
    p.grid = (int)nb;
  }
  *P = p;
  return 0;
}
