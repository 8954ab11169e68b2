"""The launch cells of gode_igemm (gan-ode_amd/csrc/igemm_plan.h: igemm_launch_cell -- the function the launch dispatches on,
reported by gode_igemm_launch_cell) as plain data: one row per cell, each at the smallest shape that reaches it.  Shared by
tests/test_host_igemm_cells.py (every row's op, built over fake pointers of the stated alignment, gets the row's label; the
labels cover every cell) and tests/test_gpu_igemm_cells.py (every row runs on the GPU against a float64 reference).

A label reads "<kernel> <tile> ks<K split>:<split-K finish> xcd<grid order> <phase table>[ tapskip]" for the tiled GEMM, the
kernel's name alone for the kernels beside it, and "E_ARG" for an op gode_igemm refuses.  "ks1" with a split-K finish: a plan
that splits K served unsplit (no workspace, or src / scale off a 16-byte boundary), the finish run over that one slab."""
import collections
import ctypes as C

import gan_ode_amd._lib as L
from gan_ode_amd.engine import conv_out, make_geom

# name: (N, Ci, Co, (Di, Hi, Wi), k, s, p) in conv orientation
SHAPES = {
    "d8": (2, 32, 64, (1, 8, 8), (1, 4, 4), (1, 2, 2), (0, 1, 1)),          # FAST geometry, starved grid: every plan splits K
    "c6": (3, 6, 32, (1, 8, 8), (1, 3, 3), (1, 1, 1), (0, 1, 1)),           # DGRAD: 6 output columns
    "one": (1, 64, 64, (1, 4, 4), (1, 3, 3), (1, 1, 1), (0, 1, 1)),         # one m-block
    "nb3": (6, 32, 160, (1, 6, 6), (1, 3, 3), (1, 1, 1), (0, 1, 1)),        # three n-blocks of 64
    "d16": (16, 32, 64, (1, 16, 16), (1, 4, 4), (1, 2, 2), (0, 1, 1)),      # 8 m-blocks: contiguous runs per XCD
    "d16n64": (64, 32, 64, (1, 16, 16), (1, 4, 4), (1, 2, 2), (0, 1, 1)),   # enough rows that no requested tile splits K
    "k3s2": (8, 32, 32, (1, 7, 7), (1, 3, 3), (1, 2, 2), (0, 1, 1)),        # uneven stride phases (1, 2, 2 and 4 taps)
    "live": (2, 32, 64, (5, 6, 6), (3, 2, 2), (1, 2, 2), (0, 1, 1)),        # DGRAD with temporal taps off the ends: live-tap plan
    "live10": (10, 32, 64, (5, 6, 6), (3, 2, 2), (1, 2, 2), (0, 1, 1)),
    "live4": (5, 64, 64, (6, 8, 8), (4, 4, 4), (1, 2, 2), (0, 1, 1)),       # ... deep enough for a K split
    "smallk": (2, 1, 16, (1, 64, 64), (1, 2, 2), (1, 2, 2), (0, 0, 0)),
    "dot": (7, 32, 1, (1, 4, 4), (1, 4, 4), (1, 1, 1), (0, 0, 0)),
    "patch": (2, 3, 64, (1, 32, 32), (1, 4, 4), (1, 2, 2), (0, 1, 1)),
    "patch8": (2, 3, 32, (1, 16, 16), (1, 4, 4), (1, 2, 2), (0, 1, 1)),     # an output row of 8 positions: conv_patch.hip declines it
    "pw1": (165, 1, 32, (1, 5, 5), (1, 1, 1), (1, 1, 1), (0, 2, 2)),        # DGRAD of a cropping 1x1 convolution, one column
    "pw2": (165, 2, 32, (1, 5, 5), (1, 1, 1), (1, 1, 1), (0, 2, 2)),        # ... two columns
    "pwt": (64, 3, 16, (1, 64, 64), (1, 4, 4), (1, 2, 2), (0, 1, 1)),       # DGRAD, 3 columns, 4 phases x 4 taps, 65536 positions per phase
    "g24": (5, 24, 40, (1, 9, 9), (1, 3, 3), (1, 2, 2), (0, 1, 1)),         # channels in fours, not in whole slabs: generic float4
    "g5": (5, 5, 7, (1, 9, 9), (1, 3, 3), (1, 2, 2), (0, 1, 1)),            # odd channel counts: generic scalar
    "g24k4": (5, 24, 40, (1, 8, 8), (1, 4, 4), (1, 2, 2), (0, 1, 1)),       # the same two with k4: their input gradients gather
    "g5k4": (5, 5, 7, (1, 8, 8), (1, 4, 4), (1, 2, 2), (0, 1, 1)),          # padding too (k3 s2 p1 on 9x9 gathers none)
}

NONE, RELU, LRELU, LRELU01 = L.ACT_NONE, L.ACT_RELU, L.ACT_LRELU, L.ACT_LRELU01
F, D = L.FPROP, L.DGRAD

Row = collections.namedtuple("Row", "name shape dir label tile groups border act affine epi stats src scale out work strides")


def row(name, shape, dir, label, tile=0, groups=1, border=0, act=NONE, affine=False, tanh=False, stats=False, src=0, scale=0, out=0,
        work=0, strides="cl"):
    """src / scale / out / work: floats past a 16-byte boundary (scale: scale and shift both); work=None: a NULL workspace.
    strides: "cl" channels-last contiguous (the op's gs all zero), "pad4" / "pad1" a channels-last view whose N / D / H / W
    strides are padded to other multiples of 4 / to odd numbers."""
    return Row(name, shape, dir, label, tile, groups, border, act, affine, L.EPI_TANH if tanh else L.EPI_RAW, stats, src, scale, out,
               work, strides)


KERNELS = ["fast-dma", "fast-dma-live", "fast-xf", "fast-reg", "generic-vec4", "generic-scalar", "pointwise1", "pointwise-tap1",
           "pointwise-taps", "smallk", "dot", "patch"]
TILES = {1: "128x128", 2: "128x64", 3: "128x32", 4: "64x64", 6: "256x128"}
REDUCES = ["none", "vec", "scalar"]
TABLES = ["plain", "border", "interleaved"]
ERRORS = {-1: "E_ARG", -2: "E_SHAPE", -3: "E_KIND"}

XF_RELU, XF_LRELU, XF_LRELU01 = dict(act=RELU, affine=True), dict(act=LRELU, affine=True), dict(act=LRELU01, affine=True)
XF_ACT_ONLY, XF_AFFINE_ONLY = dict(act=LRELU, affine=False), dict(act=NONE, affine=True)
# the five operand transforms, one per tile in the tile x kernel rows below
_XF = {1: ("relu", XF_RELU), 2: ("lrelu", XF_LRELU), 3: ("lrelu01", XF_LRELU01), 4: ("act-only", XF_ACT_ONLY), 6: ("affine-only", XF_AFFINE_ONLY)}

ROWS = []
# ---- tile x kernel: every tile by request on FAST geometry (d8, live) and off it (g24, g5); every row has padding taps
for _t, _tn in TILES.items():
    _x, _xf = _XF[_t]
    ROWS += [
        row(f"dma-t{_t}", "d8", F, f"fast-dma {_tn} ks4:vec xcd0 plain", tile=_t),
        row(f"live-t{_t}", "live", D, f"fast-dma-live {_tn} ks1:none xcd{1 if _t == 4 else 0} plain tapskip", tile=_t),
        row(f"xf-t{_t}-{_x}", "d8", F, f"fast-xf {_tn} ks4:vec xcd0 plain", tile=_t, **_xf),
        row(f"vec4-t{_t}-{_x}", *(("g24", F) if _t % 2 else ("g24k4", D)), f"generic-vec4 {_tn} ks1:none xcd0 plain", tile=_t, **_xf),
        row(f"scalar-t{_t}-{_x}", *(("g5k4", D) if _t % 2 else ("g5", F)), f"generic-scalar {_tn} ks1:none xcd0 plain", tile=_t, **_xf),
    ]
ROWS += [
    # ---- the plans the planner makes by itself (tile 0), both directions, transform-free
    row("dma-fprop", "d8", F, "fast-dma 64x64 ks4:vec xcd0 plain"),
    row("dma-dgrad", "d8", D, "fast-dma 128x32 ks2:vec xcd0 plain"),
    row("vec4-fprop", "g24", F, "generic-vec4 128x64 ks1:none xcd0 plain"),
    row("vec4-dgrad", "g24", D, "generic-vec4 128x32 ks1:none xcd0 plain", stats=True),
    row("scalar-fprop", "g5", F, "generic-scalar 128x32 ks1:none xcd0 plain", stats=True),
    row("scalar-dgrad", "g5", D, "generic-scalar 128x32 ks1:none xcd0 plain"),
    # ---- the transform on the FAST register-staged kernel in the other direction (4 stride phases, K split 2)
    row("xf-dgrad-lrelu", "d8", D, "fast-xf 128x32 ks2:vec xcd0 plain", **XF_LRELU),
    row("xf-dgrad-act-only", "d8", D, "fast-xf 128x32 ks2:vec xcd0 plain", **XF_ACT_ONLY),
    # ---- transform x plan feature
    row("xf-ksplit-stats", "d8", F, "fast-xf 64x64 ks4:vec xcd0 plain", stats=True, **XF_RELU),
    row("xf-groups-stats", "d8", F, "fast-xf 64x64 ks4:vec xcd0 plain", groups=2, stats=True, **XF_LRELU),
    row("xf-border1", "d16", D, "fast-xf 64x64 ks1:none xcd0 border", tile=4, border=1, stats=True, **XF_LRELU01),
    row("xf-border2", "d16", D, "fast-xf 64x64 ks1:none xcd0 interleaved4", tile=4, border=2, stats=True, **XF_RELU),
    row("xf-border1-t6", "d16n64", D, "fast-xf 256x128 ks1:none xcd0 border", tile=6, border=1, **XF_ACT_ONLY),
    row("xf-border2-t1", "d16n64", D, "fast-xf 128x128 ks1:none xcd0 interleaved4", tile=1, border=2, **XF_AFFINE_ONLY),
    row("xf-live", "live", D, "fast-xf 128x32 ks1:none xcd0 plain tapskip", **XF_LRELU),
    row("xf-live-ksplit", "live4", D, "fast-xf 64x64 ks4:vec xcd2 plain tapskip", stats=True, **XF_RELU),
    row("xf-k3s2", "k3s2", D, "fast-xf 128x32 ks1:none xcd0 plain", **XF_RELU),
    row("xf-k3s2-fprop", "k3s2", F, "fast-xf 128x32 ks2:vec xcd0 plain", **XF_LRELU01),
    row("xf-k3s2-border", "k3s2", D, "fast-xf 64x64 ks1:none xcd0 border", tile=4, border=2, **XF_LRELU),
    row("xf-xcd3", "d16", F, "fast-xf 64x64 ks4:vec xcd3 plain", **XF_LRELU01),
    # ---- border tables without a transform, by request and (N = 64) on the tiles the border tests do not ask for
    row("border1", "d16", D, "fast-dma 64x64 ks1:none xcd0 border", tile=4, border=1),
    row("border2", "d16", D, "fast-dma 64x64 ks1:none xcd0 interleaved4", tile=4, border=2),
    row("border1-t2", "d16n64", D, "fast-dma 128x64 ks1:none xcd0 border", tile=2, border=1, stats=True),
    row("border2-t3", "d16n64", D, "fast-dma 128x32 ks1:none xcd0 interleaved4", tile=3, border=2),
    row("border-ksplit-stays-plain", "d16", D, "fast-dma 128x32 ks2:vec xcd0 plain", border=1),
    # ---- the split-K finish
    row("ksplit-scalar-ncols", "c6", D, "fast-dma 128x32 ks2:scalar xcd0 plain"),
    row("ksplit-scalar-out-off", "d8", F, "fast-dma 64x64 ks4:scalar xcd0 plain", out=1),
    row("ksplit-scalar-work-off", "d8", F, "fast-dma 64x64 ks4:scalar xcd0 plain", work=1),
    row("ksplit-vec-tanh", "d8", F, "fast-dma 64x64 ks4:vec xcd0 plain", tanh=True),
    row("ksplit-scalar-tanh", "c6", D, "fast-dma 128x32 ks2:scalar xcd0 plain", tanh=True),
    row("ksplit-vec-stats", "d8", F, "fast-dma 64x64 ks4:vec xcd0 plain", stats=True),
    row("ksplit-vec-stats-groups", "d8", F, "fast-dma 64x64 ks4:vec xcd0 plain", groups=2, stats=True),
    row("ksplit-scalar-stats", "c6", D, "fast-dma 128x32 ks2:scalar xcd0 plain", stats=True),
    row("ksplit-scalar-stats-groups", "d8", F, "fast-dma 64x64 ks4:scalar xcd0 plain", groups=2, stats=True, out=1),
    row("ksplit-live", "live4", D, "fast-dma-live 64x64 ks4:vec xcd2 plain tapskip", stats=True),
    row("ksplit-live-t1", "live4", D, "fast-dma-live 128x128 ks8:vec xcd1 plain tapskip", tile=1),
    row("ksplit-one-mblock", "one", F, "fast-dma 64x64 ks4:vec xcd0 plain"),
    row("ksplit-one-mblock-dgrad", "one", D, "fast-xf 64x64 ks4:vec xcd0 plain", **XF_RELU),
    row("ksplit-nb3", "nb3", F, "fast-dma 64x64 ks2:vec xcd0 plain", stats=True),
    # ---- grid orders at sizes where a wrong block map shows in a few tiles
    row("xcd1", "live10", D, "fast-dma-live 128x32 ks1:none xcd1 plain tapskip"),
    row("xcd2", "live10", D, "fast-dma-live 64x64 ks1:none xcd2 plain tapskip", tile=4, stats=True),
    row("xcd3", "d16", F, "fast-dma 64x64 ks4:vec xcd3 plain"),
    row("xcd3-t1", "d16", F, "fast-dma 128x128 ks4:vec xcd3 plain", tile=1),
    # ---- source strides
    row("pad4-dma", "d8", F, "fast-dma 64x64 ks4:vec xcd0 plain", strides="pad4"),
    row("pad4-xf", "d8", D, "fast-xf 128x32 ks2:vec xcd0 plain", strides="pad4", **XF_LRELU),
    row("pad4-vec4", "g24", F, "generic-vec4 128x64 ks1:none xcd0 plain", strides="pad4", **XF_RELU),
    row("pad1-fast-geometry", "d8", F, "generic-scalar 128x64 ks1:none xcd0 plain", strides="pad1"),
    row("pad1-vec4-geometry", "g24", D, "generic-scalar 128x32 ks1:none xcd0 plain", strides="pad1", **XF_LRELU01),
    # ---- alignment fall-backs of plans that do not split K: vector kernels -> generic scalar, tile kept
    row("src-off-live", "live", D, "generic-scalar 128x32 ks1:none xcd0 plain tapskip", src=1, stats=True),
    row("scale-off-fast", "k3s2", D, "generic-scalar 128x32 ks1:none xcd0 plain", scale=1, **XF_RELU),
    row("src-off-vec4", "g24", F, "generic-scalar 128x64 ks1:none xcd0 plain", src=1),
    row("scale-off-vec4", "g24", D, "generic-scalar 128x32 ks1:none xcd0 plain", scale=1, **XF_LRELU),
    row("src-off-border", "d16", D, "generic-scalar 64x64 ks1:none xcd0 border", tile=4, border=1, src=1),
    # ---- the kernels beside the tiled GEMM, each next to its unaligned twin
    row("pointwise1", "pw1", D, "pointwise1"),
    row("pointwise1-src-off", "pw1", D, "generic-scalar 128x32 ks1:none xcd0 plain", src=1),
    row("pointwise-tap1", "pw2", D, "pointwise-tap1"),
    row("pointwise-taps", "pwt", D, "pointwise-taps"),
    row("pointwise-taps-src-off", "pwt", D, "generic-scalar 128x32 ks1:none xcd0 plain", src=1),
    row("smallk", "smallk", F, "smallk"),
    row("smallk-out-off", "smallk", F, "generic-scalar 128x32 ks1:none xcd0 plain", out=1),
    row("dot", "dot", F, "dot"),
    row("dot-src-off", "dot", F, "generic-scalar 128x32 ks1:none xcd0 plain", src=1),
    row("patch", "patch", F, "patch"),
    row("patch-src-off", "patch", F, "patch", src=1),            # (the LDS-patch kernel gathers scalars: it stays)
    row("patch-declined", "patch8", F, "generic-scalar 128x32 ks1:none xcd0 plain"),
    # ---- a plan that splits K without its workspace, or with src / scale off a 16-byte boundary: served unsplit by the generic
    # kernel, the split-K finish run over that one slab (work, or out in place) so that the statistics keep the plan's layout
    row("unsplit-work-null", "d8", F, "generic-vec4 64x64 ks1:vec xcd0 plain", work=None),
    row("unsplit-src-off", "d8", F, "generic-scalar 64x64 ks1:vec xcd0 plain", src=1),
    row("unsplit-scale-off", "d8", F, "generic-scalar 64x64 ks1:vec xcd0 plain", scale=1, **XF_RELU),
    row("unsplit-work-null-stats-groups", "d8", F, "generic-vec4 64x64 ks1:vec xcd0 plain", work=None, groups=2, stats=True, **XF_LRELU),
    row("unsplit-work-null-tanh-out-off", "d8", D, "generic-vec4 128x32 ks1:scalar xcd0 plain", work=None, tanh=True, out=1),
    row("unsplit-src-off-stats", "c6", D, "generic-scalar 128x32 ks1:scalar xcd0 plain", src=1, stats=True),
    row("unsplit-src-off-live", "live4", D, "generic-scalar 64x64 ks1:vec xcd0 plain tapskip", src=1, stats=True),
]
BY_NAME = {r.name: r for r in ROWS}
assert len(BY_NAME) == len(ROWS)


def gathered_dims(r):
    """[N, D, H, W, C] of the operand the op gathers."""
    N, Ci, Co, xi, k, s, p = SHAPES[r.shape]
    yo = tuple(conv_out(xi[a], k[a], s[a], p[a]) for a in range(3))
    return (N, *xi, Ci) if r.dir == F else (N, *yo, Co)


def out_dims(r):
    N, Ci, Co, xi, k, s, p = SHAPES[r.shape]
    yo = tuple(conv_out(xi[a], k[a], s[a], p[a]) for a in range(3))
    return (N, *yo, Co) if r.dir == F else (N, *xi, Ci)


def gather_strides(r):
    """Element strides {N, D, H, W, C} of the row's source view, or None for channels-last contiguous; and its span in floats."""
    n, d, h, w, c = gathered_dims(r)
    if r.strides == "cl":
        return None, n * d * h * w * c
    pad = {"pad4": (4, 8, 4, 12), "pad1": (1, 3, 1, 5)}[r.strides]
    sw = c + pad[0]
    sh = w * sw + pad[1]
    sd = h * sh + pad[2]
    sn = d * sd + pad[3]
    gs = (sn, sd, sh, sw, 1)
    return gs, 1 + (n - 1) * sn + (d - 1) * sd + (h - 1) * sh + (w - 1) * sw + (c - 1)


def geom(r):
    N, Ci, Co, xi, k, s, p = SHAPES[r.shape]
    return make_geom(N, Ci, Co, xi, tuple(conv_out(xi[a], k[a], s[a], p[a]) for a in range(3)), k, s, p)


def make_op(r, src, wpack, out, scale=None, shift=None, stats=None, work=None, border=None):
    """The row's op over the given addresses (integers; nothing here dereferences them)."""
    xf = r.affine
    op = L.IgemmOp(g=geom(r), dir=r.dir, act=r.act, epilogue=r.epi, tile=r.tile, src=src, wpack=wpack, out=out,
                   scale=scale if xf else None, shift=shift if xf else None, stats=stats if r.stats else None, work=work,
                   groups=r.groups, border=r.border if border is None else border)
    gs, _ = gather_strides(r)
    if gs is not None:
        for i in range(5):
            op.gs[i] = gs[i]
    return op


def fake_op(r):
    """The row's op over fake non-null pointers of the row's alignment."""
    base = 1 << 20
    return make_op(r, src=base + 4 * r.src, wpack=2 * base, out=3 * base + 4 * r.out, scale=4 * base + 4 * r.scale,
                   shift=5 * base + 4 * r.scale, stats=6 * base, work=None if r.work is None else 7 * base + 4 * r.work)


def cell_label(op):
    """The label of the op's launch cell, from gode_igemm_launch_cell."""
    cell = (C.c_int32 * 8)()
    rc = L.lib().gode_igemm_launch_cell(C.byref(op), cell)
    if rc != 0:
        return ERRORS[rc]
    kernel, tile, reduce, ksplit, xcd, table, interleave, tapskip = cell
    if kernel < 0:
        return "nothing"
    if tile == 0:
        return KERNELS[kernel]
    tab = TABLES[table] + (str(interleave) if table == 2 else "")
    return f"{KERNELS[kernel]} {TILES[tile]} ks{ksplit}:{REDUCES[reduce]} xcd{xcd} {tab}" + (" tapskip" if tapskip else "")


def parse(label):
    """A label's fields: kernel, and for the tiled GEMM tile, ksplit, reduce, xcd, table, tapskip."""
    f = label.split(" ")
    if len(f) == 1:
        return dict(kernel=f[0], tile=None)
    ks, red = f[2][2:].split(":")
    return dict(kernel=f[0], tile=f[1], ksplit=int(ks), reduce=red, xcd=int(f[3][3:]), table=f[4].rstrip("0123456789"),
                tapskip=f[-1] == "tapskip")


def transform(r):
    """Which of the five operand transforms the row fuses into the load, or None."""
    if r.affine:
        return {NONE: "affine-only", RELU: "relu", LRELU: "lrelu", LRELU01: "lrelu01"}[r.act]
    return None if r.act == NONE else "act-only"


def has_padding_taps(r):
    """Whether some tap of some output position gathers outside the tensor (where zero padding must follow the transform)."""
    N, Ci, Co, xi, k, s, p = SHAPES[r.shape]
    for a in range(3):
        yo = conv_out(xi[a], k[a], s[a], p[a])
        if r.dir == F:
            if any(not 0 <= o * s[a] - p[a] + j < xi[a] for o in range(yo) for j in range(k[a])):
                return True
        elif any((i + p[a] - j) % s[a] == 0 and not 0 <= (i + p[a] - j) // s[a] < yo for i in range(xi[a]) for j in range(k[a])):
            return True
    return False
