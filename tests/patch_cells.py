"""The launch cells of the two LDS-patch kernels as plain data: conv_patch_fprop_kernel<KD, KH, KC2> (gan-ode_amd/csrc/conv_patch.hip,
planned by conv_patch_plan in igemm_plan.h) and wgrad_patch_kernel<NBW, CO> (gan-ode_amd/csrc/wgrad.hip, planned by wgrad_patch_shape
in wgrad_plan.h).  One shape per instantiation and launch form, each at the smallest size that gets the stated plan, and the
cells that run them: a shape on one kernel in one x layout with its operands aligned or one float off.  Shared by
tests/test_host_patch_cells.py (every shape gets exactly the plan written here -- from a stand-alone sanitized build of the two
planners -- and the shapes together reach every instantiation and every feature listed there) and
tests/test_gpu_patch_cells.py (every cell runs on the GPU against a float64 reference)."""
import collections

from gan_ode_amd.engine import conv_out

# name: (N, Ci, Co, (Di, Hi, Wi), k, s, p)
SHAPES = {
    # ---- forward, and where the name says so the weight gradient of the same shape
    "f3d3_32": (1, 3, 32, (5, 5, 19), (4, 4, 4), (1, 1, 1), (1, 1, 1)),
    "f3d3_64": (2, 3, 64, (5, 8, 34), (4, 4, 4), (1, 2, 2), (1, 1, 1)),
    "f3d3_128": (1, 3, 128, (4, 6, 70), (4, 4, 4), (1, 1, 2), (0, 0, 1)),
    "f2d3_32": (3, 3, 32, (1, 9, 20), (1, 4, 4), (1, 1, 1), (0, 1, 1)),
    "f2d3_64": (2, 3, 64, (1, 32, 32), (1, 4, 4), (1, 2, 2), (0, 1, 1)),        # the "patch" shape of tests/igemm_cells.py
    "f2d3_128": (2, 3, 128, (1, 10, 90), (1, 4, 4), (1, 2, 2), (0, 1, 1)),
    "f3d1_32": (3, 1, 32, (3, 9, 33), (2, 2, 2), (1, 2, 2), (0, 1, 1)),         # segs % SPI != 0: table slots past the last slab
    "f3d1_64": (2, 1, 64, (3, 7, 70), (2, 2, 2), (1, 1, 2), (1, 0, 1)),
    "f3d1_128": (2, 1, 128, (3, 6, 32), (2, 2, 2), (1, 2, 2), (0, 1, 1)),
    "f2d1_32": (3, 1, 32, (1, 9, 34), (1, 4, 4), (1, 2, 2), (0, 1, 1)),
    "f2d1_64s3": (3, 1, 64, (1, 10, 100), (1, 4, 4), (1, 1, 3), (0, 1, 1)),     # sw = 3, Wo = 33: a segment of one position; short last workgroup
    "f2d1_128": (2, 1, 128, (1, 7, 63), (1, 4, 4), (1, 1, 1), (0, 2, 2)),       # Wo = 64: two whole segments
    "f2d_c2kw2": (2, 2, 64, (1, 12, 40), (1, 4, 2), (1, 1, 2), (0, 1, 0)),      # <1,4,2> is keyed on kw*Ci/2: also Ci = 2, kw = 2
    "f2d_c4kw3": (2, 4, 128, (1, 9, 40), (1, 4, 3), (1, 1, 2), (0, 2, 1)),      # <1,4,6> likewise: also Ci = 4, kw = 3
    "f_chunk2": (1025, 1, 128, (1, 32, 32), (1, 4, 4), (1, 2, 2), (0, 1, 1)),   # 33 iterations per workgroup: a second table chunk
    # ---- weight gradient only
    "w2_32": (2, 4, 32, (4, 5, 20), (4, 4, 4), (1, 1, 1), (1, 1, 1)),
    "w3_32": (2, 4, 32, (5, 5, 20), (5, 4, 4), (1, 1, 1), (2, 1, 1)),
    "w4_32": (2, 4, 32, (5, 6, 20), (5, 5, 4), (1, 1, 1), (2, 2, 1)),
    "w2_64": (2, 4, 64, (1, 9, 36), (1, 5, 5), (1, 1, 2), (0, 2, 2)),
    "w4_64": (2, 4, 64, (4, 5, 20), (4, 4, 4), (1, 1, 1), (1, 1, 1)),
    "w1_128": (2, 2, 128, (1, 9, 36), (1, 3, 3), (1, 1, 2), (0, 1, 1)),         # Kt = 18, just above the THIN path's 16
    "w3_128": (2, 3, 128, (1, 9, 36), (1, 5, 5), (1, 1, 2), (0, 2, 2)),
    "w4_128": (2, 4, 128, (1, 9, 36), (1, 5, 5), (1, 1, 2), (0, 2, 2)),
    "w_chunk2": (4097, 3, 32, (1, 32, 32), (1, 4, 4), (1, 2, 2), (0, 1, 1)),    # 129 slabs per workgroup: a second table chunk
    # ---- shapes conv_patch_plan declines: they run the tiled GEMM
    "d_lwc": (2, 4, 32, (1, 9, 20), (1, 4, 3), (1, 1, 1), (0, 2, 1)),           # LWC = 136 > CP_MAXCOL * 64 threads per staging group
    "d_patch8": (2, 3, 32, (1, 16, 16), (1, 4, 4), (1, 2, 2), (0, 1, 1)),       # Wo = 8
    "d_mnist_video": (3, 1, 64, (16, 28, 28), (2, 2, 2), (1, 2, 2), (0, 1, 1)),  # MNIST video discriminator, layer 0: Wo = 15
    "d_mnist_image": (12, 1, 64, (1, 28, 28), (1, 4, 4), (1, 2, 2), (0, 1, 1)),  # MNIST image discriminator, layer 0: Wo = 14
    "d_k3": (2, 3, 64, (1, 32, 32), (1, 3, 3), (1, 1, 1), (0, 1, 1)),           # Conv2d(3, 64, 3, 1, 1): kw * Ci is odd
}

FPlan = collections.namedtuple("FPlan", "variant CB SPI LWC nseg segs iters_per_wg wgs")
WPlan = collections.namedtuple("WPlan", "nbw RB CB nseg segs segs_per_wg splits")

# conv_patch_fprop_kernel's template arguments by ConvPatchPlan.variant (conv_patch.hip: gode_launch_conv_patch_fprop)
VARIANTS = {1: (4, 4, 6), 2: (1, 4, 6), 3: (2, 2, 1), 4: (1, 4, 2)}

# shape: the plan conv_patch_plan must give it
FPROP_PLANS = {
    "f3d3_32": FPlan(1, 1, 4, 105, 1, 16, 4, 1),
    "f3d3_64": FPlan(1, 2, 2, 198, 1, 32, 4, 4),
    "f3d3_128": FPlan(1, 4, 1, 198, 2, 6, 6, 1),
    "f2d3_32": FPlan(2, 1, 4, 105, 1, 24, 6, 1),
    "f2d3_64": FPlan(2, 2, 2, 198, 1, 32, 4, 4),
    "f2d3_128": FPlan(2, 4, 1, 198, 2, 20, 4, 5),
    "f3d1_32": FPlan(3, 1, 4, 64, 1, 30, 4, 2),
    "f3d1_64": FPlan(3, 2, 2, 64, 2, 96, 4, 12),
    "f3d1_128": FPlan(3, 4, 1, 64, 1, 16, 4, 4),
    "f2d1_32": FPlan(4, 1, 4, 66, 1, 12, 3, 1),
    "f2d1_64s3": FPlan(4, 2, 2, 97, 2, 54, 5, 6),
    "f2d1_128": FPlan(4, 4, 1, 35, 2, 32, 4, 8),
    "f2d_c2kw2": FPlan(4, 2, 2, 128, 1, 22, 6, 2),
    "f2d_c4kw3": FPlan(2, 4, 1, 260, 1, 20, 4, 5),
    "f_chunk2": FPlan(4, 4, 1, 66, 1, 16400, 33, 497),
}
# shape: the plan wgrad_make_plan must give it (path: the patch kernel)
WGRAD_PLANS = {
    "f2d3_32": WPlan(1, 1, 2, 1, 24, 2, 12),
    "w2_32": WPlan(2, 1, 8, 1, 24, 2, 12),
    "w3_32": WPlan(3, 1, 10, 1, 40, 2, 20),
    "w4_32": WPlan(4, 1, 13, 1, 60, 2, 30),
    "f2d3_64": WPlan(1, 2, 2, 1, 32, 2, 16),
    "w2_64": WPlan(2, 2, 4, 1, 18, 2, 9),
    "f3d3_64": WPlan(3, 2, 6, 1, 32, 2, 16),
    "w4_64": WPlan(4, 2, 8, 1, 24, 2, 12),
    "w1_128": WPlan(1, 4, 1, 1, 18, 2, 9),
    "f2d3_128": WPlan(2, 4, 2, 2, 20, 2, 10),
    "w3_128": WPlan(3, 4, 3, 1, 18, 2, 9),
    "w4_128": WPlan(4, 4, 4, 1, 18, 2, 9),
    "w_chunk2": WPlan(1, 1, 2, 1, 65552, 129, 509),
}
WGRAD_DECLINED = ["f3d3_128"]      # nbw would be 6 > WP_MAXB: the tiled GEMM
BIG = {"f_chunk2", "w_chunk2"}     # ~135 MB each; every other shape is under 1 MB

ACT_NONE, ACT_LRELU = 0, 2         # gan_ode_amd._lib's codes (this module loads no library)

Cell = collections.namedtuple("Cell", "name shape kernel layout src y work xform scale base")


def cell(name, shape, kernel, layout="cl", src=0, y=0, work=0, xform=False, scale=0, base=None):
    """kernel: "fprop" / "wgrad".  layout of x: "cl" channels-last contiguous (the op's strides all zero), "ncdhw" an
    [N, C, D, H, W] tensor read in place, "pad1" a channels-last view with odd padded strides (igemm_cells' pad1).  src / y /
    work / scale: floats past a 16-byte boundary of x, y, work, scale and shift.  xform (wgrad): BatchNorm scale / shift +
    LeakyReLU(0.2) applied to y on load.  base: the cell whose result this one must repeat bit for bit."""
    return Cell(name, shape, kernel, layout, src, y, work, xform, scale, base)


CELLS = [cell(f"{s}", s, "fprop") for s in FPROP_PLANS] + [cell(f"{s}-w", s, "wgrad") for s in WGRAD_PLANS]
# ---- x layouts and x one float off: every forward instantiation, and one weight-gradient shape per Co (one of them 3-D)
for _s in ("f3d3_64", "f2d3_128", "f3d1_32", "f2d1_64s3", "f2d_c2kw2", "f2d_c4kw3"):
    CELLS += [cell(f"{_s}-ncdhw", _s, "fprop", layout="ncdhw", base=_s), cell(f"{_s}-pad1", _s, "fprop", layout="pad1", base=_s),
              cell(f"{_s}-src-off", _s, "fprop", src=1, base=_s)]
for _s in ("f2d3_32", "f3d3_64", "f2d3_128"):
    CELLS += [cell(f"{_s}-w-ncdhw", _s, "wgrad", layout="ncdhw", base=f"{_s}-w"), cell(f"{_s}-w-pad1", _s, "wgrad", layout="pad1", base=f"{_s}-w"),
              cell(f"{_s}-w-src-off", _s, "wgrad", src=1, base=f"{_s}-w")]
CELLS += [
    # ---- the transform on y, one shape per Co (the thread -> channel mapping yc4 = tid % (Co / 4) differs); then scale / shift
    # one float off (the kernel reads them with scalar loads: same bits)
    cell("w2_32-w-yxf", "w2_32", "wgrad", xform=True),
    cell("f2d3_64-w-yxf", "f2d3_64", "wgrad", xform=True),
    cell("w4_128-w-yxf", "w4_128", "wgrad", xform=True),
    cell("w2_32-w-yxf-scale-off", "w2_32", "wgrad", xform=True, scale=1, base="w2_32-w-yxf"),
    cell("f2d3_64-w-yxf-scale-off", "f2d3_64", "wgrad", xform=True, scale=1, base="f2d3_64-w-yxf"),
    cell("w4_128-w-yxf-scale-off", "w4_128", "wgrad", xform=True, scale=1, base="w4_128-w-yxf"),
    # ---- y one float off (yvec = 0) on Co = 32 and Co = 128 (tests/test_gpu_wgrad_paths.py has Co = 64)
    cell("w3_32-w-y-off", "w3_32", "wgrad", y=1, base="w3_32-w"),
    cell("w1_128-w-y-off", "w1_128", "wgrad", y=1, base="w1_128-w"),
    cell("w4_128-w-yxf-y-off", "w4_128", "wgrad", xform=True, y=1, base="w4_128-w-yxf"),
    # ---- work one float off behind the float4 reduce (fewer than 16 slabs): the scalar reduce
    cell("w4_128-w-work-off", "w4_128", "wgrad", work=1, base="w4_128-w"),
]
BY_NAME = {c.name: c for c in CELLS}
assert len(BY_NAME) == len(CELLS)

# Ops conv_patch_plan must decline: (name, shape, stats, transform, requested tile).  gode_igemm serves them by the tiled GEMM.
DECLINED = [
    ("lwc", "d_lwc", False, False, 0),
    ("patch8", "d_patch8", False, False, 0),
    ("mnist-video", "d_mnist_video", False, False, 0),
    ("mnist-image", "d_mnist_image", False, False, 0),
    ("conv2d-k3", "d_k3", False, False, 0),
    ("patch-stats", "f2d3_64", True, False, 0),
    ("patch-transform", "f2d3_64", False, True, 0),
    ("patch-tile", "f2d3_64", False, False, 2),
]


def out_extent(shape):
    N, Ci, Co, xi, k, s, p = SHAPES[shape]
    return tuple(conv_out(xi[a], k[a], s[a], p[a]) for a in range(3))


def x_strides(shape, layout):
    """Element strides {N, D, H, W, C} of x in the layout, or None for channels-last contiguous; and the floats they span."""
    N, Ci, Co, (d, h, w), k, s, p = SHAPES[shape]
    if layout == "cl":
        return None, N * d * h * w * Ci
    if layout == "ncdhw":
        return (Ci * d * h * w, h * w, w, 1, d * h * w), N * Ci * d * h * w
    assert layout == "pad1"
    sw = Ci + 1
    sh = w * sw + 3
    sd = h * sh + 1
    sn = d * sd + 5
    return (sn, sd, sh, sw, 1), 1 + (N - 1) * sn + (d - 1) * sd + (h - 1) * sh + (w - 1) * sw + (Ci - 1)


def plan_line(name, shape, kernel, layout="cl", src=0, y=0, work=0, xform=0, scale=0, stats=False, act=ACT_NONE, tile=0):
    """One input line of tests/hostcheck/patch_plan_check.cpp."""
    N, Ci, Co, xi, k, s, p = SHAPES[shape]
    gs, _ = x_strides(shape, layout)
    f = [name, kernel[0], N, Ci, Co, *xi, *k, *s, *p, *(gs or (0, 0, 0, 0, 0)), src, y, work, int(xform), scale, int(stats), act, tile]
    return " ".join(str(v) for v in f)


def cell_line(c):
    return plan_line(c.name, c.shape, c.kernel, c.layout, c.src, c.y, c.work, int(c.xform), c.scale, act=ACT_LRELU if c.xform else ACT_NONE)


def padded_sides(shape):
    """Which sides of x some tap of some output position reaches past: a subset of {"d-", "d+", "h-", "h+", "w-", "w+"}."""
    N, Ci, Co, xi, k, s, p = SHAPES[shape]
    yo = out_extent(shape)
    sides = set()
    for a, ax in enumerate("dhw"):
        if p[a] > 0:
            sides.add(ax + "-")
        if (yo[a] - 1) * s[a] - p[a] + k[a] - 1 >= xi[a]:
            sides.add(ax + "+")
    return sides
