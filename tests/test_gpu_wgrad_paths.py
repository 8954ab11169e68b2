"""GPU: gode_wgrad on the launch-plan cells (gan-ode_amd/csrc/wgrad_plan.h: path, launched tile, kernel family, vx, vy, LDS-DMA,
reduce kind) that the CASES of test_gpu_kernels.py do not reach, each at the smallest shape that reaches it -- the shapes are
the "paths.*" geometries of tests/hostcheck/wgrad_plan_check.cpp, whose plans tests/golden/wgrad_plans.txt pins; the split
count in each row below is read off that golden and checked here through gode_wgrad_work_size.  Reference: F.conv3d's weight
gradient on the CPU, computed once per (shape, transform); bound: the suite's 2e-4 for gradients through long reductions.
An operand "off" is the same values one float past a 16-byte boundary."""
import ctypes as C
import functools

import pytest
import torch
import torch.nn.functional as F

from conftest import rel_err

import gan_ode_amd._lib as L
from gan_ode_amd.engine import conv_out, make_geom

pytestmark = pytest.mark.gpu

# name: (N, Ci, Co, (Di, Hi, Wi), k, s, p), position splits of the plan
SHAPES = {
    "t256x128": ((8, 64, 256, (1, 64, 64), (1, 4, 4), (1, 2, 2), (0, 1, 1)), 32),    # Co % 256 == 0 and exactly 2^31 MACs: the floor of the 256x128 tile
    "t128x256": ((16, 64, 128, (1, 64, 64), (1, 4, 4), (1, 2, 2), (0, 1, 1)), 64),   # Co = 128, Kt = 1024, 2^31 MACs: the floor of the 128x256 tile
    "thin": ((2, 1, 8, (1, 28, 28), (1, 4, 4), (1, 2, 2), (0, 1, 1)), 7),            # Kt = 16
    "patch": ((2, 3, 64, (4, 32, 32), (4, 4, 4), (1, 2, 2), (0, 1, 1)), 16),         # 16 slabs of Co * Kt = 12288 sums
    "kt27": ((2, 3, 16, (1, 8, 8), (1, 3, 3), (1, 1, 1), (0, 1, 1)), 2),             # Kt % 4 != 0
    "t64": ((4, 8, 64, (1, 8, 8), (1, 3, 3), (1, 1, 1), (0, 1, 1)), 4),
    "t128": ((4, 8, 128, (1, 8, 8), (1, 3, 3), (1, 1, 1), (0, 1, 1)), 4),
}

# (shape, x off, y off, work off, BN+ReLU on "x" / "y" / None): the cell it reaches
CELLS = [
    ("t256x128", 0, 0, 0, None),    # 256x128 FAST, LDS-DMA
    ("t256x128", 0, 0, 0, "x"),     # 256x128 FAST, register staging
    ("t256x128", 1, 0, 0, None),    # splits of the 256x128 tile on the generic 128x128 kernel, x scalar / y float4
    ("t128x256", 0, 0, 0, None),    # 128x256 FAST, LDS-DMA
    ("t128x256", 0, 0, 0, "x"),     # 128x256 FAST, register staging
    ("t128x256", 0, 1, 0, None),    # splits of the 128x256 tile on the generic 128x128 kernel, x float4 / y scalar
    ("thin", 0, 0, 0, None),        # THIN kernel, vec4 reduce
    ("thin", 0, 1, 0, None),        # thin-eligible with y off: the THIN rule's splits on the generic 32x128 kernel, both scalar
    ("thin", 0, 0, 1, None),        # THIN kernel, scalar reduce (work off)
    ("patch", 0, 0, 0, None),       # PATCH kernel, small reduce by its own 32768 bound
    ("patch", 0, 1, 0, None),       # PATCH kernel reading y rows as scalars
    ("kt27", 0, 0, 0, None),        # scalar reduce (Kt % 4 != 0)
    ("t64", 0, 0, 0, "x"),          # 64x128 FAST, register staging
    ("t64", 0, 0, 0, "y"),          # ... with the transform on y
    ("t64", 1, 0, 0, None),         # 64x128 generic: x scalar / y float4
    ("t64", 0, 1, 0, None),         #                 x float4 / y scalar
    ("t64", 1, 1, 0, None),         #                 both scalar
    ("t128", 0, 0, 0, "x"),         # 128x128 FAST, register staging
    ("t128", 1, 1, 0, None),        # 128x128 generic, both scalar
]


@functools.lru_cache(maxsize=None)
def _reference(shape, xform):
    (N, Ci, Co, xi, k, s, p), _ = SHAPES[shape]
    yo = tuple(conv_out(xi[a], k[a], s[a], p[a]) for a in range(3))
    gen = torch.Generator().manual_seed(sorted(SHAPES).index(shape) * 3 + (0 if xform is None else 1 + "xy".index(xform)))
    x = torch.randn(N, Ci, *xi, generator=gen)
    y = torch.randn(N, Co, *yo, generator=gen)
    Cx = Co if xform == "y" else Ci
    sc, sh = torch.rand(Cx, generator=gen) + 0.5, torch.randn(Cx, generator=gen)
    bn_relu = lambda t: F.relu(t * sc.view(1, -1, 1, 1, 1) + sh.view(1, -1, 1, 1, 1))
    xa, ya = (bn_relu(x) if xform == "x" else x), (bn_relu(y) if xform == "y" else y)
    w = torch.zeros(Co, Ci, *k, requires_grad=True)
    F.conv3d(xa, w, stride=s, padding=p).backward(ya)
    return x, y, sc, sh, w.grad


def _placed(t, off):
    """t's values on the GPU, `off` floats past a 16-byte boundary."""
    buf = torch.empty(t.numel() + 4, device="cuda")
    v = buf[off:off + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 * off
    return v


@pytest.mark.parametrize("shape,xo,yo,wo,xform", CELLS)
def test_wgrad_plan_cell(shape, xo, yo, wo, xform):
    (N, Ci, Co, xi, k, s, p), splits = SHAPES[shape]
    g = make_geom(N, Ci, Co, xi, tuple(conv_out(xi[a], k[a], s[a], p[a]) for a in range(3)), k, s, p)
    x, y, sc, sh, ref = _reference(shape, xform)
    xc, yc = _placed(x.permute(0, 2, 3, 4, 1).contiguous(), xo), _placed(y.permute(0, 2, 3, 4, 1).contiguous(), yo)
    scd, shd = sc.cuda(), sh.cuda()
    dw = torch.full(ref.shape, float("nan"), device="cuda")
    op = L.WgradOp(g=g, act=L.ACT_NONE if xform is None else L.ACT_RELU, xform_on_y=int(xform == "y"), splits=0, accumulate=0,
                   x=xc.data_ptr(), y=yc.data_ptr(), scale=None if xform is None else scd.data_ptr(),
                   shift=None if xform is None else shd.data_ptr(), dw=dw.data_ptr())
    need = L.lib().gode_wgrad_work_size(C.byref(op))
    assert need == splits * ref.numel()
    work = torch.empty(need + 4, device="cuda")[wo:]
    assert work.data_ptr() % 16 == 4 * wo
    op.work = work.data_ptr()
    L.run_one(op, torch.cuda.current_stream().cuda_stream)
    assert rel_err(dw.cpu(), ref) < 2e-4
