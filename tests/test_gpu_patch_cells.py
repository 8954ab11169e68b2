"""GPU: conv_patch_fprop_kernel (through gode_igemm) and wgrad_patch_kernel (through gode_wgrad) on every cell of
tests/patch_cells.py -- all 4 x 3 forward launches and all 12 weight-gradient instantiations, every x layout, operands one
float off, the transform on y, and the second chunk of both kernels' 128-entry slab tables; tests/test_host_patch_cells.py
proves on the CPU that each shape gets the plan the table states and that the table is complete.

Inputs: seeded fp32 normals, weights x 0.2.  Reference: F.conv3d, or its weight gradient, in float64 on the CPU from the same
fp32 inputs, computed once per (shape, transform) and accumulated over blocks of images so that the two large shapes stay
bounded in memory.

Bounds, per element, U = 2^-24.  Derived, not measured; the worst ratio of every cell is printed.
  forward          |out - ref| <= 2 K U (|x| conv |w|),  K = kd kh kw Ci
      the worst case of K rounded multiply-adds in any order, doubled for the MFMA unit's internal rounding, which is not
      documented.  One wrong or missing tap moves an element by about 1/K of that sum: 10^2 - 10^4 times the bound.
  weight gradient  |dw - ref| <= 2 (32 segs_per_wg + 2) U sum |x y|
      fp32 accumulation of the 32 segs_per_wg products of a workgroup, then the float64 sum over workgroups and one rounding;
      with the transform, y is BN + LeakyReLU of y in float64.  The suite's rel_err < 2e-4 holds as well.
  w_chunk2         a dropped slab is 3e-5 of an element's sum and would pass that bound, so the shape runs once more with y
      zero except in the slabs with local index >= 126 of every workgroup (the last two of the first table chunk and the one
      of the second); the bound then counts those slabs only (exact zeros add no rounding error).  f_chunk2 needs no probe:
      every output element has its own bound.

Besides: every output, and the weight gradient's workspace, starts as NaN between 64 guard floats on either side; the guards
keep their bits and the interior comes back without a NaN.  A second run gives the same bits.  A cell with another x layout
or an operand one float off gives the bits of its aligned channels-last twin: neither kernel's arithmetic depends on where
its operands lie."""
import ctypes as C
import functools

import pytest
import torch
import torch.nn.functional as Fn

from conftest import rel_err

import gan_ode_amd._lib as L
import igemm_cells as I
import patch_cells as T
from gan_ode_amd.engine import make_geom

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
GUARD = 64
NAN_BITS = 0x7FC5A5A5      # a quiet NaN with a payload: the pre-fill of outputs and guards
BLOCK = 64                 # images per block of the float64 reference
PROBE_FROM = 126           # w_chunk2's probe: the slabs of every workgroup with this local index and above
PROBE = (PROBE_FROM, 1 << 30)


def _geom(shape):
    N, Ci, Co, xi, k, s, p = T.SHAPES[shape]
    return make_geom(N, Ci, Co, xi, T.out_extent(shape), k, s, p)


@functools.lru_cache(maxsize=2)        # (deterministic, so an evicted entry comes back the same; w_chunk2's y is 134 MB)
def _inputs(shape, xform=False, probe=None):
    """fp32 inputs: x [N, Ci, D, H, W], w [Co, Ci, kd, kh, kw], y [N, Co, Do, Ho, Wo], scale and shift [Co].  probe = (lo, hi): y
    zeroed outside the slabs (32-position segments of an output row, numbered as the kernel does) whose index within their
    workgroup is in [lo, hi)."""
    N, Ci, Co, xi, k, s, p = T.SHAPES[shape]
    gen = torch.Generator().manual_seed(7 + 2 * sorted(T.SHAPES).index(shape) + int(xform))
    x = torch.randn(N, Ci, *xi, generator=gen)
    w = torch.randn(Co, Ci, *k, generator=gen) * 0.2
    yo = T.out_extent(shape)
    y = torch.randn(N, Co, *yo, generator=gen)
    # O(1) scales of both signs and shifts: the activation's two slopes both occur in every channel
    sign = torch.where(torch.rand(Co, generator=gen) < 0.5, -1.0, 1.0)
    sc, sh = (torch.rand(Co, generator=gen) + 0.5) * sign, torch.randn(Co, generator=gen)
    if probe:
        plan = T.WGRAD_PLANS[shape]
        row = torch.arange(N * yo[0] * yo[1]).view(N, 1, yo[0], yo[1], 1)
        seg = torch.arange(yo[2]).view(1, 1, 1, 1, -1) // 32
        local = (row * plan.nseg + seg) % plan.segs_per_wg
        live = (local >= probe[0]) & (local < probe[1])
        y = y * live
    return x, w, y, sc, sh


def _fprop_blocks(shape):
    """(n0, n1, reference, bound) per block of images, float64 channels-last [n, Do, Ho, Wo, Co]."""
    N, Ci, Co, xi, k, s, p = T.SHAPES[shape]
    x, w, _, _, _ = _inputs(shape)
    w64 = w.double()
    K = k[0] * k[1] * k[2] * Ci
    for n0 in range(0, N, BLOCK):
        x64 = x[n0:n0 + BLOCK].double()
        ref = Fn.conv3d(x64, w64, stride=s, padding=p)
        bound = 2 * K * U * Fn.conv3d(x64.abs(), w64.abs(), stride=s, padding=p)
        yield n0, n0 + x64.shape[0], ref.permute(0, 2, 3, 4, 1), bound.permute(0, 2, 3, 4, 1)


@functools.lru_cache(maxsize=None)
def _fprop_reference(shape):
    return list(_fprop_blocks(shape))


@functools.lru_cache(maxsize=None)
def _wgrad_reference(shape, xform, probe=None):
    """The weight gradient and sum |x y| per element, float64 [Co, Ci, kd, kh, kw]; the probe skips the images whose y is all zero."""
    N, Ci, Co, xi, k, s, p = T.SHAPES[shape]
    x, w, y, sc, sh = _inputs(shape, xform, probe)
    ref, mag = torch.zeros(w.shape, dtype=torch.float64), torch.zeros(w.shape, dtype=torch.float64)
    assert not (probe and xform)                 # (the transform of a zero is not zero)
    live = torch.nonzero(y.flatten(1).abs().amax(1) > 0).flatten() if probe else torch.arange(N)
    v = (lambda t: t.double().view(1, -1, 1, 1, 1))
    for i in range(0, live.numel(), BLOCK):
        idx = live[i:i + BLOCK]
        x64, y64 = x[idx].double(), y[idx].double()
        if xform:
            pre = y64 * v(sc) + v(sh)
            ya = torch.where(pre > 0, pre, pre * 0.2)
        else:
            ya = y64
        ref += torch.nn.grad.conv3d_weight(x64, w.shape, ya, stride=s, padding=p)
        mag += torch.nn.grad.conv3d_weight(x64.abs(), w.shape, ya.abs(), stride=s, padding=p)
    return ref, mag


class Guarded:
    """n floats `off` floats past a 16-byte boundary between GUARD floats on either side, all of them NAN_BITS."""

    def __init__(self, n, off):
        self.n, self.lo = n, GUARD + off
        self.buf = torch.empty(2 * GUARD + off + n + 4, device="cuda")
        self.buf.view(torch.int32).fill_(NAN_BITS)
        self.data = self.buf[self.lo:self.lo + n]
        assert self.data.data_ptr() % 16 == 4 * off and bool(torch.isnan(self.buf).all())

    def ptr(self):
        return self.data.data_ptr()

    def check(self):
        """The guards kept their bits; the interior holds no NaN."""
        g = self.buf.view(torch.int32)
        assert bool((g[:self.lo] == NAN_BITS).all()) and bool((g[self.lo + self.n:] == NAN_BITS).all()), "a guard float was written"
        assert not bool(torch.isnan(self.data).any()), "an element was not written"


def _placed(t, off):
    """t's values on the GPU, `off` floats past a 16-byte boundary."""
    buf = torch.empty(t.numel() + 4, device="cuda")
    v = buf[off:off + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 * off
    return v


def _x_view(c, x):
    """x [N, Ci, D, H, W] on the GPU in the cell's layout, `c.src` floats off: the view as [N, D, H, W, Ci] and its element
    strides (None: channels-last contiguous); the floats between the elements of a padded view are NaN."""
    gs, span = T.x_strides(c.shape, c.layout)
    cl = x.permute(0, 2, 3, 4, 1)
    buf = torch.full((span + 4,), float("nan"), device="cuda")
    view = buf[c.src:].as_strided(cl.shape, gs) if gs else buf[c.src:c.src + span].view(cl.shape)
    view.copy_(cl)
    assert view.data_ptr() % 16 == 4 * c.src
    return view, gs


def _run_fprop(c):
    """One launch of the cell's op over fresh buffers: out [N, Do, Ho, Wo, Co] on the CPU."""
    lib = L.lib()
    stream = torch.cuda.current_stream().cuda_stream
    N, Ci, Co, xi, k, s, p = T.SHAPES[c.shape]
    x, w, _, _, _ = _inputs(c.shape)
    g = _geom(c.shape)
    wp = torch.empty(lib.gode_pack_size(C.byref(g), L.FPROP), device="cuda")
    wd = w.cuda()
    L.check(lib.gode_pack_weights(C.byref(g), L.FPROP, wd.data_ptr(), wp.data_ptr(), None, 0, stream))
    xv, gs = _x_view(c, x)
    dims = (N, *T.out_extent(c.shape), Co)
    out = Guarded(dims[0] * dims[1] * dims[2] * dims[3] * dims[4], 0)
    op = L.IgemmOp(g=g, dir=L.FPROP, act=L.ACT_NONE, epilogue=L.EPI_RAW, tile=0, src=xv.data_ptr(), wpack=wp.data_ptr(), out=out.ptr(),
                   scale=None, shift=None, stats=None, work=None, groups=1, border=0)
    for i in range(5):
        op.gs[i] = gs[i] if gs else 0
    assert I.cell_label(op) == "patch"
    L.check(lib.gode_igemm(C.byref(op), stream))
    torch.cuda.synchronize()
    out.check()
    return out.data.view(dims).cpu()


def _run_wgrad(c, probe=None):
    """One launch of the cell's op over fresh buffers: dw [Co, Ci, kd, kh, kw] on the CPU."""
    lib = L.lib()
    stream = torch.cuda.current_stream().cuda_stream
    N, Ci, Co, xi, k, s, p = T.SHAPES[c.shape]
    x, w, y, sc, sh = _inputs(c.shape, c.xform, probe)
    plan = T.WGRAD_PLANS[c.shape]
    xv, gs = _x_view(c, x)
    yv = _placed(y.permute(0, 2, 3, 4, 1).contiguous(), c.y)
    scd, shd = _placed(sc, c.scale), _placed(sh, c.scale)
    dw = Guarded(w.numel(), 0)
    op = L.WgradOp(g=_geom(c.shape), act=L.ACT_LRELU if c.xform else L.ACT_NONE, xform_on_y=int(c.xform), splits=0, accumulate=0,
                   x=xv.data_ptr(), y=yv.data_ptr(), scale=scd.data_ptr() if c.xform else None, shift=shd.data_ptr() if c.xform else None,
                   dw=dw.ptr())
    for i in range(5):
        op.xs[i] = gs[i] if gs else 0
    need = lib.gode_wgrad_work_size(C.byref(op))
    assert need == plan.splits * w.numel()
    work = Guarded(need, c.work)
    op.work = work.ptr()
    L.check(lib.gode_wgrad(C.byref(op), stream))
    torch.cuda.synchronize()
    dw.check()
    work.check()
    return dw.data.view(w.shape).cpu()


@functools.lru_cache(maxsize=None)
def _first_run(name):
    """The cell's first run, kept for the cells that must repeat its bits (not for the two large shapes' forward outputs)."""
    c = T.BY_NAME[name]
    return _run_fprop(c) if c.kernel == "fprop" else _run_wgrad(c)


FPROP_CELLS = [c for c in T.CELLS if c.kernel == "fprop"]
WGRAD_CELLS = [c for c in T.CELLS if c.kernel == "wgrad"]


@pytest.mark.parametrize("c", FPROP_CELLS, ids=[c.name for c in FPROP_CELLS])
def test_fprop_patch_cell(c):
    big = c.shape in T.BIG
    one = _run_fprop(c) if big else _first_run(c.name)
    worst = 0.0
    for n0, n1, ref, bound in (_fprop_blocks(c.shape) if big else _fprop_reference(c.shape)):
        err = (one[n0:n1].double() - ref).abs()
        worst = max(worst, float((err / bound.clamp_min(1e-300)).max()))
        assert bool((err <= bound).all()), (n0, worst)
    print(f"{c.name}: plan {tuple(T.FPROP_PLANS[c.shape])}: worst |out - ref| / bound = {worst:.3f}")
    assert torch.equal(one, _run_fprop(c))                          # a second run: the same bits
    if c.base:
        assert torch.equal(one, _first_run(c.base))                 # the layout and the alignment of x change no bit


def _check_wgrad(c, dw, probe):
    plan = T.WGRAD_PLANS[c.shape]
    ref, mag = _wgrad_reference(c.shape, c.xform, probe)
    slabs = plan.segs_per_wg - PROBE_FROM if probe else plan.segs_per_wg
    assert slabs > 0
    bound = 2 * (32 * slabs + 2) * U * mag
    err = (dw.double() - ref).abs()
    worst = float((err / bound.clamp_min(1e-300)).max())
    print(f"{c.name}{' probe' if probe else ''}: plan {tuple(plan)}: worst |dw - ref| / bound = {worst:.3f}, rel_err = {rel_err(dw.double(), ref):.2e}")
    assert bool((err <= bound).all()), worst
    assert rel_err(dw.double(), ref) < 2e-4


@pytest.mark.parametrize("c", WGRAD_CELLS, ids=[c.name for c in WGRAD_CELLS])
def test_wgrad_patch_cell(c):
    one = _first_run(c.name)
    _check_wgrad(c, one, probe=None)
    assert torch.equal(one, _run_wgrad(c))                          # a second run: the same bits
    if c.base:
        assert torch.equal(one, _first_run(c.base))                 # layouts, alignments and the reduce kernel change no bit
    if T.WGRAD_PLANS[c.shape].segs_per_wg > PROBE_FROM:
        _check_wgrad(c, _run_wgrad(c, probe=PROBE), probe=PROBE)      # the hand-over between the table's chunks, slab by slab
