"""GPU: gode_igemm on every launch cell of tests/igemm_cells.py (kernel x tile, operand transform, split-K finish, grid
order, phase table, source strides, pointer alignment, the kernels beside the tiled GEMM, K-splitting plans served unsplit),
one case per row, each at the smallest shape that reaches its cell; tests/test_host_igemm_cells.py proves the rows complete.

Reference: float64 on the CPU from the same fp32 inputs -- a = act(x*scale + shift), zero padding applied to a, F.conv3d
(FPROP) or F.conv_transpose3d (DGRAD), tanh where asked -- computed once per (shape, direction, transform).

Bounds.  Raw outputs, per element (U = 2^-24, K = taps x gathered channels):
    |got - ref| <= 4U conv(|x*scale| + |shift|, |w|) + (K + 2) U conv(|a|, |w|)
the bound tests/test_gpu_dcgan.py uses for this op with the convolution of magnitudes in place of its matrix product: the
first term is the fp32 transform (a product, a sum and the activation's slope, each within U, on magnitudes up to
|x*scale| + |shift|), the second the K-term fp32 accumulation and the rounding of the result.  It is derived, not measured; the
worst ratio of every cell is printed.  Every row, tanh rows included: rel_err < 1e-4, the suite's bound for this family.
Statistics: column sums and sums of squares per image group against float64 at 1e-4.

Besides: the cell of the real op is the row's; out, stats and work sit between 64 guard floats of a fixed bit pattern on
either side, which all survive; out and stats start as NaN and come back finite; two runs are bit-identical; a border row,
with a transform or without, is bit-identical to the same op with border = 0.  With no workspace the finish of an unsplit
launch runs in place over out: the NaN pre-fill and the guards show that it reads nothing it did not write."""
import ctypes as C
import functools

import pytest
import torch
import torch.nn.functional as Fn

from conftest import rel_err

import gan_ode_amd._lib as L
import igemm_cells as T

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
GUARD = 64
PATTERN = 0x5A5AA5A5      # the guard floats' bits
SLOPE = {L.ACT_NONE: 1.0, L.ACT_RELU: 0.0, L.ACT_LRELU: 0.2, L.ACT_LRELU01: 0.1}


def _conv(r, a, w):
    """The row's convolution in a's precision: a [N, C, D, H, W] -> [N, C', D', H', W']."""
    N, Ci, Co, xi, k, s, p = T.SHAPES[r.shape]
    if r.dir == T.F:
        return Fn.conv3d(a, w, stride=s, padding=p)
    yo = a.shape[2:]
    opad = tuple(xi[i] - ((yo[i] - 1) * s[i] - 2 * p[i] + k[i]) for i in range(3))
    return Fn.conv_transpose3d(a, w, stride=s, padding=p, output_padding=opad)


@functools.lru_cache(maxsize=None)
def _reference(shape, direction, act, affine):
    """fp32 inputs and the float64 reference of every row with this (shape, direction, transform): the source (channels-last),
    weights, scale, shift; the raw reference and the per-element bound, channels-last [N, D, H, W, C]."""
    r = T.row("", shape, direction, "", act=act, affine=affine)
    N, Ci, Co, xi, k, s, p = T.SHAPES[shape]
    gen = torch.Generator().manual_seed(1000 * sorted(T.SHAPES).index(shape) + 100 * direction + 10 * act + int(affine))
    n, d, h, w_, c = T.gathered_dims(r)
    src = torch.randn(n, c, d, h, w_, generator=gen)
    w = torch.randn(Co, Ci, *k, generator=gen) * 0.2
    # O(1) shifts and scales of both signs: act(shift) != 0 is what a padded tap would wrongly contribute
    sign = torch.where(torch.rand(c, generator=gen) < 0.5, -1.0, 1.0)
    sc, sh = (torch.rand(c, generator=gen) + 0.5) * sign, torch.randn(c, generator=gen)
    x64, w64 = src.double(), w.double()
    v = (lambda t: t.view(1, -1, 1, 1, 1))
    pre = x64 * v(sc.double()) + v(sh.double()) if affine else x64
    a = torch.where(pre > 0, pre, pre * SLOPE[act])
    ref = _conv(r, a, w64)
    mag = (x64 * v(sc.double())).abs() + v(sh.double()).abs() if affine else x64.abs()
    K = k[0] * k[1] * k[2] * c
    bound = 4 * U * _conv(r, mag, w64.abs()) + (K + 2) * U * _conv(r, a.abs(), w64.abs())
    cl = (lambda t: t.permute(0, 2, 3, 4, 1).contiguous())
    return cl(src), w, sc, sh, cl(ref), cl(bound)


def _placed(t, off):
    """t's values on the GPU, `off` floats past a 16-byte boundary."""
    buf = torch.empty(t.numel() + 4, device="cuda")
    v = buf[off:off + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 * off
    return v


class Guarded:
    """n floats `off` floats past a 16-byte boundary, between GUARD floats of PATTERN on either side."""

    def __init__(self, n, off, nan):
        self.n, self.lo = n, GUARD + off
        self.buf = torch.empty(2 * GUARD + off + n, device="cuda")
        self.buf.view(torch.int32).fill_(PATTERN)
        self.data = self.buf[self.lo:self.lo + n]
        if nan:
            self.data.fill_(float("nan"))
        assert self.data.data_ptr() % 16 == 4 * off

    def ptr(self):
        return self.data.data_ptr()

    def guards_intact(self):
        g = self.buf.view(torch.int32)
        return bool((g[self.lo - GUARD:self.lo] == PATTERN).all()) and bool((g[self.lo + self.n:self.lo + self.n + GUARD] == PATTERN).all())


def _source(r, src):
    """The row's source view on the GPU: the op's pointer; the buffer's other floats are NaN."""
    gs, span = T.gather_strides(r)
    if gs is None:
        return _placed(src, r.src)
    buf = torch.full((span + 4,), float("nan"), device="cuda")
    view = buf[r.src:].as_strided(src.shape, gs)
    view.copy_(src)
    assert view.data_ptr() % 16 == 4 * r.src
    return view


def _run(r, border=None):
    """One launch of the row's op over fresh buffers, whose guard floats must survive it: return code, cell label, out, stats,
    rows of image group 0."""
    lib = L.lib()
    stream = torch.cuda.current_stream().cuda_stream
    src, w, sc, sh, _, _ = _reference(r.shape, r.dir, r.act, r.affine)
    g = T.geom(r)
    pdir = r.dir | (L.PACK_BORDER if r.border else 0)
    wp = torch.empty(lib.gode_pack_size(C.byref(g), pdir), device="cuda")
    wd = w.cuda()
    L.check(lib.gode_pack_weights(C.byref(g), pdir, wd.data_ptr(), wp.data_ptr(), None, 0, stream))
    srcv, scd, shd = _source(r, src), _placed(sc, r.scale), _placed(sh, r.scale)
    dims = T.out_dims(r)
    out = Guarded(dims[0] * dims[1] * dims[2] * dims[3] * dims[4], r.out, nan=True)
    op = T.make_op(r, src=srcv.data_ptr(), wpack=wp.data_ptr(), out=out.ptr(), scale=scd.data_ptr(), shift=shd.data_ptr(),
                   stats=1 << 20, work=1 << 20, border=border)       # (placeholders until the sizes are known)
    need = lib.gode_igemm_work_size(C.byref(op))
    rows, rows0 = lib.gode_igemm_stats_rows(C.byref(op)), lib.gode_igemm_stats_rows0(C.byref(op))
    assert need >= 0 and rows > 0
    work = Guarded(max(need, 1), r.work or 0, nan=False)
    stats = Guarded(2 * dims[4] * rows, 0, nan=True)
    op.work = None if r.work is None else work.ptr()
    op.stats = stats.ptr() if r.stats else None
    label = T.cell_label(op) if border is None else None
    rc = getattr(lib, op.FN)(C.byref(op), stream)
    torch.cuda.synchronize()
    assert out.guards_intact() and stats.guards_intact() and work.guards_intact()
    return dict(rc=rc, label=label, out=out.data.view(dims).cpu(), stats=stats.data.view(2, dims[4], rows).cpu(), rows0=rows0)


@pytest.mark.parametrize("r", T.ROWS, ids=[r.name for r in T.ROWS])
def test_igemm_launch_cell(r):
    _, _, _, _, ref, bound = _reference(r.shape, r.dir, r.act, r.affine)
    one = _run(r)
    assert one["label"] == r.label
    assert one["rc"] == 0
    out = one["out"].double()
    assert bool(torch.isfinite(out).all())
    want = torch.tanh(ref) if r.epi == L.EPI_TANH else ref
    if r.epi == L.EPI_RAW:
        ratio = float(((out - ref).abs() / bound.clamp_min(1e-300)).max())
        print(f"{r.name}: {r.label}: worst |got - ref| / bound = {ratio:.3f}, rel_err = {rel_err(out, want):.2e}")
        assert bool(((out - ref).abs() <= bound).all()), ratio
    assert rel_err(out, want) < 1e-4
    if r.stats:
        st = one["stats"].double()
        assert bool(torch.isfinite(st).all())
        N, cols = ref.shape[0], ref.shape[-1]
        assert one["rows0"] == st.shape[2] or r.groups == 2
        parts = [(0, N, 0, st.shape[2])] if r.groups != 2 else [(0, N // 2, 0, one["rows0"]), (N // 2, N, one["rows0"], st.shape[2])]
        for n0, n1, r0, r1 in parts:
            assert r1 > r0
            flat = ref[n0:n1].reshape(-1, cols)
            assert rel_err(st[0, :, r0:r1].sum(1), flat.sum(0)) < 1e-4
            assert rel_err(st[1, :, r0:r1].sum(1), (flat * flat).sum(0)) < 1e-4
    # deterministic: a second launch over fresh buffers gives the same bits
    two = _run(r)
    assert two["rc"] == 0 and torch.equal(one["out"], two["out"])
    if r.stats:
        assert torch.equal(one["stats"], two["stats"])
    # a border-split table changes no raw output, with a transform on load as without
    if r.border:
        plain = _run(r, border=0)
        assert plain["rc"] == 0 and torch.equal(one["out"], plain["out"])
