"""GPU: gode_igemm_op.border == 2 (border-split table taken without the cost model's comparison, phase-interleaved grid)
against border == 1 (same table, sub-phase after sub-phase) and border == 0 (plain table) on the same operands, single ops
through L.run_one with the tiles 128x64 and 64x64 requested.  The grid order only permutes which workgroup computes which tile
and the statistics row of a tile travels with its sub-phase, so raw outputs are bit-identical across the three forms and the
partial-statistics buffers bit-identical between border 1 and 2; against the plain form the partial sums are grouped
differently, so the finalized mean / invstd agree to fp32 rounding (1e-6 relative).

Shapes (ConvTranspose 32 -> 64 channels; K = 4 slabs, so no launch splits K): k4 s2 p1 on 4x4 and 8x8 with 24 and 40 images
-- the interior sub-phases have 2 ... 31 m-blocks: fewer than 8, exactly two runs of 8, and runs of 8 plus a remainder --
3x3, the non-square 4x10, k3 s2 p1 4x4 -> 7x7 (stride phases of different taps and extents: keeps the order of border == 1)
and the 3-D k = (3,4,4) shape of the border corpus (two depth runs per stride phase: keeps the order too; 1040 images, below
~1000 its plain launch would split K and every form stays plain)."""
import ctypes as C

import pytest
import torch

from conftest import rel_err

import gan_ode_amd._lib as L
from gan_ode_amd.engine import make_geom

pytestmark = pytest.mark.gpu

CIN, COUT = 32, 64
TILES = {"128x64": 2, "64x64": 4}
# name -> (N, ConvTranspose input extent (d, h, w), output extent, k, s, p, grid is phase-interleaved under border == 2)
SHAPES = {
    "k4s2p1-4x4-n24": (24, (1, 4, 4), (1, 8, 8), (1, 4, 4), (1, 2, 2), (0, 1, 1), True),
    "k4s2p1-4x4-n40": (40, (1, 4, 4), (1, 8, 8), (1, 4, 4), (1, 2, 2), (0, 1, 1), True),
    "k4s2p1-8x8-n24": (24, (1, 8, 8), (1, 16, 16), (1, 4, 4), (1, 2, 2), (0, 1, 1), True),
    "k4s2p1-8x8-n40": (40, (1, 8, 8), (1, 16, 16), (1, 4, 4), (1, 2, 2), (0, 1, 1), True),
    "k4s2p1-3x3-n24": (24, (1, 3, 3), (1, 6, 6), (1, 4, 4), (1, 2, 2), (0, 1, 1), True),
    "k4s2p1-4x10-n24": (24, (1, 4, 10), (1, 8, 20), (1, 4, 4), (1, 2, 2), (0, 1, 1), True),
    "k3s2p1-4x4-to-7x7-n24": (24, (1, 4, 4), (1, 7, 7), (1, 3, 3), (1, 2, 2), (0, 1, 1), False),
    "3d-k344-2x1x1-n1040": (1040, (2, 1, 1), (2, 2, 2), (3, 4, 4), (1, 2, 2), (1, 1, 1), False),
}


def stream():
    return torch.cuda.current_stream().cuda_stream


_operands = {}


def operands(name):
    """One set of operands per shape, shared by its cases and left unchanged."""
    if name not in _operands:
        n, yin, _, k, _, _, _ = SHAPES[name]
        gen = torch.Generator().manual_seed(sum(map(ord, name)))
        x = torch.randn(n, *yin, CIN, generator=gen).cuda()                 # channels-last input of the ConvTranspose
        w = (torch.randn(CIN, COUT, *k, generator=gen) * 0.1).cuda()        # ConvTranspose weight [in, out, kd, kh, kw]
        _operands[name] = (x, w)
    return _operands[name]


def run(name, tile, border):
    """-> raw output, partial-statistics buffer [2, COUT, rows], (mean, invstd) of gode_bn_finalize on it"""
    n, yin, xout, k, s, p, _ = SHAPES[name]
    g = make_geom(n, COUT, CIN, xout, yin, k, s, p)       # the convolution whose input gradient the ConvTranspose is
    x, w = operands(name)
    lib = L.lib()
    d = L.DGRAD | (L.PACK_BORDER if border else 0)
    nw = lib.gode_pack_size(C.byref(g), d)
    assert nw > 0
    wp = torch.full((nw,), float("nan"), device="cuda")
    L.check(lib.gode_pack_weights(C.byref(g), d, w.data_ptr(), wp.data_ptr(), None, 0, stream()))
    out = torch.full((n, *xout, COUT), float("nan"), device="cuda")
    op = L.IgemmOp(g=g, dir=L.DGRAD, act=L.ACT_NONE, epilogue=L.EPI_RAW, tile=tile, src=x.data_ptr(), wpack=wp.data_ptr(),
                   out=out.data_ptr(), border=border)
    assert lib.gode_igemm_work_size(C.byref(op)) == 0          # (no K split: the flag is not ignored)
    rows = lib.gode_igemm_stats_rows(C.byref(op))
    assert rows > 0
    stats = torch.full((2, COUT, rows), float("nan"), device="cuda")
    op.stats = stats.data_ptr()
    L.run_one(op, stream())
    r = {key: torch.empty(COUT, device="cuda") for key in ("mean", "invstd", "scale", "shift")}
    gamma, beta = torch.ones(COUT, device="cuda"), torch.zeros(COUT, device="cuda")
    rm, rv, nbt = torch.zeros(COUT).cuda(), torch.ones(COUT).cuda(), torch.zeros((), dtype=torch.int64).cuda()
    fin = L.BnFinalizeOp(stats=stats.data_ptr(), rows=rows, ncols=COUT, C=COUT, count=out.numel() // COUT, gamma=gamma.data_ptr(),
                         beta=beta.data_ptr(), running_mean=rm.data_ptr(), running_var=rv.data_ptr(),
                         num_batches_tracked=nbt.data_ptr(), mean=r["mean"].data_ptr(), invstd=r["invstd"].data_ptr(),
                         scale=r["scale"].data_ptr(), shift=r["shift"].data_ptr(), momentum=0.1, eps=1e-5, training=1)
    L.run_one(fin, stream())
    torch.cuda.synchronize()
    return out, stats, (r["mean"], r["invstd"])


@pytest.mark.parametrize("tile", list(TILES))
@pytest.mark.parametrize("name", list(SHAPES))
def test_three_forms_of_one_launch(name, tile):
    y0, st0, (mean0, inv0) = run(name, TILES[tile], 0)
    y1, st1, (mean1, inv1) = run(name, TILES[tile], 1)
    y2, st2, (mean2, inv2) = run(name, TILES[tile], 2)
    for y in (y0, y1, y2):
        assert not torch.isnan(y).any()
    assert torch.equal(y0, y1) and torch.equal(y0, y2)
    if SHAPES[name][6]:
        assert st1.shape[2] > st0.shape[2]                      # (the flagged launches did take the 16 sub-phases)
    assert st1.shape == st2.shape and not torch.isnan(st2).any() and torch.equal(st1, st2)
    em, ei = rel_err(mean2.cpu(), mean0.cpu()), rel_err(inv2.cpu(), inv0.cpu())
    print(f"{name} tile {tile}: stats rows {st0.shape[2]} -> {st2.shape[2]}, mean rel {em:.2e}, invstd rel {ei:.2e}")
    assert em <= 1e-6 and ei <= 1e-6
    assert torch.equal(mean1, mean2) and torch.equal(inv1, inv2)


def test_against_torch_float64():
    """The phase-interleaved launch against ConvTranspose2d in float64, on the shape with runs of 8 m-blocks and a remainder."""
    name = "k4s2p1-8x8-n24"
    y2, _, _ = run(name, TILES["128x64"], 2)
    x, w = operands(name)
    ref = torch.nn.functional.conv_transpose2d(x[:, 0].permute(0, 3, 1, 2).double().cpu(), w[:, :, 0].double().cpu(), stride=2, padding=1)
    assert rel_err(y2[:, 0].permute(0, 3, 1, 2).cpu(), ref) <= 1e-4
