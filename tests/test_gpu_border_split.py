"""GPU: the border-split form of the stride-2 ConvTranspose GEMMs (gode_igemm_op.border: every stride phase cut into
interior / edge / corner sub-phases without out-of-range taps) against the same op without the flag, on the same input and
weights.  The live products of an output element are added in the same order and the ones left out were exact zeros, so the
raw outputs must be bit-identical; only the grouping of the BatchNorm partial sums per m-block differs, so the finalized
scale / shift agree to fp32 rounding (1e-6 relative)."""
import ctypes as C
import os

import pytest
import torch
import torch.nn.functional as F

from conftest import rel_err, seed_all

import gan_ode_amd as G
import gan_ode_amd._lib as L
from gan_ode_amd.engine import make_geom

pytestmark = pytest.mark.gpu

TILES = {"128x64": 2, "128x128": 1, "256x128": 6}


def stream():
    return torch.cuda.current_stream().cuda_stream


def convt_geom(n, cin, cout, h):
    """ConvTranspose2d(cin, cout, 4, 2, 1) on h x h as the conv whose input gradient it is."""
    return make_geom(n, cout, cin, (1, 2 * h, 2 * h), (1, h, h), (1, 4, 4), (1, 2, 2), (0, 1, 1))


def run(g, x, w, tile, border, gamma, beta):
    """-> raw output [N,1,2h,2h,Cout], statistics rows, (scale, shift) of gode_bn_finalize on the launch's partial sums"""
    lib = L.lib()
    d = L.DGRAD | (L.PACK_BORDER if border else 0)
    n = lib.gode_pack_size(C.byref(g), d)
    assert n > 0
    wp = torch.full((n,), float("nan"), device="cuda")
    L.check(lib.gode_pack_weights(C.byref(g), d, w.data_ptr(), wp.data_ptr(), None, 0, stream()))
    out = torch.full((g.N, 1, g.Hi, g.Wi, g.Ci), float("nan"), device="cuda")
    op = L.IgemmOp(g=g, dir=L.DGRAD, act=L.ACT_NONE, epilogue=L.EPI_RAW, tile=tile, src=x.data_ptr(), wpack=wp.data_ptr(),
                   out=out.data_ptr(), border=1 if border else 0)
    work = torch.empty(max(lib.gode_igemm_work_size(C.byref(op)), 1), device="cuda")
    op.work = work.data_ptr()
    rows = lib.gode_igemm_stats_rows(C.byref(op))
    assert rows > 0
    stats = torch.full((2, g.Ci, rows), float("nan"), device="cuda")
    op.stats = stats.data_ptr()
    L.run_one(op, stream())
    Cc = g.Ci
    r = {k: torch.empty(Cc, device="cuda") for k in ("mean", "invstd", "scale", "shift")}
    rm, rv, nbt = torch.zeros(Cc).cuda(), torch.ones(Cc).cuda(), torch.zeros((), dtype=torch.int64).cuda()
    fin = L.BnFinalizeOp(stats=stats.data_ptr(), rows=rows, ncols=Cc, C=Cc, count=g.N * g.Hi * g.Wi, gamma=gamma.data_ptr(),
                         beta=beta.data_ptr(), running_mean=rm.data_ptr(), running_var=rv.data_ptr(),
                         num_batches_tracked=nbt.data_ptr(), mean=r["mean"].data_ptr(), invstd=r["invstd"].data_ptr(),
                         scale=r["scale"].data_ptr(), shift=r["shift"].data_ptr(), momentum=0.1, eps=1e-5, training=1)
    L.run_one(fin, stream())
    torch.cuda.synchronize()
    return out, rows, (r["scale"], r["shift"])


_inputs = {}


def inputs(n, cin, cout, h):
    """One set of operands per shape, shared by the tiles' cases and left unchanged."""
    key = (n, cin, cout, h)
    if key not in _inputs:
        gen = torch.Generator().manual_seed(1000 * n + 10 * h + cin)
        x = torch.randn(n, 1, h, h, cin, generator=gen).cuda()              # channels-last input of the ConvTranspose
        w = (torch.randn(cin, cout, 4, 4, generator=gen) * 0.1).cuda()      # ConvTranspose2d weight [in, out, kh, kw]
        gamma, beta = (torch.rand(cout, generator=gen) + 0.5).cuda(), torch.randn(cout, generator=gen).cuda()
        _inputs[key] = (x, w, gamma, beta)
    return _inputs[key]


def compare(n, cin, cout, h, tile):
    g = convt_geom(n, cin, cout, h)
    x, w, gamma, beta = inputs(n, cin, cout, h)
    y0, rows0, (sc0, sh0) = run(g, x, w, tile, False, gamma, beta)
    y1, rows1, (sc1, sh1) = run(g, x, w, tile, True, gamma, beta)
    assert not torch.isnan(y0).any() and not torch.isnan(y1).any()
    assert torch.equal(y0, y1)
    es, eh = rel_err(sc1.cpu(), sc0.cpu()), rel_err(sh1.cpu(), sh0.cpu())
    print(f"N={n} {cin}->{cout} h={h} tile={tile}: stats rows {rows0} -> {rows1}, scale rel {es:.2e}, shift rel {eh:.2e}")
    assert es <= 1e-6 and eh <= 1e-6
    return y1, rows0, rows1


@pytest.mark.parametrize("tile", list(TILES))
@pytest.mark.parametrize("h", [1, 2, 3, 4])
@pytest.mark.parametrize("cin,cout", [(32, 32), (64, 96)])
@pytest.mark.parametrize("n", [2, 5])
def test_border_form_equals_the_plain_launch(n, cin, cout, h, tile):
    _, rows0, rows1 = compare(n, cin, cout, h, TILES[tile])
    if cin == 32:
        # (K = 4 slabs: no K split, so these shapes do take the border form -- one tile per sub-phase: 4 corners of a 1x1
        # input, 16 sub-phases otherwise; the 64-channel shapes split K when plain, and a K-split launch ignores the flag)
        assert (rows0, rows1) == (4, 4 if h == 1 else 16)


@pytest.mark.parametrize("tile", list(TILES))
@pytest.mark.parametrize("n,cin,cout,h", [
    (150, 64, 96, 4),     # interior 1350 rows: 11 m-blocks of 128 (a run of 8 + 3), partial last tiles, 2 n-blocks of 64
    (70, 32, 32, 3),      # edges of 140 rows (2 m-blocks of 128), corners of 70, 128-wide tiles mostly column padding
])
def test_border_form_over_several_tiles(n, cin, cout, h, tile):
    _, rows0, rows1 = compare(n, cin, cout, h, TILES[tile])
    bm = 256 if tile == "256x128" else 128
    cdiv = lambda a, b: -(-a // b)  # noqa: E731
    i, e = (h - 1) ** 2, h - 1
    assert rows1 == 4 * (cdiv(n * i, bm) + 2 * cdiv(n * e, bm) + cdiv(n, bm)) and rows0 == 4 * cdiv(n * h * h, bm)


def test_border_form_against_torch_float64():
    n, cin, cout, h = 5, 64, 96, 3
    y1, _, _ = compare(150, 64, 96, 4, TILES["128x64"])
    x, w, _, _ = inputs(150, 64, 96, 4)
    ref = F.conv_transpose2d(x[:, 0].permute(0, 3, 1, 2).double().cpu(), w.double().cpu(), stride=2, padding=1)
    assert rel_err(y1[:, 0].permute(0, 3, 1, 2).cpu(), ref) <= 1e-4
    # and a shape of the small set
    y1, _, _ = compare(n, 32, 32, h, TILES["128x64"])
    x, w, _, _ = inputs(n, 32, 32, h)
    ref = F.conv_transpose2d(x[:, 0].permute(0, 3, 1, 2).double().cpu(), w.double().cpu(), stride=2, padding=1)
    assert rel_err(y1[:, 0].permute(0, 3, 1, 2).cpu(), ref) <= 1e-4


def test_model_chosen_form_at_the_flagship_shape():
    """The decoder's 512 -> 256 layer on 4x4 at the benchmark's 512 rows with tile = 0: whatever form and tile the cost
    model picks for the flagged op, it computes what the plain op computes."""
    compare(512, 512, 256, 4, 0)


def test_sampling_with_and_without_the_border_form(monkeypatch):
    """A generator's decoder stack flags its three k4 s2 p1 layers in every forward program (packs of their own);
    GODE_BORDER_SPLIT=0, read when a stack is built, leaves them plain.  1e-5: the project's figure for tile-shape rounding
    (test_joint_generator_pass_equals_the_two_calls).  A no-grad pass and the pass a backward follows run the same
    program: bit-identical frames."""
    vids = []
    for knob in ("0", "1"):
        monkeypatch.setenv("GODE_BORDER_SPLIT", knob)
        seed_all(71)
        gen = G.VideoGeneratorMNISTODE(1, 50, 0, 16, 16, ngf=16).cuda()
        seed_all(72)
        with torch.no_grad():
            vid, _ = gen.sample_videos(3)
        seed_all(72)
        vid2, _ = gen.sample_videos(3)
        torch.cuda.synchronize()
        assert torch.equal(vid, vid2.detach())
        stack = gen._pool.plans[(3, 16, False)][0].stack
        assert sorted(stack._border) == ([1, 2, 3] if knob == "1" else [])      # the three k4 s2 p1 layers
        flagged = [op for op in stack._fwd[True][0].ops if isinstance(op, L.IgemmOp) and op.border]
        assert len(flagged) == (3 if knob == "1" else 0)
        vids.append(vid.detach().clone())
    assert vids[0].shape == vids[1].shape
    assert float((vids[0] - vids[1]).abs().max()) <= 1e-5
