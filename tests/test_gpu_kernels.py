"""GPU: every libgode entry point called through the C ABI (ctypes) and compared with the CPU oracle
(torch CPU functional ops / oracle.ode_ref) on the same seeded inputs.  Tolerance: north_star's 1e-4 relative
(fp32); gradients through long reductions get 2e-4."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import golden, rel_err

import gan_ode_amd._lib as L
from gan_ode_amd.engine import conv_out, make_geom

pytestmark = pytest.mark.gpu
TOL = 1e-4


def dev(t):
    return t.cuda()


def cl(t):
    return t.permute(0, 2, 3, 4, 1).contiguous()


def uncl(t):
    return t.permute(0, 4, 1, 2, 3)


def stream():
    return torch.cuda.current_stream().cuda_stream


def pack(g, direction, w, perm=None):
    lib = L.lib()
    n = lib.gode_pack_size(C.byref(g), direction)
    assert n > 0
    wp = torch.empty(n, device="cuda")
    L.check(lib.gode_pack_weights(C.byref(g), direction, w.data_ptr(), wp.data_ptr(),
                                  None if perm is None else perm.data_ptr(), 0, stream()))
    return wp


def igemm(g, direction, src, w, out_dims, scale=None, shift=None, act=L.ACT_NONE, epi=L.EPI_RAW, strides=None,
          tile=0, want_stats=False, perm=None):
    lib = L.lib()
    wp = pack(g, direction, w, perm)
    out = torch.full(out_dims, float("nan"), device="cuda")
    op = L.IgemmOp(g=g, dir=direction, act=act, epilogue=epi, tile=tile, src=src.data_ptr(), wpack=wp.data_ptr(),
                   out=out.data_ptr(), scale=None if scale is None else scale.data_ptr(),
                   shift=None if shift is None else shift.data_ptr())
    if strides is not None:
        for i in range(5):
            op.gs[i] = strides[i]
    wsz = lib.gode_igemm_work_size(C.byref(op))
    work = torch.empty(max(wsz, 1), device="cuda")
    op.work = work.data_ptr()
    stats = None
    if want_stats:
        rows = lib.gode_igemm_stats_rows(C.byref(op))
        stats = torch.full((2, out_dims[-1], rows), float("nan"), device="cuda")      # [sum | sum of squares][column][row]
        op.stats = stats.data_ptr()
    L.run_one(op, stream())
    torch.cuda.synchronize()
    return out, stats


CASES = [
    # (Ci, Co, (Di,Hi,Wi), k, s, p, N)
    (1, 8, (16, 28, 28), (2, 2, 2), (1, 2, 2), (0, 1, 1), 3),
    (8, 16, (15, 15, 15), (2, 2, 2), (1, 2, 2), (0, 1, 1), 3),
    (64, 128, (15, 15, 15), (2, 2, 2), (1, 2, 2), (0, 1, 1), 2),   # full-width MNIST video-D layer 1
    (16, 1, (12, 3, 3), (2, 2, 2), (1, 1, 1), (0, 0, 0), 5),
    (3, 8, (6, 16, 16), (4, 4, 4), (1, 2, 2), (0, 1, 1), 2),
    (32, 64, (1, 8, 8), (1, 4, 4), (1, 2, 2), (0, 1, 1), 9),
    (128, 256, (1, 8, 8), (1, 4, 4), (1, 2, 2), (0, 1, 1), 40),    # 128x128 tile path, several m-blocks
    (1, 8, (1, 28, 28), (1, 1, 1), (1, 1, 1), (0, 2, 2), 4),
    (12, 1, (1, 3, 3), (1, 4, 4), (1, 2, 2), (0, 1, 1), 7),
    (5, 7, (3, 7, 9), (3, 2, 2), (1, 3, 2), (1, 1, 0), 2),
    (64, 128, (1, 32, 32), (1, 4, 4), (1, 2, 2), (0, 1, 1), 6),    # decoder layer 3 at full width (128x64 FAST tile)
    (256, 512, (1, 8, 8), (1, 4, 4), (1, 2, 2), (0, 1, 1), 70),    # decoder layer 1 at full width, XCD-remapped grid
    (256, 512, (13, 5, 5), (2, 2, 2), (1, 2, 2), (0, 1, 1), 8),    # video-D layer 3 at full width (64x64 tile)
    (1, 64, (1, 28, 28), (1, 1, 1), (1, 1, 1), (0, 2, 2), 8),      # MNIST generator head at full width: pointwise streaming kernel (DGRAD)
    (2, 32, (1, 28, 28), (1, 1, 1), (1, 1, 1), (0, 2, 2), 9),      # same kernel, 2 columns, 8 lanes per position
    (1, 64, (16, 28, 28), (2, 2, 2), (1, 2, 2), (0, 1, 1), 3),     # MNIST video-D layer 0 at full width: tiny-K kernel (K = 8), also strided
    (1, 64, (1, 28, 28), (1, 4, 4), (1, 2, 2), (0, 1, 1), 12),     # MNIST image-D layer 0 at full width: tiny-K kernel (K = 16)
    (2, 16, (1, 30, 30), (1, 3, 3), (1, 1, 1), (0, 1, 1), 3),      # tiny-K kernel with 2 channels x 9 taps, 4 lanes per position
    (3, 64, (1, 64, 64), (1, 4, 4), (1, 2, 2), (0, 1, 1), 5),      # UCF generator head at full width (DGRAD, 3 columns, 4 phases x 4 taps): streaming kernel
    (64, 3, (1, 32, 32), (1, 4, 4), (1, 2, 2), (0, 1, 1), 20),     # few-column FPROP with 16 taps (K = 1024) through the same kernel
    (1, 32, (6, 28, 28), (2, 2, 2), (1, 2, 2), (0, 1, 1), 4),      # video-D layer-0 input gradient shape (DGRAD, 1 column, 8 lanes per position)
    # BASELINE configs[3]: the four k=4 Conv3d layers of the UCF video discriminator at full width AND batch 16
    (3, 64, (16, 64, 64), (4, 4, 4), (1, 2, 2), (0, 1, 1), 16),
    (64, 128, (13, 32, 32), (4, 4, 4), (1, 2, 2), (0, 1, 1), 16),
    (128, 256, (10, 16, 16), (4, 4, 4), (1, 2, 2), (0, 1, 1), 16),
    (256, 512, (7, 8, 8), (4, 4, 4), (1, 2, 2), (0, 1, 1), 16),
    (512, 1, (4, 4, 4), (4, 4, 4), (1, 1, 1), (0, 0, 0), 16),
    # their input gradients walk the live temporal taps only (FAST kernel MODE 3): few rows -> K split over the live slabs
    # with depth-major rows; one image -> image-major tiles of whole planes
    (256, 512, (7, 8, 8), (4, 4, 4), (1, 2, 2), (0, 1, 1), 2),
    (64, 128, (13, 32, 32), (4, 4, 4), (1, 2, 2), (0, 1, 1), 1),
    (128, 256, (10, 16, 16), (4, 4, 4), (1, 2, 2), (0, 1, 1), 3),
    # weight gradients through the LDS-patch kernel (few input channels, many taps): a short output row (one partial
    # 32-position segment), a row of one and a half segments with Co = 128, and Co = 32 with a depth tap
    (3, 32, (1, 40, 40), (1, 4, 4), (1, 2, 2), (0, 1, 1), 3),
    (2, 128, (2, 20, 96), (2, 3, 3), (1, 1, 2), (0, 1, 1), 2),
    (4, 32, (5, 18, 66), (3, 3, 3), (1, 2, 2), (1, 0, 1), 2),
    # the patch kernel's tap-validity word holds 5 depth bits: kd = 5 is its last eligible depth (with a padded depth
    # border), kd = 6 must fall back to the generic path (advisor r2: depth bits aliased the row bits there)
    (3, 32, (7, 12, 40), (5, 2, 2), (1, 1, 1), (2, 1, 0), 2),
    (3, 32, (8, 12, 40), (6, 2, 2), (1, 1, 1), (2, 1, 0), 2),
]


@pytest.mark.parametrize("case", CASES)
def test_igemm_fprop_dgrad_wgrad(case):
    """The first FPROP passes `stats`, so conv_patch_plan declines it whatever the shape: it never runs the LDS-patch kernel.
    On the first-layer cases only the second FPROP (x read in place) does, and that one is compared with the first at 1e-5,
    not with a reference; tests/test_gpu_patch_cells.py holds both patch kernels to a float64 reference."""
    Ci, Co, xi, k, s, p, N = case
    yo = tuple(conv_out(xi[a], k[a], s[a], p[a]) for a in range(3))
    g = make_geom(N, Ci, Co, xi, yo, k, s, p)
    gen = torch.Generator().manual_seed(abs(hash(case)) % 997)
    x = torch.randn(N, Ci, *xi, generator=gen)
    w = torch.randn(Co, Ci, *k, generator=gen) * 0.2
    gy = torch.randn(N, Co, *yo, generator=gen)
    xr, wr = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    y_ref = F.conv3d(xr, wr, stride=s, padding=p)
    y_ref.backward(gy)
    # FPROP (channels-last source) + BN partial statistics
    out, stats = igemm(g, L.FPROP, dev(cl(x)), dev(w), (N, *yo, Co), want_stats=True)
    assert rel_err(uncl(out).cpu(), y_ref.detach()) < TOL
    flat = y_ref.detach().permute(0, 2, 3, 4, 1).reshape(-1, Co).double()
    assert rel_err(stats[0].double().sum(1).cpu(), flat.sum(0)) < TOL
    assert rel_err(stats[1].double().sum(1).cpu(), (flat * flat).sum(0)) < TOL
    # FPROP reading the NCDHW tensor in place
    xd = dev(x)
    st = (xd.stride(0), xd.stride(2), xd.stride(3), xd.stride(4), xd.stride(1))
    out2, _ = igemm(g, L.FPROP, xd, dev(w), (N, *yo, Co), strides=st)
    assert rel_err(out2.cpu(), out.cpu()) < 1e-5     # generic strided path vs FAST (possibly split-K) path: summation order differs
    # DGRAD
    gx, _ = igemm(g, L.DGRAD, dev(cl(gy)), dev(w), (N, *xi, Ci))
    assert rel_err(uncl(gx).cpu(), xr.grad) < TOL
    # WGRAD
    lib = L.lib()
    dw = torch.full_like(w, float("nan")).cuda()
    xc, gyc = dev(cl(x)), dev(cl(gy))
    op = L.WgradOp(g=g, act=L.ACT_NONE, xform_on_y=0, splits=0, accumulate=0, x=xc.data_ptr(), y=gyc.data_ptr(),
                   dw=dw.data_ptr())
    work = torch.empty(lib.gode_wgrad_work_size(C.byref(op)), device="cuda")
    op.work = work.data_ptr()
    L.run_one(op, stream())
    assert rel_err(dw.cpu(), wr.grad) < 2e-4


@pytest.mark.parametrize("tile", [1, 2, 3, 4, 6])
def test_igemm_all_tiles_with_fused_bn_relu(tile):
    """Every tile configuration of the GENERIC kernel (24 channels are not whole 32-deep slabs: this geometry never reaches the
    FAST kernels -- tests/test_gpu_igemm_cells.py does), with the previous layer's BatchNorm+ReLU fused into the operand load
    and zero padding applied AFTER the transform."""
    N, Ci, Co, hw = 5, 24, 40, 9
    g = make_geom(N, Ci, Co, (1, hw, hw), (1, 5, 5), (1, 3, 3), (1, 2, 2), (0, 1, 1))
    gen = torch.Generator().manual_seed(tile)
    x = torch.randn(N, Ci, 1, hw, hw, generator=gen)
    w = torch.randn(Co, Ci, 1, 3, 3, generator=gen) * 0.1
    sc, sh = torch.rand(Ci, generator=gen) + 0.5, torch.randn(Ci, generator=gen)
    a = F.relu(x * sc.view(1, -1, 1, 1, 1) + sh.view(1, -1, 1, 1, 1))
    y_ref = F.conv3d(a, w, stride=(1, 2, 2), padding=(0, 1, 1))
    out, _ = igemm(g, L.FPROP, dev(cl(x)), dev(w), (N, 1, 5, 5, Co), scale=dev(sc), shift=dev(sh), act=L.ACT_RELU,
                   tile=tile)
    assert rel_err(uncl(out).cpu(), y_ref) < TOL
    # tanh epilogue on the transposed direction
    gy = torch.randn(N, Co, 1, 5, 5, generator=gen)
    ref = torch.tanh(F.conv_transpose3d(gy, w, stride=(1, 2, 2), padding=(0, 1, 1)))
    gx, _ = igemm(g, L.DGRAD, dev(cl(gy)), dev(w), (N, 1, hw, hw, Ci), epi=L.EPI_TANH, tile=tile)
    assert rel_err(uncl(gx).cpu(), ref) < TOL


def test_wgrad_transform_on_either_side_and_accumulate():
    N, Ci, Co = 6, 8, 16
    g = make_geom(N, Ci, Co, (1, 8, 8), (1, 4, 4), (1, 4, 4), (1, 2, 2), (0, 1, 1))
    gen = torch.Generator().manual_seed(5)
    x = torch.randn(N, Ci, 1, 8, 8, generator=gen)
    y = torch.randn(N, Co, 1, 4, 4, generator=gen)
    lib = L.lib()
    for on_y in (0, 1):
        Cx = Co if on_y else Ci
        sc, sh = torch.rand(Cx, generator=gen) + 0.5, torch.randn(Cx, generator=gen)
        if on_y:
            xa, ya = x, F.leaky_relu(y * sc.view(1, -1, 1, 1, 1) + sh.view(1, -1, 1, 1, 1), 0.2)
        else:
            xa, ya = F.leaky_relu(x * sc.view(1, -1, 1, 1, 1) + sh.view(1, -1, 1, 1, 1), 0.2), y
        wr = torch.zeros(Co, Ci, 1, 4, 4, requires_grad=True)
        F.conv3d(xa, wr, stride=(1, 2, 2), padding=(0, 1, 1)).backward(ya)
        base = torch.randn(Co, Ci, 1, 4, 4, generator=gen)
        dw = base.clone().cuda()
        xc, yc, scd, shd = dev(cl(x)), dev(cl(y)), dev(sc), dev(sh)
        op = L.WgradOp(g=g, act=L.ACT_LRELU, xform_on_y=on_y, splits=3, accumulate=1, x=xc.data_ptr(), y=yc.data_ptr(),
                       scale=scd.data_ptr(), shift=shd.data_ptr(), dw=dw.data_ptr())
        work = torch.empty(lib.gode_wgrad_work_size(C.byref(op)), device="cuda")
        op.work = work.data_ptr()
        L.run_one(op, stream())
        assert rel_err(dw.cpu() - base, wr.grad) < 2e-4


@pytest.mark.parametrize("M,Cc", [(3000, 32), (5000, 128), (700, 512), (257, 8)])
def test_bn_finalize_and_backward(M, Cc):
    gen = torch.Generator().manual_seed(9)
    y = torch.randn(M, Cc, generator=gen) * 2 + 1
    ga = torch.randn(M, Cc, generator=gen)
    bn = torch.nn.BatchNorm1d(Cc)
    with torch.no_grad():
        bn.weight.uniform_(0.5, 1.5, generator=gen); bn.bias.normal_(generator=gen)
    yr = y.clone().requires_grad_(True)
    out = F.leaky_relu(bn(yr), 0.2)
    out.backward(ga)
    # statistics as the GEMM epilogue would deliver them: rows of partial (sum, sumsq)
    rows = 7
    chunks = torch.chunk(y, rows)
    stats = torch.stack([torch.stack([c.sum(0), (c * c).sum(0)]) for c in chunks])        # [rows][2][C]
    stats = stats.permute(1, 2, 0).contiguous().cuda()                                    # the ABI layout [2][C][rows]
    d = {k: torch.empty(Cc, device="cuda") for k in ("mean", "invstd", "scale", "shift")}
    rm, rv, nbt = torch.zeros(Cc).cuda(), torch.ones(Cc).cuda(), torch.zeros((), dtype=torch.int64).cuda()
    gam, bet = dev(bn.weight.detach()), dev(bn.bias.detach())
    op = L.BnFinalizeOp(stats=stats.data_ptr(), rows=rows, ncols=Cc, C=Cc, count=M, gamma=gam.data_ptr(), beta=bet.data_ptr(),
                        running_mean=rm.data_ptr(), running_var=rv.data_ptr(), num_batches_tracked=nbt.data_ptr(),
                        mean=d["mean"].data_ptr(), invstd=d["invstd"].data_ptr(), scale=d["scale"].data_ptr(),
                        shift=d["shift"].data_ptr(), momentum=0.1, eps=1e-5, training=1)
    L.run_one(op, stream())
    assert rel_err(rm.cpu(), bn.running_mean) < TOL and rel_err(rv.cpu(), bn.running_var) < TOL and int(nbt) == 1
    yd, g = dev(y), dev(ga)
    dg, db = torch.empty(Cc, device="cuda"), torch.empty(Cc, device="cuda")
    work = torch.empty(L.lib().gode_bn_bwd_work_size(M, Cc), device="cuda")
    bop = L.BnBwdOp(g=g.data_ptr(), y=yd.data_ptr(), M=M, C=Cc, act=L.ACT_LRELU, gamma=gam.data_ptr(),
                    mean=d["mean"].data_ptr(), invstd=d["invstd"].data_ptr(), scale=d["scale"].data_ptr(),
                    shift=d["shift"].data_ptr(), dgamma=dg.data_ptr(), dbeta=db.data_ptr(), work=work.data_ptr())
    L.run_one(bop, stream())
    assert rel_err(g.cpu(), yr.grad) < TOL
    assert rel_err(dg.cpu(), bn.weight.grad) < TOL and rel_err(db.cpu(), bn.bias.grad) < TOL
    # eval mode: scale/shift from running statistics
    op.training = 0
    L.run_one(op, stream())
    bn.eval()
    ref = bn(y)
    assert rel_err((yd * d["scale"] + d["shift"]).cpu(), ref.detach()) < TOL


@pytest.mark.parametrize("form", ["segments", "two_arrays"])
@pytest.mark.parametrize("order", [0, 1])
def test_bn_finalize_two_batches_of_unequal_size(form, order):
    """gode_bn_finalize_op with two BatchNorm batches of DIFFERENT size in one launch (the joint generator pass: 512 video
    rows + 32 image rows): the partial rows of the two batches given as {begin, split, end} segments of one array (one per
    stride phase) or as two arrays (one GEMM launch per batch); per-batch statistics against torch, the running statistics
    after BOTH momentum updates in the order the reference made its two forward calls, num_batches_tracked += 2."""
    gen = torch.Generator().manual_seed(5 + order)
    Cc, n0, n1, eps, mom = 32, 1536, 96, 1e-5, 0.1
    ys = [torch.randn(n0, Cc, generator=gen) * 2 + 1, torch.randn(n1, Cc, generator=gen) * 0.5 - 2]

    def partials(y, rows):
        return torch.stack([torch.stack([c.sum(0), (c * c).sum(0)]) for c in torch.chunk(y, rows)])     # [rows][2][C]
    gam, bet = (torch.rand(Cc, generator=gen) + 0.5).cuda(), torch.randn(Cc, generator=gen).cuda()
    rm, rv, nbt = torch.zeros(Cc).cuda(), torch.ones(Cc).cuda(), torch.zeros((), dtype=torch.int64).cuda()
    d = {k: torch.empty(2, Cc, device="cuda") for k in ("mean", "invstd", "scale", "shift")}
    op = L.BnFinalizeOp(ncols=Cc, C=Cc, count=n0, count1=n1, gamma=gam.data_ptr(), beta=bet.data_ptr(), running_mean=rm.data_ptr(),
                        running_var=rv.data_ptr(), num_batches_tracked=nbt.data_ptr(), mean=d["mean"].data_ptr(),
                        invstd=d["invstd"].data_ptr(), scale=d["scale"].data_ptr(), shift=d["shift"].data_ptr(), momentum=mom,
                        eps=eps, training=1, groups=2, order=order)
    if form == "segments":       # two "phases": rows [0,6) = 4 of batch 0 + 2 of batch 1, rows [6,11) = 4 + 1
        p0, p1 = partials(ys[0], 8), partials(ys[1], 3)
        allrows = torch.cat([p0[:4], p1[:2], p0[4:], p1[2:]])
        stats = allrows.permute(1, 2, 0).contiguous().cuda()              # the ABI layout [2][C][rows]
        op.stats, op.rows, op.nseg = stats.data_ptr(), 11, 2
        for k, v in enumerate((0, 4, 6, 6, 10, 11)):
            op.seg[k] = v
    else:
        s0 = partials(ys[0], 5).permute(1, 2, 0).contiguous().cuda()
        s1 = partials(ys[1], 2).permute(1, 2, 0).contiguous().cuda()
        op.stats, op.rows, op.stats1, op.rows1 = s0.data_ptr(), 5, s1.data_ptr(), 2
    L.run_one(op, stream())
    torch.cuda.synchronize()
    bn = torch.nn.BatchNorm1d(Cc, eps=eps, momentum=mom)
    with torch.no_grad():
        bn.weight.copy_(gam.cpu()); bn.bias.copy_(bet.cpu())
    for grp in ((1, 0) if order else (0, 1)):
        bn(ys[grp])                                                       # the reference's two forward calls, in its order
    assert rel_err(rm.cpu(), bn.running_mean) < 1e-5 and rel_err(rv.cpu(), bn.running_var) < 1e-5 and int(nbt) == 2
    for grp in range(2):
        yy = ys[grp].double()
        mean, inv = yy.mean(0), 1.0 / torch.sqrt(yy.var(0, unbiased=False) + eps)
        assert rel_err(d["mean"][grp].cpu(), mean.float()) < 1e-5 and rel_err(d["invstd"][grp].cpu(), inv.float()) < 1e-5
        sc = gam.cpu().double() * inv
        assert rel_err(d["scale"][grp].cpu(), sc.float()) < 1e-5
        assert rel_err(d["shift"][grp].cpu(), (bet.cpu().double() - mean * sc).float()) < 1e-5


@pytest.mark.parametrize("M,Cc", [(2 * 700, 64), (2 * 257, 8), (2 * 4096, 256)])
def test_bn_backward_two_groups_in_one_launch_triple_is_bitwise_two_passes(M, Cc):
    """gode_bn_bwd_op.groups == 2 (the paired discriminator pass): rows [0, M/2) and [M/2, M) with their own batch
    statistics in ONE reduce / finalize / apply triple against two single-group ops on the halves (the second adding to
    dgamma / dbeta): bit-identical gradients."""
    gen = torch.Generator().manual_seed(M + Cc)
    y = torch.randn(M, Cc, generator=gen) * 2 + 1
    ga = torch.randn(M, Cc, generator=gen)
    gam = (torch.rand(Cc, generator=gen) + 0.5).cuda()
    h = M // 2
    st = {}
    for k in ("mean", "invstd", "scale", "shift"):
        st[k] = torch.empty(2, Cc, device="cuda")
    for grp in range(2):
        yy = y[grp * h:(grp + 1) * h].double()
        mean, var = yy.mean(0), yy.var(0, unbiased=False)
        inv = 1.0 / torch.sqrt(var + 1e-5)
        st["mean"][grp] = mean.float().cuda(); st["invstd"][grp] = inv.float().cuda()
        st["scale"][grp] = (gam.cpu().double() * inv).float().cuda()
        st["shift"][grp] = (0.3 - mean * gam.cpu().double() * inv).float().cuda()
    lib = L.lib()
    yd = y.cuda()
    work = torch.empty(lib.gode_bn_bwd_work_size(M, Cc), device="cuda")
    base = torch.randn(2, Cc, generator=gen).cuda()
    outs = []
    for mode in ("grouped", "two"):
        g = ga.clone().cuda()
        dg, db = base[0].clone(), base[1].clone()
        if mode == "grouped":
            op = L.BnBwdOp(g=g.data_ptr(), y=yd.data_ptr(), M=M, C=Cc, act=L.ACT_LRELU, gamma=gam.data_ptr(),
                           mean=st["mean"].data_ptr(), invstd=st["invstd"].data_ptr(), scale=st["scale"].data_ptr(),
                           shift=st["shift"].data_ptr(), dgamma=dg.data_ptr(), dbeta=db.data_ptr(), work=work.data_ptr(),
                           accumulate=1, groups=2)
            L.run_one(op, stream())
        else:
            for grp in range(2):
                off = 4 * h * Cc * grp
                op = L.BnBwdOp(g=g.data_ptr() + off, y=yd.data_ptr() + off, M=h, C=Cc, act=L.ACT_LRELU, gamma=gam.data_ptr(),
                               mean=st["mean"][grp].data_ptr(), invstd=st["invstd"][grp].data_ptr(),
                               scale=st["scale"][grp].data_ptr(), shift=st["shift"][grp].data_ptr(), dgamma=dg.data_ptr(),
                               dbeta=db.data_ptr(), work=work.data_ptr(), accumulate=1)
                L.run_one(op, stream())
        torch.cuda.synchronize()
        outs.append((g.clone(), dg.clone(), db.clone()))
    for a, b in zip(*outs):
        assert torch.equal(a, b)


@pytest.mark.parametrize("groups", [0, 2])
def test_bn_backward_with_a_rank1_upstream_gradient_is_bitwise_the_materialised_one(groups):
    """gode_bn_bwd_op.r1_s: the gradient entering the BatchNorm backward is w[c] * s[crop(row)] (the MNIST generator's
    head is a 1x1 convolution to one channel on the centre 28x28 of the 32x32 map, models/mocogan.py:151).  Formed in
    registers it must give the bits of the op run on the materialised [M][C] tensor -- also with two BatchNorm batches of
    unequal size (the joint generator pass)."""
    gen = torch.Generator().manual_seed(91 + groups)
    N, H, W, hh, ww, off, Cc = 5, 32, 32, 28, 28, 2, 64
    M = N * H * W
    y = (torch.randn(M, Cc, generator=gen) * 2 + 1).cuda()
    w = torch.randn(Cc, generator=gen).cuda()
    s = torch.randn(N, hh, ww, generator=gen).cuda()
    full = torch.zeros(N, H, W, device="cuda")
    full[:, off:off + hh, off:off + ww] = s
    ga = (full.reshape(M, 1) * w.reshape(1, Cc)).contiguous()          # one rounding per element, as the head's dgrad kernel
    gam = (torch.rand(Cc, generator=gen) + 0.5).cuda()
    ng = 2 if groups == 2 else 1
    M0 = 3 * H * W if groups == 2 else 0
    st = {k: torch.empty(ng, Cc, device="cuda") for k in ("mean", "invstd", "scale", "shift")}
    bounds = [(0, M0), (M0, M)] if groups == 2 else [(0, M)]
    for grp, (a, b) in enumerate(bounds):
        yy = y[a:b].double()
        mean, var = yy.mean(0), yy.var(0, unbiased=False)
        inv = 1.0 / torch.sqrt(var + 1e-5)
        st["mean"][grp] = mean.float(); st["invstd"][grp] = inv.float()
        st["scale"][grp] = (gam.double() * inv).float()
        st["shift"][grp] = (0.1 - mean * gam.double() * inv).float()
    lib = L.lib()
    work = torch.empty(lib.gode_bn_bwd_work_size(M, Cc), device="cuda")
    outs = []
    for rank1 in (False, True):
        g = ga.clone() if not rank1 else torch.full((M, Cc), float("nan"), device="cuda")     # rank 1: g is write-only
        dg, db = torch.zeros(Cc, device="cuda"), torch.zeros(Cc, device="cuda")
        op = L.BnBwdOp(g=g.data_ptr(), y=y.data_ptr(), M=M, C=Cc, act=L.ACT_RELU, gamma=gam.data_ptr(),
                       mean=st["mean"].data_ptr(), invstd=st["invstd"].data_ptr(), scale=st["scale"].data_ptr(),
                       shift=st["shift"].data_ptr(), dgamma=dg.data_ptr(), dbeta=db.data_ptr(), work=work.data_ptr(),
                       accumulate=0, groups=groups, M0=M0)
        if rank1:
            op.r1_s, op.r1_w = s.data_ptr(), w.data_ptr()
            op.r1_H, op.r1_W, op.r1_h, op.r1_wd, op.r1_off = H, W, hh, ww, off
        L.run_one(op, stream())
        torch.cuda.synchronize()
        outs.append((g.clone(), dg.clone(), db.clone()))
    for a, b in zip(*outs):
        assert torch.isfinite(a).all() and torch.equal(a, b)
    bad = L.BnBwdOp(g=outs[0][0].data_ptr(), y=y.data_ptr(), M=M, C=Cc, act=L.ACT_RELU, gamma=gam.data_ptr(),
                    mean=st["mean"].data_ptr(), invstd=st["invstd"].data_ptr(), scale=st["scale"].data_ptr(),
                    shift=st["shift"].data_ptr(), work=work.data_ptr(), groups=groups, M0=M0, r1_s=s.data_ptr(),
                    r1_w=w.data_ptr(), r1_H=H, r1_W=W + 1, r1_h=hh, r1_wd=ww, r1_off=off)      # M is not a multiple of H * W
    with pytest.raises(RuntimeError):
        L.run_one(bad, stream())


def test_batched_weight_packing_brick_kernel_is_bitwise_the_elementwise_map():
    """Runs of pack ops in a program go through gode_pack_batch_: panels with regular shapes take the LDS brick kernel
    (pack_tile_kernel), the rest the element-wise one; a single gode_pack_weights call always takes the element-wise map
    of conv_geom.h.  Same permutation of the same floats: bit-identical panels, for every layer shape of the three configs
    in both directions (incl. 64 taps = two tap blocks, a 1-channel first layer and the permuted full-K generator input)."""
    from gan_ode_amd.engine import conv_out, make_geom

    def g3(N, Ci, Co, xi, k, s, p):
        return make_geom(N, Ci, Co, xi, tuple(conv_out(xi[a], k[a], s[a], p[a]) for a in range(3)), k, s, p)
    geoms = [make_geom(4, 256, 512, (1, 8, 8), (1, 4, 4), (1, 4, 4), (1, 2, 2), (0, 1, 1)),
             make_geom(4, 64, 128, (1, 32, 32), (1, 16, 16), (1, 4, 4), (1, 2, 2), (0, 1, 1)),
             g3(2, 64, 128, (15, 15, 15), (2, 2, 2), (1, 2, 2), (0, 1, 1)),
             g3(2, 128, 256, (10, 16, 16), (4, 4, 4), (1, 2, 2), (0, 1, 1)),
             g3(2, 3, 64, (16, 64, 64), (4, 4, 4), (1, 2, 2), (0, 1, 1)),
             g3(2, 1, 64, (16, 28, 28), (2, 2, 2), (1, 2, 2), (0, 1, 1)),
             make_geom(4, 48, 80, (1, 8, 8), (1, 4, 4), (1, 4, 4), (1, 2, 2), (0, 1, 1)),
             make_geom(4, 512, 72, (1, 4, 4), (1, 1, 1), (1, 4, 4), (1, 1, 1), (0, 0, 0))]
    lib = L.lib()
    gen = torch.Generator().manual_seed(17)
    ops, keep, refs = [], [], []
    for g in geoms:
        w = torch.randn(g.Co, g.Ci, g.kd, g.kh, g.kw, generator=gen).cuda()
        for d in (L.FPROP, L.DGRAD):
            n = lib.gode_pack_size(C.byref(g), d)
            assert n > 0
            ref = torch.full((n,), float("nan"), device="cuda")
            L.check(lib.gode_pack_weights(C.byref(g), d, w.data_ptr(), ref.data_ptr(), None, 0, stream()))
            out = torch.full((n,), float("nan"), device="cuda")
            ops.append(L.PackOp(g=g, dir=d, co_canon=0, w=w.data_ptr(), wpack=out.data_ptr(), co_perm=None))
            keep.append((w, out)); refs.append(ref)
    L.Program(ops).run(stream())
    torch.cuda.synchronize()
    for (w, out), ref, op in zip(keep, refs, ops):
        assert torch.equal(out, ref), (op.g.key(), op.dir)


@pytest.mark.parametrize("N", [8200, 6200])
def test_operands_beyond_2_gib_take_the_register_staged_kernels(N):
    """The LDS-DMA GEMM loops address their operands as raw buffers (32-bit byte offsets); an operand of 2 GiB or more makes
    gode_igemm / gode_wgrad fall back to the register-staged kernels.  Conv2d 64 -> 64 k3 p1 on 8,200 images of 32x32
    (2.0 GiB in, 2.0 GiB out): the first and the last images against the same op on those images alone (small tensors: the
    DMA kernels), and the weight gradient against the sum of the weight gradients of two halves."""
    lib = L.lib()
    Cc, HW = 64, 32
    g = make_geom(N, Cc, Cc, (1, HW, HW), (1, HW, HW), (1, 3, 3), (1, 1, 1), (0, 1, 1))
    gen = torch.Generator(device="cuda").manual_seed(3)
    x = torch.randn(N, 1, HW, HW, Cc, device="cuda", generator=gen)
    # N = 8200: 2.0 GiB, the fallback; N = 6200: 1.5 GiB, still the DMA kernels, with byte offsets above 2^30
    assert (x.numel() * 4 >= 2 ** 31) == (N == 8200) and x.numel() * 4 > 2 ** 30
    w = torch.randn(Cc, Cc, 1, 3, 3, device="cuda", generator=gen) * 0.05
    wp = torch.empty(lib.gode_pack_size(C.byref(g), L.FPROP), device="cuda")
    L.check(lib.gode_pack_weights(C.byref(g), L.FPROP, w.data_ptr(), wp.data_ptr(), None, 0, stream()))

    def conv(geom, src):
        out = torch.empty(geom.N, 1, HW, HW, Cc, device="cuda")
        op = L.IgemmOp(g=geom, dir=L.FPROP, act=L.ACT_NONE, epilogue=L.EPI_RAW, tile=0, src=src.data_ptr(), wpack=wp.data_ptr(),
                       out=out.data_ptr())
        ws = lib.gode_igemm_work_size(C.byref(op))
        work = torch.empty(max(ws, 1), device="cuda")
        op.work = work.data_ptr()
        L.run_one(op, stream())
        torch.cuda.synchronize()
        return out
    big = conv(g, x)
    g8 = make_geom(8, Cc, Cc, (1, HW, HW), (1, HW, HW), (1, 3, 3), (1, 1, 1), (0, 1, 1))
    for a in (0, N - 8):
        small = conv(g8, x[a:a + 8].contiguous())
        assert float((big[a:a + 8] - small).abs().max()) <= 1e-5 * float(small.abs().max())
    # weight gradient: x beyond 2 GiB -> register-staged kernel; halves (1 GiB each) -> DMA kernel
    y = torch.randn(N, 1, HW, HW, Cc, device="cuda", generator=gen) * 0.1

    def wgrad(geom, xs, ys):
        dw = torch.empty(Cc, Cc, 1, 3, 3, device="cuda")
        op = L.WgradOp(g=geom, act=L.ACT_NONE, xform_on_y=0, splits=0, accumulate=0, x=xs.data_ptr(), y=ys.data_ptr(), dw=dw.data_ptr())
        work = torch.empty(lib.gode_wgrad_work_size(C.byref(op)), device="cuda")
        op.work = work.data_ptr()
        L.run_one(op, stream())
        torch.cuda.synchronize()
        return dw
    whole = wgrad(g, x, y)
    h = N // 2
    gh = make_geom(h, Cc, Cc, (1, HW, HW), (1, HW, HW), (1, 3, 3), (1, 1, 1), (0, 1, 1))
    halves = wgrad(gh, x[:h], y[:h]) + wgrad(gh, x[h:], y[h:])
    assert float((whole - halves).abs().max()) <= 2e-5 * float(halves.abs().max())


@pytest.mark.parametrize("shape", [((6, 10, 10), (4, 4, 4), (1, 2, 2), (0, 1, 1)), ((5, 9, 9), (3, 3, 3), (2, 2, 2), (1, 1, 1)),
                                   ((1, 12, 12), (1, 4, 4), (1, 2, 2), (0, 1, 1))])
def test_thin_input_conv_input_gradient_as_pixel_gemm_plus_3d_col2im(shape):
    """The input gradient of a convolution with <= 4 input channels as ONE GEMM over its output positions (gode_igemm, DGRAD
    of the geometry {N = positions, Di x Hi x Wi = kd x kh x kw, Do = Ho = Wo = 1}) + gode_col2im in its 3-D form, against
    autograd through F.conv3d (the UCF video discriminator's first layer, models/mocogan.py:100, takes this path in the
    generator step)."""
    xin, k, st, pad = shape
    N, Ci, Co = 3, 3, 64
    gen = torch.Generator().manual_seed(sum(xin))
    x = torch.randn(N, Ci, *xin, generator=gen, requires_grad=True)
    w = torch.randn(Co, Ci, *k, generator=gen) * 0.1
    y = F.conv3d(x, w, stride=st, padding=pad)
    gy = torch.randn(y.shape, generator=gen)
    y.backward(gy)
    Do, Ho, Wo = y.shape[2:]
    assert xin[0] == (Do - 1) * st[0] - 2 * pad[0] + k[0] and xin[1] == (Ho - 1) * st[1] - 2 * pad[1] + k[1]
    lib = L.lib()
    pos = N * Do * Ho * Wo
    tg = make_geom(pos, Ci, Co, k, (1, 1, 1), k, (1, 1, 1), (0, 0, 0))
    wd = w.cuda().contiguous()
    wp = torch.empty(lib.gode_pack_size(C.byref(tg), L.DGRAD), device="cuda")
    L.check(lib.gode_pack_weights(C.byref(tg), L.DGRAD, wd.data_ptr(), wp.data_ptr(), None, 0, stream()))
    g0 = gy.permute(0, 2, 3, 4, 1).contiguous().cuda()                       # [N, Do, Ho, Wo, Co]
    taps = k[0] * k[1] * k[2]
    cols = torch.empty(pos * taps * Ci, device="cuda")
    op = L.IgemmOp(g=tg, dir=L.DGRAD, act=L.ACT_NONE, epilogue=L.EPI_RAW, tile=0, src=g0.data_ptr(), wpack=wp.data_ptr(), out=cols.data_ptr())
    ws = lib.gode_igemm_work_size(C.byref(op))
    work = torch.empty(max(ws, 1), device="cuda")
    op.work = work.data_ptr()
    L.run_one(op, stream())
    out = torch.full((N, xin[0], xin[1], xin[2], Ci), float("nan"), device="cuda")
    c2i = L.Col2imOp(cols=cols.data_ptr(), out=out.data_ptr(), N=N, Hi=Ho, Wi=Wo, Ho=xin[1], Wo=xin[2], C=Ci, kh=k[1], kw=k[2],
                     sh=st[1], sw=st[2], ph=pad[1], pw=pad[2], epilogue=L.EPI_RAW, Di=Do, Do=xin[0], kd=k[0], sd=st[0], pd=pad[0])
    L.run_one(c2i, stream())
    torch.cuda.synchronize()
    want = x.grad.permute(0, 2, 3, 4, 1)
    assert rel_err(out.cpu(), want) < 1e-5
    c2i.Do = xin[0] + 1                                                        # not the transposed-convolution relation
    with pytest.raises(RuntimeError):
        L.run_one(c2i, stream())


def _ode_setup(N, T, seed, prenet=True):
    from oracle.mocogan_ref import OdeRhs
    torch.manual_seed(seed)
    f = OdeRhs(16, 16)
    pre = torch.nn.Sequential(torch.nn.Linear(16, 64), torch.nn.LeakyReLU(0.2), torch.nn.Linear(64, 16),
                              torch.nn.LeakyReLU(0.2))
    x = torch.randn(N, 16)
    return f, pre, x


@pytest.mark.parametrize("N,T,sub", [(8, 16, 1), (37, 16, 1), (5, 8, 1), (20, 16, 3)])
def test_ode_forward_and_adjoint(N, T, sub):
    from oracle import ode_ref
    f, pre, x = _ode_setup(N, T, 100 + N)
    t = torch.linspace(0, 1, T).float()
    opts = None if sub == 1 else None
    # oracle; substeps>1 is the build's own extension: compare with the oracle on the refined grid
    if sub == 1:
        grid = t
    else:
        grid = torch.cat([t[j] + (t[j + 1] - t[j]) / sub * torch.arange(sub) for j in range(T - 1)] + [t[-1:]])
    x0 = pre(x)
    sol_all = ode_ref.odeint_adjoint(f, x0, grid, method="rk4")
    sol = sol_all[::sub]
    gsol = torch.randn(T, N, 16, generator=torch.Generator().manual_seed(1))
    content = torch.randn(N, 50, generator=torch.Generator().manual_seed(2))
    if sub == 1:
        sol.backward(gsol)
        ref_grads = [p.grad for p in list(pre.parameters()) + list(f.parameters())]
    # device
    P = [dev(p.detach()) for p in list(pre.parameters()) + list(f.parameters())]
    op = L.OdeParams(*[p.data_ptr() for p in P])
    xd, cd = dev(x), dev(content)
    dt = dev(t[1:] - t[:-1])
    z = torch.full((N * T, 72), float("nan"), device="cuda")
    traj = torch.empty(N, T, 16, device="cuda")
    fop = L.OdeFwdOp(p=op, x=xd.data_ptr(), content=cd.data_ptr(), dt=dt.data_ptr(), sel_t=None, z=z.data_ptr(),
                     traj=traj.data_ptr(), N=N, T=T, substeps=sub, prenet=1, zcols=72)
    L.run_one(fop, stream())
    zz = z.cpu().view(N, T, 72)
    tol = TOL if sub == 1 else 5e-4   # substeps divide dt in fp32 differently from the refined oracle grid
    assert rel_err(zz[:, :, :16], sol.detach().transpose(0, 1)) < tol
    assert torch.equal(zz[:, :, 16:66], content[:, None, :].expand(N, T, 50))
    assert float(zz[:, :, 66:].abs().max()) == 0.0
    assert rel_err(traj.cpu(), sol.detach().transpose(0, 1)) < tol
    if sub != 1:
        return
    gz = torch.zeros(N * T, 72, device="cuda")
    gz.view(N, T, 72)[:, :, :16] = dev(gsol.transpose(0, 1).contiguous())
    grads = torch.full((L.ODE_NPARAM,), float("nan"), device="cuda")
    work = torch.empty(L.lib().gode_ode_bwd_work_size(N), device="cuda")
    bop = L.OdeBwdOp(p=op, x=xd.data_ptr(), traj=traj.data_ptr(), dt=dt.data_ptr(), sel_t=None, gz=gz.data_ptr(),
                     work=work.data_ptr(), grads=grads.data_ptr(), N=N, T=T, substeps=1, prenet=1, accumulate=0, zcols=72)
    L.run_one(bop, stream())
    g = grads.cpu()
    off = 0
    for name, r in zip(("Wa", "ba", "Wb", "bb", "W1", "b1", "W2", "b2"), ref_grads):
        n = r.numel()
        assert rel_err(g[off:off + n].view_as(r), r) < 2e-4, name
        off += n


def test_ode_golden_fixture_and_row_selection():
    """ode_rk4.npz (weights, x, solution and adjoint gradients produced with the reference's ODEFunc class) and the
    sample_images row-selection mode."""
    g = golden("ode_rk4.npz")
    N, T = g["x"].shape[0], g["t"].shape[0]
    names = ["fn.0.weight", "fn.0.bias", "fn.2.weight", "fn.2.bias"]
    P = [torch.from_numpy(g[f"w/{k}"]).cuda() for k in names]
    op = L.OdeParams(None, None, None, None, *[p.data_ptr() for p in P])
    x = torch.from_numpy(g["x"]).cuda()
    tt = torch.from_numpy(g["t"])
    dt = (tt[1:] - tt[:-1]).cuda()
    z = torch.zeros(N * T, 72, device="cuda")
    traj = torch.empty(N, T, 16, device="cuda")
    fop = L.OdeFwdOp(p=op, x=x.data_ptr(), content=None, dt=dt.data_ptr(), sel_t=None, z=z.data_ptr(), traj=traj.data_ptr(),
                     N=N, T=T, substeps=1, prenet=0, zcols=72)
    L.run_one(fop, stream())
    assert rel_err(traj.cpu().transpose(0, 1), g["sol"]) < TOL
    gz = torch.zeros(N * T, 72, device="cuda")
    gz.view(N, T, 72)[:, :, :16] = torch.from_numpy(g["grad_sol"]).transpose(0, 1).cuda()
    grads = torch.full((L.ODE_NPARAM,), 7.5, device="cuda")
    work = torch.empty(L.lib().gode_ode_bwd_work_size(N), device="cuda")
    bop = L.OdeBwdOp(p=op, x=x.data_ptr(), traj=traj.data_ptr(), dt=dt.data_ptr(), sel_t=None, gz=gz.data_ptr(),
                     work=work.data_ptr(), grads=grads.data_ptr(), N=N, T=T, substeps=1, prenet=0, accumulate=0, zcols=72)
    L.run_one(bop, stream())
    gg = grads.cpu()
    for k, o, n in (("fn.0.weight", 2128, 256), ("fn.0.bias", 2384, 16), ("fn.2.weight", 2400, 256), ("fn.2.bias", 2656, 16)):
        assert rel_err(gg[o:o + n].view(g[f"g/{k}"].shape), g[f"g/{k}"]) < 2e-4, k
    assert bool((gg[:2128] == 7.5).all())     # no pre-net: its block of the gradient vector is never touched
    # row selection: row n holds time sel[n]
    sel = torch.tensor([(3 * i) % T for i in range(N)], dtype=torch.int32).cuda()
    z2 = torch.zeros(N, 72, device="cuda")
    fop2 = L.OdeFwdOp(p=op, x=x.data_ptr(), content=None, dt=dt.data_ptr(), sel_t=sel.data_ptr(), z=z2.data_ptr(),
                      traj=traj.data_ptr(), N=N, T=T, substeps=1, prenet=0, zcols=72)
    L.run_one(fop2, stream())
    want = torch.stack([traj[i, int(sel[i])] for i in range(N)])
    assert torch.equal(z2[:, :16], want)


def test_bce_and_adam():
    gen = torch.Generator().manual_seed(4)
    x = torch.randn(32, 11, 2, 2, generator=gen) * 3
    for tgt in (0.0, 1.0):
        xr = x.clone().requires_grad_(True)
        ref = torch.nn.BCEWithLogitsLoss()(xr, torch.full_like(xr, tgt))
        ref.backward()
        xd = x.cuda()
        grad, loss = torch.empty_like(xd), torch.empty((), device="cuda")
        L.run_one(L.BceOp(logits=xd.data_ptr(), grad=grad.data_ptr(), loss=loss.data_ptr(), n=xd.numel(), target=tgt,
                          gscale=1.0, accumulate=0), stream())
        assert rel_err(loss.cpu(), ref.detach()) < 1e-5 and rel_err(grad.cpu(), xr.grad) < 1e-5
    p = torch.randn(1000, generator=gen)
    pr = torch.nn.Parameter(p.clone())
    opt = torch.optim.Adam([pr], lr=2e-4, betas=(0.5, 0.999), weight_decay=1e-5)
    pd, m, v = p.cuda(), torch.zeros(1000).cuda(), torch.zeros(1000).cuda()
    for step in range(1, 4):
        gr = torch.randn(1000, generator=gen)
        pr.grad = gr.clone()
        opt.step()
        gd = gr.cuda()
        L.run_one(L.AdamOp(p=pd.data_ptr(), g=gd.data_ptr(), m=m.data_ptr(), v=v.data_ptr(), n=1000, lr=2e-4, beta1=0.5,
                           beta2=0.999, eps=1e-8, weight_decay=1e-5, gscale=1.0, step=step), stream())
    assert float((pd.cpu() - pr.detach()).abs().max()) < 1e-6


FULL_SIZE = [
    # BASELINE configs[1] layer shapes at full size (R = 512 latent rows / batch 32 clips): (Ci, Co, xi, k, s, p, N)
    (256, 512, (1, 8, 8), (1, 4, 4), (1, 2, 2), (0, 1, 1), 512),      # decoder ConvT 512->256
    (128, 256, (1, 16, 16), (1, 4, 4), (1, 2, 2), (0, 1, 1), 512),    # decoder ConvT 256->128
    (64, 128, (1, 32, 32), (1, 4, 4), (1, 2, 2), (0, 1, 1), 512),     # decoder ConvT 128->64
    (64, 128, (15, 15, 15), (2, 2, 2), (1, 2, 2), (0, 1, 1), 32),     # video-D Conv3d 64->128
    (128, 256, (14, 8, 8), (2, 2, 2), (1, 2, 2), (0, 1, 1), 32),      # video-D Conv3d 128->256
    (256, 512, (13, 5, 5), (2, 2, 2), (1, 2, 2), (0, 1, 1), 32),      # video-D Conv3d 256->512
]


@pytest.mark.parametrize("case", FULL_SIZE)
def test_full_size_adjoint_identities(case):
    """Size-independent property at BASELINE's full sizes (too large for the CPU oracle to redo in seconds): the three
    kernels of one layer are mutually adjoint,  <conv(x; W), y> = <x, conv^T(y; W)> = <W, wgrad(x, y)>,  which ties
    FPROP, DGRAD (all stride phases, XCD-remapped grids, split-K where planned) and WGRAD together at full size."""
    Ci, Co, xi, k, s, p, N = case
    yo = tuple(conv_out(xi[a], k[a], s[a], p[a]) for a in range(3))
    g = make_geom(N, Ci, Co, xi, yo, k, s, p)
    gen = torch.Generator(device="cuda").manual_seed(11)
    x = torch.randn(N, *xi, Ci, device="cuda", generator=gen)            # channels-last
    y = torch.randn(N, *yo, Co, device="cuda", generator=gen)
    w = torch.randn(Co, Ci, *k, device="cuda", generator=gen) * 0.05
    fx, _ = igemm(g, L.FPROP, x, w, (N, *yo, Co))
    dy, _ = igemm(g, L.DGRAD, y, w, (N, *xi, Ci))
    lib = L.lib()
    dw = torch.empty_like(w)
    op = L.WgradOp(g=g, act=L.ACT_NONE, xform_on_y=0, splits=0, accumulate=0, x=x.data_ptr(), y=y.data_ptr(), dw=dw.data_ptr())
    work = torch.empty(lib.gode_wgrad_work_size(C.byref(op)), device="cuda")
    op.work = work.data_ptr()
    L.run_one(op, stream())
    a = float((fx.double() * y.double()).sum())
    b = float((x.double() * dy.double()).sum())
    c = float((w.double() * dw.double()).sum())
    scale = float((fx.double().norm() * y.double().norm()))
    assert abs(a - b) / scale < 1e-6 and abs(a - c) / scale < 1e-6, (a, b, c, scale)
    assert torch.isfinite(fx).all() and torch.isfinite(dy).all() and torch.isfinite(dw).all()


@pytest.mark.parametrize("case", [(64, 3, 32, 32, 4, 2, 1, 6, L.EPI_TANH), (32, 2, 9, 13, 3, 2, 0, 3, L.EPI_RAW),
                                  (32, 4, 8, 8, 4, 1, 2, 2, L.EPI_RAW)])
def test_thin_conv_transpose_as_pixel_gemm_plus_col2im(case):
    """ConvTranspose2d with <= 4 output channels = plain GEMM over the input pixels (DGRAD of the kernel-sized geometry,
    one 'image' per pixel) + gode_col2im; reference: torch's conv_transpose2d on the CPU."""
    Cin, Cout, H, W, k, s, p, N, epi = case
    gen = torch.Generator().manual_seed(5)
    x = torch.randn(N, Cin, H, W, generator=gen)
    w = torch.randn(Cin, Cout, k, k, generator=gen) * 0.2          # ConvTranspose2d layout = conv weight [Co=Cin][Ci=Cout]
    ref = F.conv_transpose2d(x, w, stride=s, padding=p)
    if epi == L.EPI_TANH:
        ref = torch.tanh(ref)
    Ho, Wo = ref.shape[2], ref.shape[3]
    hg = make_geom(N * H * W, Cout, Cin, (1, k, k), (1, 1, 1), (1, k, k), (1, 1, 1), (0, 0, 0))
    xcl = dev(x.permute(0, 2, 3, 1).contiguous())                # [N, H, W, Cin] = [pixels][Cin]
    cols, _ = igemm(hg, L.DGRAD, xcl, dev(w.reshape(Cin, Cout, 1, k, k)), (N * H * W, 1, k, k, Cout))
    out = torch.full((N, Ho, Wo, Cout), float("nan"), device="cuda")
    op = L.Col2imOp(cols=cols.data_ptr(), out=out.data_ptr(), N=N, Hi=H, Wi=W, Ho=Ho, Wo=Wo, C=Cout, kh=k, kw=k, sh=s, sw=s,
                    ph=p, pw=p, epilogue=epi)
    L.run_one(op, stream())
    torch.cuda.synchronize()
    assert rel_err(out.permute(0, 3, 1, 2).cpu(), ref) < TOL


def _random_cases(n, seed):
    """Seeded random conv geometries that steer through the kernel-selection rules: channel counts on and off the vector
    / FAST-path multiples, thin first layers (patch / thin weight-gradient kernels), temporal kernels with stride 1
    (live-tap input gradients), odd extents (uneven stride phases), batches around the split-K thresholds."""
    rng = np.random.RandomState(seed)
    cases = []
    while len(cases) < n:
        three_d = rng.rand() < 0.5
        Ci = int(rng.choice([1, 2, 3, 4, 8, 24, 32, 64, 96]))
        Co = int(rng.choice([1, 3, 4, 8, 32, 64, 128]))
        k = (int(rng.choice([1, 2, 3, 4])) if three_d else 1, int(rng.choice([1, 2, 3, 4])), int(rng.choice([1, 2, 3, 4])))
        s = (1, int(rng.choice([1, 2])), int(rng.choice([1, 2, 3])))
        p = (int(rng.choice([0, 1])) if three_d and k[0] > 1 else 0, int(rng.choice([0, 1, 2])), int(rng.choice([0, 1, 2])))
        xi = (int(rng.randint(k[0], k[0] + 6)) if three_d else 1, int(rng.randint(max(k[1], 3), 40)), int(rng.randint(max(k[2], 3), 40)))
        if any(p[a] >= k[a] and k[a] > 1 for a in range(3)) or any(p[a] > 0 and k[a] == 1 for a in range(3)):
            continue
        yo = tuple(conv_out(xi[a], k[a], s[a], p[a]) for a in range(3))
        if min(yo) < 1:
            continue
        N = int(rng.choice([1, 2, 3, 5, 8, 16]))
        macs = N * yo[0] * yo[1] * yo[2] * Co * Ci * k[0] * k[1] * k[2]
        if macs > float(os.environ.get("GODE_FUZZ_MACS", "3e8")) or N * Ci * xi[0] * xi[1] * xi[2] > 4e6:
            continue
        cases.append((Ci, Co, xi, k, s, p, N))
    return cases


# GODE_FUZZ="n,seed" widens the sweep for a one-off fuzz run on the GPU box
_FUZZ = tuple(int(v) for v in os.environ.get("GODE_FUZZ", "48,20261005").split(","))


@pytest.mark.parametrize("case", _random_cases(*_FUZZ))
def test_igemm_random_geometries(case):
    test_igemm_fprop_dgrad_wgrad(case)
