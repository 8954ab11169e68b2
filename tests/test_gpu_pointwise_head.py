"""GPU: the 1x1 ConvTranspose with padding 2 (a crop) through gode_igemm -- the MNIST generator head -- on the pointwise
streaming kernels: 32 and 64 input channels (8 / 16 lanes per position), 1 / 2 / 4 output columns (one column has a kernel
of its own), with and without the previous layer's scale/shift + ReLU on load, raw and tanh epilogue, against float64
torch at the tolerance tests/test_gpu_kernels.py uses for this family (1e-4 relative).

The plan only gives an op to this family from 4096 positions up, so the frame counts are the smallest that reach it
and still leave a partial last position group and a partial last wave: 165 frames of 9x9 -> 5x5 (4125 positions) and 457
frames of 7x7 -> 3x3 (4113 positions; rows shorter than a wave's position group, where the position cannot be stepped
and is decoded per group).  One case is large enough (171 frames of 32x32 -> 28x28) for a wave to run the loop twice."""
import ctypes as C

import pytest
import torch

from conftest import rel_err

import gan_ode_amd._lib as L
from gan_ode_amd.engine import make_geom

pytestmark = pytest.mark.gpu
TOL = 1e-4
POINTWISE = 2      # gode_igemm_family


def _head(cin, cols, h, n, xf, tanh):
    """-> relative error of the op against float64, after asserting that its plan is of the pointwise family"""
    hs = h + 4
    g = make_geom(n, cols, cin, (1, h, h), (1, hs, hs), (1, 1, 1), (1, 1, 1), (0, 2, 2))      # as the conv whose DGRAD it is
    gen = torch.Generator().manual_seed(1000 * cin + 100 * cols + 10 * h + 2 * xf + tanh)
    x = torch.randn(n, hs, hs, cin, generator=gen)                    # channels-last source
    w = torch.randn(cin, cols, 1, 1, 1, generator=gen) * 0.2
    sc, sh = torch.rand(cin, generator=gen) + 0.5, torch.randn(cin, generator=gen)
    xd, wd = x.cuda(), w.cuda()
    lib = L.lib()
    npack = lib.gode_pack_size(C.byref(g), L.DGRAD)
    wp = torch.empty(npack, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    L.check(lib.gode_pack_weights(C.byref(g), L.DGRAD, wd.data_ptr(), wp.data_ptr(), None, 0, stream))
    out = torch.full((n, h, h, cols), float("nan"), device="cuda")
    scd, shd = sc.cuda(), sh.cuda()
    op = L.IgemmOp(g=g, dir=L.DGRAD, act=L.ACT_RELU if xf else L.ACT_NONE, epilogue=L.EPI_TANH if tanh else L.EPI_RAW, tile=0,
                   src=xd.data_ptr(), wpack=wp.data_ptr(), out=out.data_ptr(), scale=scd.data_ptr() if xf else None,
                   shift=shd.data_ptr() if xf else None)
    assert lib.gode_igemm_family(C.byref(op)) == POINTWISE
    L.run_one(op, stream)
    torch.cuda.synchronize()
    a = x.double()
    if xf:
        a = torch.relu(a * sc.double() + sh.double())
    ref = a[:, 2:-2, 2:-2, :] @ w.double().view(cin, cols)            # the crop of a 1x1 transposed convolution
    if tanh:
        ref = torch.tanh(ref)
    got = out.cpu()
    assert bool(torch.isfinite(got).all())
    return rel_err(got, ref)


@pytest.mark.parametrize("tanh", [0, 1])
@pytest.mark.parametrize("xf", [0, 1])
@pytest.mark.parametrize("h,n", [(5, 165), (3, 457)])
@pytest.mark.parametrize("cols", [1, 2, 4])
@pytest.mark.parametrize("cin", [32, 64])
def test_pointwise_head(cin, cols, h, n, xf, tanh):
    err = _head(cin, cols, h, n, xf, tanh)
    print(f"rel err {err:.3e}")
    assert err < TOL


def test_pointwise_head_several_iterations_per_wave():
    err = _head(64, 1, 28, 171, 1, 1)
    print(f"rel err {err:.3e}")
    assert err < TOL
