"""CPU: the Neural-SDE motion latent's host side -- torchsde's fixed-step schedule (sde_grid_arrays), the seeded
construction of VideoGeneratorSDE against the reference's own class (tests/golden/gen_sde_init.npz, written by
scripts/make_sde_golden.py), the refusals, and the C ABI sizes of the two new op kinds."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import golden

import gan_ode_amd as G
import gan_ode_amd._lib as L
from gan_ode_amd.modules import sde_grid_arrays


def _torchsde_loop(T, dt):
    """torchsde 0.2.x BaseSDESolver.integrate (fixed step) + linear_interp, restated: -> step sizes, and per output j
    (prev_t, t, step index) of the interpolation."""
    ts = torch.linspace(0, 1, T).float()
    t = ts[0]
    prev_t = t
    steps, outs = [], [None]
    for out_t in ts[1:]:
        while t < out_t:
            nt = min(t + dt, ts[-1])
            prev_t = t
            steps.append(nt - t)
            t = nt
        outs.append((prev_t, t, out_t, len(steps) - 1))
    return steps, outs


@pytest.mark.parametrize("T,dt", [(16, 2.5e-2), (5, 2.5e-2), (2, 2.5e-2), (16, 0.1), (7, 0.03), (3, 0.5), (1, 2.5e-2)])
def test_sde_grid_matches_torchsde_loop(T, dt):
    g = sde_grid_arrays(T, dt)
    steps, outs = _torchsde_loop(T, dt)
    assert g["S"] == len(steps)
    assert torch.equal(g["dt"], torch.stack(steps) if steps else torch.zeros(0))
    assert torch.equal(g["sqrt_dt"], torch.sqrt(g["dt"]))
    assert int(g["emit_at"][0]) == -1 and float(g["w0"][0]) == 0.0 and float(g["w1"][0]) == 1.0
    for j in range(1, T):
        prev_t, t, out_t, k = outs[j]
        assert int(g["emit_at"][j]) == k
        assert torch.equal(g["w0"][j], (t - out_t) / (t - prev_t))
        assert torch.equal(g["w1"][j], (out_t - prev_t) / (t - prev_t))
    assert (g["dt"] > 0).all()


def test_sde_grid_of_the_reference_call():
    """T = 16, dt = 2.5e-2: 41 steps, the last about 4e-7 long (the fp32 time sum stops at 0.9999996)."""
    g = sde_grid_arrays(16, 2.5e-2)
    assert g["S"] == 41
    assert 0 < float(g["dt"][-1]) < 1e-6
    assert g["emit_at"].tolist() == [-1, 2, 5, 7, 10, 13, 15, 18, 21, 23, 26, 29, 32, 34, 37, 40]
    assert float(g["dt"].sum()) == pytest.approx(1.0, abs=1e-6)


def test_sde_generator_state_dict_matches_reference_construction():
    ref = golden("gen_sde_init.npz")
    torch.manual_seed(int(ref["seed"]))
    np.random.seed(int(ref["seed"]))
    gen = G.VideoGeneratorSDE(1, 50, 0, 16, 16, ngf=int(ref["ngf"]))
    sd = gen.state_dict()
    keys = [k[2:] for k in ref.files if k.startswith("w/")]
    assert list(sd.keys()) == keys
    for k in keys:
        a, b = sd[k].numpy(), ref["w/" + k]
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), k


def test_sde_drop_in_module_and_surface():
    from models.mocogan_sde import SDEFunc, VideoGeneratorSDE
    assert VideoGeneratorSDE is G.VideoGeneratorSDE and SDEFunc is G.SDEFunc
    torch.manual_seed(0)
    gen = VideoGeneratorSDE(1, 50, 0, 16, 16, linear=False, ngf=8)
    assert isinstance(gen.linear, torch.nn.Identity)
    assert gen.ode_fn.noise_type == "diagonal" and gen.ode_fn.sde_type == "ito"
    assert gen.sde_dt == 2.5e-2
    _, sde = gen._param_list()
    assert len(sde) == 8 and [id(p) for p in gen._arena_tail()] == [id(p) for p in sde]
    with pytest.raises(RuntimeError):
        gen.ode_fn.f(0.0, torch.zeros(1, 16))
    with pytest.raises(RuntimeError):
        gen.ode_fn.g(0.0, torch.zeros(1, 16))
    with pytest.raises(RuntimeError):          # CPU module: no fallback
        gen.sample_videos(2)
    gen.sde_dt = 0.1
    assert gen._steps(16) == sde_grid_arrays(16, 0.1)["S"]


def test_sde_generator_refusals():
    with pytest.raises(NotImplementedError):
        G.VideoGeneratorSDE(1, 50, 0, 16, 16, dim_hidden=32, ngf=8)
    with pytest.raises(NotImplementedError):
        G.VideoGeneratorSDE(1, 50, 0, 16, 16, ode_fn=G.ODEFunc, ngf=8)

    class Other(torch.nn.Module):
        def __init__(self, dim, dim_hidden):
            super().__init__()

    with pytest.raises(NotImplementedError):
        G.VideoGeneratorSDE(1, 50, 0, 16, 16, ode_fn=Other, ngf=8)

    class Scalar(G.SDEFunc):
        def __init__(self, dim, dim_hidden):
            super().__init__(dim, dim_hidden)
            self.noise_type = "scalar"

    with pytest.raises(NotImplementedError):
        G.VideoGeneratorSDE(1, 50, 0, 16, 16, ode_fn=Scalar, ngf=8)


def test_sde_trainer_refuses_graph_capture():
    torch.manual_seed(0)
    gen = G.VideoGeneratorSDE(1, 50, 0, 16, 16, ngf=8)
    dv = G.VideoDiscriminator(1, ndf=8)
    di = G.PatchImageDiscriminator(1, ndf=8)
    with pytest.raises(NotImplementedError):
        G.GanTrainer(gen, dv, di, graph=True)


def test_sde_op_sizes_match_ctypes():
    lib = L.lib()
    assert (L.OP_SDE_FWD, L.OP_SDE_BWD) == (14, 15)
    assert lib.gode_sizeof(14) == C.sizeof(L.SdeFwdOp)
    assert lib.gode_sizeof(15) == C.sizeof(L.SdeBwdOp)
    assert L.SDE_NPARAM == 3216
    lib.gode_sde_bwd_work_size.restype = C.c_int64
    assert lib.gode_sde_bwd_work_size(33) == 3 * 3216


def test_sde_ops_reject_bad_arguments():
    lib = L.lib()
    op = L.SdeFwdOp(N=4, T=3, S=2, zcols=96)       # no pointers
    assert lib.gode_sde_fwd(C.byref(op), None) == -1
    bop = L.SdeBwdOp(N=4, T=3, S=2, zcols=96)
    assert lib.gode_sde_bwd(C.byref(bop), None) == -1
