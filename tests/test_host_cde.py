"""CPU: the Neural-CDE motion latent's host side -- the backward-difference Hermite spline restated in tests/cde_ref.py
against scipy, the time-channel slope table, the seeded construction of VideoGeneratorCDE against the reference's own
class (tests/golden/gen_cde_init.npz, written by scripts/make_cde_golden.py), the drop-in module and its surface, the
refusals, and the C ABI of the two new op kinds."""
import ctypes as C
import inspect

import numpy as np
import pytest
import torch

import cde_ref as R
from conftest import golden

import gan_ode_amd as G
import gan_ode_amd._lib as L
from gan_ode_amd.modules import cde_time_slopes


@pytest.mark.parametrize("T", [16, 5, 2])
def test_spline_restatement_matches_scipy_hermite(T):
    from scipy.interpolate import CubicHermiteSpline
    rng = np.random.default_rng(T)
    knots = np.arange(T, dtype=np.float64)
    for vals in (rng.standard_normal(T), np.linspace(0, 1, T)):
        v = torch.from_numpy(vals)
        d = R.slopes(v)
        dydx = np.concatenate([d[:1].numpy(), d.numpy()])       # slope at knot k = d_{k-1}, d_{-1} := d_0
        ref = CubicHermiteSpline(knots, vals, dydx)
        co = R.hermite_coeffs(d)
        ts = np.concatenate([rng.uniform(0, T - 1, 50), knots])
        for t in ts:
            assert abs(float(R.spline_value(v, co, float(t), T)) - ref(t)) < 1e-12
            assert abs(float(R.spline_deriv(co, float(t), T)) - ref(t, 1)) < 1e-12
        for k in range(1, T - 1):                              # C1 at the inner knots: both intervals agree
            bl, cl, dl = (c[k - 1] for c in co)
            assert abs(float(bl + cl + dl) - float(co[0][k])) < 1e-12
            assert abs(float(v[k - 1] + bl + cl / 2 + dl / 3) - float(v[k])) < 1e-12
    # the linear time channel: exact, constant slope
    tt = torch.linspace(0, 1, T, dtype=torch.float64)
    co = R.hermite_coeffs(R.slopes(tt))
    for t in np.linspace(0, T - 1, 37):
        assert abs(float(R.spline_value(tt, co, float(t), T)) - t / (T - 1)) < 1e-12
        assert abs(float(R.spline_deriv(co, float(t), T)) - 1 / (T - 1)) < 1e-12


@pytest.mark.parametrize("T", [16, 5, 2])
def test_time_slope_table_is_the_fp32_linspace_differences(T):
    tt = torch.linspace(0, 1, T).float()
    want = tt[1:] - tt[:-1]
    got = cde_time_slopes(T)
    assert got.dtype == torch.float32 and torch.equal(got, want)
    assert torch.equal(R.time_slopes(T), want.double())


def test_cde_generator_state_dict_matches_reference_construction():
    ref = golden("gen_cde_init.npz")
    torch.manual_seed(int(ref["seed"]))
    np.random.seed(int(ref["seed"]))
    gen = G.VideoGeneratorCDE(1, 50, 0, 16, 16, ngf=int(ref["ngf"]))
    sd = gen.state_dict()
    keys = [k[2:] for k in ref.files if k.startswith("w/")]
    assert list(sd.keys()) == keys
    for k in keys:
        a, b = sd[k].numpy(), ref["w/" + k]
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), k


def test_cde_drop_in_module_and_surface():
    from models.mocogan_cde import CDEFunc, VideoGeneratorCDE
    assert VideoGeneratorCDE is G.VideoGeneratorCDE and CDEFunc is G.CDEFunc
    sig = inspect.signature(VideoGeneratorCDE.__init__)
    assert list(sig.parameters)[1:] == ["n_channels", "dim_z_content", "dim_z_category", "dim_z_motion", "video_length",
                                        "ode_fn", "cde_input_dim", "dim_hidden", "linear", "ngf"]
    assert sig.parameters["ode_fn"].default is CDEFunc and sig.parameters["cde_input_dim"].default == 2
    assert sig.parameters["dim_hidden"].default is None and sig.parameters["linear"].default is True
    assert sig.parameters["ngf"].default == 64
    for name, args in (("sample_z_m", ["num_samples", "video_len"]), ("sample_z_video", ["num_samples", "video_len"]),
                       ("sample_videos", ["num_samples", "video_len"]), ("sample_images", ["num_samples"])):
        assert list(inspect.signature(getattr(VideoGeneratorCDE, name)).parameters)[1:] == args, name
    torch.manual_seed(0)
    gen = VideoGeneratorCDE(1, 50, 0, 16, 16, ngf=8)
    assert (gen.ode_fn.input_dim, gen.ode_fn.hidden_dim) == (2, 16)
    assert tuple(gen.ode_fn.linear1.weight.shape) == (128, 16) and tuple(gen.ode_fn.linear2.weight.shape) == (32, 128)
    assert tuple(gen.f[0].weight.shape) == (64, 2) and tuple(gen.f[2].weight.shape) == (16, 64)
    assert (gen.cde_rtol, gen.cde_atol) == (1e-4, 1e-6)
    assert gen._gode_graph_capture is False
    _, cde = gen._param_list()
    tail = gen._arena_tail()
    assert len(cde) == 8 and [id(p) for p in tail] == [id(p) for p in cde]
    assert sum(p.numel() for p in cde) == L.CDE_NPARAM == 6304 + 1232
    dead = list(gen.linear.parameters()) + list(gen.recurrent.parameters())
    assert dead and not any(p is q for p in dead for q in tail)
    with pytest.raises(RuntimeError):
        gen.ode_fn(0.0, torch.zeros(1, 16))
    with pytest.raises(RuntimeError):          # CPU module: no fallback
        gen.sample_videos(2)


def test_cde_generator_refusals():
    with pytest.raises(NotImplementedError, match="cde_input_dim"):
        G.VideoGeneratorCDE(1, 50, 0, 16, 16, cde_input_dim=3, ngf=8)
    with pytest.raises(NotImplementedError, match="dim_hidden"):
        G.VideoGeneratorCDE(1, 50, 0, 16, 16, dim_hidden=32, ngf=8)
    G.VideoGeneratorCDE(1, 50, 0, 16, 16, dim_hidden=16, ngf=8)
    with pytest.raises(NotImplementedError):
        G.VideoGeneratorCDE(1, 50, 0, 8, 8, ngf=8)              # dim_z_motion != 16
    with pytest.raises(NotImplementedError, match="ode_fn"):
        G.VideoGeneratorCDE(1, 50, 0, 16, 16, ode_fn=G.ODEFunc, ngf=8)

    class Other(torch.nn.Module):
        def __init__(self, dim, dim_hidden):
            super().__init__()

    with pytest.raises(NotImplementedError, match="ode_fn"):
        G.VideoGeneratorCDE(1, 50, 0, 16, 16, ode_fn=Other, ngf=8)

    class Wide(G.CDEFunc):
        def __init__(self, dim, dim_hidden):
            super().__init__(dim, dim_hidden)
            self.linear1 = torch.nn.Linear(dim_hidden, 64)
            self.linear2 = torch.nn.Linear(64, dim * dim_hidden)

    with pytest.raises(NotImplementedError, match="linear1"):
        G.VideoGeneratorCDE(1, 50, 0, 16, 16, ode_fn=Wide, ngf=8)


def test_cde_video_len_refusal():
    torch.manual_seed(0)
    gen = G.VideoGeneratorCDE(1, 50, 0, 16, 16, ngf=8)
    with pytest.raises(ValueError, match="video_len"):
        gen.sample_z_m(2, video_len=5)
    with pytest.raises(ValueError, match="video_len"):
        gen.sample_videos(2, video_len=8)


def test_cde_trainer_refuses_graph_capture():
    torch.manual_seed(0)
    gen = G.VideoGeneratorCDE(1, 50, 0, 16, 16, ngf=8)
    dv = G.VideoDiscriminator(1, ndf=8)
    di = G.PatchImageDiscriminator(1, ndf=8)
    with pytest.raises(NotImplementedError, match="graph"):
        G.GanTrainer(gen, dv, di, graph=True)


def test_cde_op_sizes_match_ctypes():
    lib = L.lib()
    assert (L.OP_CDE_FWD, L.OP_CDE_BWD) == (16, 17)
    assert lib.gode_sizeof(16) == C.sizeof(L.CdeFwdOp)
    assert lib.gode_sizeof(17) == C.sizeof(L.CdeBwdOp)
    assert L.CDE_NPARAM == 7536
    assert lib.gode_cde_bwd_work_size(33) == 3 * 7536
    assert lib.gode_cde_sync_size(16) == 0 and lib.gode_cde_sync_size(33) > 0
    assert lib.gode_cde_state_size(3, 10) == 3 * 11 * 16


def _valid_ops():
    """ops whose every pointer is a (never dereferenced: the calls below are refused before any launch) non-null dummy"""
    fake = 0x1000
    p = L.CdeParams(*([fake] * 8))
    ptrs = dict(x=fake, tslope=fake, sel_t=None, states=fake, sched=fake, counts=fake)
    fop = L.CdeFwdOp(p=p, content=None, z=fake, sync=fake, N=4, T=16, S_cap=8, zcols=16, rtol=1e-4, atol=1e-6, **ptrs)
    bop = L.CdeBwdOp(p=p, gz=fake, work=fake, grads=fake, N=4, T=16, S_cap=8, accumulate=0, zcols=16, **ptrs)
    return fop, bop


@pytest.mark.parametrize("field,value", [("N", 0), ("N", -1), ("N", 4097), ("T", 1), ("T", 17), ("S_cap", 0),
                                         ("x", None), ("states", None), ("sched", None), ("counts", None),
                                         ("tslope", None), ("zcols", 18)])
def test_cde_ops_reject_bad_arguments(field, value):
    lib = L.lib()
    fop, bop = _valid_ops()
    for op, fn in ((fop, lib.gode_cde_fwd), (bop, lib.gode_cde_bwd)):
        setattr(op, field, value)
        assert fn(C.byref(op), None) == -1, (field, value)


def test_cde_ops_reject_missing_pointers():
    lib = L.lib()
    fop, bop = _valid_ops()
    fop.z = None
    assert lib.gode_cde_fwd(C.byref(fop), None) == -1
    fop, _ = _valid_ops()
    fop.N, fop.sync = 33, None                                   # more than one workgroup needs the exchange words
    assert lib.gode_cde_fwd(C.byref(fop), None) == -1
    fop, _ = _valid_ops()
    fop.p.W2 = None
    assert lib.gode_cde_fwd(C.byref(fop), None) == -1
    fop, _ = _valid_ops()
    fop.rtol = 0.0
    assert lib.gode_cde_fwd(C.byref(fop), None) == -1
    for f in ("gz", "work", "grads"):
        _, bop = _valid_ops()
        setattr(bop, f, None)
        assert lib.gode_cde_bwd(C.byref(bop), None) == -1, f
    assert lib.gode_cde_fwd(None, None) == -1 and lib.gode_cde_bwd(None, None) == -1
