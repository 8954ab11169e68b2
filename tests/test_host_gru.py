"""CPU: the GRU (original MoCoGAN) generator's host side -- the drop-in `models.mocogan.VideoGenerator`, its seeded
construction against the reference's own class (tests/golden/gen_gru_tiny.npz, written by scripts/make_gru_golden.py),
its surface and refusals, the C ABI of op kinds 19 / 20, and tests/gru_ref.py's BPTT against torch.autograd."""
import ctypes as C
import inspect

import numpy as np
import pytest
import torch

import gru_ref as R
from conftest import golden

import gan_ode_amd as G
import gan_ode_amd._lib as L


def test_drop_in_import_is_the_gru_generator():
    from models.mocogan import VideoGenerator, VideoDiscriminator, PatchImageDiscriminator
    assert VideoGenerator is G.VideoGeneratorGRU
    assert VideoDiscriminator is G.VideoDiscriminator and PatchImageDiscriminator is G.PatchImageDiscriminator
    sig = inspect.signature(VideoGenerator.__init__)
    assert list(sig.parameters)[1:] == ["n_channels", "dim_z_content", "dim_z_category", "dim_z_motion", "video_length",
                                        "ngf"]
    assert sig.parameters["ngf"].default == 64
    for name, args in (("sample_z_m", ["num_samples", "video_len"]), ("sample_z_video", ["num_samples", "video_len"]),
                       ("sample_z_content", ["num_samples", "video_len"]),
                       ("sample_videos", ["num_samples", "video_len"]), ("sample_images", ["num_samples"])):
        assert list(inspect.signature(getattr(VideoGenerator, name)).parameters)[1:] == args, name


def test_gru_generator_state_dict_matches_reference_construction():
    ref = golden("gen_gru_tiny.npz")
    torch.manual_seed(int(ref["seed"]))
    np.random.seed(int(ref["seed"]))
    from models.mocogan import VideoGenerator
    gen = VideoGenerator(3, 50, 0, 16, 16, ngf=int(ref["ngf"]))
    sd = gen.state_dict()
    keys = [k[2:] for k in ref.files if k.startswith("w/")]
    assert list(sd.keys()) == keys
    assert all(k.startswith(("recurrent.", "main.")) for k in keys)
    for k in keys:
        a, b = sd[k].numpy(), ref["w/" + k]
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), k


def test_gru_generator_parameters_and_arena_tail():
    torch.manual_seed(0)
    gen = G.VideoGeneratorGRU(3, 50, 0, 16, 16, ngf=8)
    assert {n.split(".")[0] for n, _ in gen.named_children()} == {"recurrent", "main"}
    dec, rnn = gen._param_list()
    r = gen.recurrent
    assert [id(p) for p in rnn] == [id(p) for p in (r.weight_ih, r.weight_hh, r.bias_ih, r.bias_hh)]
    assert [id(p) for p in gen._arena_tail()] == [id(p) for p in rnn]
    assert sum(p.numel() for p in rnn) == L.GRU_NPARAM == 1632
    assert len(dec) + len(rnn) == len(list(gen.parameters()))
    assert gen._gode_graph_capture is False and gen._gode_direct_grads is True
    # sample_z_categ keeps the reference's convention
    z, labels = gen.sample_z_categ(3, 16)
    assert z is None and np.array_equal(labels, np.zeros(3))


def test_gru_generator_refusals():
    with pytest.raises(NotImplementedError, match="categorical"):
        G.VideoGeneratorGRU(3, 50, 1, 16, 16, ngf=8)
    with pytest.raises(NotImplementedError, match="dim_z_motion"):
        G.VideoGeneratorGRU(3, 50, 0, 8, 16, ngf=8)
    with pytest.raises(NotImplementedError, match="dim_z_content"):
        G.VideoGeneratorGRU(3, 40, 0, 16, 16, ngf=8)
    torch.manual_seed(0)
    gen = G.VideoGeneratorGRU(3, 50, 0, 16, 16, ngf=8)
    for call in (lambda: gen.sample_videos(2), lambda: gen.sample_images(2), lambda: gen.sample_z_m(2)):
        with pytest.raises(RuntimeError, match="GPU"):          # CPU module: no fallback
            call()
    with pytest.raises(RuntimeError):
        gen(torch.zeros(1))


def test_gru_trainer_refuses_graph_capture():
    torch.manual_seed(0)
    gen = G.VideoGeneratorGRU(3, 50, 0, 16, 16, ngf=8)
    dv = G.VideoDiscriminator(3, ndf=8)
    di = G.PatchImageDiscriminator(3, ndf=8)
    with pytest.raises(NotImplementedError, match="graph"):
        G.GanTrainer(gen, dv, di, graph=True)


def test_gru_op_sizes_match_ctypes():
    lib = L.lib()
    assert (L.OP_GRU_FWD, L.OP_GRU_BWD) == (19, 20)
    assert lib.gode_sizeof(19) == C.sizeof(L.GruFwdOp)
    assert lib.gode_sizeof(20) == C.sizeof(L.GruBwdOp)
    assert lib.gode_version() == 105
    assert lib.gode_gru_bwd_work_size(1) == 1632 and lib.gode_gru_bwd_work_size(32) == 1632
    assert lib.gode_gru_bwd_work_size(33) == 2 * 1632 and lib.gode_gru_bwd_work_size(4096) == 128 * 1632


def _valid_ops():
    """ops whose every pointer is a (never dereferenced: the calls below are refused before any launch) non-null dummy"""
    fake = 0x1000
    p = L.GruParams(*([fake] * 4))
    fop = L.GruFwdOp(p=p, noise=fake, content=None, sel_t=None, z=fake, hs=fake, N=4, T=16, zcols=16)
    bop = L.GruBwdOp(p=p, noise=fake, hs=fake, sel_t=None, gz=fake, work=fake, grads=fake, N=4, T=16, accumulate=0,
                     zcols=16)
    return fop, bop


@pytest.mark.parametrize("field,value", [("N", 0), ("N", -1), ("T", 0), ("noise", None), ("hs", None), ("zcols", 15)])
def test_gru_ops_reject_bad_arguments(field, value):
    lib = L.lib()
    fop, bop = _valid_ops()
    for op, fn in ((fop, lib.gode_gru_fwd), (bop, lib.gode_gru_bwd)):
        if field == "hs" and op is fop:
            continue                                             # the forward's hs is optional
        setattr(op, field, value)
        assert fn(C.byref(op), None) == -1, (field, value)


def test_gru_ops_reject_missing_pointers():
    lib = L.lib()
    fop, _ = _valid_ops()
    fop.z = None
    assert lib.gode_gru_fwd(C.byref(fop), None) == -1
    fop, _ = _valid_ops()
    fop.content, fop.zcols = 0x1000, 64                         # the content broadcast needs zcols >= 68, % 4 == 0
    assert lib.gode_gru_fwd(C.byref(fop), None) == -1
    fop, _ = _valid_ops()
    fop.p.Whh = None
    assert lib.gode_gru_fwd(C.byref(fop), None) == -1
    for f in ("gz", "work", "grads"):
        _, bop = _valid_ops()
        setattr(bop, f, None)
        assert lib.gode_gru_bwd(C.byref(bop), None) == -1, f
    assert lib.gode_gru_fwd(None, None) == -1 and lib.gode_gru_bwd(None, None) == -1
    fop, bop = _valid_ops()
    assert lib.gode_gru_fwd_multi(C.byref(fop), 0, None) == -1 and lib.gode_gru_fwd_multi(C.byref(fop), 9, None) == -1
    assert lib.gode_gru_bwd_multi(C.byref(bop), 0, None) == -1 and lib.gode_gru_bwd_multi(C.byref(bop), 9, None) == -1


def _torch_chain(cell, noise):
    h = noise[0]
    out = []
    for t in range(noise.shape[0] - 1):
        h = cell(noise[t + 1], h)
        out.append(h)
    return torch.stack(out, dim=1)                                # [N, T, 16]: row n*T + t = h_{t+1}


@pytest.mark.parametrize("N,T", [(1, 1), (5, 16), (3, 7)])
def test_gru_ref_matches_torch_autograd(N, T):
    torch.manual_seed(100 + N * T)
    cell = torch.nn.GRUCell(16, 16).double()
    with torch.no_grad():
        for p in cell.parameters():
            p.mul_(3.0)                                            # saturate some gates too
    noise = torch.randn(T + 1, N, 16, dtype=torch.float64)
    g = torch.randn(N, T, 16, dtype=torch.float64)
    out = _torch_chain(cell, noise)
    (out * g).sum().backward()
    W = [cell.weight_ih.detach().numpy(), cell.weight_hh.detach().numpy(), cell.bias_ih.detach().numpy(),
         cell.bias_hh.detach().numpy()]
    hs = R.forward(*W, noise.numpy())
    assert hs.shape == (N, T + 1, 16)
    assert np.abs(hs[:, 0] - noise[0].numpy()).max() == 0.0
    assert np.abs(R.latent_rows(hs) - out.detach().reshape(-1, 16).numpy()).max() < 1e-12
    grads = R.backward(*W, noise.numpy(), hs, g.numpy())
    assert grads.shape == (R.NPARAM,)
    for got, p in zip(R.split(grads), (cell.weight_ih, cell.weight_hh, cell.bias_ih, cell.bias_hh)):
        want = p.grad.numpy()
        assert np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max())


@pytest.mark.parametrize("n,T", [(1, 16), (3, 1), (16, 16), (512, 16)])
def test_gru_noise_draw_is_bitwise_the_reference_call_sequence(n, T):
    """VideoGeneratorGRU draws the [T+1, n, 16] noise stack with one normal_(); the reference makes T+1 calls
    FloatTensor(n, 16).normal_() (models/mocogan.py:297-301) after NumPy's content draw.  Same values, same generator
    state afterwards."""
    torch.manual_seed(0)
    gen = G.VideoGeneratorGRU(3, 50, 0, 16, T, ngf=8)
    torch.manual_seed(9)
    np.random.seed(9)
    content, noise = gen._draw(n, T)
    after = torch.rand(4)
    torch.manual_seed(9)
    np.random.seed(9)
    want_c = np.random.normal(0, 1, (n, 50)).astype(np.float32)
    want = torch.stack([torch.FloatTensor(n, 16).normal_() for _ in range(T + 1)])
    assert np.array_equal(content.numpy(), want_c)
    assert torch.equal(noise, want) and torch.equal(torch.rand(4), after)
    torch.manual_seed(9)
    m = gen._draw_motion(n, T)
    torch.manual_seed(9)
    assert torch.equal(m, torch.stack([torch.FloatTensor(n, 16).normal_() for _ in range(T + 1)]))
