"""CPU: the Wasserstein-loss / parameter-noise feature's host side -- the Philox restatement against known answers, the
noise_off layout, argument refusals, the defaults building exactly what they built before, and the ABI sizes."""
import ctypes as C

import numpy as np
import pytest
import torch

import gan_ode_amd as G
from gan_ode_amd import _lib as L
import wgan_ref as W


@pytest.mark.parametrize("ctr,key,want", [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
])
def test_philox_known_answers(ctr, key, want):
    got = W.philox4x32_10(np.array([ctr], dtype=np.uint64), np.array(key, dtype=np.uint64))[0]
    assert tuple(int(x) for x in got) == want


def test_uniforms_are_exact_in_fp32_and_open():
    words = np.array([0, 511, 512, 0xFFFFFFFF, 0x80000000, 12345678], dtype=np.uint32)
    u = W.uniforms(words)
    assert np.all(u > 0) and np.all(u < 1)
    assert np.array_equal(u.astype(np.float32).astype(np.float64), u)
    assert u[0] == u[1] == 2.0 ** -24 and u[3] == 1 - 2.0 ** -24


def test_stream_is_a_function_of_the_element_index_only():
    full = W.noise_words(7, 1, 3, 0, 37)
    for off in (1, 2, 5, 13):
        assert np.array_equal(W.noise_words(7, 1, 3, off, 37 - off), full[off:])
    z = W.noise_normals(7, 1, 3, 0, 4096)
    assert abs(z.mean()) < 5 / 64 and abs(z.std() - 1) < 0.05
    assert not np.array_equal(W.noise_words(7, 1, 4, 0, 8), W.noise_words(7, 1, 3, 0, 8))
    assert not np.array_equal(W.noise_words(7, 2, 3, 0, 8), W.noise_words(7, 1, 3, 0, 8))
    assert not np.array_equal(W.noise_words(8, 1, 3, 0, 8), W.noise_words(7, 1, 3, 0, 8))


def test_noise_offsets_cover_every_parameter_including_the_dead_gru_cell():
    torch.manual_seed(0)
    gen, dv, di = G.build_mnist(ngf=8, ndf=8)
    for m in (gen, dv, di):
        ps = list(m.parameters())
        offs = G.FusedAdam.noise_offsets(ps)
        assert offs == W.noise_offsets(ps)
        assert offs[0] == 0 and all(o % 4 == 0 for o in offs)
        for a, b, p in zip(offs, offs[1:], ps):
            assert b - a == (p.numel() + 3) // 4 * 4
    names = [n for n, _ in gen.named_parameters()]
    assert any(n.startswith("recurrent.") for n in names)
    assert len(G.FusedAdam.noise_offsets(list(gen.parameters()))) == len(names)


def test_argument_refusals():
    for kw in (dict(reduction="none"), dict(reduction="max"), dict(override_train_ops=lambda *a: None)):
        with pytest.raises(ValueError):
            G.WassersteinGeneratorLoss(**kw)
    for kw in (dict(reduction="none"), dict(clip=(-0.01, 0.01)), dict(override_train_ops=lambda *a: None)):
        with pytest.raises(ValueError):
            G.WassersteinDiscriminatorLoss(**kw)
    with pytest.raises(RuntimeError):
        G.WassersteinGeneratorLoss()(torch.zeros(4))                     # CPU tensors: no fallback
    with pytest.raises(RuntimeError):
        G.WassersteinDiscriminatorLoss()(torch.zeros(4), torch.zeros(4))
    p = [torch.nn.Parameter(torch.zeros(3))]
    with pytest.raises(ValueError):
        G.FusedAdam(p, noise_sigma=-1e-5)
    with pytest.raises(ValueError):
        G.FusedAdam(p, noise_sigma=float("nan"))
    with pytest.raises(ValueError):
        G.FusedAdam(p, noise_sigma=1e-5, noise_stream=-1)
    with pytest.raises(TypeError):
        G.FusedAdam(p, noise_sigma=1e-5, noise_seed="7")
    gen, dv, di = G.build_mnist(ngf=8, ndf=8)
    with pytest.raises(ValueError):
        G.GanTrainer(gen, dv, di, loss="hinge")


def _hyper(opt):
    return [{k: v for k, v in g.items() if k != "params"} for g in opt.param_groups]


def test_defaults_build_what_they_built_before():
    torch.manual_seed(3)
    gen, dv, di = G.build_mnist(ngf=8, ndf=8)
    plain = G.FusedAdam(gen.parameters())
    assert set(_hyper(plain)[0]) == {"lr", "betas", "eps", "weight_decay", "amsgrad", "maximize", "foreach", "capturable",
                                     "differentiable", "fused", "decoupled_weight_decay"}
    assert G.FusedAdam(gen.parameters(), noise_sigma=0.0).state_dict() == plain.state_dict()
    tr = G.GanTrainer(gen, dv, di)
    assert tr.loss == "bce" and tr.param_noise == 0.0 and tr.noise_seed is None
    for o in (tr.gen_opt, tr.vid_opt, tr.img_opt):
        assert _hyper(o) == _hyper(plain)


def test_noisy_trainer_seeds_without_drawing_from_the_cpu_generator():
    torch.manual_seed(11)
    gen, dv, di = G.build_mnist(ngf=8, ndf=8)
    before = torch.get_rng_state().clone()
    tr = G.GanTrainer(gen, dv, di, loss="wasserstein", param_noise=1e-4)
    assert torch.equal(torch.get_rng_state(), before)
    assert tr.loss == "wasserstein" and tr.noise_seed == torch.initial_seed() == 11
    for o, k in ((tr.gen_opt, 0), (tr.vid_opt, 1), (tr.img_opt, 2)):
        g = o.param_groups[0]
        assert (g["noise_sigma"], g["noise_seed"], g["noise_stream"], g["noise_step"]) == (1e-4, 11, k, 0)
    tr2 = G.GanTrainer(gen, dv, di, param_noise=1e-5, noise_seed=2 ** 64 - 5)
    assert tr2.gen_opt.param_groups[0]["noise_seed"] == 2 ** 64 - 5


def test_noise_step_travels_with_the_state_dict():
    p = [torch.nn.Parameter(torch.zeros(5))]
    a = G.FusedAdam(p, noise_sigma=1e-5, noise_seed=4, noise_stream=2)
    a.param_groups[0]["noise_step"] = 9
    b = G.FusedAdam(p, noise_sigma=1e-5, noise_seed=99)
    b.load_state_dict(a.state_dict())
    g = b.param_groups[0]
    assert (g["noise_step"], g["noise_seed"], g["noise_stream"]) == (9, 4, 2)
    b.load_state_dict(torch.optim.Adam(p).state_dict())     # a stock state: the stream starts over
    g = b.param_groups[0]
    assert (g["noise_step"], g["noise_seed"], g["noise_stream"], g["noise_sigma"]) == (0, 99, 0, 1e-5)
    torch.optim.Adam(p).load_state_dict(a.state_dict())     # and the noisy state still loads into stock torch


def test_ctypes_mirror_matches_the_compiled_abi():
    lib = L.lib()
    assert lib.gode_version() == 105
    assert C.sizeof(L.WganOp) == lib.gode_sizeof(L.OP_WGAN) == 64
    assert C.sizeof(L.AdamNoiseTensor) == lib.gode_sizeof(L.REC_ADAM_NOISE) == 48
    assert L.OP_WGAN == 18
    # argument errors are reported, not launched
    assert lib.gode_wgan_logits(C.byref(L.WganOp()), None) < 0
    assert lib.gode_param_noise(None, 4, 0, 0, 1, 0, 1.0, 0, None) < 0
    assert lib.gode_adam_noise_multi(None, 1, 4, 1e-3, 0.5, 0.999, 1e-8, 0.0, 1.0, 1, 0, 0, 1, 1.0, None) < 0
