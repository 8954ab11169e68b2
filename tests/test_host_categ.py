"""Class-conditional MoCoGAN, host side (no GPU): constructor surface, state_dict layout, the latent column map, the RNG
order of the categorical draws against tests/categ_ref.py, the refusals and the trainer's argument validation."""
import inspect

import numpy as np
import pytest
import torch

from conftest import seed_all

import categ_ref as R
import gan_ode_amd as G
from gan_ode_amd import modules as Mod


def _gen(cls, C, ngf=8):
    if cls is G.VideoGenerator:
        return cls(3, 50, C, 16, 16, dim_hidden=16, ngf=ngf)
    return cls(1, 50, C, 16, 16, ngf=ngf)


@pytest.mark.parametrize("cls", [G.VideoGenerator, G.VideoGeneratorMNIST, G.VideoGeneratorMNISTODE])
@pytest.mark.parametrize("C", [1, 6, 30])
def test_generator_state_dict_matches_the_restatement(cls, C):
    gen = _gen(cls, C)
    ref = R.Generator(gen.n_channels, 50, C, 16, 16, dim_hidden=16, ngf=8, mnist=gen.mnist)
    sd, rsd = gen.state_dict(), ref.state_dict()
    assert list(sd.keys()) == list(rsd.keys())
    assert all(tuple(sd[k].shape) == tuple(rsd[k].shape) for k in sd)
    assert gen.main[0].weight.shape[0] == 66 + C and gen.dim_z_category == C
    ref.load_state_dict(sd)            # strict


def test_constructor_signatures_are_the_references():
    # models/mocogan.py:168 -- CategoricalVideoDiscriminator(n_channels, dim_categorical, n_output_neurons=1, use_noise=False,
    # noise_sigma=None); ndf / ksize are trailing keyword extensions
    p = inspect.signature(G.CategoricalVideoDiscriminator.__init__).parameters
    assert list(p)[:6] == ["self", "n_channels", "dim_categorical", "n_output_neurons", "use_noise", "noise_sigma"]
    assert list(p)[6:] == ["ndf", "ksize"]
    assert (p["n_output_neurons"].default, p["use_noise"].default, p["noise_sigma"].default) == (1, False, None)
    p = inspect.signature(G.VideoGeneratorMNISTODE.__init__).parameters
    assert list(p)[:6] == ["self", "n_channels", "dim_z_content", "dim_z_category", "dim_z_motion", "video_length"]
    import models.mocogan as drop_in
    assert drop_in.CategoricalVideoDiscriminator is G.CategoricalVideoDiscriminator
    assert issubclass(G.CategoricalVideoDiscriminator, G.VideoDiscriminator)


@pytest.mark.parametrize("C,n_out", [(1, 1), (4, 1), (6, 1), (30, 1), (5, 2)])
def test_categorical_discriminator_head_and_split(C, n_out):
    d = G.CategoricalVideoDiscriminator(1, C, n_output_neurons=n_out, ndf=8, ksize=2)
    ref = R.CategoricalVideoDisc(1, C, n_output_neurons=n_out, ndf=8, ksize=2)
    assert list(d.state_dict().keys()) == list(ref.state_dict().keys())
    ref.load_state_dict(d.state_dict())
    assert d.main[-1].weight.shape[0] == n_out + C == d.n_output_neurons and d.dim_categorical == C
    h = torch.arange(3 * (n_out + C), dtype=torch.float32).view(3, n_out + C)
    a, b = d.split(h)
    ra, rb = ref.split(h)
    assert a.shape == (3, n_out) and b.shape == (3, C) and torch.equal(a, ra) and torch.equal(b, rb)
    assert a.data_ptr() == h.data_ptr()          # views of the one head buffer
    specs = d._specs((2, 1, 16, 28, 28))
    assert specs[-1].geom.Co == n_out + C


def test_wide_head_limits():
    G.VideoDiscriminator(1, n_output_neurons=31, ndf=8, ksize=2)
    with pytest.raises(NotImplementedError):
        G.VideoDiscriminator(1, n_output_neurons=32, ndf=8, ksize=2)
    with pytest.raises(NotImplementedError):
        G.CategoricalVideoDiscriminator(1, 31, ndf=8, ksize=2)
    with pytest.raises(NotImplementedError):
        G.CategoricalVideoDiscriminator(1, 0, ndf=8, ksize=2)


@pytest.mark.parametrize("C", [0, 1, 6, 30])
def test_latent_column_map(C):
    perm = Mod.latent_co_perm(C)
    assert len(perm) == Mod.Z_COLS == 96
    used, pad = perm[:66 + C], perm[66 + C:]
    assert sorted(used) == list(range(66 + C)) and all(p == -1 for p in pad)
    # [motion 16 | content 50 | one-hot C] -> the reference's rows [content | category | motion]
    assert perm[:16] == [50 + C + i for i in range(16)]
    assert perm[16:66] == list(range(50))
    assert perm[66:66 + C] == [50 + c for c in range(C)]


def test_c31_and_bad_values_are_refused():
    with pytest.raises(NotImplementedError):
        _gen(G.VideoGeneratorMNISTODE, 31)
    with pytest.raises(NotImplementedError):
        _gen(G.VideoGeneratorMNISTODE, -1)


def test_other_generators_still_refuse_categories():
    for make in (lambda: G.VideoGeneratorGRU(3, 50, 1, 16, 16, ngf=8),
                 lambda: G.VideoGeneratorMNISTODERNN(1, 50, 2, 16, 16, ngf=8),
                 lambda: G.VideoGeneratorSDE(1, 50, 2, 16, 16, ngf=8),
                 lambda: G.VideoGeneratorCDE(1, 50, 2, 16, 16, ngf=8)):
        with pytest.raises(NotImplementedError, match="categorical"):
            make()


@pytest.mark.parametrize("C", [1, 6, 30])
def test_sample_z_categ_draw_order_and_values(C):
    gen = _gen(G.VideoGeneratorMNISTODE, C)
    ref = R.Generator(1, 50, C, 16, 16, ngf=8)
    seed_all(7)
    oh, cls = gen.sample_z_categ(5, 3)
    tail = np.random.rand()
    seed_all(7)
    roh, rcls = ref.sample_z_categ(5, 3)
    assert np.random.rand() == tail                       # exactly one randint draw
    assert oh.shape == (15, C) and torch.equal(oh, roh) and np.array_equal(cls, rcls)
    assert isinstance(cls, np.ndarray) and cls.dtype == rcls.dtype


@pytest.mark.parametrize("select", [False, True])
def test_host_draws_follow_the_reference_order(select):
    """content, classes, motion noise (then the row choice of sample_images): the host inputs of a call equal the draws of
    the restatement's sample_z_video under the same seeds, and leave both generators in the same state."""
    C, B, T = 6, 3, 16
    gen = _gen(G.VideoGeneratorMNISTODE, C)
    seed_all(11)
    x, content, sel, cls = gen._host_inputs(select, B, T)
    after = (np.random.rand(), float(torch.rand(1)))
    seed_all(11)
    n = B * T * 2 if select else B
    rc = np.random.normal(0, 1, (n, 50)).astype(np.float32)
    rk = np.random.randint(C, size=n)
    rx = torch.randn(n, 16)
    if select:
        j = np.sort(np.random.choice(n * T, B, replace=False)).astype(np.int64)
        assert np.array_equal(sel.numpy(), (j % T).astype(np.int32))
        rc, rk, rx = rc[j // T], rk[j // T], rx[j // T]
    else:
        assert sel is None
    assert after == (np.random.rand(), float(torch.rand(1)))
    assert torch.equal(content, torch.from_numpy(rc)) and np.array_equal(cls, rk) and torch.equal(x, rx)


def test_unconditional_host_draws_are_unchanged():
    gen = _gen(G.VideoGeneratorMNISTODE, 0)
    seed_all(3)
    out = gen._host_inputs(False, 4, 16)
    assert len(out) == 3
    seed_all(3)
    rc = np.random.normal(0, 1, (4, 50)).astype(np.float32)
    assert torch.equal(out[1], torch.from_numpy(rc)) and torch.equal(out[0], torch.randn(4, 16))
    z, labels = gen.sample_z_categ(4)
    assert z is None and labels.dtype == np.float64 and labels.shape == (4,)


def test_trainer_argument_validation():
    gen = _gen(G.VideoGeneratorMNISTODE, 6)
    di = G.PatchImageDiscriminator(1, ndf=8)
    with pytest.raises(ValueError):
        G.GanTrainer(gen, G.VideoDiscriminator(1, ndf=8, ksize=2), di)
    with pytest.raises(ValueError):
        G.GanTrainer(gen, G.CategoricalVideoDiscriminator(1, 5, ndf=8, ksize=2), di)
    with pytest.raises(ValueError):
        G.GanTrainer(_gen(G.VideoGeneratorMNISTODE, 0), G.CategoricalVideoDiscriminator(1, 6, ndf=8, ksize=2), di)
    with pytest.raises(ValueError):
        G.GanTrainer(gen, G.CategoricalVideoDiscriminator(1, 6, n_output_neurons=2, ndf=8, ksize=2), di)
    dv = G.CategoricalVideoDiscriminator(1, 6, ndf=8, ksize=2)
    with pytest.raises(NotImplementedError):
        G.GanTrainer(gen, dv, di, loss="wasserstein")
    with pytest.raises(NotImplementedError):
        G.GanTrainer(gen, dv, di, graph=True)
    tr = G.GanTrainer(gen, dv, di)
    imgs = [torch.zeros(2, 1, 28, 28)] * 2
    vids = [torch.zeros(2, 16, 1, 28, 28)] * 2
    with pytest.raises(ValueError, match="real_labels"):
        tr.step(imgs, vids)
    with pytest.raises(ValueError, match="real_labels"):
        tr.step(imgs, vids, [torch.zeros(2, dtype=torch.int64)] * 2)        # not on the device
    with pytest.raises(ValueError, match="real_labels"):
        tr.step(imgs, vids, [torch.zeros(2)] * 2)                          # not int64
    plain = G.GanTrainer(_gen(G.VideoGeneratorMNISTODE, 0), G.VideoDiscriminator(1, ndf=8, ksize=2), di)
    with pytest.raises(ValueError, match="unconditional"):
        plain.step(imgs, vids, [torch.zeros(2, dtype=torch.int64)] * 2)


def test_losses_refuse_cpu_tensors():
    x, y = torch.zeros(4, 7), torch.zeros(4, dtype=torch.int64)
    for call in (lambda: G.categorical_cross_entropy(x[:, 1:], y), lambda: G.bce_ce_head(x, 1.0, y),
                 lambda: G.bce_ce_head_pair(x, 1.0, y, torch.zeros(4), 1.0),
                 lambda: G.bce_ce_head_halves(x, 1.0, 0.0, y[:2]), lambda: G.bce_ce_heads(x, 1.0, y, x, 0.0)):
        with pytest.raises(RuntimeError, match="GPU"):
            call()
