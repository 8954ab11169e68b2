"""CPU: host side of stage 2's CIFAR DCGAN (gan_ode_amd.dcgan): the notebook's class surface with its globals as keyword
arguments, the layer plan handed to ConvStack, refusals (no CPU path), and the distance of the GPU tests' problems from the
ReLU / LeakyReLU kinks."""
import ctypes as C
import inspect

import pytest
import torch
import torch.nn as nn

import dc_ref as R
from gan_ode_amd import _lib as L
from gan_ode_amd import dcgan
from gan_ode_amd.ode_training import FD_H, stage_plan


def test_signatures_keys_shapes_and_same_seed_weights():
    assert list(inspect.signature(dcgan.Generator.__init__).parameters) == ["self", "ngpu", "nz", "ngf", "nc"]
    assert list(inspect.signature(dcgan.Discriminator.__init__).parameters) == ["self", "ngpu", "ndf", "nc"]
    assert [p.default for p in list(inspect.signature(dcgan.Generator.__init__).parameters.values())[2:]] == [128, 64, 3]
    assert [p.default for p in list(inspect.signature(dcgan.Discriminator.__init__).parameters.values())[2:]] == [64, 3]
    assert list(inspect.signature(dcgan.BCEWithLogitsLoss().forward).parameters) == ["input", "target"]
    for nz, w in ((128, 64), (16, 8)):
        # the notebook's order: Generator, its weights_init, Discriminator, its weights_init
        torch.manual_seed(4711)
        G = dcgan.Generator(1, nz=nz, ngf=w)
        G.apply(R.weights_init)
        D = dcgan.Discriminator(1, ndf=w)
        D.apply(R.weights_init)
        gsd, dsd = R.initial_weights(nz, w, w, 4711)
        for mine, rsd in ((G, gsd), (D, dsd)):
            sd = mine.state_dict()
            assert list(sd) == list(rsd)
            for k in sd:
                assert sd[k].shape == rsd[k].shape and torch.equal(sd[k], rsd[k]), k
            assert [n for n, _ in mine.named_parameters()] == [k for k in sd if "running" not in k and "tracked" not in k]
        assert tuple(gsd["project.weight"].shape) == (w * 128, nz, 1, 1) and tuple(gsd["main.9.weight"].shape) == (3, w, 3, 3)
        assert [tuple(gsd[f"main.{i}.weight"].shape) for i in (0, 3, 6)] == [(8 * w, 4 * w, 4, 4), (4 * w, 2 * w, 4, 4), (2 * w, w, 4, 4)]
        assert list(dsd) == list(R.D_CONVS)
        assert [tuple(dsd[k].shape) for k in R.D_CONVS] == [
            (w, 3, 3, 3), (w, w, 4, 4), (2 * w, w, 3, 3), (2 * w, 2 * w, 4, 4), (4 * w, 2 * w, 3, 3), (4 * w, 4 * w, 4, 4),
            (8 * w, 4 * w, 3, 3), (1, 8 * w, 4, 4)]
        assert isinstance(G.project, nn.Conv2d) and isinstance(G.main, nn.Sequential) and isinstance(D.main, nn.Sequential)
        assert [type(m) for m in G.main] == [type(m) for m in R.Generator(1, nz, w).main]
        assert [type(m) for m in D.main] == [type(m) for m in R.Discriminator(1, w).main]
        assert all(m.negative_slope == 0.1 for m in D.main if isinstance(m, nn.LeakyReLU))
        assert not any(True for _ in D.buffers()) and "_pool" not in G.state_dict()


def test_stage2_shim_exports_the_notebook_names():
    from stage2.cifar_gan import BCEWithLogitsLoss, Discriminator, Generator
    assert (Generator, Discriminator, BCEWithLogitsLoss) == (dcgan.Generator, dcgan.Discriminator, dcgan.BCEWithLogitsLoss)
    import gan_ode_amd
    assert gan_ode_amd.dcgan is dcgan and "dcgan" in gan_ode_amd.__all__


def test_constructor_and_shape_validation():
    for bad in (0, 2, None):
        with pytest.raises(ValueError):
            dcgan.Generator(bad)
        with pytest.raises(ValueError):
            dcgan.Discriminator(bad)
    G, D = dcgan.Generator(1, nz=16, ngf=8), dcgan.Discriminator(1, ndf=8)
    for shape in ((2, 3, 64, 64), (2, 3, 28, 28), (2, 1, 32, 32), (2, 3, 32), (0, 3, 32, 32)):
        with pytest.raises(ValueError):
            D(torch.zeros(shape))                       # any other image size: refused before anything runs
    for shape in ((2, 16), (2, 128, 1, 1), (2, 16, 2, 2)):
        with pytest.raises(ValueError):
            G(torch.zeros(shape))


def test_cpu_tensors_and_other_reductions_are_refused():
    G, D = dcgan.Generator(1, nz=16, ngf=8), dcgan.Discriminator(1, ndf=8)
    with pytest.raises(RuntimeError, match="no CPU or PyTorch fallback"):
        G(torch.zeros(2, 16, 1, 1))
    with pytest.raises(RuntimeError, match="no CPU or PyTorch fallback"):
        D(torch.zeros(2, 3, 32, 32))
    crit = dcgan.BCEWithLogitsLoss()
    with pytest.raises(RuntimeError, match="no CPU or PyTorch fallback"):
        crit(torch.zeros(3), torch.ones(3))
    with pytest.raises(ValueError):
        crit(torch.zeros(3, 1), torch.ones(3))              # shapes must agree
    for red in ("sum", "none"):
        with pytest.raises(ValueError):
            dcgan.BCEWithLogitsLoss(reduction=red)
    with pytest.raises(ValueError):
        dcgan.BCEWithLogitsLoss(weight=torch.ones(3))
    with pytest.raises(ValueError):
        dcgan.BCEWithLogitsLoss(pos_weight=torch.ones(3))


def test_layer_plan_of_both_networks():
    """The specs handed to ConvStack: geometry the library accepts, the first product's column permutation, the activation ids."""
    lib = L.lib()
    G, D = dcgan.Generator(1), dcgan.Discriminator(1)
    perm = G._project_perm(torch.device("cpu"))
    assert perm.dtype == torch.int32 and sorted(perm.tolist()) == list(range(8192))
    for h, w, c in ((0, 0, 0), (1, 2, 3), (3, 3, 511), (2, 0, 77)):
        assert int(perm[(h * 4 + w) * 512 + c]) == c * 16 + h * 4 + w          # (h, w, c) column <- row c * 16 + h * 4 + w
    for B in (1, 16, 64):
        gs, ds = G._specs(B), D._specs(B)
        assert [s.fwd_dir for s in gs] == [L.FPROP, L.DGRAD, L.DGRAD, L.DGRAD, L.FPROP]
        assert [(s.act, s.has_bn) for s in gs] == [(L.ACT_NONE, False)] + [(L.ACT_RELU, True)] * 3 + [(L.ACT_NONE, False)]
        assert gs[-1].epilogue == L.EPI_TANH and gs[0].co_perm is not None
        # the first product's output buffer is the first transposed convolution's channels-last input
        assert gs[0].out_dims() == (B, 1, 1, 1, 8192) and gs[1].in_dims() == (B, 1, 4, 4, 512)
        for a, b in zip(gs[1:-1], gs[2:]):
            assert a.out_dims() == b.in_dims()
        assert gs[-1].out_dims() == (B, 1, 32, 32, 3)
        assert [s.act for s in ds] == [L.ACT_LRELU01] * 7 + [L.ACT_NONE] and not any(s.has_bn for s in ds)
        assert ds[0].in_dims() == (B, 1, 32, 32, 3) and ds[-1].out_dims() == (B, 1, 1, 1, 1)
        for a, b in zip(ds[:-1], ds[1:]):
            assert a.out_dims() == b.in_dims()
        for s in gs + ds:
            assert lib.gode_pack_size(C.byref(s.geom), L.FPROP) > 0 and lib.gode_pack_size(C.byref(s.geom), L.DGRAD) > 0
    assert L.ACT_LRELU01 == 6 and L.OP_BCE_T == 36 and C.sizeof(L.BceTOp) == 48


def test_stage_plan_is_untouched():
    assert stage_plan("euler", 0.01, 0.01, True) == [({1: -0.01}, -0.01, 1)]
    assert stage_plan("euler", 0.01, 0.0, False) == [({1: -0.01}, None, 1)]
    assert stage_plan("rk2", 0.02, 0.5, True) == [({1: -0.02}, None, 1), ({1: 0.01, 2: -0.01}, -0.01, 1)]
    lr = 0.03
    assert stage_plan("rk4", lr, 0.1, True) == [
        ({1: -lr / 2}, None, 1), ({1: lr / 2, 2: -lr / 2}, None, 1), ({2: lr / 2, 3: -lr}, None, 2),
        ({1: -lr / 6, 2: -lr / 3, 3: 2 * lr / 3, 4: -lr / 6}, -0.1 * lr, 1)]


def test_invalidate_packs_forgets_the_packed_versions():
    D = dcgan.Discriminator(1, ndf=8)
    D._pool.pack_cache[("ver", 0, L.FPROP)] = (0, 0, 0)
    D._pool.pack_cache[("buf", 0, L.FPROP)] = "kept"
    D.invalidate_packs()
    assert list(D._pool.pack_cache) == [("buf", 0, L.FPROP)]


def test_narrow_problems_stay_clear_of_the_kinks():
    """(a) and the trainer problems: for the committed seeds the fp64 restatement's smallest |ReLU / LeakyReLU input|, over the
    generator's three BatchNorm outputs and every discriminator pass of the problem (the trainer problems: along the whole step),
    exceeds 1e-5 -- no element can change side of a kink between two correct fp32 evaluations."""
    worst = {f"a {w} B={B}": R.a_reference(w, B)[2] for w, B in R.A_CASES}
    worst.update({f"trainer {m}": R.trainer_reference(m)[2] for m in R.TRAINER_SEED})
    worst["penalty"] = R.penalty_reference(FD_H)[2]
    print(worst)
    assert all(v > 1e-5 for v in worst.values()), worst


def test_full_width_problems_are_sign_definite_and_kink_free():
    """(b): every pre-activation of the full-width discriminator has the input's sign and is further than 1e-2 from zero;
    (c): every ReLU input of the full-width generator (BatchNorm with beta = +6) is positive and further than 1e-2 from zero,
    and the rescaled head leaves the tanh unsaturated."""
    for B in R.B_CASES:
        for sign in (1, -1):
            r64, _, kink = R.b_reference(B, sign, False)
            print(f"b B={B} sign={sign}: smallest |pre-activation| {kink:.3e}, |out| <= {float(r64['out'].abs().max()):.3f}")
            assert kink > 1e-2
            assert bool((r64["out"] * sign > 0).all()) and 0.1 < float(r64["out"].abs().max()) < 10
    for B in R.C_CASES:
        r64, _, kink = R.c_reference(B, False)
        print(f"c B={B}: smallest |ReLU input| {kink:.3e}, |out| <= {float(r64['train/out'].abs().max()):.4f}")
        assert kink > 1e-2
        assert float(r64["train/out"].abs().max()) < 0.999
    # the sign: one negative BatchNorm output would have been recorded as a small or large |input| alike, so check it directly
    G = R.Generator(1)
    G.load_state_dict(R.c_weights())
    seen = []
    hooks = [G.main[i].register_forward_hook(lambda m, i, o: seen.append(float(o.min()))) for i in R.G_BNS]
    with torch.no_grad():
        G.double()(R.c_input(3)[0].double())
    for h in hooks:
        h.remove()
    assert len(seen) == 3 and min(seen) > 1e-2, seen
