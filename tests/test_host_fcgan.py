"""CPU: host side of stage 2's fully-connected MNIST GAN (gan_ode_amd.fcgan): the notebook's class surface, the dropout
stream's NumPy restatement, the one CPU-generator draw per discriminator forward, refusals (no CPU path), and the distance of
the GPU tests' problems from the LeakyReLU kink."""
import inspect

import numpy as np
import pytest
import torch

import fc_ref as R
from gan_ode_amd import fcgan
from gan_ode_amd.ode_training import FD_H


def test_signatures_keys_shapes_and_same_seed_weights():
    assert list(inspect.signature(fcgan.Generator.__init__).parameters) == ["self", "g_input_dim", "g_output_dim"]
    assert list(inspect.signature(fcgan.Discriminator.__init__).parameters) == ["self", "d_input_dim"]
    assert list(inspect.signature(fcgan.BCELoss().forward).parameters) == ["input", "target"]
    torch.manual_seed(97382)
    G, D = fcgan.Generator(g_input_dim=100, g_output_dim=784), fcgan.Discriminator(784)
    torch.manual_seed(97382)
    rG, rD = R.Generator(100, 784), R.Discriminator(784)
    for mine, ref in ((G, rG), (D, rD)):
        sd, rsd = mine.state_dict(), ref.state_dict()
        assert list(sd) == list(rsd) == [f"fc{i}.{n}" for i in (1, 2, 3, 4) for n in ("weight", "bias")]
        for k in sd:
            assert sd[k].shape == rsd[k].shape and torch.equal(sd[k], rsd[k]), k
        assert [n for n, _ in mine.named_parameters()] == list(sd)
    assert [tuple(G.state_dict()[f"fc{i}.weight"].shape) for i in (1, 2, 3, 4)] == [(256, 100), (512, 256), (1024, 512), (784, 1024)]
    assert [tuple(D.state_dict()[f"fc{i}.weight"].shape) for i in (1, 2, 3, 4)] == [(1024, 784), (512, 1024), (256, 512), (1, 256)]
    assert all(isinstance(getattr(m, f"fc{i}"), torch.nn.Linear) for m in (G, D) for i in (1, 2, 3, 4))


def test_stage2_shim_exports_the_notebook_names():
    from stage2.mnist_gan import BCELoss, Discriminator, Generator
    assert (Generator, Discriminator, BCELoss) == (fcgan.Generator, fcgan.Discriminator, fcgan.BCELoss)


def test_one_cpu_generator_draw_per_discriminator_forward_and_none_for_the_generator(monkeypatch):
    keys = []
    monkeypatch.setattr(fcgan, "_check_input", lambda *a: None)
    monkeypatch.setattr(fcgan._FcNet, "_apply_net", lambda self, x, key, what: keys.append(key))
    G, D = fcgan.Generator(100, 784), fcgan.Discriminator(784)
    torch.manual_seed(11)
    np.random.seed(11)
    np_state = np.random.get_state()
    G(torch.zeros(2, 100))
    assert torch.equal(torch.get_rng_state(), torch.manual_seed(11).get_state()), "the generator consumed host randomness"
    D.eval()
    D(torch.zeros(2, 784))
    D(torch.zeros(2, 784))
    after = torch.get_rng_state()
    torch.manual_seed(11)
    want = [int(torch.randint(0, 2 ** 62, (1,))) for _ in range(2)]
    assert keys == [0] + want and want[0] != want[1]
    assert torch.equal(torch.get_rng_state(), after)
    assert all(np.array_equal(a, b) for a, b in zip(np.random.get_state(), np_state)), "NumPy's generator was touched"
    # the restatement draws at the same point
    rD = R.Discriminator(784)
    torch.manual_seed(11)
    with torch.no_grad():
        rD(torch.zeros(2, 784)), rD(torch.zeros(2, 784))
    assert rD.keys == want and torch.equal(torch.get_rng_state(), after)


def test_cpu_tensors_and_other_reductions_are_refused():
    G, D = fcgan.Generator(100, 784), fcgan.Discriminator(784)
    with pytest.raises(RuntimeError, match="no CPU or PyTorch fallback"):
        G(torch.zeros(2, 100))
    state = torch.get_rng_state()
    with pytest.raises(RuntimeError, match="no CPU or PyTorch fallback"):
        D(torch.zeros(2, 784))
    assert torch.equal(torch.get_rng_state(), state), "a refused forward must not draw a key"
    with pytest.raises(RuntimeError, match="no CPU or PyTorch fallback"):
        fcgan.BCELoss()(torch.full((3, 1), 0.5), torch.ones(3, 1))
    for red in ("sum", "none"):
        with pytest.raises(ValueError):
            fcgan.BCELoss(reduction=red)
    with pytest.raises(ValueError):
        fcgan.BCELoss(weight=torch.ones(3))


def test_philox_known_answers_and_mask_layout():
    """Random123's known-answer vectors for Philox4x32-10, and the element -> (quad, lane) layout of the mask."""
    kat = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 4, (0xffffffff, 0xffffffff), (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for ctr, key, want in kat:
        got = R.philox4x32_10([np.array([c], dtype=np.uint64) for c in ctr], key[0], key[1])[:, 0]
        assert tuple(int(v) for v in got) == want
    key = (0x1234567 << 32) | 0x89abcdef
    full = R.keep_mask(key, 2, 4099)
    assert np.array_equal(R.keep_mask(key, 2, 10), full[:10])             # a prefix does not depend on n
    w = R.philox4x32_10([np.array([7], dtype=np.uint64), [0], [R.DROP_TAG | 2], [0]], key & 0xFFFFFFFF, key >> 32)[:, 0]
    assert np.array_equal(full[28:32], R.uniform23(w) >= R.DROP_P)
    assert not np.array_equal(full, R.keep_mask(key, 1, 4099)) and not np.array_equal(full, R.keep_mask(key + 1, 2, 4099))
    u = R.uniform23(np.array([0, 0xFFFFFFFF], dtype=np.uint32))
    assert u[0] == np.float32(2.0 ** -24) and u[1] == np.float32(1 - 2.0 ** -24)


def test_keep_rate_of_the_numpy_mask():
    n = 100 * 1024
    rate = R.keep_mask(0x2545F4914F6CDD1D, 0, n).mean()
    sigma = (0.21 / n) ** 0.5
    assert abs(rate - 0.7) <= 5 * sigma, rate              # +- 0.0072


def _kinks():
    yield from ((f"{tag} B={B}", R.module_reference(tag, B)[2]) for tag in ("G", "D") for B in R.MODULE_B)
    yield from ((f"trainer {m}", R.trainer_reference(m)[2]) for m in ("euler", "rk2", "rk4"))
    yield "penalty", R.penalty_reference(FD_H)[3]
    yield "adam", R.adam_reference()[1]


def test_gpu_test_problems_stay_clear_of_the_leaky_relu_kink():
    """For the seeds of tests/test_gpu_fcgan.py the fp64 restatement's smallest |LeakyReLU input|, over every forward of the
    problem, exceeds 1e-5: no element can change side of the kink between two correct fp32 evaluations."""
    worst = dict(_kinks())
    print(worst)
    assert all(v > 1e-5 for v in worst.values()), worst


def test_invalidate_packs_forgets_the_cached_weight_packs():
    D = fcgan.Discriminator(784)
    D.__dict__["_packs"] = fcgan._Packs()
    assert "_packs" not in D.state_dict() and not any(True for _ in D.buffers())
    D.invalidate_packs()
    assert "_packs" not in D.__dict__
    D.invalidate_packs()                 # nothing cached: a no-op
