"""CPU: the discriminators' instance noise (use_noise=True) -- the counter layout of the stream, the constructor refusals,
the state_dict and per-layer flags, the plans it builds and the ABI of the new op kind."""
import ctypes as C
import importlib.util
import math
import os

import numpy as np
import pytest
import torch

import dnoise_ref as R
import wgan_ref as W
from conftest import REPO

import gan_ode_amd as G
import gan_ode_amd._lib as L
from gan_ode_amd.engine import ConvStack


def test_philox_known_answers_and_counter_layout():
    # Random123's Philox4x32-10 known answers (kat_vectors)
    assert [hex(v) for v in W.philox4x32_10(np.zeros(4, np.uint32), np.zeros(2, np.uint32))] == \
        ["0x6627e8d5", "0xe169c58d", "0xbc57ac4c", "0x9b00dbd8"]
    ones = np.full(4, 0xFFFFFFFF, np.uint32)
    assert [hex(v) for v in W.philox4x32_10(ones, ones[:2])] == ["0x408f276d", "0x41c83b0e", "0xa20bc7c6", "0x6d5451fd"]
    # (q low, call, 0x80000000 | stream << 8 | layer, q high), q = e >> 2
    e = np.array([0, 3, 4, (5 << 34) + 9], dtype=np.uint64)
    ctr = R.counters(2, 3, 7, e)
    assert ctr.tolist() == [[0, 7, 0x80000203, 0], [0, 7, 0x80000203, 0], [1, 7, 0x80000203, 0],
                            [((5 << 32) + 2) & 0xFFFFFFFF, 7, 0x80000203, 5]]
    # the tag bit keeps every instance-noise stream away from the parameter-noise streams 0 / 1 / 2
    assert all(R.tag(s, l) >= 0x80000000 for s in (0, 1, 2) for l in range(4))
    # lane e & 3 of the quad's four words, any offset
    seed = 0xDEADBEEF_01234567
    full = R.words(seed, 1, 2, 5, 0, 64)
    assert np.array_equal(R.words(seed, 1, 2, 5, 13, 30), full[13:43])
    k = np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint64)
    quad = W.philox4x32_10(R.counters(1, 2, 5, np.array([16]))[0], k)
    assert np.array_equal(full[16:20], quad)
    # calls, layers and streams draw different words
    assert not np.array_equal(full, R.words(seed, 1, 2, 6, 0, 64))
    assert not np.array_equal(full, R.words(seed, 1, 3, 5, 0, 64))
    assert not np.array_equal(full, R.words(seed, 2, 2, 5, 0, 64))
    z = R.normals(seed, 1, 2, 5, 0, 1 << 16)
    assert abs(z.mean()) < 5 / 256 and abs(z.var() - 1) < 5 * math.sqrt(2 / (1 << 16))


@pytest.mark.parametrize("sigma", [None, -0.1, float("nan"), float("inf"), "x", True])
def test_bad_sigma_is_refused(sigma):
    for ctor in (lambda: G.VideoDiscriminator(1, ksize=2, ndf=8, use_noise=True, noise_sigma=sigma),
                 lambda: G.PatchImageDiscriminator(1, ndf=8, use_noise=True, noise_sigma=sigma),
                 lambda: G.Noise(True, sigma)):
        with pytest.raises(ValueError):
            ctor()


def test_noise_free_default_is_unchanged():
    for d in (G.VideoDiscriminator(1, ksize=2, ndf=8), G.PatchImageDiscriminator(1, ndf=8),
              G.VideoDiscriminator(3, ndf=8, noise_sigma=None)):
        assert d.use_noise is False
        assert not any(s.noise for s in d._specs((2, d.n_channels, 16, 64, 64) if isinstance(d, G.VideoDiscriminator)
                                                 else (2, d.n_channels, 64, 64)))
    assert G.Noise(False, None)(torch.ones(2)).sum() == 2


def test_state_dict_keys_and_plain_attributes():
    torch.manual_seed(123)
    for ctor in (lambda **k: G.VideoDiscriminator(3, ndf=8, **k), lambda **k: G.PatchImageDiscriminator(3, ndf=8, **k)):
        plain, noisy = ctor(), ctor(use_noise=True, noise_sigma=0.1)
        assert list(plain.state_dict()) == list(noisy.state_dict())
        assert [n for n, _ in plain.named_buffers()] == [n for n, _ in noisy.named_buffers()]
        assert noisy.noise_sigma == 0.1 and noisy.noise_seed == 123 and noisy._noise_call == 0
    assert G.VideoDiscriminator(1, use_noise=True, noise_sigma=0.1).noise_stream == 1
    assert G.PatchImageDiscriminator(1, use_noise=True, noise_sigma=0.1).noise_stream == 2


def test_noise_flags_per_layer():
    v = G.VideoDiscriminator(1, ksize=2, ndf=8, use_noise=True, noise_sigma=0.1)
    assert [s.noise for s in v._specs((4, 1, 16, 28, 28))] == [True, True, True, True, False]
    i = G.PatchImageDiscriminator(1, ndf=8, use_noise=True, noise_sigma=0.1)
    assert [s.noise for s in i._specs((4, 1, 28, 28))] == [True, True, True, True]
    # sigma 0 adds exact zeros: the plan stays the noise-free one
    z = G.VideoDiscriminator(1, ksize=2, ndf=8, use_noise=True, noise_sigma=0.0)
    assert not any(s.noise for s in z._specs((4, 1, 16, 28, 28)))


def _program_kinds(dis, shape, groups):
    specs = dis._specs(shape)
    plan = ConvStack(specs, dis._layer_params(), "cpu", owns_input=False, groups=groups)
    prog, patch = plan._build_fwd(True)
    return plan, [op.KIND for op in prog.ops], patch


@pytest.mark.parametrize("groups", [1, 2])
def test_plans_materialise_every_noised_input(groups):
    for noisy in (False, True):
        dis = G.VideoDiscriminator(1, ksize=2, ndf=8, use_noise=noisy, noise_sigma=0.1 if noisy else None)
        plan, kinds, patch = _program_kinds(dis, (4, 1, 16, 28, 28), groups)
        if not noisy:
            assert L.OP_DNOISE not in kinds and plan.x0n is None
            continue
        # layer 0: one gather op per caller tensor ahead of the first GEMM; layers 1-3: one apply op each
        assert kinds[:groups] == [L.OP_DNOISE] * groups and kinds.count(L.OP_DNOISE) == groups + 3
        assert plan.x0n is not None and all(plan.a[l] is not None for l in range(3))   # inputs of layers 1-3
        layers = sorted(op.layer for op in prog_noise_ops(kinds, patch))
        assert layers == [0] * groups + [1, 2, 3]
        for op in prog_noise_ops(kinds, patch):
            if op.layer > 0:
                assert op.M0 == (op.M // 2 if groups == 2 else 0) and op.act == L.ACT_LRELU
                assert (op.scale is None) == (op.layer == 1)        # layer 0 has no BatchNorm


def prog_noise_ops(kinds, patch):
    return [op for op, *_ in patch["noise"]]


def test_dnoise_abi_and_binding_stub():
    lib = L.lib()
    assert lib.gode_version() == 105
    assert C.sizeof(L.DnoiseOp) == lib.gode_sizeof(L.OP_DNOISE) == lib.gode_sizeof(21) == 152
    spec = importlib.util.spec_from_file_location("_stubgen", os.path.join(REPO, "scripts", "gen_binding_stub.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    stub = m.generate()
    assert "class gode_dnoise_op(C.Structure):" in stub and "21: gode_dnoise_op" in stub
    assert stub in open(os.path.join(REPO, "INTEGRATION.md")).read()
