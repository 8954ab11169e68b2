"""CPU: differentiable augmentation (gode_diffaug) -- the host parameter function against the NumPy
restatement, parameter ranges, the tag family, the restatement's backward against autograd, policy parsing, the ABI and
argument errors (all returned before any launch), and the refusals of the Python surface."""
import ctypes as C

import numpy as np
import pytest
import torch

import diffaug_ref as R

import gan_ode_amd as G
import gan_ode_amd._lib as L
import gan_ode_amd.modules as Mod

E_ARG, E_SHAPE = -1, -2
SEEDS = [0, 1, 0xC0FFEE_0123456789, 0xFFFFFFFF_FFFFFFFF]
SIZES = [(28, 28), (64, 64), (5, 7), (7, 5), (1, 1), (2, 3), (8, 8), (12, 33)]


@pytest.mark.parametrize("H,W", SIZES)
def test_host_params_match_the_restatement(H, W):
    for seed in SEEDS:
        for stream, call, g0, n in [(0, 0, 0, 9), (1, 7, 5, 4), (2, 0xFFFFFFFE, (1 << 32) + 3, 6), ((1 << 21) - 1, 1 << 31, (5 << 32) - 2, 5)]:
            ints, unis = G.diffaug_params(n, H, W, seed, stream, call, g0)
            rints, runis = R.params(n, H, W, seed, stream, call, g0)
            assert ints.dtype == np.int32 and ints.shape == (n, 4) and unis.dtype == np.float32 and unis.shape == (n, 3)
            assert np.array_equal(ints, rints), (seed, stream, call, g0)
            assert np.array_equal(unis, runis), (seed, stream, call, g0)


def test_word_to_parameter_rules():
    """The restatement's own rules on hand-made words: U(w) and the umulhi ranges' end points."""
    H, W = 5, 8
    Sx, Sy, cw, ch = R.sizes(H, W)
    assert (Sx, Sy, cw, ch) == (1, 1, 4, 3)
    assert R.sizes(28, 28) == (4, 4, 14, 14) and R.sizes(64, 64) == (8, 8, 32, 32) and R.sizes(1, 1) == (0, 0, 1, 1)
    top = 0xFFFFFFFF
    assert (top * (2 * Sx + 1)) >> 32 == 2 * Sx and (top * (W + 1 - cw % 2)) >> 32 == W and (top * (H + 1 - ch % 2)) >> 32 == H - 1
    assert ((top >> 9) + 0.5) * 2.0 ** -23 < 1.0 and (0 + 0.5) * 2.0 ** -23 > 0.0
    # a sample's parameters depend on g alone: a batch drawn at an offset is the tail of the whole
    a = G.diffaug_params(8, H, W, 3, 1, 2, 0)
    b = G.diffaug_params(5, H, W, 3, 1, 2, 3)
    assert np.array_equal(a[0][3:], b[0]) and np.array_equal(a[1][3:], b[1])


@pytest.mark.parametrize("H,W", SIZES)
def test_parameter_ranges(H, W):
    ints, unis = G.diffaug_params(4096, H, W, 11, 1, 3)
    Sx, Sy, cw, ch = R.sizes(H, W)
    tx, ty, cx, cy = ints.T
    assert tx.min() >= -Sx and tx.max() <= Sx and ty.min() >= -Sy and ty.max() <= Sy
    assert cx.min() >= 0 and cx.max() <= W - cw % 2 and cy.min() >= 0 and cy.max() <= H - ch % 2
    assert unis.min() > 0.0 and unis.max() < 1.0
    # every value of the small ranges occurs (4096 draws of at most 17 values)
    if 2 * Sx + 1 <= 17:
        assert set(tx.tolist()) == set(range(-Sx, Sx + 1))
    if 2 * Sy + 1 <= 17:
        assert set(ty.tolist()) == set(range(-Sy, Sy + 1))
    # the cutout always overlaps the map in a box of at least half its own size per axis
    for row in ints[:256]:
        y0, y1, x0, x1 = R.box(row, H, W)
        assert y1 - y0 >= (ch + 1) // 2 and x1 - x0 >= (cw + 1) // 2
    assert abs(float(unis.mean()) - 0.5) < 5 * (1 / 12 / unis.size) ** 0.5


def test_another_call_stream_or_seed_changes_the_parameters():
    base = G.diffaug_params(64, 28, 28, 5, 1, 0)
    for other in (G.diffaug_params(64, 28, 28, 5, 1, 1), G.diffaug_params(64, 28, 28, 5, 2, 0), G.diffaug_params(64, 28, 28, 6, 1, 0),
                  G.diffaug_params(64, 28, 28, 5, 1, 0, g0=1 << 32)):
        assert not np.any(np.all(base[1] == other[1], axis=1))        # every sample's uniforms moved
        assert not np.array_equal(base[0], other[0])


def test_tag_family_bits():
    for stream in (0, 1, 2, (1 << 21) - 1):
        for field in (0, 1, 255):
            t = R.tag(stream, field)
            assert t & 0x20000000 and not t & 0xC0000000                  # bit 29 set, bits 30 / 31 clear
            assert (t >> 8) & 0x1FFFFF == stream and t & 0xFF == field
    # disjoint from dropout (0x40000000 | layer), the latents (0x60000000 | ...) and the instance noise (0x80000000 | ...)
    assert R.tag((1 << 21) - 1, 255) < 0x40000000 and R.tag(0, 0) >= 1 << 29


@pytest.mark.parametrize("mask", [1, 2, 4, 7, 8, 16, 24, 31])
@pytest.mark.parametrize("shape", [(3, 2, 3, 5, 7), (2, 3, 6, 8), (4, 1, 2, 8, 8)])
def test_restatement_backward_is_autograd_of_its_forward(mask, shape):
    gen = torch.Generator().manual_seed(sum(shape) + mask)
    x = (torch.rand(*shape, generator=gen, dtype=torch.float64) * 2 - 1).requires_grad_(True)
    g = torch.rand(*shape, generator=gen, dtype=torch.float64) * 2 - 1
    ints, unis = R.params(shape[0], shape[-2], shape[-1], 9, 1, mask)
    y = R.forward(x, ints, unis, mask)
    assert y.shape == x.shape
    y.backward(g)
    want = x.grad
    got = R.backward(g, ints, unis, mask)
    assert float((got - want).abs().max()) <= 1e-15 * max(1.0, float(want.abs().max()))


def test_policy_parsing():
    m = Mod.diffaug_mask
    assert m(None) == 0 and m("") == 0 and m(" ") == 0
    assert m("color") == 7 and m("translation") == 8 and m("cutout") == 16
    assert m("color,translation,cutout") == m("cutout, color ,translation") == 31
    assert m("translation,cutout") == m("cutout,translation") == 24
    for bad in ("colour", "color,flip", "Color", 7, ["color"]):
        with pytest.raises(ValueError):
            m(bad)
    with pytest.raises(ValueError):
        G.DiffAugment("brightness")
    aug = G.DiffAugment("cutout,color", seed=5, stream=3)
    assert (aug.mask, aug.seed, aug.stream, aug.call, aug.sample_offset) == (23, 5, 3, 0, 0)
    assert not list(aug.buffers()) and not list(aug.parameters()) and not aug.state_dict()
    torch.manual_seed(1234)
    assert G.DiffAugment("color").seed == 1234
    x = torch.zeros(2, 1, 4, 4)
    off = G.DiffAugment(None)
    assert off(x) is x and G.DiffAugment("")(x) is x and off.call == 0


def _op(**kw):
    d = dict(x=64, out=128, work=256, xs=(C.c_int64 * 5)(48, 16, 4, 1, 16), seed=1, g0=0, N=2, C=1, D=3, H=4, W=4, mask=31,
             backward=0, stream=1, call=0)
    d.update(kw)
    return L.DiffAugOp(**d)


def test_abi_and_argument_errors_before_any_launch():
    lib = L.lib()
    assert L.OP_DIFFAUG == 43 and L.DiffAugOp.KIND == 43 and L.DiffAugOp.FN == "gode_diffaug"
    assert C.sizeof(L.DiffAugOp) == lib.gode_sizeof(43) == 128
    for name in ("gode_diffaug", "gode_diffaug_params", "gode_diffaug_work_size", "gode_diffaug_chunks"):
        assert name in L.EXPORTS
    assert lib.gode_version() == 105
    # (the pointers are never dereferenced: every refusal comes before the launch, and there is no GPU here)
    assert lib.gode_diffaug(None, None) == E_ARG
    assert lib.gode_diffaug(C.byref(L.DiffAugOp()), None) == E_ARG
    for kw in (dict(x=None), dict(out=None), dict(N=0), dict(C=0), dict(D=0), dict(H=0), dict(W=-1), dict(mask=0), dict(mask=32),
               dict(mask=-1), dict(backward=2), dict(backward=-1), dict(stream=-1), dict(stream=1 << 21), dict(g0=-1),
               dict(work=None), dict(work=260), dict(mask=4, work=None)):
        assert lib.gode_diffaug(C.byref(_op(**kw)), None) == E_ARG, kw
    for kw in (dict(D=1 << 11, H=1 << 10, W=1 << 10), dict(C=3, D=1 << 10, H=1 << 10, W=1 << 10),
               dict(N=(1 << 31) - 1, D=16, H=64, W=64)):
        assert lib.gode_diffaug(C.byref(_op(**kw)), None) == E_SHAPE, kw
    kinds = (C.c_int32 * 1)(43)
    ops = (C.c_void_p * 1)(C.addressof(L.DiffAugOp()))
    assert lib.gode_run(kinds, ops, 1, None) == -1000
    ints, unis = np.zeros((2, 4), np.int32), np.zeros((2, 3), np.float32)
    P = lib.gode_diffaug_params
    assert P(ints.ctypes.data, unis.ctypes.data, 2, 1, 0, 0, 0, 4, 4) == 0
    for a in ((None, unis.ctypes.data, 2, 1, 0, 0, 0, 4, 4), (ints.ctypes.data, None, 2, 1, 0, 0, 0, 4, 4),
              (ints.ctypes.data, unis.ctypes.data, -1, 1, 0, 0, 0, 4, 4), (ints.ctypes.data, unis.ctypes.data, 2, 1, 1 << 21, 0, 0, 4, 4),
              (ints.ctypes.data, unis.ctypes.data, 2, 1, 0, 0, -1, 4, 4), (ints.ctypes.data, unis.ctypes.data, 2, 1, 0, 0, 0, 0, 4),
              (ints.ctypes.data, unis.ctypes.data, 2, 1, 0, 0, 0, 4, 0)):
        assert P(*a) == E_ARG, a


def test_work_size_and_chunks():
    lib = L.lib()
    ch = lib.gode_diffaug_chunks
    assert ch(1, 1, 1) == 1 and ch(1, 28, 28) == 1 and ch(1, 32, 32) == 1 and ch(1, 32, 33) == 2
    assert ch(16, 28, 28) == 13 and ch(16, 64, 64) == 64 and ch(64, 128, 128) == 64 and ch(0, 4, 4) == 0
    ws = lib.gode_diffaug_work_size
    for mask in range(1, 32):
        want = 2 * 5 * 13 if mask & 4 else 0                          # floats: one double per (sample, chunk)
        assert ws(5, 16, 28, 28, mask) == want, mask
    assert ws(16, 16, 64, 64, 31) == 2 * 16 * 64 and ws(0, 16, 64, 64, 31) == 0


def test_discriminator_attributes_and_state_dict():
    torch.manual_seed(77)
    for dis, stream in ((G.PatchImageDiscriminator(1, ndf=8), 2), (G.VideoDiscriminator(1, ksize=2, ndf=8), 1),
                        (G.CategoricalVideoDiscriminator(1, 3, ndf=8, ksize=2), 1)):
        assert dis.diffaug is None and dis.diffaug_seed == 77 and dis.diffaug_stream == stream and dis.diffaug_call == 0
        keys = list(dis.state_dict())
        dis.diffaug = "color,cutout"
        assert list(dis.state_dict()) == keys and not any("diffaug" in k for k in keys)


def test_cpu_tensors_are_refused():
    with pytest.raises(RuntimeError, match="MI355X"):
        G.DiffAugment("color")(torch.zeros(2, 1, 8, 8))
    dis = G.PatchImageDiscriminator(1, ndf=8)
    dis.diffaug = "translation"
    with pytest.raises(RuntimeError, match="MI355X"):
        dis(torch.zeros(2, 1, 28, 28))
    assert dis.diffaug_call == 0


def test_trainer_sets_the_policy_and_refuses_graph_capture():
    gen, dv, di = G.build_mnist(ngf=8, ndf=8)
    with pytest.raises(NotImplementedError, match="DiffAugment"):
        G.GanTrainer(gen, dv, di, graph=True, diffaug="color,translation,cutout")
    with pytest.raises(ValueError):
        G.GanTrainer(gen, dv, di, diffaug="color,shear")
    gen, dv, di = G.build_mnist(ngf=8, ndf=8)
    tr = G.GanTrainer(gen, dv, di, diffaug="translation,color", diffaug_seed=99)
    assert dv.diffaug == di.diffaug == "translation,color" and dv.diffaug_seed == di.diffaug_seed == 99
    assert (dv.diffaug_stream, di.diffaug_stream) == (1, 2)
    # shards rewind the call counter and take their own sample offsets, as the instance noise does
    dv.diffaug_call = 7
    tr._noise_shard(dv, 2, 4, 3, tr._calls0(dv))
    assert dv.diffaug_call == 7 and dv._diffaug_sample_offset == 8
    # a policy set on the modules beforehand is refused under graph=True as well; none at all changes nothing
    with pytest.raises(NotImplementedError, match="DiffAugment"):
        G.GanTrainer(gen, dv, di, graph=True)
    gen, dv, di = G.build_mnist(ngf=8, ndf=8)
    G.GanTrainer(gen, dv, di)
    assert dv.diffaug is None and di.diffaug is None
