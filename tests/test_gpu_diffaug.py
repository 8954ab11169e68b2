"""GPU: differentiable augmentation (gode_diffaug, DiffAugment, dis.diffaug, GanTrainer(diffaug=...)) against
the restatement of tests/diffaug_ref.py -- the op forward and backward on every mask, shape and input layout, the stream's
properties, the discriminators with a policy, and one trainer iteration against the reference loop."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import diffaug_ref as R
import dnoise_ref as DN
from conftest import assert_weights_after_adam, rel_err, seed_all

import gan_ode_amd as G
import gan_ode_amd._lib as L
from gan_ode_amd.modules import dnoise_normals
from oracle import mocogan_ref as M

pytestmark = pytest.mark.gpu
TOL, GTOL = 1e-4, 5e-4                  # tests/test_gpu_dnoise.py's, for the discriminators behind a policy
MASKS = [1, 2, 4, 7, 8, 16, 24, 31]
SEED, STREAM = 0x5EED_0DD5_1234_ABCD, 1
# (N, C, D, H, W): MNIST clip, MNIST image, UCF clip (a sample spans 64 workgroups), UCF images, odd sizes with both cutout
# parities and C = 2 (the any-C kernel), many samples, one sample
SHAPES = {"mnist_clip": (3, 1, 16, 28, 28), "mnist_img": (4, 1, 1, 28, 28), "ucf_clip": (2, 3, 16, 64, 64),
          "ucf_img": (5, 3, 1, 64, 64), "odd": (3, 2, 3, 5, 7), "many": (70, 1, 1, 8, 8), "one": (1, 3, 2, 9, 6)}
G0 = {"odd": (1 << 32) + 5, "ucf_img": 11}      # global sample offsets (default 0)


def stream():
    return torch.cuda.current_stream().cuda_stream


def _covers_borders(ints, H, W):
    """tx = +-Sx, ty = +-Sy and a cutout clipped at each of the four borders all occur among the samples."""
    Sx, Sy, cw, ch = R.sizes(H, W)
    tx, ty, cx, cy = ints.T
    x0, y0 = cx - cw // 2, cy - ch // 2
    return bool((tx == Sx).any() and (tx == -Sx).any() and (ty == Sy).any() and (ty == -Sy).any() and (x0 < 0).any()
                and (x0 + cw > W).any() and (y0 < 0).any() and (y0 + ch > H).any())


@functools.lru_cache(None)
def _call_for(name):
    """The call index of a case.  For the two border cases: the first call (found on the CPU, through the host parameter
    function) whose parameters reach every border."""
    N, _, _, H, W = SHAPES[name]
    if name not in ("many", "mnist_clip"):
        return 3
    for call in range(200000):
        if _covers_borders(G.diffaug_params(N, H, W, SEED, STREAM, call, G0.get(name, 0))[0], H, W):
            return call
    raise AssertionError("no call covers the borders")


@functools.lru_cache(None)
def _values(name):
    """The case's input and cotangent [N, C, D, H, W], uniform in [-1, 1] (fp32 values, on the CPU)."""
    gen = torch.Generator().manual_seed(len(name) + sum(SHAPES[name]))
    return tuple(torch.rand(*SHAPES[name], generator=gen) * 2 - 1 for _ in range(2))


def _reference(name, mask, backward):
    """(float64 result, float32 result, the float32 run's error) of the restatement; every layout of a case shares it."""
    N, _, _, H, W = SHAPES[name]
    ints, unis = G.diffaug_params(N, H, W, SEED, STREAM, _call_for(name), G0.get(name, 0))
    fn = R.backward if backward else R.forward
    v = _values(name)[1 if backward else 0]
    y64, y32 = fn(v, ints, unis, mask), fn(v, ints, unis, mask, dtype=torch.float32)
    return y64, y32, rel_err(y32, y64)


def _layouts(v):
    """The same [N, C, D, H, W] values on the device in three memory layouts."""
    x = v.cuda()
    return {"contiguous": x.contiguous(),
            "channels_last": x.permute(0, 2, 3, 4, 1).contiguous().permute(0, 4, 1, 2, 3),     # the generator's view
            "transposed": x.transpose(1, 2).contiguous().transpose(1, 2)}                    # [B, T, C, H, W].transpose(1, 2)


def run_op(x, mask, backward, call, g0=0, seed=SEED, stream_id=STREAM, call_dev=None):
    """gode_diffaug on x [N, C, D, H, W] (any strides) with NaN sentinels behind `out` and `work` -> [N, C, D, H, W] view."""
    N, Cc, D, H, W = x.shape
    n = x.numel()
    nwork = L.lib().gode_diffaug_work_size(N, D, H, W, mask)
    assert nwork == (2 * N * L.lib().gode_diffaug_chunks(D, H, W) if mask & 4 else 0)
    out = torch.full((n + 64,), float("nan"), device="cuda")
    work = torch.full((nwork + 16,), float("nan"), device="cuda")
    sg = seed - (1 << 64) if seed >= 1 << 63 else seed
    op = L.DiffAugOp(x=x.data_ptr(), out=out.data_ptr(), work=work.data_ptr(), call_dev=None if call_dev is None else call_dev.data_ptr(),
                     xs=(C.c_int64 * 5)(x.stride(0), x.stride(2), x.stride(3), x.stride(4), x.stride(1)), seed=sg, g0=g0, N=N, C=Cc,
                     D=D, H=H, W=W, mask=mask, backward=backward, stream=stream_id, call=call)
    L.check(L.lib().gode_diffaug(C.byref(op), stream()), "gode_diffaug")
    assert bool(torch.isnan(out[n:]).all()) and bool(torch.isnan(work[nwork:]).all())
    assert not bool(torch.isnan(out[:n]).any())
    if mask & 4:
        assert not bool(torch.isnan(work[:nwork]).any())
    else:
        assert bool(torch.isnan(work).all())                  # masks without contrast never touch work
    return out[:n].view(N, D, H, W, Cc).permute(0, 4, 1, 2, 3)


def test_border_cases_reach_every_border():
    for name in ("many", "mnist_clip"):
        N, _, _, H, W = SHAPES[name]
        ints, _ = G.diffaug_params(N, H, W, SEED, STREAM, _call_for(name), G0.get(name, 0))
        assert _covers_borders(ints, H, W), name


@pytest.mark.parametrize("backward", [0, 1], ids=["fwd", "bwd"])
@pytest.mark.parametrize("mask", MASKS)
@pytest.mark.parametrize("name", list(SHAPES))
def test_op_against_the_restatement(name, mask, backward):
    N, _, _, H, W = SHAPES[name]
    call, g0 = _call_for(name), G0.get(name, 0)
    if name in ("many", "mnist_clip"):
        assert _covers_borders(G.diffaug_params(N, H, W, SEED, STREAM, call, g0)[0], H, W)
    y64, y32, e32 = _reference(name, mask, backward)
    first = None
    for layout, x in _layouts(_values(name)[1 if backward else 0]).items():
        got = run_op(x, mask, backward, call, g0).cpu()
        if mask & ~24 == 0:
            assert torch.equal(got, y32), (name, mask, layout)                  # data movement: the restatement's bits
        else:
            err = rel_err(got, y64)
            print(f"diffaug {name} mask {mask} {'bwd' if backward else 'fwd'} {layout}: kernel {err:.3e}, fp32 restatement {e32:.3e}")
            assert err <= 8 * e32, (name, mask, layout, err, e32)
        if first is None:
            first = got
            assert torch.equal(run_op(x, mask, backward, call, g0).cpu(), got)  # a second identical call: the same bits
        else:
            assert torch.equal(got, first), layout                              # the layout does not enter the values


def test_call_is_read_from_device_memory_when_given():
    x = _layouts(_values("odd")[0])["channels_last"]
    dev = torch.tensor([5], dtype=torch.int32, device="cuda")
    assert torch.equal(run_op(x, 31, 0, 7), run_op(x, 31, 0, 2, call_dev=dev))
    wrap = torch.tensor([-1], dtype=torch.int32, device="cuda")                 # 0xFFFFFFFF + 8 wraps to 7
    assert torch.equal(run_op(x, 31, 0, 7), run_op(x, 31, 0, 8, call_dev=wrap))


# ---- the module and the stream's properties ---------------------------------------------------------------------------
def test_module_forward_and_backward_one_node():
    name = "odd"
    N, _, _, H, W = SHAPES[name]
    v, g = _values(name)
    aug = G.DiffAugment("cutout,color,translation", seed=SEED, stream=STREAM)
    aug.call, aug.sample_offset = _call_for(name), G0[name]
    x = _layouts(v)["transposed"].requires_grad_(True)
    y = aug(x)
    assert y.shape == x.shape and aug.call == _call_for(name) + 1
    assert y.permute(0, 2, 3, 4, 1).is_contiguous()                             # a permuted view of the channels-last result
    assert y.grad_fn is not None and type(y.grad_fn).__name__ == "_DiffAugFnBackward"
    assert torch.equal(y.detach(), run_op(x.detach(), 31, 0, _call_for(name), G0[name]))
    gp = _layouts(g)["channels_last"]
    y.backward(gp)
    assert torch.equal(x.grad, run_op(gp, 31, 1, _call_for(name), G0[name]))
    # 4-D input: an image batch is a clip of one frame
    v4 = _values("ucf_img")[0]
    aug4 = G.DiffAugment("color,translation,cutout", seed=SEED, stream=STREAM)
    aug4.call, aug4.sample_offset = 3, G0["ucf_img"]
    y4 = aug4(v4[:, :, 0].cuda())
    assert y4.shape == (5, 3, 64, 64)
    assert torch.equal(y4.cpu(), run_op(v4.cuda(), 31, 0, 3, G0["ucf_img"]).cpu()[:, :, 0])
    with pytest.raises(RuntimeError):
        aug4(torch.zeros(2, 3, 8, device="cuda"))
    with pytest.raises(RuntimeError):
        aug4(torch.zeros(2, 3, 8, 8, device="cuda", dtype=torch.float64))


def test_a_batch_drawn_in_two_halves_equals_the_whole():
    x = _values("many")[0][:, :, 0].cuda()                                      # [70, 1, 8, 8]
    aug = G.DiffAugment("color,translation,cutout", seed=3, stream=2)
    g0 = (1 << 32) - 30                                                         # the halves straddle 2^32
    aug.sample_offset = g0
    whole = aug(x)
    parts = []
    for lo, hi in ((0, 33), (33, 70)):
        aug.call, aug.sample_offset = 0, g0 + lo
        parts.append(aug(x[lo:hi]))
    assert torch.equal(whole, torch.cat(parts))


def test_another_call_changes_every_sample():
    x = _values("many")[0][:, :, 0].cuda()
    aug = G.DiffAugment("color", seed=3, stream=2)
    a, b = aug(x), aug(x)
    assert aug.call == 2
    assert bool((a != b).flatten(1).any(1).all())
    aug.call = 0
    assert torch.equal(aug(x), a)


def test_mask_zero_returns_the_input_and_launches_nothing():
    x = torch.zeros(2, 1, 8, 8, device="cuda")
    before = L.LAUNCHES
    for policy in (None, "", " , "):
        aug = G.DiffAugment(policy)
        assert aug(x) is x and aug.call == 0
    assert L.LAUNCHES == before


# ---- the discriminators with a policy ---------------------------------------------------------------------------------
VID = [("mnist", lambda **k: G.VideoDiscriminator(1, ksize=2, ndf=8, **k), lambda: M.VideoDisc(1, ksize=2, ndf=8), (4, 16, 1, 28, 28)),
       ("ucf", lambda **k: G.VideoDiscriminator(3, ndf=8, **k), lambda: M.VideoDisc(3, ndf=8), (2, 16, 3, 64, 64))]
IMG = [("mnist", lambda **k: G.PatchImageDiscriminator(1, ndf=8, **k), lambda: M.PatchImageDisc(1, ndf=8), (8, 1, 28, 28)),
       ("ucf", lambda **k: G.PatchImageDiscriminator(3, ndf=8, **k), lambda: M.PatchImageDisc(3, ndf=8), (8, 3, 64, 64))]
IDS = [f"vid_{v[0]}" for v in VID] + [f"img_{v[0]}" for v in IMG]
POLICY = "color,translation,cutout"


def _input(shape, seed):
    x = torch.rand(*shape, generator=torch.Generator().manual_seed(seed))
    return x.transpose(1, 2) if len(shape) == 5 else x       # videos: the [B,T,C,H,W] -> [B,C,T,H,W] view the scripts feed


def _twins(ctor, **kw):
    torch.manual_seed(3)
    a = ctor(**kw).cuda()
    b = ctor(**kw).cuda()
    b.load_state_dict(a.state_dict())
    return a, b


def _fwd_bwd(dis, x, pre=None):
    x = x.clone().cuda().requires_grad_(True)
    out, _ = dis(x if pre is None else pre(x))
    G.bce_with_logits_const(out, 1.0).backward()
    res = [out.detach(), x.grad] + [p.grad for p in dis.parameters()] + [v for k, v in dis.state_dict().items() if "running_" in k]
    for p in dis.parameters():
        p.grad = None
    return res


@pytest.mark.parametrize("tag,ctor,octor,shape", VID + IMG, ids=IDS)
def test_policy_is_bitwise_the_plain_discriminator_behind_the_module(tag, ctor, octor, shape):
    dis, plain = _twins(ctor)
    dis.diffaug, dis.diffaug_seed = POLICY, 41
    aug = G.DiffAugment(POLICY, seed=41, stream=dis.diffaug_stream)
    for it in range(2):                                      # two calls: both counters move on
        got, want = _fwd_bwd(dis, _input(shape, 10 + it)), _fwd_bwd(plain, _input(shape, 10 + it), pre=aug)
        assert dis.diffaug_call == aug.call == it + 1
        assert len(got) == len(want)
        for a, b in zip(got, want):
            assert torch.equal(a, b)
    # and it is no identity
    assert not torch.equal(got[0], _fwd_bwd(plain, _input(shape, 11))[0])


@pytest.mark.parametrize("tag,ctor,octor,shape", VID[:1] + IMG[:1], ids=["vid", "img"])
def test_eval_mode_passes_the_input_unchanged(tag, ctor, octor, shape):
    dis, plain = _twins(ctor)
    dis.diffaug = POLICY
    dis.eval(); plain.eval()
    for a, b in zip(_fwd_bwd(dis, _input(shape, 12)), _fwd_bwd(plain, _input(shape, 12))):
        assert torch.equal(a, b)
    assert dis.diffaug_call == 0


@pytest.mark.parametrize("tag,ctor,octor,shape", VID[:1] + IMG[:1], ids=["vid", "img"])
def test_paired_pass_draws_what_two_forwards_draw(tag, ctor, octor, shape):
    dis, plain = _twins(ctor)
    dis.diffaug, dis.diffaug_seed = POLICY, 43
    aug = G.DiffAugment(POLICY, seed=43, stream=dis.diffaug_stream)
    a, b = _input(shape, 20).cuda(), _input(shape, 21).cuda()
    with torch.no_grad():
        joint = dis.forward_pair_joint(a, b)
        assert dis.diffaug_call == 2
        want = plain.forward_pair_joint(aug(a), aug(b))      # calls 0 and 1
        assert aug.call == 2 and torch.equal(joint, want)
        dis.diffaug_call = 0
        oa, _ = dis(a)
        ob, _ = dis(b)
    assert dis.diffaug_call == 2
    B = a.shape[0]
    assert rel_err(joint[:B].squeeze().cpu(), oa.cpu()) < TOL and rel_err(joint[B:].squeeze().cpu(), ob.cpu()) < TOL


def _gpu_z(seed, s):
    return lambda layer, call, off, n: dnoise_normals(n, seed, s, layer, call, off).cpu()


@pytest.mark.parametrize("tag,ctor,octor,shape", VID + IMG, ids=IDS)
def test_policy_with_instance_noise_against_the_restatement(tag, ctor, octor, shape):
    torch.manual_seed(5)
    dis = ctor(use_noise=True, noise_sigma=0.1)
    dis.diffaug, dis.diffaug_seed = POLICY, 47
    noisy = DN.NoisyRef(octor(), 0.1, dis.noise_seed, dis.noise_stream, _gpu_z(dis.noise_seed, dis.noise_stream))
    ref = R.AugRef(noisy, POLICY, 47, dis.diffaug_stream, params_fn=G.diffaug_params)
    ref.load_state_dict(dis.state_dict())
    dis.cuda()
    for it in range(2):
        x = _input(shape, 30 + it)
        xg = x.clone().cuda().requires_grad_(True)
        xr = x.clone().requires_grad_(True)
        out, _ = dis(xg)
        want, _ = ref(xr)
        assert rel_err(out.detach().cpu(), want.detach()) < TOL, it
        G.bce_with_logits_const(out, 1.0).backward()
        torch.nn.BCEWithLogitsLoss()(want, torch.ones_like(want)).backward()
        assert rel_err(xg.grad.cpu(), xr.grad) < GTOL
        for (k, p), q in zip(dis.named_parameters(), noisy.disc.parameters()):
            assert rel_err(p.grad.cpu(), q.grad) < GTOL, k
            p.grad = None; q.grad = None
    assert dis.diffaug_call == ref.call == 2 and dis._noise_call == noisy.call == 2


# ---- the trainer ------------------------------------------------------------------------------------------------------
def test_trainer_iteration_against_reference_loop():
    seed_all(81)
    gen, dv, di = G.build_mnist(ngf=8, ndf=8)
    ogen, odv, odi = M.build_mnist(ngf=8, ndf=8)
    for m, o in zip((gen, dv, di), (ogen, odv, odi)):
        o.load_state_dict(m.state_dict())
        m.cuda()
    tr = G.GanTrainer(gen, dv, di, diffaug=POLICY, diffaug_seed=2024)
    assert dv.diffaug == di.diffaug == POLICY and dv.diffaug_seed == di.diffaug_seed == 2024
    odv, odi = (R.AugRef(o, POLICY, 2024, s, params_fn=G.diffaug_params) for o, s in ((odv, 1), (odi, 2)))
    opts = M.make_optimizers(ogen, odv, odi)
    rng = torch.Generator().manual_seed(8)
    imgs = [torch.rand(4, 1, 28, 28, generator=rng) for _ in range(2)]
    vids = [torch.rand(4, 16, 1, 28, 28, generator=rng) for _ in range(2)]
    seed_all(82)
    got = [float(v) for v in tr.step([t.cuda() for t in imgs], [t.cuda() for t in vids])]
    seed_all(82)
    want = [float(v) for v in M.train_step(ogen, odv, odi, opts, imgs, vids)]
    assert dv.diffaug_call == odv.call == 5 and di.diffaug_call == odi.call == 5
    print("diffaug trainer losses", got, want)
    for a, b in zip(got, want):
        assert abs(a - b) <= 1e-4 * abs(b), (got, want)
    for m, o in zip((gen, dv, di), (ogen, odv, odi)):
        osd = o.state_dict()
        for k, v in m.state_dict().items():
            w = osd[k]
            if v.dtype == torch.int64:
                assert int(v) == int(w), k
            elif "running_" in k:
                assert rel_err(v.cpu(), w) < 5e-3, k
            else:
                assert_weights_after_adam(v, w, k)
