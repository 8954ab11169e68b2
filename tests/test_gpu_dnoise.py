"""GPU: the discriminators' instance noise (use_noise=True; gode_dnoise) against the restatement of
tests/dnoise_ref.py -- the raw stream, the op's two modes, both discriminators' forward / backward, the paired pass, shards,
the trainer against the reference loop, and graph replay."""
import ctypes as C

import numpy as np
import pytest
import torch

import dnoise_ref as R
from conftest import assert_weights_after_adam, rel_err, seed_all

import gan_ode_amd as G
import gan_ode_amd._lib as L
from gan_ode_amd.modules import dnoise_normals
from oracle import mocogan_ref as M

pytestmark = pytest.mark.gpu
TOL, GTOL = 1e-4, 5e-4


def stream():
    return torch.cuda.current_stream().cuda_stream


@pytest.mark.parametrize("off,n", [(0, 1), (1, 5), (3, 4097), (7, 1 << 20), (1000003, 12345), ((3 << 32) + 5, 999)])
def test_raw_stream_matches_the_restatement(off, n):
    seed, s, layer, call = 0x0123_4567_89AB_CDEF, 1, 3, 0xFFFFFFFE
    w = dnoise_normals(n, seed, s, layer, call, off, raw=True).cpu().numpy().view(np.uint32)
    assert np.array_equal(w, R.words(seed, s, layer, call, off, n))
    z = dnoise_normals(n, seed, s, layer, call, off).cpu().double().numpy()
    assert np.abs(z - R.normals(seed, s, layer, call, off, n)).max() < 1e-5


def test_stream_moments_and_correlations():
    N = 1 << 22
    a = dnoise_normals(N, 9, 1, 0, 0).double()
    m, v = float(a.mean()), float(a.var())
    assert abs(m) < 5 / N ** 0.5 and abs(v - 1) < 5 * (2 / N) ** 0.5, (m, v)
    for other in (dnoise_normals(N, 9, 1, 1, 0), dnoise_normals(N, 9, 1, 0, 1), dnoise_normals(N, 9, 2, 0, 0),
                  dnoise_normals(N, 9, 1, 0, 0, offset=4), a[1:].float()):
        b = other.double()[:a.numel() - 1] if other.numel() == N else other.double()
        r = float(((a[:b.numel()] - m) * (b - b.mean())).mean() / (a[:b.numel()].std() * b.std()))
        assert abs(r) < 5 / N ** 0.5, r


def _op(**kw):
    op = L.DnoiseOp(**kw)
    L.check(L.lib().gode_dnoise(C.byref(op), stream()), "gode_dnoise")


@pytest.mark.parametrize("M0", [0, 192])
def test_apply_mode_is_bn_apply_plus_noise(M0):
    Mr, Cc, seed, call, sig = 384, 64, 77, 5, np.float32(0.3)
    g = torch.Generator().manual_seed(1)
    y = torch.randn(Mr, Cc, generator=g).cuda()
    sc, sh = torch.randn(2 * Cc, generator=g).cuda(), torch.randn(2 * Cc, generator=g).cuda()
    a = torch.empty_like(y)
    bop = L.BnApplyOp(y=y.data_ptr(), out=a.data_ptr(), scale=sc.data_ptr(), shift=sh.data_ptr(), M=Mr, C=Cc, act=L.ACT_LRELU,
                      M0=M0)
    L.check(L.lib().gode_bn_apply(C.byref(bop), stream()), "bn_apply")
    e_off = 3 * 4 * Cc
    want = a.clone().view(-1)
    n0 = (M0 or Mr) * Cc
    want[:n0] += dnoise_normals(n0, seed, 1, 2, call, e_off) * sig
    if M0:
        want[n0:] += dnoise_normals(want.numel() - n0, seed, 1, 2, call + 1, e_off) * sig
    dev_call = torch.tensor([call - 2], dtype=torch.int32, device="cuda")
    for sigma, expect, kw in ((0.0, a.view(-1), {}), (sig, want, {}), (sig, want, dict(call_dev=dev_call.data_ptr()))):
        out = torch.full_like(y, float("nan"))
        _op(x=y.data_ptr(), out=out.data_ptr(), scale=sc.data_ptr(), shift=sh.data_ptr(), M=Mr, C=Cc, act=L.ACT_LRELU, M0=M0,
            e_off=e_off, seed=seed, stream=1, layer=2, call=2 if kw else call, sigma=float(sigma), **kw)
        assert torch.equal(out.view(-1), expect)


def test_gather_mode_reads_a_transposed_view():
    B, T, Cc, H, W = 3, 5, 3, 10, 7
    x = torch.randn(B, T, Cc, H, W, generator=torch.Generator().manual_seed(2)).cuda()
    v = x.transpose(1, 2)                                          # [B, C, T, H, W], not contiguous
    out = torch.empty(B, T, H, W, Cc, device="cuda")
    n = out.numel()
    _op(x=v.data_ptr(), out=out.data_ptr(), M=B * T * H * W, C=Cc, N=B, D=T, H=H, W=W,
        xs=(C.c_int64 * 5)(v.stride(0), v.stride(2), v.stride(3), v.stride(4), v.stride(1)), e_off=7 * T * H * W * Cc, seed=4,
        stream=2, layer=0, call=9, sigma=0.25)
    want = v.permute(0, 2, 3, 4, 1).reshape(-1) + dnoise_normals(n, 4, 2, 0, 9, 7 * T * H * W * Cc) * np.float32(0.25)
    assert torch.equal(out.view(-1), want)


def test_standalone_noise_module():
    torch.manual_seed(11)
    nz = G.Noise(True, 0.2)
    x = torch.randn(2, 3, 4, 5, device="cuda", requires_grad=True)
    y = nz(x)
    z = dnoise_normals(x.numel(), 11, 0, 0, 0).view(2, 4, 5, 3).permute(0, 3, 1, 2)
    assert torch.equal(y.detach(), x.detach() + z * np.float32(0.2)) and nz.noise_call == 1
    y.sum().backward()
    assert torch.equal(x.grad, torch.ones_like(x))


VID = [("mnist", lambda **k: G.VideoDiscriminator(1, ksize=2, ndf=8, **k), lambda: M.VideoDisc(1, ksize=2, ndf=8), (4, 16, 1, 28, 28)),
       ("ucf", lambda **k: G.VideoDiscriminator(3, ndf=8, **k), lambda: M.VideoDisc(3, ndf=8), (2, 16, 3, 64, 64))]
IMG = [("mnist", lambda **k: G.PatchImageDiscriminator(1, ndf=8, **k), lambda: M.PatchImageDisc(1, ndf=8), (8, 1, 28, 28)),
       ("ucf", lambda **k: G.PatchImageDiscriminator(3, ndf=8, **k), lambda: M.PatchImageDisc(3, ndf=8), (8, 3, 64, 64))]


def _input(shape, seed):
    x = torch.rand(*shape, generator=torch.Generator().manual_seed(seed))
    return x.transpose(1, 2) if len(shape) == 5 else x       # videos: the [B,T,C,H,W] -> [B,C,T,H,W] view the scripts feed


def _gpu_z(seed, s):
    return lambda layer, call, off, n: dnoise_normals(n, seed, s, layer, call, off).cpu()


@pytest.mark.parametrize("tag,ctor,octor,shape", VID + IMG, ids=[f"vid_{v[0]}" for v in VID] + [f"img_{v[0]}" for v in IMG])
def test_sigma_zero_is_bitwise_the_noise_free_discriminator(tag, ctor, octor, shape):
    torch.manual_seed(3)
    plain = ctor().cuda()
    noisy = ctor(use_noise=True, noise_sigma=0.0).cuda()
    noisy.load_state_dict(plain.state_dict())
    res = []
    for d in (plain, noisy):
        x = _input(shape, 4).cuda().requires_grad_(True)
        out, _ = d(x)
        G.bce_with_logits_const(out, 1.0).backward()
        res.append([out.detach(), x.grad] + [p.grad for p in d.parameters()])
    assert noisy._noise_call == 1
    for a, b in zip(*res):
        assert torch.equal(a, b)


@pytest.mark.parametrize("train", [True, False])
@pytest.mark.parametrize("tag,ctor,octor,shape", VID + IMG, ids=[f"vid_{v[0]}" for v in VID] + [f"img_{v[0]}" for v in IMG])
def test_noisy_discriminator_against_the_restatement(tag, ctor, octor, shape, train):
    torch.manual_seed(5)
    dis = ctor(use_noise=True, noise_sigma=0.1)
    ref = R.NoisyRef(octor(), 0.1, dis.noise_seed, dis.noise_stream, _gpu_z(dis.noise_seed, dis.noise_stream))
    ref.load_state_dict(dis.state_dict())
    dis.cuda()
    dis.train(train); ref.train(train)
    for it in range(2):                                       # two calls: the counter moves on
        x = _input(shape, 10 + it)
        xg = x.clone().cuda().requires_grad_(True)
        xr = x.clone().requires_grad_(True)
        out, _ = dis(xg)
        want, _ = ref(xr)
        assert rel_err(out.detach().cpu(), want.detach()) < TOL, it
        G.bce_with_logits_const(out, 1.0).backward()
        torch.nn.BCEWithLogitsLoss()(want, torch.ones_like(want)).backward()
        assert rel_err(xg.grad.cpu(), xr.grad) < GTOL
        for (k, p), q in zip(dis.named_parameters(), ref.disc.parameters()):
            assert rel_err(p.grad.cpu(), q.grad) < GTOL, k
            p.grad = None; q.grad = None
    assert dis._noise_call == ref.call == 2
    for k, v in dis.state_dict().items():
        if "running_" in k:
            assert rel_err(v.cpu(), ref.state_dict()[k]) < TOL, k


def _x0n(dis, key):
    return dis._pool.plans[key][0].x0n.clone()


@pytest.mark.parametrize("tag,ctor,octor,shape", VID[:1] + IMG[:1], ids=["vid", "img"])
def test_paired_pass_draws_what_two_forwards_draw(tag, ctor, octor, shape):
    torch.manual_seed(6)
    dis = ctor(use_noise=True, noise_sigma=0.1).cuda()
    a, b = _input(shape, 20).cuda(), _input(shape, 21).cuda()
    skey = tuple(a.shape) + ("noise",)
    with torch.no_grad():
        joint = dis.forward_pair_joint(a, b)
        assert dis._noise_call == 2
        pair0 = _x0n(dis, ("pair",) + skey)
        dis._noise_call = 0
        oa, _ = dis(a)
        xa = _x0n(dis, skey)
        ob, _ = dis(b)
        xb = _x0n(dis, skey)
    assert dis._noise_call == 2
    assert torch.equal(pair0, torch.cat([xa, xb]))
    B = a.shape[0]
    assert rel_err(joint[:B].squeeze().cpu(), oa.cpu()) < TOL and rel_err(joint[B:].squeeze().cpu(), ob.cpu()) < TOL


def test_shards_draw_the_halves_of_the_full_batch():
    torch.manual_seed(7)
    dis = G.VideoDiscriminator(1, ksize=2, ndf=8, use_noise=True, noise_sigma=0.1).cuda()
    x = _input((8, 16, 1, 28, 28), 30).cuda()
    with torch.no_grad():
        dis(x)
        full = _x0n(dis, tuple(x.shape) + ("noise",))
        halves = []
        for k in range(2):
            dis._noise_call, dis._noise_sample_offset = 0, 4 * k
            dis(x[4 * k:4 * k + 4])
            halves.append(_x0n(dis, (4,) + tuple(x.shape[1:]) + ("noise",)))
    assert torch.equal(full, torch.cat(halves))
    # deeper layers: the same element indices (their inputs differ by the shards' own BatchNorm statistics)
    z_full = dnoise_normals(8 * 100, dis.noise_seed, 1, 2, 0)
    assert torch.equal(z_full[400:], dnoise_normals(400, dis.noise_seed, 1, 2, 0, offset=400))


def test_noisy_and_noise_free_discriminators_do_not_perturb_each_other():
    torch.manual_seed(8)
    plain = G.PatchImageDiscriminator(1, ndf=8).cuda()
    x = _input((8, 1, 28, 28), 40).cuda()

    def noisy():
        torch.manual_seed(8)
        d = G.PatchImageDiscriminator(1, ndf=8, use_noise=True, noise_sigma=0.1).cuda()
        d.load_state_dict(plain.state_dict())
        return d
    with torch.no_grad():
        p0 = plain(x)[0].clone()
        n0 = noisy()(x)[0].clone()
        d = noisy()
        n1 = d(x)[0].clone()
        p1 = plain(x)[0].clone()
        n2 = d(x)[0].clone()
    assert torch.equal(p0, p1) and torch.equal(n0, n1) and not torch.equal(n0, n2) and not torch.equal(p0, n0)


def test_trainer_iteration_batch32_against_reference_loop():
    seed_all(81)
    gen, dv, di = G.build_mnist(ngf=16, ndf=16, use_noise=True, noise_sigma=0.1)
    ogen, odv, odi = M.build_mnist(ngf=16, ndf=16)
    for m, o in zip((gen, dv, di), (ogen, odv, odi)):
        o.load_state_dict(m.state_dict())
        m.cuda()
    tr = G.GanTrainer(gen, dv, di, noise_seed=2024)
    assert dv.noise_seed == di.noise_seed == 2024
    odv, odi = (R.NoisyRef(o, 0.1, 2024, s, _gpu_z(2024, s)) for o, s in ((odv, 1), (odi, 2)))
    opts = M.make_optimizers(ogen, odv, odi)
    rng = torch.Generator().manual_seed(8)
    imgs = [torch.rand(32, 1, 28, 28, generator=rng) for _ in range(2)]
    vids = [torch.rand(32, 16, 1, 28, 28, generator=rng) for _ in range(2)]
    seed_all(82)
    got = [float(v) for v in tr.step([t.cuda() for t in imgs], [t.cuda() for t in vids])]
    seed_all(82)
    want = [float(v) for v in M.train_step(ogen, odv, odi, opts, imgs, vids)]
    assert dv._noise_call == odv.call == 5 and di._noise_call == odi.call == 5
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


def _run_trainer(graph, iters=5):
    seed_all(31)
    gen, dv, di = G.build_mnist(ngf=16, ndf=16, use_noise=True, noise_sigma=0.1)
    gen.cuda(); dv.cuda(); di.cuda()
    tr = G.GanTrainer(gen, dv, di, graph=graph, noise_seed=77)
    rng = torch.Generator().manual_seed(10)
    losses = []
    for it in range(iters):
        imgs = [torch.rand(8, 1, 28, 28, generator=rng).cuda() for _ in range(2)]
        vids = [torch.rand(8, 16, 1, 28, 28, generator=rng).cuda() for _ in range(2)]
        seed_all(300 + it)
        losses.append([float(v) for v in tr.step(imgs, vids)])
    torch.cuda.synchronize()
    state = [v.detach().clone() for m in (gen, dv, di) for v in m.state_dict().values()]
    return tr, losses, state, (dv._noise_call, di._noise_call)


def test_graph_replay_is_bitwise_the_eager_schedule_with_instance_noise():
    runs = []
    for graph in (True, False):
        tr, losses, state, calls = _run_trainer(graph)
        assert (tr._graph is not None) == graph
        runs.append((losses, state, calls))
    assert runs[0][0] == runs[1][0], (runs[0][0], runs[1][0])
    for a, b in zip(runs[0][1], runs[1][1]):
        assert torch.equal(a, b)
    assert runs[0][2] == runs[1][2] == (25, 25)
