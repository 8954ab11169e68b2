"""GPU: the ODE-GAN update kernels (gode_ode_step, gode_axpy_multi) against fp64 evaluations of the same sums, and
GANODETrainer on the package's networks against the reference class's results in tests/golden/odegan_tiny.npz
(scripts/make_odegan_goldens.py), with tolerances taken from the reference's own fp32-vs-fp64 difference stored there."""
import numpy as np
import pytest
import torch

import odegan_cases as K
import odegan_ref as R
from conftest import golden, load_sd, seed_all

import gan_ode_amd as G
from gan_ode_amd.ode_training import _Device, FD_H

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
SIZES = (1, 3, 255, 256, 257, 4099, 70001)
GUARD = 8
# element offset of each tensor's start past a 16-byte boundary, for p and for the gradients: equal -> vector body between a
# scalar head and tail (0: no head), different -> the element-by-element path
P_OFF = (0, 1, 2, 3, 0, 1, 3)
G_OFF = (0, 1, 2, 3, 1, 2, 3)
NULL_AT = 4                       # this tensor's gradient is None


@pytest.fixture(scope="module")
def fix():
    return golden("odegan_tiny.npz")


def _views(offs, seed, scale=1.0):
    """One buffer holding a view per size at the given offsets past a 16-byte boundary, GUARD elements apart."""
    pos, spans = 0, []
    for n, o in zip(SIZES, offs):
        start = (pos + GUARD + 3) // 4 * 4 + o
        spans.append((start, n))
        pos = start + n
    buf = (torch.randn(pos + GUARD + 4, generator=torch.Generator().manual_seed(seed)) * scale).cuda()
    assert buf.data_ptr() % 16 == 0
    return buf, [buf[s:s + n] for s, n in spans], spans


def _outside(buf, spans):
    mask = torch.ones(buf.numel(), dtype=torch.bool)
    for s, n in spans:
        mask[s:s + n] = False
    return buf.cpu()[mask]


@pytest.mark.parametrize("name,ks,with_q", [("euler", (1,), False), ("euler+q", (1,), True), ("heun2", (1, 2), False),
                                            ("heun2+q", (1, 2), True), ("rk4s4", (1, 2, 3, 4), False),
                                            ("rk4s4+q", (1, 2, 3, 4), True), ("rk4s3", (2, 3), False)])
def test_ode_step_kernel(name, ks, with_q):
    lr = 0.02
    coef = {1: -lr / 6, 2: -lr / 3, 3: 2 * lr / 3, 4: -lr / 6}
    pbuf, ps, spans = _views(P_OFF, 1)
    before = pbuf.clone()
    grads, keepalive = {}, []
    for k in ks:
        gbuf, gv, _ = _views(G_OFF, 10 + k, scale=3.0)
        gv[NULL_AT] = None
        grads[k] = gv
        keepalive.append(gbuf)
    q, cq = None, -0.01 * lr * 237.3
    if with_q:
        qa, qp, _ = _views(G_OFF, 20)
        qb, qm, _ = _views(G_OFF, 21)
        q = (qp, qm)
    dev = _Device(ps)
    dev.step("t", {k: coef[k] for k in ks}, grads, cq=cq if with_q else None, q=q)
    torch.cuda.synchronize()
    worst = 0.0
    for i, (p, (s, n)) in enumerate(zip(ps, spans)):
        was = before[s:s + n].cpu().numpy()
        if i == NULL_AT:
            assert np.array_equal(p.cpu().numpy().view(np.uint32), was.view(np.uint32)), "a skipped tensor changed"
            continue
        ref, mag = R.ode_step_sum64(was, [(coef[k], grads[k][i].cpu().numpy()) for k in ks], cq if with_q else None,
                                    q[0][i].cpu().numpy() if with_q else None, q[1][i].cpu().numpy() if with_q else None)
        err = np.abs(p.cpu().numpy().astype(np.float64) - ref)
        worst = max(worst, float((err / (U * mag)).max()))
        assert (err <= 12 * U * mag).all(), (name, n, float((err / (U * mag)).max()))
        assert not np.array_equal(p.cpu().numpy(), was)
    print(f"{name}: worst error {worst:.2f} x 2^-24 x magnitude (bound 12)")
    assert torch.equal(_outside(pbuf, spans), _outside(before, spans)), "a guard element changed"


def test_ode_step_reads_the_device_scale():
    pbuf, ps, spans = _views(P_OFF, 2)
    before = pbuf.clone()
    _, g, _ = _views(P_OFF, 3)
    _, qp, _ = _views(P_OFF, 4)
    _, qm, _ = _views(P_OFF, 5)
    scale = torch.tensor([0.0, 123.5], device="cuda")
    _Device(ps).step("t", {1: -0.5}, {1: g}, cq=-0.25, q=(qp, qm), cq_dev=scale[1:2])
    for p, (s, n), gi, a, b in zip(ps, spans, g, qp, qm):
        ref, mag = R.ode_step_sum64(before[s:s + n].cpu().numpy(), [(-0.5, gi.cpu().numpy())], -0.25 * 123.5, a.cpu().numpy(), b.cpu().numpy())
        assert (np.abs(p.cpu().numpy() - ref) <= 12 * U * mag).all()


def test_axpy_multi():
    pbuf, ps, spans = _views(P_OFF, 6)
    bbuf, base, _ = _views(P_OFF, 7)
    vbuf, v, _ = _views(G_OFF[::-1], 8, scale=2.0)           # partly misaligned against p
    v[NULL_AT] = None
    before = pbuf.clone()
    dev = _Device(ps)
    a = 0.3712
    outs = []
    for _ in range(2):
        dev.axpy("t", ps, base, v, a, h=FD_H)
        torch.cuda.synchronize()
        outs.append((pbuf.clone(), dev.sums.clone(), dev.fd.clone()))
    assert all(torch.equal(x, y) for x, y in zip(*outs)), "two runs differ"
    a32 = float(np.float32(a))
    sv = sb = 0.0
    for i, (p, b) in enumerate(zip(ps, base)):
        b64 = b.cpu().double().numpy()
        v64 = v[i].cpu().double().numpy() if v[i] is not None else np.zeros_like(b64)
        ref = b64 + a32 * v64
        assert (np.abs(p.cpu().double().numpy() - ref) <= 2 * 2.0 ** -23 * np.abs(ref) + 1e-45).all(), SIZES[i]
        sv += float((v64 * v64).sum()); sb += float((b64 * b64).sum())
    got = dev.sums.cpu().numpy()
    assert abs(got[0] - sv) <= 1e-6 * sv and abs(got[1] - sb) <= 1e-6 * sb, (got, sv, sb)
    eps = FD_H * (1 + sb ** 0.5) / sv ** 0.5
    fd = dev.fd.cpu().numpy()
    assert abs(fd[0] - eps) <= 4 * U * eps and abs(fd[1] - 1 / eps) <= 8 * U / eps
    assert torch.equal(_outside(pbuf, spans), _outside(before, spans)), "a guard element changed"
    # a == 0 and v == None copy bit for bit; the device scale multiplies a
    dev.axpy("t", ps, base, v, 0.0)
    assert all(torch.equal(p, b) for p, b in zip(ps, base))
    dev.axpy("t", ps, base, None, 1.0)
    assert all(torch.equal(p, b) for p, b in zip(ps, base))
    dev.axpy("t", ps, base, v, -1.0, a_dev=dev.fd)
    e32 = float(fd[0])
    for i, (p, b) in enumerate(zip(ps, base)):
        if v[i] is not None:
            ref = b.cpu().double().numpy() - e32 * v[i].cpu().double().numpy()
            assert (np.abs(p.cpu().double().numpy() - ref) <= 2 * 2.0 ** -23 * np.abs(ref) + 1e-45).all()


def _delta_check(tag, fix, prefix, module, before, untouched=()):
    worst = {}
    for n, p in module.named_parameters():
        if n in untouched:
            assert torch.equal(p.detach().cpu(), before[n]), n
            continue
        ref, own = fix[f"{prefix}/delta/{n}"], float(fix[f"{prefix}/self/{n}"])
        err = K.delta_err((p.detach().cpu() - before[n]).numpy(), ref)
        worst[n] = (err, own)
        print(f"{tag} {prefix} {n}: err {err:.3e}, reference fp32-vs-fp64 {own:.3e}, ratio {err / own:.2f}")
    bad = {n: v for n, v in worst.items() if not v[0] <= 8 * v[1]}
    assert not bad, bad


DISCS = {"img": ("disc_img_mnist_tiny.npz", lambda: G.PatchImageDiscriminator(1, ndf=8)),
         "vid": ("disc_vid_mnist_tiny.npz", lambda: G.VideoDiscriminator(1, ksize=2, ndf=8))}


@pytest.mark.parametrize("method", K.METHODS)
@pytest.mark.parametrize("tag", ["img", "vid"])
def test_discriminator_step_against_reference(fix, tag, method):
    z = golden(DISCS[tag][0])
    dis = load_sd(DISCS[tag][1](), z, "w").cuda()
    real = torch.from_numpy(z["x"]).float().cuda()
    fake = torch.from_numpy(fix[f"d{tag}/fake"].astype(np.float32)).cuda()
    before = {n: p.detach().cpu().clone() for n, p in dis.named_parameters()}
    loss = K.disc_loss(dis, real, fake, bce=G.bce_with_logits_const)
    tr = G.GANODETrainer([], dis.parameters(), None, None, loss, None, lr=K.LR, reg=0.0, method=method)
    first = tr.step(model="dis_img")
    assert np.isfinite(float(first.detach()))
    _delta_check("gpu", fix, f"d{tag}/{method}", dis, before)


def _tiny_gen():
    return load_sd(G.VideoGeneratorMNISTODE(1, 50, 0, 16, 16, ngf=8), golden("gen_mnist_tiny.npz"), "w").cuda()


def test_generator_rk4_step_against_reference(fix):
    gen = _tiny_gen()
    dv = load_sd(G.VideoDiscriminator(1, ksize=2, ndf=8), golden("disc_vid_mnist_tiny.npz"), "w").cuda()
    before = {n: p.detach().cpu().clone() for n, p in gen.named_parameters()}
    loss = K.gen_video_loss(gen, dv, bce=G.bce_with_logits_const)
    tr = G.GANODETrainer(gen.parameters(), [], None, loss, None, None, lr=K.LR, reg=0.0, method="rk4")
    seed_all(K.GEN_SEED)
    tr.step(model="gen")
    after_step = R.rng_state()
    seed_all(K.GEN_SEED)
    with torch.no_grad():
        for _ in range(4):                                    # four sets of latent draws, one per stage
            gen.sample_videos(K.GEN_VIDEOS)
    s = R.rng_state()
    assert torch.equal(s[0], after_step[0]) and all(np.array_equal(a, b) for a, b in zip(s[1], after_step[1]))
    _delta_check("gpu", fix, "gen/rk4", gen, before, untouched=[n for n in before if n.startswith("recurrent.")])


def test_penalty_against_exact_and_buffers_restored(fix):
    gen = _tiny_gen()
    di = load_sd(G.PatchImageDiscriminator(1, ndf=8), golden("disc_img_mnist_tiny.npz"), "w").cuda()
    g_loss = K.gen_image_loss(gen, di, bce=G.bce_with_logits_const)
    tr = G.GANODETrainer(gen.parameters(), di.parameters(), None, g_loss, None, None, lr=K.LR, reg=0.01, method="euler",
                         modules=(gen, di, None))
    # what one g_loss call leaves in the buffers
    twin, twin_d = _tiny_gen(), load_sd(G.PatchImageDiscriminator(1, ndf=8), golden("disc_img_mnist_tiny.npz"), "w").cuda()
    seed_all(K.PEN_SEED)
    K.gen_image_loss(twin, twin_d, bce=G.bce_with_logits_const)()
    want = [b.detach().cpu().clone() for m in (twin, twin_d) for b in m.buffers()]
    before = [p.detach().cpu().clone() for p in gen.parameters()]
    seed_all(K.PEN_SEED)
    gp = tr.grad_penalty("dis_img")
    assert all(torch.equal(p.detach().cpu(), b) for p, b in zip(gen.parameters(), before)), "generator not restored bitwise"
    got = [b.detach().cpu() for m in (gen, di) for b in m.buffers()]
    assert all(torch.equal(a, b) for a, b in zip(got, want)), "BatchNorm buffers not restored bitwise"
    eps = float(tr._dev["gen"].fd[0])
    print(f"eps gpu {eps:.6e}, cpu fp32 {float(fix['pen/eps32']):.6e}")
    bad, vs_central = {}, {}
    own_central = max(float(fix[f"pen/self/{n}"]) for n, _ in di.named_parameters())
    for (n, _), g in zip(di.named_parameters(), gp):
        err, own = K.delta_err(g.cpu().numpy(), fix[f"pen/exact/{n}"]), float(fix[f"pen/err32/{n}"])
        vs_central[n] = K.delta_err(g.cpu().numpy(), fix[f"pen/central64/{n}"])
        print(f"penalty {n}: vs exact {err:.3e} (cpu fp32 central difference {own:.3e}, ratio {err / own:.2f}); "
              f"vs fp64 central difference {vs_central[n]:.3e} (cpu fp32 {float(fix[f'pen/self/{n}']):.3e})")
        if not err <= 4 * own:
            bad[n] = (err, own)
    assert not bad, bad
    # the same finite difference in fp64 on CPU: the GPU may be 8x as far from it as the CPU's own fp32 run at its worst tensor
    assert max(vs_central.values()) <= 8 * own_central, (vs_central, own_central)


def test_drop_in_loop():
    gen = _tiny_gen()
    di = load_sd(G.PatchImageDiscriminator(1, ndf=8), golden("disc_img_mnist_tiny.npz"), "w").cuda()
    real = torch.from_numpy(golden("disc_img_mnist_tiny.npz")["x"]).float().cuda()[:K.PEN_IMAGES]
    bce = G.bce_with_logits_const

    def d_loss(x):
        with torch.no_grad():
            fake, _ = gen.sample_images(K.PEN_IMAGES)
        return bce(di(x)[0], 1.0) + bce(di(fake)[0], 0.0)

    tr = G.GANODETrainer(gen.parameters(), di.parameters(), None, K.gen_image_loss(gen, di, bce=bce), d_loss, None,
                         lr=K.LR, reg=0.01, method="rk4", modules=(gen, di, None))
    before = {(i, n): p.detach().cpu().clone() for i, m in enumerate((gen, di)) for n, p in m.named_parameters()}
    seed_all(5)
    for _ in range(3):
        losses = [tr.step(real, model="dis_img") for _ in range(tr.d_iter)] + [tr.step(model="gen")]
        assert all(np.isfinite(float(v.detach())) for v in losses)
    for i, m in enumerate((gen, di)):
        for n, p in m.named_parameters():
            assert torch.isfinite(p).all()
            if n.startswith("recurrent."):
                assert torch.equal(p.detach().cpu(), before[i, n])
            else:
                assert not torch.equal(p.detach().cpu(), before[i, n]), n
