"""GPU: class-conditional MoCoGAN on the Neural-ODE generators -- the one-hot latent op, the categorical generator and
discriminator, the fused cross-entropy and one training iteration -- through the public classes and the C ABI, against
tests/categ_ref.py (stock torch.nn on the CPU) with the state_dict copied.  Tolerances are the project's:
frames, logits and losses 1e-4, fixture-level gradients 5e-4, kernel-level reductions 2e-4; the full-size iteration uses the
acceptance of tests/test_gpu_configs.py (first-pass losses 1e-4, later ones 1e-3, post-Adam weights by
assert_weights_after_adam).  Generator gradients are taken with every BatchNorm/ReLU kink out of reach (beta = +6, head
weights x 0.05), as tests/test_gpu_modules.py::test_fixture_generators_kink_free_gradients_at_1e_4 does and for its reason:
one flipped kink moves a channel of a tiny net by 4e-3, which says nothing about the kernels."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import assert_weights_after_adam, rel_err, seed_all

import categ_ref as R
import gan_ode_amd as G
from gan_ode_amd import _lib as L
from gan_ode_amd import modules as Mod
from gan_ode_amd.engine import stream_ptr
from oracle import mocogan_ref as M

pytestmark = pytest.mark.gpu
TOL, GTOL, KTOL = 1e-4, 5e-4, 2e-4


def _pair(C, mnist=True, method="rk4", ngf=8, kink_free=False, seed=0):
    seed_all(seed)
    gen = (G.VideoGeneratorMNISTODE(1, 50, C, 16, 16, ngf=ngf) if mnist
           else G.VideoGenerator(3, 50, C, 16, 16, dim_hidden=16, ngf=ngf))
    gen.ode_method = method
    ref = R.Generator(1 if mnist else 3, 50, C, 16, 16, dim_hidden=16, ngf=ngf, mnist=mnist, ode_method=method)
    if kink_free:
        with torch.no_grad():
            for mod in gen.main:
                if isinstance(mod, torch.nn.BatchNorm2d):
                    mod.bias.fill_(6.0)
            gen.main[12].weight.mul_(0.05)
    ref.load_state_dict({k: v.detach().clone() for k, v in gen.state_dict().items()})
    return gen.cuda(), ref


# ---------------------------------------------------------------------------------------------------------------------
# one-hot op
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [1, 6, 30])
@pytest.mark.parametrize("select", [False, True])
def test_onehot_columns_of_the_latent_rows(C, select):
    """The plan's latent buffer after a call: category columns exactly the expected 0/1, pad exactly zero, motion and
    content columns bitwise those of a C == 0 generator fed the same draws (same ODE weights)."""
    B, T = 3, 16
    gen, _ = _pair(C)
    plain, _ = _pair(0)
    plain.load_state_dict({k: v for k, v in gen.state_dict().items() if not k.startswith("main.")}, strict=False)
    seed_all(5)
    x, content, sel, cls = gen._host_inputs(select, B, T)
    with torch.no_grad():
        if select:
            seed_all(5)
            gen.sample_images(B)
            plan = gen._pool.plans[(B, T, True)][0]
        else:
            seed_all(5)
            _, labels = gen.sample_videos(B)
            plan = gen._pool.plans[(B, T, False)][0]
            assert labels.dtype == torch.int64 and labels.is_cuda and np.array_equal(labels.cpu().numpy(), cls)
        plain._run(B, T, select, x, content, sel)
    z = plan.stack.x_in.view(-1, Mod.Z_COLS).cpu()
    z0 = plain._pool.plans[(B, T, select)][0].stack.x_in.view(-1, Mod.Z_COLS).cpu()
    rows_per = 1 if select else T
    want = torch.zeros(B * rows_per, C)
    want[torch.arange(B * rows_per), torch.from_numpy(np.repeat(cls, rows_per))] = 1
    assert torch.equal(z[:, 66:66 + C], want)
    assert float(z[:, 66 + C:].abs().max()) == 0.0 if C < 30 else True
    assert torch.equal(z[:, :66], z0[:, :66])
    assert float(z0[:, 66:].abs().max()) == 0.0


def test_onehot_op_through_the_c_abi_rewrites_a_dirty_buffer():
    n, T, C = 5, 4, 6
    cls = torch.tensor([0, 5, 2, 2, 3], dtype=torch.int32, device="cuda")
    z = torch.full((n * T, 96), 7.0, device="cuda")
    labels = torch.empty(n, dtype=torch.int64, device="cuda")
    L.run_one(L.CategOp(cls=cls.data_ptr(), z=z.data_ptr(), labels_out=labels.data_ptr(), n_traj=n, rows_per=T, C=C,
                        zcols=96, col0=66), stream_ptr())
    want = F.one_hot(cls.long().repeat_interleave(T), C).float()
    assert torch.equal(z[:, 66:72], want) and float((z[:, :66] - 7).abs().max()) == 0 and float((z[:, 72:] - 7).abs().max()) == 0
    assert torch.equal(labels, cls.long())
    bad = L.CategOp(cls=cls.data_ptr(), z=z.data_ptr(), labels_out=None, n_traj=n, rows_per=T, C=31, zcols=96, col0=66)
    with pytest.raises(RuntimeError):
        L.run_one(bad, stream_ptr())                      # 66 + 31 > 96: refused before any launch


# ---------------------------------------------------------------------------------------------------------------------
# generator
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mnist,method,C", [(True, "rk4", 6), (True, "dopri5", 10), (False, "rk4", 1), (False, "dopri5", 30),
                                            (True, "rk4", 30)])
def test_generator_frames_classes_and_gradients(mnist, method, C):
    gen, ref = _pair(C, mnist=mnist, method=method, kink_free=True, seed=20 + C)
    nv, ni = (4, 4) if mnist else (2, 3)
    seed_all(31)
    vid, labels = gen.sample_videos(nv)
    seed_all(32)
    img, none = gen.sample_images(ni)
    seed_all(31)
    rvid, rlabels = ref.sample_videos(nv)
    seed_all(32)
    rimg, _ = ref.sample_images(ni)
    assert none is None and labels.dtype == torch.int64 and labels.is_cuda
    assert torch.equal(labels.cpu(), rlabels)
    ev, ei = rel_err(vid.detach().cpu(), rvid.detach()), rel_err(img.detach().cpu(), rimg.detach())
    print("frames", ev, ei)
    assert ev < TOL and ei < TOL
    rng = torch.Generator().manual_seed(3)
    wv, wi = torch.randn(vid.shape, generator=rng), torch.randn(img.shape, generator=rng)
    ((vid * wv.cuda()).sum() + (img * wi.cuda()).sum()).backward()
    ((rvid * wv).sum() + (rimg * wi).sum()).backward()
    rp = dict(ref.named_parameters())
    errs = {}
    for k, p in gen.named_parameters():
        if rp[k].grad is None:
            assert p.grad is None, k
        else:
            errs[k] = rel_err(p.grad.cpu(), rp[k].grad)
    # the category rows of the first decoder weight, on their own scale
    gw, rw = gen.main[0].weight.grad.cpu()[50:50 + C], rp["main.0.weight"].grad[50:50 + C]
    errs["main.0.weight[category rows]"] = rel_err(gw, rw)
    print("grads", errs)
    # dopri5: the motion-latent tensors sit behind two adaptive solves whose accepted steps differ between the build and
    # the restatement (sample_images integrates the selected trajectories only); their bound is the one
    # tests/test_gpu_modules.py::test_dopri5_method_against_oracle asserts for them, 2e-3
    for k, e in errs.items():
        assert e < (GTOL if (method == "rk4" or k.startswith("main.")) else 2e-3), (k, errs)
    for k, v in gen.state_dict().items():
        if "running_" in k:
            assert rel_err(v.cpu(), ref.state_dict()[k]) < TOL, k
    gen.eval(); ref.eval()
    seed_all(34)
    with torch.no_grad():
        e, el = gen.sample_videos(nv)
    seed_all(34)
    with torch.no_grad():
        r, rl = ref.sample_videos(nv)
    assert rel_err(e.cpu(), r) < TOL and torch.equal(el.cpu(), rl)


@pytest.mark.parametrize("C", [0, 6])
def test_sample_z_video_public_surface(C):
    """sample_z_m (a latent-only plan) and sample_z_video = cat([content, category, motion]) with and without categories."""
    gen, ref = _pair(C, seed=35)
    seed_all(36)
    z, cls = gen.sample_z_video(3)
    seed_all(36)
    rz, rcls = ref.sample_z_video(3)
    assert tuple(z.shape) == (48, 66 + C) and np.array_equal(cls, rcls)
    assert rel_err(z.detach().cpu(), rz.detach()) < TOL
    if C:
        assert torch.equal(z[:, 50:50 + C].detach().cpu(), rz[:, 50:50 + C].detach())


@pytest.mark.parametrize("method", ["rk4", "dopri5"])
def test_joint_pass_and_prefetch_are_bitwise_the_calls(method):
    C, B = 6, 4
    gen, _ = _pair(C, method=method, seed=40)
    state = {k: v.clone() for k, v in gen.state_dict().items()}

    def run(mode):
        gen.load_state_dict(state)
        seed_all(41)
        with torch.no_grad():
            if mode == "calls":
                v = gen.sample_videos(B)
                i = gen.sample_images(B)
            elif mode == "pair":
                assert gen.can_pair(B, B)
                v, i = gen.sample_pair(B, B)
            elif mode == "prefetch":
                gen.prefetch_latents([("videos", B), ("images", B)])
                v = gen.sample_videos(B)
                i = gen.sample_images(B)
            else:
                gen.prefetch_latents([("pair_vi", (B, B))])
                v, i = gen.sample_pair(B, B)
        torch.cuda.synchronize()
        return v[0].clone(), v[1].clone(), i[0].clone(), {k: t.clone() for k, t in gen.state_dict().items() if "running" in k}

    base = run("calls")
    for mode in ("pair", "prefetch", "prefetch_pair"):
        got = run(mode)
        assert torch.equal(got[0], base[0]) and torch.equal(got[1], base[1]) and torch.equal(got[2], base[2]), mode
        assert all(torch.equal(got[3][k], base[3][k]) for k in base[3]), mode
    assert base[1].dtype == torch.int64


def test_unconditional_generator_is_bitwise_the_path_without_the_categorical_ops(monkeypatch):
    """C == 0: frames and labels with this code equal those of the same process with the categorical pieces made
    unreachable (any use of the one-hot op or of the class draw raises)."""
    gen, _ = _pair(0, seed=50)
    seed_all(51)
    with torch.no_grad():
        v0, l0 = gen.sample_videos(4)
        i0, _ = gen.sample_images(4)
    def boom(*a, **k):
        raise AssertionError("categorical code reached with dim_z_category == 0")
    monkeypatch.setattr(L, "CategOp", boom)
    monkeypatch.setattr(type(gen), "_draw_categorical", boom)
    gen2, _ = _pair(0, seed=50)
    seed_all(51)
    with torch.no_grad():
        v1, l1 = gen2.sample_videos(4)
        i1, _ = gen2.sample_images(4)
    assert torch.equal(v0, v1) and torch.equal(i0, i1)
    assert l0.dtype == l1.dtype == torch.float64 and float(l0.abs().sum()) == 0.0
    assert gen2._pool.plans[(4, 16, False)][0]._in.numel() == 4 * (16 + 51)


# ---------------------------------------------------------------------------------------------------------------------
# discriminator head
# ---------------------------------------------------------------------------------------------------------------------
def _disc_pair(C, ksize, use_noise=0.0, seed=60):      # use_noise: the instance-noise sigma (0: off)
    seed_all(seed)
    d = G.CategoricalVideoDiscriminator(1, C, ndf=8, ksize=ksize, use_noise=bool(use_noise), noise_sigma=use_noise or None)
    ref = R.CategoricalVideoDisc(1, C, ndf=8, ksize=ksize)
    ref.load_state_dict(d.state_dict())
    return d.cuda(), ref


# geometry: "k4" = ksize 4 on 16 x 64 x 64 videos -> a 1x1x1 output, the head is [B, 1 + C] with K = 8 ndf 4^3; "k2" = the
# MNIST discriminator (ksize 2 on 16 x 28 x 28) -> 11 x 2 x 2 output positions, the reference's split gives 5-D halves
GEOMS = {"k4": (4, (16, 64, 64), (1, 1, 1)), "k2": (2, (16, 28, 28), (11, 2, 2))}


@pytest.mark.parametrize("width,geom", [(2, "k4"), (5, "k4"), (7, "k4"), (31, "k4"), (7, "k2"), (31, "k2")])
@pytest.mark.parametrize("which", ["labels", "categ", "both"])
def test_wide_head_logits_split_and_gradients(width, geom, which):
    C = width - 1
    ksize, dims, pos = GEOMS[geom]
    d, ref = _disc_pair(C, ksize)
    rng = torch.Generator().manual_seed(width)
    x = torch.rand(3, 1, *dims, generator=rng)
    xg = x.cuda().requires_grad_(True)
    xr = x.clone().requires_grad_(True)
    labels, categ = d(xg)
    rlabels, rcateg = ref(xr)
    assert tuple(labels.shape) == tuple(rlabels.shape) and tuple(categ.shape) == tuple(rcateg.shape)
    assert tuple(categ.shape) == ((3, C) if geom == "k4" else (3, C, *pos))
    assert categ.data_ptr() == labels.data_ptr() + 4              # two views of the one head buffer
    e = (rel_err(labels.detach().cpu(), rlabels.detach()), rel_err(categ.detach().cpu(), rcateg.detach()))
    print("logits", e)
    assert max(e) < TOL
    gl, gc = torch.randn(labels.shape, generator=rng), torch.randn(categ.shape, generator=rng)
    loss = rloss = 0
    if which in ("labels", "both"):
        loss, rloss = loss + (labels * gl.cuda()).sum(), rloss + (rlabels * gl).sum()
    if which in ("categ", "both"):
        loss, rloss = loss + (categ * gc.cuda()).sum(), rloss + (rcateg * gc).sum()
    plan = d._pool.plans[tuple(xg.shape)][0]
    calls = []
    orig = plan.backward
    plan.backward = lambda *a, **k: (calls.append(1), orig(*a, **k))[1]
    loss.backward()
    rloss.backward()
    assert len(calls) == 1                                           # the stack's backward ran once
    errs = {"x": rel_err(xg.grad.cpu(), xr.grad)}
    for (k, p), (_, q) in zip(d.named_parameters(), ref.named_parameters()):
        errs[k] = rel_err(p.grad.cpu(), q.grad)
    print("grads", errs)
    assert all(v < GTOL for v in errs.values()), errs


@pytest.mark.parametrize("width,geom", [(2, "k4"), (5, "k4"), (7, "k4"), (31, "k4"), (11, "k2")])
def test_wide_head_paired_pass_equals_two_passes(width, geom):
    C = width - 1
    ksize, dims, pos = GEOMS[geom]
    d, _ = _disc_pair(C, ksize)
    state = {k: v.clone() for k, v in d.state_dict().items()}
    rng = torch.Generator().manual_seed(1)
    a, b = torch.rand(4, 1, *dims, generator=rng).cuda(), torch.rand(4, 1, *dims, generator=rng).cuda()
    ha, hb = d.forward_head(a), d.forward_head(b)
    ya = torch.tensor([0, C - 1, 0, C // 2], device="cuda")
    G.bce_ce_heads(ha, 1.0, ya, hb, 0.0).backward()
    two = {k: p.grad.clone() for k, p in d.named_parameters()}
    stats = {k: v.clone() for k, v in d.state_dict().items() if "running" in k}
    d.load_state_dict(state)
    d.zero_grad()
    joint = d.forward_pair_joint(a, b)
    assert tuple(joint.shape) == (8, *pos, width)
    assert float((joint.detach()[:4].reshape(ha.shape) - ha.detach()).abs().max()) < 1e-6
    assert float((joint.detach()[4:].reshape(hb.shape) - hb.detach()).abs().max()) < 1e-6
    G.bce_ce_head_halves(joint, 1.0, 0.0, ya).backward()
    for k, p in d.named_parameters():
        assert rel_err(p.grad.cpu(), two[k].cpu()) < GTOL, k
    for k, v in stats.items():
        assert rel_err(d.state_dict()[k].cpu(), v.cpu()) < 1e-6, k


def test_categorical_discriminator_with_instance_noise_runs():
    d, _ = _disc_pair(6, 2, use_noise=0.1)
    x = torch.rand(4, 1, 16, 28, 28).cuda()
    labels, categ = d(x)
    labels2, _ = d(x)
    assert tuple(categ.shape) == (4, 6, 11, 2, 2) and bool(torch.isfinite(categ).all())
    assert not torch.equal(labels, labels2)                          # a fresh draw per call
    joint = d.forward_pair_joint(x, x)
    G.bce_ce_head_halves(joint, 1.0, 0.0, torch.zeros(4, dtype=torch.int64, device="cuda")).backward()
    assert all(bool(torch.isfinite(p.grad).all()) for p in d.parameters())


# ---------------------------------------------------------------------------------------------------------------------
# loss kernel
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 32, 257])
@pytest.mark.parametrize("C", [1, 10, 30])
def test_cross_entropy_value_gradient_stability_and_determinism(B, C):
    rng = torch.Generator().manual_seed(B * 100 + C)
    head = (torch.rand(B, 1 + C, generator=rng) * 2 - 1) * 80.0          # logits up to +-80
    y = torch.randint(0, C, (B,), generator=rng)
    hg = head.cuda().requires_grad_(True)
    hr = head.clone().double().requires_grad_(True)
    loss = G.categorical_cross_entropy(hg[:, 1:], y.cuda())
    rloss = F.cross_entropy(hr[:, 1:], y)
    loss.backward()
    rloss.backward()
    e = (abs(float(loss) - float(rloss)) / max(abs(float(rloss)), 1e-30), rel_err(hg.grad.cpu(), hr.grad))
    print("ce", float(loss), float(rloss), e)
    assert bool(torch.isfinite(loss)) and e[0] < KTOL and e[1] < KTOL
    assert float(hg.grad[:, 0].abs().max()) == 0.0
    again = G.categorical_cross_entropy(hg.detach()[:, 1:], y.cuda())
    assert torch.equal(again, loss.detach())
    # fused forms: one scalar, the whole head gradient written by the loss launches
    hg2 = head.cuda().requires_grad_(True)
    fused = G.bce_ce_head(hg2, 1.0, y.cuda())
    fused.backward(gradient=G.unit_grad(fused.device))
    want = F.binary_cross_entropy_with_logits(hr[:, 0].detach(), torch.ones(B, dtype=torch.float64)) + rloss.detach()
    assert abs(float(fused) - float(want)) / abs(float(want)) < KTOL
    assert torch.equal(hg2.grad[:, 1:], hg.grad[:, 1:])
    rb = (torch.sigmoid(hr[:, 0].detach()) - 1) / B
    # (fp32 sigmoid(x) - 1 near saturation carries half an ulp of 1.0 absolute error, whatever the size of the result)
    assert float((hg2.grad[:, 0].cpu().double() - rb).abs().max()) <= KTOL * float(rb.abs().max()) + 2.0 ** -23 / B
    with pytest.raises(RuntimeError):
        G.categorical_cross_entropy(hg[:, 1:], y.cuda().int())


def test_fused_halves_zero_the_unlabelled_rows_and_match_the_parts():
    B, C = 6, 5
    rng = torch.Generator().manual_seed(9)
    joint = torch.randn(2 * B, 1, 1, 1, 1 + C, generator=rng).cuda().requires_grad_(True)
    y = torch.randint(0, C, (B,), generator=rng).cuda()
    loss = G.bce_ce_head_halves(joint, 1.0, 0.0, y)
    loss.backward(gradient=G.unit_grad(loss.device))
    j = joint.detach().view(2 * B, 1 + C).cpu().double()
    want = (F.binary_cross_entropy_with_logits(j[:B, 0], torch.ones(B).double())
            + F.binary_cross_entropy_with_logits(j[B:, 0], torch.zeros(B).double()) + F.cross_entropy(j[:B, 1:], y.cpu()))
    assert abs(float(loss) - float(want)) / float(want) < KTOL
    g = joint.grad.view(2 * B, 1 + C)
    assert float(g[B:, 1:].abs().max()) == 0.0 and float(g[:B, 1:].abs().max()) > 0 and float(g[:, 0].abs().min()) > 0


def test_fused_losses_on_a_patch_head_take_the_video_label_at_every_position():
    B, C, pos = 5, 4, (11, 2, 2)
    rng = torch.Generator().manual_seed(10)
    head = torch.randn(B, *pos, 1 + C, generator=rng).cuda().requires_grad_(True)
    y = torch.randint(0, C, (B,), generator=rng)
    loss = G.bce_ce_head(head, 1.0, y.cuda())
    loss.backward()
    hr = head.detach().cpu().double().requires_grad_(True)
    nchw = hr.permute(0, 4, 1, 2, 3)
    want = F.binary_cross_entropy_with_logits(nchw[:, :1], torch.ones(B, 1, *pos).double()) + R.cross_entropy(nchw[:, 1:], y)
    want.backward()
    assert abs(float(loss) - float(want)) / float(want) < KTOL and rel_err(head.grad.cpu(), hr.grad) < KTOL


# ---------------------------------------------------------------------------------------------------------------------
# training
# ---------------------------------------------------------------------------------------------------------------------
def _train_setup(C, ngf, ndf, B, seed):
    seed_all(seed)
    gen = G.VideoGeneratorMNISTODE(1, 50, C, 16, 16, ngf=ngf)
    dv = G.CategoricalVideoDiscriminator(1, C, ndf=ndf, ksize=2)
    di = G.PatchImageDiscriminator(1, ndf=ndf)
    refs = R.build_mnist(C, ngf=ngf, ndf=ndf)
    for m, o in zip((gen, dv, di), refs):
        o.load_state_dict(m.state_dict())
    for m in (gen, dv, di):
        m.cuda()
    rng = torch.Generator().manual_seed(seed + 1)
    imgs = [torch.rand(B, 1, 28, 28, generator=rng) for _ in range(2)]
    vids = [torch.rand(B, 16, 1, 28, 28, generator=rng) for _ in range(2)]
    labels = [torch.randint(0, C, (B,), generator=rng) for _ in range(2)]
    return (gen, dv, di), refs, imgs, vids, labels


@pytest.mark.parametrize("tag,C,ngf,ndf,B,pair_d", [("tiny", 6, 8, 8, 4, True), ("tiny_unpaired", 6, 8, 8, 4, False),
                                                    ("config", 10, 64, 64, 32, True)])
def test_categorical_training_iteration_step_by_step(tag, C, ngf, ndf, B, pair_d):
    nets, refs, imgs, vids, labels = _train_setup(C, ngf, ndf, B, 70)
    tr = G.GanTrainer(*nets, pair_d_passes=pair_d)
    log = []
    for name in ("d_image_step", "d_video_step", "g_step"):
        def wrap(fn):
            def inner(*a, **k):
                out = fn(*a, **k)
                log.append(out)
                return out
            return inner
        setattr(tr, name, wrap(getattr(tr, name)))
    seed_all(71)
    got3 = tr.step([t.cuda() for t in imgs], [t.cuda() for t in vids], [t.cuda() for t in labels])
    got = [float(v) for v in log]
    rlog = []
    seed_all(71)
    want3 = R.train_step(*refs, M.make_optimizers(*refs), imgs, vids, labels, log=rlog)
    want = [float(v) for v in rlog]
    print(tag, "losses", got, want)
    assert len(got) == len(want) == 5
    assert [float(v) for v in got3] == [got[2], got[3], got[4]] and float(want3[2]) == want[4]
    assert np.allclose(got[:2], want[:2], rtol=TOL, atol=0), (got, want)          # first pass: initial weights
    assert np.allclose(got[2:], want[2:], rtol=1e-3, atol=0), (got, want)         # behind Adam's sign-like first steps
    for m, o in zip(nets, refs):
        for (k, v), (_, w) in zip(m.state_dict().items(), o.state_dict().items()):
            if v.dtype == torch.int64:
                assert int(v) == int(w), k
            elif "running_" in k:
                assert rel_err(v.cpu(), w) < 5e-3, k
            else:
                assert_weights_after_adam(v, w, k)


def test_unconditional_trainer_is_bitwise_without_the_categorical_ops(monkeypatch):
    def run(block):
        seed_all(80)
        nets = G.build_mnist(ngf=8, ndf=8)
        for m in nets:
            m.cuda()
        if block:
            def boom(*a, **k):
                raise AssertionError("categorical code reached by an unconditional trainer")
            for name in ("CategOp", "CeOp"):
                monkeypatch.setattr(L, name, boom)
        tr = G.GanTrainer(*nets)
        rng = torch.Generator().manual_seed(81)
        imgs = [torch.rand(4, 1, 28, 28, generator=rng).cuda() for _ in range(2)]
        vids = [torch.rand(4, 16, 1, 28, 28, generator=rng).cuda() for _ in range(2)]
        seed_all(82)
        losses = [tr.step(imgs, vids) for _ in range(2)][-1]
        torch.cuda.synchronize()
        return [v.clone() for v in losses], [p.detach().clone() for m in nets for p in m.parameters()]
    l0, w0 = run(False)
    l1, w1 = run(True)
    assert all(torch.equal(a, b) for a, b in zip(l0, l1)) and all(torch.equal(a, b) for a, b in zip(w0, w1))
