"""GPU: the Neural-CDE motion latent (models/mocogan_cde.py; gode_cde_fwd / gode_cde_bwd) against the float64
restatement of tests/cde_ref.py.  The kernels are replayed exactly on their own accepted schedule (outputs, states and
the autograd gradient of the replay), the controller against a float64 dopri5 solve, the discrete gradient against the
continuous adjoint; the generator class against the oracle's MNIST decoder fed with the replayed latent, and one
GanTrainer iteration against a stock-torch loop."""
import numpy as np
import pytest
import torch
import torch.nn as nn

import cde_ref as R
from cde_driver import KINK, Solve, _guards_intact, _params, _split
from conftest import assert_weights_after_adam, golden, rel_err, seed_all

import gan_ode_amd as G
import gan_ode_amd._lib as L
from gan_ode_amd.modules import _CdeGenPlan
from oracle import mocogan_ref as M

pytestmark = pytest.mark.gpu


def stream():
    return torch.cuda.current_stream().cuda_stream


@pytest.mark.parametrize("N,T", [(1, 16), (16, 16), (32, 16), (33, 16), (300, 16), (4096, 16), (20, 5)])
def test_cde_kernels_against_float64_replay(N, T):
    P32, P64 = _params()
    gen = torch.Generator().manual_seed(100 + N + T)
    x = torch.randn(N, T, generator=gen)
    s = Solve(P32, x, T)
    assert s.acc > 0 and s.trials >= s.acc, (s.acc, s.trials)
    for b in (s.zb, s.sb, s.hb):
        _guards_intact(b)
    _guards_intact(s.cb, -7)
    st, sh = s.schedule()
    assert abs(float((st + sh)[-1]) - (T - 1)) < float(sh[-1]) + 1e-12 and float(st[0]) == 0.0
    assert torch.equal(st[1:], (st + sh)[:-1])
    mg = {}
    outs, states, z0 = R.replay(P64, x, T, st, sh, margin=mg)
    z = s.z.cpu().view(N, T, 16)
    assert rel_err(z, outs.detach()) <= 2e-5
    got_states = s.states.cpu().view(N, s.S_cap + 1, 16)
    assert rel_err(got_states[:, :s.acc + 1], states.detach()) <= 2e-5
    assert torch.isnan(got_states[:, s.acc + 1:]).all()         # nothing past the accepted steps
    assert rel_err(z[:, 0], z0.detach()) <= 2e-5

    # backward: all rows, then sel_t rows; accumulate 0 and 1.  Trajectories that pass within fp32 rounding of a ReLU
    # kink (|W1 z + b1| < KINK at some stage) get no upstream gradient: there the fp32 kernel and the float64 replay
    # may legitimately take different branches (measured: one such trajectory off by 13 % in its W1 share)
    keep = (mg["relu"] > KINK).to(torch.float32)[:, None, None]
    assert float(keep.mean()) > 0.5, float(keep.mean())
    gz = torch.randn(N, T, 16, generator=gen) * keep
    ref = torch.autograd.grad((outs * gz.double()).sum(), P64, retain_graph=True)
    g, gb = s.backward(gz.view(N * T, 16))
    _guards_intact(gb)
    for a, b, name in zip(_split(g), ref, "Wa ba Wb bb W1 b1 W2 b2".split()):
        assert rel_err(a, b) <= 1e-4, (name, rel_err(a, b))
    g2, _ = s.backward(gz.view(N * T, 16))
    assert torch.equal(g, g2)                                      # re-runs are bitwise equal
    init = torch.randn(L.CDE_NPARAM, generator=gen)
    g3, gb3 = s.backward(gz.view(N * T, 16), accumulate=1, init=init)
    _guards_intact(gb3)
    assert rel_err(g3 - init, g) <= 1e-5

    sel = torch.randint(0, T, (N,), generator=gen)
    s2 = Solve(P32, x, T, sel=sel)
    assert (s2.acc, s2.trials) == (s.acc, s.trials)
    assert torch.equal(s2.sched.cpu()[:s.acc], s.sched.cpu()[:s.acc])
    _guards_intact(s2.zb)
    assert torch.equal(s2.z.cpu().view(N, 16), z[torch.arange(N), sel])
    gzs = torch.randn(N, 16, generator=gen) * keep[:, 0]
    full = torch.zeros(N, T, 16, dtype=torch.float64)
    full[torch.arange(N), sel] = gzs.double()
    ref = torch.autograd.grad((outs * full).sum(), P64)
    g, gb = s2.backward(gzs)
    _guards_intact(gb)
    for a, b, name in zip(_split(g), ref, "Wa ba Wb bb W1 b1 W2 b2".split()):
        assert rel_err(a, b) <= 1e-4, (name, rel_err(a, b))

    s3 = Solve(P32, x, T)                                          # forward re-run: bitwise
    for u, v in ((s3.zb, s.zb), (s3.sb, s.sb), (s3.hb, s.hb), (s3.cb, s.cb)):
        assert u.cpu().numpy().tobytes() == v.cpu().numpy().tobytes()


@pytest.mark.parametrize("N", [32, 300])
def test_cde_controller_against_float64_dopri5(N):
    """Accepted / trial counts within +-2 of a float64 dopri5_solve of the restated field at the same tolerances.  The
    outputs differ by the solver's own global error at rtol 1e-4 over [0, 15] once one accept / reject decision
    differs: measured 2.9e-3 at N = 32, bounded at 5e-3."""
    P32, P64 = _params()
    x = torch.randn(N, 16, generator=torch.Generator().manual_seed(7))
    s = Solve(P32, x, 16)
    with torch.no_grad():
        out, acc, trials = R.solve(P64, x, 16)
    print(f"N={N}: kernel {s.acc}/{s.trials}, float64 {acc}/{trials}, "
          f"outputs {rel_err(s.z.cpu().view(N, 16, 16), out):.2e}")
    assert abs(s.acc - acc) <= 2 and abs(s.trials - trials) <= 2, (s.acc, s.trials, acc, trials)
    assert rel_err(s.z.cpu().view(N, 16, 16), out) <= 5e-3


def test_cde_discrete_gradient_against_continuous_adjoint():
    """The kernel's discrete gradient against torchdiffeq's continuous adjoint (oracle.ode_ref.odeint_adjoint) of the
    restated field at the reference's tolerances: a loose bound; the measured gap is recorded in DESIGN section 9."""
    P32, P64 = _params()
    N = 16
    gen = torch.Generator().manual_seed(8)
    x = torch.randn(N, 16, generator=gen)
    gz = torch.randn(N, 16, 16, generator=gen)
    s = Solve(P32, x, 16)
    g, _ = s.backward(gz.view(N * 16, 16))
    cont = R.continuous_adjoint(P64, x, 16, gz.double())
    gaps = [rel_err(a, b) for a, b in zip(_split(g), cont)]
    print("discrete vs continuous adjoint:", " ".join(f"{n} {v:.2e}" for n, v in zip("Wa ba Wb bb W1 b1 W2 b2".split(), gaps)))
    assert max(gaps) < 0.25, gaps          # measured 2.4e-2 .. 1.2e-1 (W1, b1 largest)


def test_cde_capacity_overflow_is_a_clean_error():
    P32, P64 = _params()
    x = torch.randn(32, 16, generator=torch.Generator().manual_seed(9))
    s = Solve(P32, x, 16, S_cap=4)
    assert s.acc == -5, (s.acc, s.trials)                          # stopped after 4 accepted steps
    for b in (s.zb, s.sb, s.hb):
        _guards_intact(b)
    _guards_intact(s.cb, -7)
    g, gb = s.backward(torch.ones(32 * 16, 16))                    # a failed forward: the backward writes nothing
    assert torch.isnan(g).all()
    _guards_intact(gb)
    seed_all(4)
    gen = G.VideoGeneratorCDE(1, 50, 0, 16, 16, ngf=8).cuda()
    gen.cde_max_steps = 4
    with pytest.raises(RuntimeError, match="cde_max_steps"):
        gen.sample_videos(8)
    with pytest.raises(RuntimeError, match="cde_max_steps"):
        gen.sample_z_m(8)


# ---- class level ----------------------------------------------------------------------------------------------------
@pytest.fixture
def schedules(monkeypatch):
    """Records the accepted schedule of every CDE solve, in launch order."""
    rec = []
    orig = _CdeGenPlan.check_solve

    def check(self):
        c = orig(self)
        s = self.sched.cpu()
        rec.append((s[:c[0]].clone(), s[self.S_cap:self.S_cap + c[0]].clone()))
        return c

    monkeypatch.setattr(_CdeGenPlan, "check_solve", check)
    return rec


class _RefCde(M.Generator):
    """The oracle's MNIST generator with the CDE latent replayed in float64 on the kernel's recorded schedules (popped in
    call order); RNG order as documented in VideoGeneratorCDE."""

    def __init__(self, ngf, schedules):
        super().__init__(1, 50, 0, 16, 16, ngf=ngf, mnist=True)
        self.ode_fn = G.CDEFunc(2, 16)               # parameter containers
        self.f = nn.Sequential(nn.Linear(2, 64), nn.LeakyReLU(0.2), nn.Linear(64, 16), nn.LeakyReLU(0.2))
        self.sched = schedules

    def _dtype(self):
        return self.f[0].weight.dtype

    def _P(self):
        fn = self.ode_fn
        return [p.double() for p in (self.f[0].weight, self.f[0].bias, self.f[2].weight, self.f[2].bias,
                                     fn.linear1.weight, fn.linear1.bias, fn.linear2.weight, fn.linear2.bias)]

    def latent(self, x):
        st, sh = self.sched.pop(0)
        return R.replay(self._P(), x, 16, st, sh)[0].float()         # [n, T, 16]

    def sample_z_m(self, n, video_len=None):
        return self.latent(torch.randn(n, 16)).reshape(-1, 16)

    def sample_images(self, n):
        T = self.video_length
        n_all = n * T * 2
        c = torch.from_numpy(np.random.normal(0, 1, (n_all, 50)).astype(np.float32))
        x = torch.randn(n_all, 16)
        j = np.sort(np.random.choice(n_all * T, n, replace=False)).astype(np.int64)
        traj, t = torch.from_numpy(j // T), torch.from_numpy(j % T)
        zm = self.latent(x[traj])[torch.arange(n), t]
        z = torch.cat([c[traj], zm], dim=1)
        return self.main(z.view(n, 66, 1, 1)), None


def _rng_state():
    return np.random.get_state()[1].copy(), torch.get_rng_state().clone()


def _same_rng(a, b):
    return np.array_equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_cde_generator_against_replayed_oracle(schedules):
    ref_npz = golden("gen_cde_init.npz")
    gen = G.VideoGeneratorCDE(1, 50, 0, 16, 16, ngf=int(ref_npz["ngf"]))
    gen.load_state_dict({k[2:]: torch.from_numpy(ref_npz[k]) for k in ref_npz.files if k.startswith("w/")})
    ref = _RefCde(int(ref_npz["ngf"]), schedules)
    ref.load_state_dict(gen.state_dict())
    gen.cuda()
    seed_all(6)
    vid, labels = gen.sample_videos(32)
    r1 = _rng_state()
    img, _ = gen.sample_images(32)
    r2 = _rng_state()
    zm = gen.sample_z_m(3)
    r3 = _rng_state()
    assert len(schedules) == 3
    seed_all(6)
    rvid, _ = ref.sample_videos(32)
    assert _same_rng(_rng_state(), r1)
    rimg, _ = ref.sample_images(32)
    assert _same_rng(_rng_state(), r2)
    rzm = ref.sample_z_m(3)
    assert _same_rng(_rng_state(), r3)
    assert vid.shape == (32, 1, 16, 28, 28) and img.shape == (32, 1, 28, 28) and zm.shape == (48, 16)
    assert rel_err(vid.detach().cpu(), rvid.detach()) < 1e-4
    assert rel_err(img.detach().cpu(), rimg.detach()) < 1e-4
    assert rel_err(zm.detach().cpu(), rzm.detach()) < 1e-4
    wv = torch.randn(vid.shape, generator=torch.Generator().manual_seed(1))
    wi = torch.randn(img.shape, generator=torch.Generator().manual_seed(2))
    wz = torch.randn(zm.shape, generator=torch.Generator().manual_seed(3))
    ((vid * wv.cuda()).sum() + (img * wi.cuda()).sum() + (zm * wz.cuda()).sum()).backward()
    ((rvid * wv).sum() + (rimg * wi).sum() + (rzm * wz).sum()).backward()
    refp = dict(ref.named_parameters())
    for k, p in gen.named_parameters():
        q = refp[k]
        if k.startswith(("recurrent.", "linear.")):
            assert p.grad is None and q.grad is None, k               # dead parameters
            continue
        assert rel_err(p.grad.cpu(), q.grad) < 1e-3, k
    assert float(gen.ode_fn.linear2.weight.grad.abs().max()) > 0


def test_cde_refusals_at_call_time():
    seed_all(1)
    gen = G.VideoGeneratorCDE(1, 50, 0, 16, 8, ngf=8).cuda()      # video_length 8 != dim_z_motion 16
    with pytest.raises(ValueError, match="video_len"):
        gen.sample_videos(2)
    with pytest.raises(ValueError, match="video_len"):
        gen.sample_z_m(2)
    gen = G.VideoGeneratorCDE(1, 50, 0, 16, 16, ngf=8).cuda()
    with pytest.raises(ValueError, match="video_len"):
        gen.sample_z_m(2, video_len=5)
    with pytest.raises(ValueError, match="4096"):
        gen.sample_videos(4097)


def _trainer_data(B, seed):
    rng = torch.Generator().manual_seed(seed)
    imgs = [torch.rand(B, 1, 28, 28, generator=rng) for _ in range(2)]
    vids = [torch.rand(B, 16, 1, 28, 28, generator=rng) for _ in range(2)]
    return imgs, vids


def test_cde_trainer_iteration_batch32_against_stock_torch_loop(schedules):
    seed_all(51)
    gen = G.VideoGeneratorCDE(1, 50, 0, 16, 16, ngf=16)
    dv, di = G.VideoDiscriminator(1, ksize=2, ndf=16), G.PatchImageDiscriminator(1, ndf=16)
    _, odv, odi = M.build_mnist(ngf=16, ndf=16)
    ogen = _RefCde(16, schedules)
    for m, o in ((gen, ogen), (dv, odv), (di, odi)):
        o.load_state_dict(m.state_dict())
        m.cuda()
    dead = {k: v.detach().clone() for k, v in gen.state_dict().items() if k.startswith(("recurrent.", "linear."))}
    tr = G.GanTrainer(gen, dv, di)
    tail = gen._arena_tail()
    assert len(tail) == 8 and all(not any(t is p for t in tail) for p in list(gen.linear.parameters()) +
                                  list(gen.recurrent.parameters()))
    opts = M.make_optimizers(ogen, odv, odi)
    imgs, vids = _trainer_data(32, 6)
    seed_all(52)
    got = [float(v) for v in tr.step([t.cuda() for t in imgs], [t.cuda() for t in vids])]
    seed_all(52)
    want = [float(v) for v in M.train_step(ogen, odv, odi, opts, imgs, vids)]
    assert not schedules
    assert np.allclose(got, want, rtol=1e-4, atol=0), (got, want)
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
    for k, v in dead.items():
        assert torch.equal(gen.state_dict()[k], v), k                  # bitwise untouched by FusedAdam
        assert torch.equal(ogen.state_dict()[k], v.cpu()), k           # and by torch's Adam
        assert dict(gen.named_parameters())[k].grad is None, k
    with pytest.raises(NotImplementedError, match="graph"):
        G.GanTrainer(gen, dv, di, graph=True)


def test_cde_prefetched_latents_are_bitwise_the_call_by_call_ones():
    runs = []
    for prefetch in (True, False):
        seed_all(53)
        gen = G.VideoGeneratorCDE(1, 50, 0, 16, 16, ngf=16)
        _, dv, di = G.build_mnist(ngf=16, ndf=16)
        gen.cuda(); dv.cuda(); di.cuda()
        tr = G.GanTrainer(gen, dv, di, prefetch_latents=prefetch)
        losses = []
        for it in range(2):
            imgs, vids = _trainer_data(8, 14 + it)
            seed_all(600 + it)
            losses.append([float(x) for x in tr.step([t.cuda() for t in imgs], [t.cuda() for t in vids])])
        torch.cuda.synchronize()
        assert not gen.__dict__.get("_prefetched")
        state = [t.detach().clone() for m in (gen, dv, di) for t in m.state_dict().values()]
        runs.append((losses, state))
    assert runs[0][0] == runs[1][0], (runs[0][0], runs[1][0])
    for a, b in zip(runs[0][1], runs[1][1]):
        assert torch.equal(a, b)


@pytest.mark.parametrize("images_first", [False, True])
def test_cde_joint_generator_pass_equals_the_two_calls(images_first):
    B = 4
    res = []
    for joint in (False, True):
        seed_all(71)
        gen = G.VideoGeneratorCDE(1, 50, 0, 16, 16, ngf=16).cuda()
        seed_all(72)
        if joint:
            (vid, _), (img, _) = gen.sample_pair(B, B, images_first=images_first)
        elif images_first:
            img, _ = gen.sample_images(B)
            vid, _ = gen.sample_videos(B)
        else:
            vid, _ = gen.sample_videos(B)
            img, _ = gen.sample_images(B)
        wv = torch.linspace(-1, 1, vid.numel(), device="cuda").view(vid.shape)
        wi = torch.linspace(1, -1, img.numel(), device="cuda").view(img.shape)
        ((vid * wv).sum() + 3.0 * (img * wi).sum()).backward()
        torch.cuda.synchronize()
        res.append((vid.detach().clone(), img.detach().clone(),
                    [(n, p.grad.clone()) for n, p in gen.named_parameters() if p.grad is not None]))
    (v0, i0, g0), (v1, i1, g1) = res
    assert float((v0 - v1).abs().max()) <= 1e-5 and float((i0 - i1).abs().max()) <= 1e-5
    assert len(g0) == len(g1) and any("ode_fn.linear1" in n for n, _ in g0)
    for (n, a), (_, b) in zip(g0, g1):
        scale = float(a.abs().max()) + 1e-6
        assert float((a - b).abs().max()) <= 5e-3 * scale, (n, float((a - b).abs().max()), scale)


def test_reference_loop_body_through_drop_in_module():
    """Two iterations of mnist_moco_cde.py's loop body (stock torch.optim.Adam, nn.BCEWithLogitsLoss) on the drop-in
    models.mocogan_cde: finite losses, nonzero CDEFunc and pre-net gradients."""
    from models.mocogan_cde import VideoGeneratorCDE
    seed_all(71)
    gen = VideoGeneratorCDE(1, 50, 0, 16, 16, ngf=16).cuda()
    dv = G.VideoDiscriminator(1, ksize=2, ndf=16).cuda()
    di = G.PatchImageDiscriminator(1, ndf=16).cuda()
    bce = torch.nn.BCEWithLogitsLoss()
    mk = lambda m: torch.optim.Adam(m.parameters(), lr=2e-4, betas=(0.5, 0.999), weight_decay=1e-5)  # noqa: E731
    og, ov, oi = mk(gen), mk(dv), mk(di)
    B = 8
    for it in range(2):
        imgs, vids = _trainer_data(B, 90 + it)
        real_img, real_vid = imgs[0].cuda(), vids[0].cuda()
        oi.zero_grad()
        pr, _ = di(real_img)
        with torch.no_grad():
            fake, _ = gen.sample_images(B)
        pf, _ = di(fake)
        li = bce(pr, torch.ones_like(pr)) + bce(pf, torch.zeros_like(pf))
        li.backward(); oi.step()
        ov.zero_grad()
        pr, _ = dv(real_vid.transpose(1, 2))
        with torch.no_grad():
            fake, _ = gen.sample_videos(B)
        pf, _ = dv(fake)
        lv = bce(pr, torch.ones_like(pr)) + bce(pf, torch.zeros_like(pf))
        lv.backward(); ov.step()
        og.zero_grad()
        fv, _ = gen.sample_videos(B)
        fi, _ = gen.sample_images(B)
        pv, _ = dv(fv)
        pi, _ = di(fi)
        lg = bce(pv, torch.ones_like(pv)) + bce(pi, torch.ones_like(pi))
        lg.backward()
        for p in list(gen.ode_fn.parameters()) + list(gen.f.parameters()):
            assert p.grad is not None and float(p.grad.abs().max()) > 0
        for p in list(gen.linear.parameters()) + list(gen.recurrent.parameters()):
            assert p.grad is None
        og.step()
        assert all(np.isfinite(float(v)) for v in (li, lv, lg))
