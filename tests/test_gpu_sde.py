"""GPU: the Neural-SDE motion latent (models/mocogan_sde.py; gode_sde_fwd / gode_sde_bwd) against a float64 restatement
of the discrete forward written here -- torchsde's fixed-step Euler-Maruyama loop on the schedule of sde_grid_arrays,
Brownian increments sqrt(dt_k) xi_k -- whose gradients come from torch autograd.  The generator class is checked against
the oracle's MNIST decoder fed with that restated latent, replaying the documented RNG order, and one GanTrainer
iteration against a stock-torch loop (oracle discriminators + Adam + the restatement)."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import assert_weights_after_adam, rel_err, seed_all

import gan_ode_amd as G
import gan_ode_amd._lib as L
from gan_ode_amd.modules import sde_grid_arrays
from oracle import mocogan_ref as M
from sde_ref import _ops, _params, _sched_dev, restate

pytestmark = pytest.mark.gpu
TOL = 1e-4
DT = 2.5e-2


def stream():
    return torch.cuda.current_stream().cuda_stream


@pytest.mark.parametrize("N,T", [(32, 16), (20, 5), (33, 2), (300, 3), (8192, 16)])
@pytest.mark.parametrize("prenet", [True, False])
def test_sde_kernels_against_float64_restatement(N, T, prenet):
    grid = sde_grid_arrays(T, DT)
    S = grid["S"]
    params = _params(prenet)
    g = torch.Generator().manual_seed(N * 31 + T)
    x = torch.randn(1 + S, N, 16, generator=g)
    content = torch.randn(N, 50, generator=g)
    sel = torch.randint(0, T, (N,), generator=g, dtype=torch.int32)
    P64 = [p.double().requires_grad_() for p in params]
    st_ref, out_ref = restate(P64, x.double(), grid, prenet)
    P = [p.cuda() for p in params]
    sd = _sched_dev(grid)
    xd, cd, seld = x.cuda(), content.cuda(), sel.cuda()
    zc = 96
    npar = L.SDE_NPARAM if prenet else L.SDE_NPARAM - 2128
    work = torch.empty(L.lib().gode_sde_bwd_work_size(N), device="cuda")
    for select in (False, True):
        rows = N if select else N * T
        z = torch.full((rows, zc), float("nan"), device="cuda")
        states = torch.full((N, S + 1, 16), float("nan"), device="cuda")
        fop, bop = _ops(P, prenet, N, T, sd, xd, cd, seld if select else None, z, states, zc)
        L.run_one(fop, stream())
        zz = z.cpu()
        assert rel_err(states.cpu(), st_ref.detach()) < TOL
        ar = torch.arange(N)
        if select:
            want = out_ref[ar, sel.long()]
            assert rel_err(zz[:, :16], want.detach()) < TOL
            assert torch.equal(zz[:, 16:66], content)
        else:
            want = out_ref
            assert rel_err(zz[:, :16].view(N, T, 16), out_ref.detach()) < TOL
            assert torch.equal(zz[:, 16:66].view(N, T, 50), content[:, None, :].expand(N, T, 50))
        assert float(zz[:, 66:].abs().max()) == 0
        # a second forward is bitwise the first
        z2 = torch.full_like(z, float("nan"))
        st2 = torch.full_like(states, float("nan"))
        fop2, _ = _ops(P, prenet, N, T, sd, xd, cd, seld if select else None, z2, st2, zc)
        L.run_one(fop2, stream())
        assert torch.equal(z2, z) and torch.equal(st2, states)
        # backward: gradients of sum(out * gup) wrt all 12 (8) tensors, into a buffer with NaN guards on both sides
        gup = torch.randn(want.shape, generator=g, dtype=torch.float64)
        ref = torch.autograd.grad((want * gup).sum(), P64, retain_graph=True)
        gz = torch.zeros(rows, zc, device="cuda")
        gz[:, :16] = gup.float().reshape(rows, 16).cuda()
        bop.gz, bop.work = gz.data_ptr(), work.data_ptr()
        for acc in (0, 1):
            guard = 64
            buf = torch.full((npar + 2 * guard,), float("nan"), device="cuda")
            base = torch.randn(npar, generator=g)
            if acc:
                buf[guard:guard + npar] = base.cuda()
            bop.grads, bop.accumulate = buf[guard:].data_ptr(), acc
            L.run_one(bop, stream())
            b = buf.cpu()
            assert torch.isnan(b[:guard]).all() and torch.isnan(b[guard + npar:]).all()
            got = b[guard:guard + npar] - (base if acc else 0)
            o = 0
            for r, p in zip(ref, params):
                k = p.numel()
                assert rel_err(got[o:o + k].view(p.shape), r) < TOL, (select, acc, o)
                o += k
            assert o == npar
            if not acc:
                first = b[guard:guard + npar].clone()
                L.run_one(bop, stream())                      # a second backward is bitwise the first
                assert torch.equal(buf.cpu()[guard:guard + npar], first)


def test_sde_noise_plumbing_moments():
    """Zero drift, diffusion 1, x0 = 0, no pre-net: output j is y_k + w1[j] sqrt(dt_k) xi_k with y_k a sum of the
    increments, so it has mean 0 and variance t_k + w1[j]^2 dt_k (read off the schedule) -- independent of the
    restatement.  N = 8192 trajectories x 16 features per output."""
    N, T = 8192, 16
    grid = sde_grid_arrays(T, DT)
    S = grid["S"]
    P = [torch.zeros(s, device="cuda") for s in [(16, 16), (16,), (16, 16), (16,)] * 2]
    P[7].fill_(1.0)                                     # bg2 = 1: g(y) = 1
    x = torch.randn(1 + S, N, 16, generator=torch.Generator().manual_seed(11))
    x[0] = 0
    sd = _sched_dev(grid)
    z = torch.empty(N * T, 16, device="cuda")
    states = torch.empty(N, S + 1, 16, device="cuda")
    fop, _ = _ops(P, False, N, T, sd, x.cuda(), None, None, z, states, 16)
    L.run_one(fop, stream())
    out = z.cpu().double().view(N, T, 16)
    tk = torch.cat([torch.zeros(1, dtype=torch.float64), torch.cumsum(grid["dt"].double(), 0)])
    M_ = N * 16
    for j in range(1, T):
        k = int(grid["emit_at"][j])
        var = float(tk[k] + grid["w1"][j].double() ** 2 * grid["dt"][k].double())
        v = out[:, j].flatten()
        assert abs(float(v.mean())) < 5 * (var / M_) ** 0.5, j
        assert abs(float(v.var()) - var) < 5 * var * (2.0 / M_) ** 0.5, j
    assert float(out[:, 0].abs().max()) == 0


# ---- class level ----------------------------------------------------------------------------------------------------
class _RefSde(M.Generator):
    """The oracle's MNIST generator with the SDE latent restated above; RNG order as documented in VideoGeneratorSDE."""

    def __init__(self, ngf):
        super().__init__(1, 50, 0, 16, 16, ngf=ngf, mnist=True)
        self.ode_fn = G.SDEFunc(16, 16)          # parameter container only
        self.grid = sde_grid_arrays(16, DT)

    def _dtype(self):
        return self.ode_fn.drift_fn[0].weight.dtype

    def _prm(self):
        d, s = self.ode_fn.drift_fn, self.ode_fn.diffusion_fn
        lin = self.linear
        return [lin[0].weight, lin[0].bias, lin[2].weight, lin[2].bias, d[0].weight, d[0].bias, d[2].weight, d[2].bias,
                s[0].weight, s[0].bias, s[2].weight, s[2].bias]

    def latent(self, x0, xi):
        return restate(self._prm(), torch.cat([x0[None], xi]), self.grid, True)[1]

    def sample_z_m(self, n, video_len=None):
        x0 = torch.randn(n, 16)
        xi = torch.randn(self.grid["S"], n, 16)
        return self.latent(x0, xi).reshape(-1, 16)

    def sample_images(self, n):
        T = self.video_length
        n_all = n * T * 2
        c = torch.from_numpy(np.random.normal(0, 1, (n_all, 50)).astype(np.float32))
        x0 = torch.randn(n_all, 16)
        j = np.sort(np.random.choice(n_all * T, n, replace=False)).astype(np.int64)
        traj, t = torch.from_numpy(j // T), torch.from_numpy(j % T)
        xi = torch.randn(self.grid["S"], n, 16)
        zm = self.latent(x0[traj], xi)[torch.arange(n), t]
        z = torch.cat([c[traj], zm], dim=1)
        return self.main(z.view(n, 66, 1, 1)), None


def _gen_pair(seed, ngf=8):
    seed_all(seed)
    gen = G.VideoGeneratorSDE(1, 50, 0, 16, 16, ngf=ngf)
    ref = _RefSde(ngf)
    ref.load_state_dict(gen.state_dict())
    return gen.cuda(), ref


def test_sde_generator_against_restated_oracle():
    gen, ref = _gen_pair(5)
    seed_all(6)
    vid, labels = gen.sample_videos(4)
    img, _ = gen.sample_images(4)
    zm = gen.sample_z_m(3)
    seed_all(6)
    rvid, _ = ref.sample_videos(4)
    rimg, _ = ref.sample_images(4)
    rzm = ref.sample_z_m(3)
    assert vid.shape == (4, 1, 16, 28, 28) and img.shape == (4, 1, 28, 28) and zm.shape == (48, 16)
    assert rel_err(vid.detach().cpu(), rvid.detach()) < TOL
    assert rel_err(img.detach().cpu(), rimg.detach()) < TOL
    assert rel_err(zm.detach().cpu(), rzm.detach()) < TOL
    wv = torch.randn(vid.shape, generator=torch.Generator().manual_seed(1))
    wi = torch.randn(img.shape, generator=torch.Generator().manual_seed(2))
    wz = torch.randn(zm.shape, generator=torch.Generator().manual_seed(3))
    ((vid * wv.cuda()).sum() + (img * wi.cuda()).sum() + (zm * wz.cuda()).sum()).backward()
    ((rvid * wv).sum() + (rimg * wi).sum() + (rzm * wz).sum()).backward()
    for (k, p), (_, q) in zip(gen.named_parameters(), ref.named_parameters()):
        if q.grad is None:
            assert p.grad is None, k          # the GRU cell is dead weight
            continue
        assert rel_err(p.grad.cpu(), q.grad) < 1e-3, k
    assert float(gen.ode_fn.diffusion_fn[0].weight.grad.abs().max()) > 0


def test_sde_generator_without_prenet_video_len_and_dt():
    seed_all(8)
    gen = G.VideoGeneratorSDE(1, 50, 0, 16, 16, linear=False, ngf=8).cuda()
    gen.sde_dt = 0.1
    grid = sde_grid_arrays(5, 0.1)
    seed_all(9)
    zm = gen.sample_z_m(7, video_len=5)
    seed_all(9)
    x0 = torch.randn(7, 16)
    xi = torch.randn(grid["S"], 7, 16)
    prm = [p.detach() for p in gen._param_list()[1]]
    _, want = restate([p.cpu().double() for p in prm], torch.cat([x0[None], xi]).double(), grid, False)
    assert rel_err(zm.detach().cpu(), want.reshape(-1, 16)) < TOL
    zm.sum().backward()
    assert gen.ode_fn.drift_fn[0].weight.grad is not None


def _trainer_data(B, seed):
    rng = torch.Generator().manual_seed(seed)
    imgs = [torch.rand(B, 1, 28, 28, generator=rng) for _ in range(2)]
    vids = [torch.rand(B, 16, 1, 28, 28, generator=rng) for _ in range(2)]
    return imgs, vids


def test_sde_trainer_iteration_batch32_against_stock_torch_loop():
    seed_all(51)
    gen = G.VideoGeneratorSDE(1, 50, 0, 16, 16, ngf=16)
    dv, di = G.VideoDiscriminator(1, ksize=2, ndf=16), G.PatchImageDiscriminator(1, ndf=16)
    _, odv, odi = M.build_mnist(ngf=16, ndf=16)
    ogen = _RefSde(16)
    for m, o in ((gen, ogen), (dv, odv), (di, odi)):
        o.load_state_dict(m.state_dict())
        m.cuda()
    tr = G.GanTrainer(gen, dv, di)
    opts = M.make_optimizers(ogen, odv, odi)
    imgs, vids = _trainer_data(32, 6)
    seed_all(52)
    got = [float(v) for v in tr.step([t.cuda() for t in imgs], [t.cuda() for t in vids])]
    seed_all(52)
    want = [float(v) for v in M.train_step(ogen, odv, odi, opts, imgs, vids)]
    assert np.allclose(got, want, rtol=TOL, atol=0), (got, want)
    for m, o in zip((gen, dv, di), (ogen, odv, odi)):
        for (k, v), (_, w) in zip(m.state_dict().items(), o.state_dict().items()):
            if v.dtype == torch.int64:
                assert int(v) == int(w), k
            elif "running_" in k:
                assert rel_err(v.cpu(), w) < 5e-3, k
            else:
                assert_weights_after_adam(v, w, k)


def test_sde_prefetched_latents_are_bitwise_the_call_by_call_ones():
    """GanTrainer(prefetch_latents=True) (default) draws every call's host inputs up front in call order and issues the
    latent kernels on a side stream: losses, weights and buffers bit-identical to the call-by-call schedule."""
    runs = []
    for prefetch in (True, False):
        seed_all(53)
        gen = G.VideoGeneratorSDE(1, 50, 0, 16, 16, ngf=16)
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
def test_sde_joint_generator_pass_equals_the_two_calls(images_first):
    """sample_pair: the two calls' latents (same draws, same order) decoded in one pass; frames equal to fp32 rounding
    of the other GEMM tiles, latent and decoder gradients up to the summation order of the weight gradients."""
    B = 4
    res = []
    for joint in (False, True):
        seed_all(71)
        gen = G.VideoGeneratorSDE(1, 50, 0, 16, 16, ngf=16).cuda()
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
    assert len(g0) == len(g1) and any("diffusion_fn" in n for n, _ in g0)
    for (n, a), (_, b) in zip(g0, g1):
        scale = float(a.abs().max()) + 1e-6
        # (4-sample BatchNorm batches amplify the summation-order difference: measured up to 1.1e-3 on main.0.weight)
        assert float((a - b).abs().max()) <= 5e-3 * scale, (n, float((a - b).abs().max()), scale)


def test_reference_loop_body_through_drop_in_module():
    """Two iterations of mnist_moco_sde.py's loop body (stock torch.optim.Adam, nn.BCEWithLogitsLoss) on the drop-in
    models.mocogan_sde: finite losses, nonzero drift and diffusion gradients."""
    from models.mocogan_sde import VideoGeneratorSDE
    seed_all(71)
    gen = VideoGeneratorSDE(1, 50, 0, 16, 16, ngf=16).cuda()
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
        for net in (gen.ode_fn.drift_fn, gen.ode_fn.diffusion_fn):
            for p in net.parameters():
                assert p.grad is not None and float(p.grad.abs().max()) > 0
        og.step()
        assert all(np.isfinite(float(v)) for v in (li, lv, lg))
