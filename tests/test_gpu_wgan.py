"""GPU: the Wasserstein loss (gode_wgan_logits) and the parameter noise (gode_param_noise, gode_adam_noise_multi[_dev])
against the restatements of tests/wgan_ref.py, and GanTrainer(loss="wasserstein", param_noise=...) against the
reference loop bodies of mnist_moco_ode_wgan.py / mnist_moco_ode_noise.py on stock torch."""
import ctypes as C
import importlib
import sys
import types

import numpy as np
import pytest
import torch

import wgan_ref as W
from conftest import assert_weights_after_adam, rel_err, seed_all
from guarded import guarded_tensors as _guarded_tensors

import gan_ode_amd as G
import gan_ode_amd._lib as L
from oracle import mocogan_ref as M

pytestmark = pytest.mark.gpu
NAN = float("nan")


def stream():
    return torch.cuda.current_stream().cuda_stream


def _words(seed, nstream, step, off, n):
    out = torch.empty(n, dtype=torch.float32, device="cuda")
    L.check(L.lib().gode_param_noise(out.data_ptr(), n, seed, nstream, step, off, 1.0, 2, stream()), "gode_param_noise")
    return out.cpu().view(torch.int32).numpy().view(np.uint32)


def _normals(seed, nstream, step, off, n):
    out = torch.empty(n, dtype=torch.float32, device="cuda")
    L.check(L.lib().gode_param_noise(out.data_ptr(), n, seed, nstream, step, off, 1.0, 0, stream()), "gode_param_noise")
    return out


@pytest.mark.parametrize("off,n", [(0, 1), (1, 5), (3, 4097), (7, 1 << 20), (1000003, 12345), (0, 1 << 24)])
def test_raw_stream_matches_the_restatement(off, n):
    seed, nstream, step = 0x1234_5678_9ABC_DEF0, 2, 17
    assert np.array_equal(_words(seed, nstream, step, off, n), W.noise_words(seed, nstream, step, off, n))
    z = _normals(seed, nstream, step, off, n).cpu().double().numpy()
    ref = W.noise_normals(seed, nstream, step, off, n)
    assert np.abs(z - ref).max() < 1e-5
    # accumulate = 1: p + fp32(z * sigma), two roundings, against torch's two CPU ops on the kernel's own normals
    if n <= 1 << 20:
        p = torch.randn(n, generator=torch.Generator().manual_seed(n)).cuda()
        q = p.clone()
        L.check(L.lib().gode_param_noise(q.data_ptr(), n, seed, nstream, step, off, 3e-4, 1, stream()), "noise")
        z32 = _normals(seed, nstream, step, off, n).cpu()
        assert torch.equal(q.cpu(), p.cpu() + z32 * np.float32(3e-4))


def test_stream_moments_and_independence():
    N = 1 << 24
    a = _normals(5, 0, 1, 0, N).double()
    m, v = float(a.mean()), float(a.var())
    assert abs(m) < 5 / N ** 0.5 and abs(v - 1) < 5 * (2 / N) ** 0.5, (m, v)
    k4 = float((a ** 4).mean())
    assert abs(k4 - 3) < 5 * (96 / N) ** 0.5, k4
    for other in (_normals(5, 0, 2, 0, N).double(), _normals(5, 1, 1, 0, N).double(), _normals(6, 0, 1, 0, N).double()):
        r = float((a * other).mean() / (a.std() * other.std()))
        assert abs(r) < 5 / N ** 0.5, r
    lag = float((a[:-1] * a[1:]).mean())
    assert abs(lag) < 5 / N ** 0.5, lag


def test_wasserstein_loss_op_against_torchgan_restatement():
    g = torch.Generator().manual_seed(3)
    for shape in ((32,), (7, 1, 3, 3), (2000,)):
        fx, fgz = torch.randn(shape, generator=g), torch.randn(shape, generator=g)
        for red in ("mean", "sum"):
            # generator, one tensor
            x = fgz.cuda().requires_grad_()
            loss = G.WassersteinGeneratorLoss(reduction=red)(x)
            loss.backward()
            r = fgz.clone().requires_grad_()
            rl = W.WassersteinGeneratorLoss(reduction=red)(r)
            rl.backward()
            assert abs(float(loss) - float(rl.detach())) <= 1e-6 * max(1.0, abs(float(rl.detach()))), (float(loss), float(rl.detach()))
            assert torch.equal(x.grad.cpu(), r.grad)
            # discriminator, two tensors
            a, b = fx.cuda().requires_grad_(), fgz.cuda().requires_grad_()
            loss = G.WassersteinDiscriminatorLoss(reduction=red)(a, b)
            loss.backward()
            ra, rb = fx.clone().requires_grad_(), fgz.clone().requires_grad_()
            rl = W.WassersteinDiscriminatorLoss(reduction=red)(ra, rb)
            rl.backward()
            assert abs(float(loss) - float(rl)) <= 1e-6 * max(1.0, abs(float(rl)))
            assert torch.equal(a.grad.cpu(), ra.grad) and torch.equal(b.grad.cpu(), rb.grad)
        # joint [real; fake] halves and the two-term generator loss (accumulate)
        j = torch.cat([fx, fgz]).cuda().requires_grad_()
        loss = G.wasserstein_discriminator_loss_halves(j)
        loss.backward()
        rj = torch.cat([fx, fgz]).requires_grad_()
        rl = W.wasserstein_discriminator_loss(rj[:fx.shape[0]], rj[fx.shape[0]:])
        rl.backward()
        assert abs(float(loss) - float(rl)) <= 1e-6 * max(1.0, abs(float(rl)))
        assert torch.equal(j.grad.cpu(), rj.grad)
        a, b = fx.cuda().requires_grad_(), fgz.cuda().requires_grad_()
        loss = G.wasserstein_generator_loss_pair(a, b)
        (loss * 3.0).backward()                      # a caller-supplied upstream gradient
        ra, rb = fx.clone().requires_grad_(), fgz.clone().requires_grad_()
        rl = W.wasserstein_generator_loss(ra) + W.wasserstein_generator_loss(rb)
        (rl * 3.0).backward()
        assert abs(float(loss) - float(rl)) <= 2e-6 * max(1.0, abs(float(rl)))
        # (torch scales before dividing by n, the loss node after: one rounding apart)
        assert torch.allclose(a.grad.cpu(), ra.grad, rtol=2e-7, atol=0) and torch.allclose(b.grad.cpu(), rb.grad, rtol=2e-7, atol=0)


def _adam64(p, g, m, v, step, lr=2e-4, b1=0.5, b2=0.999, eps=1e-8, wd=1e-5):
    g = g + wd * p
    m = b1 * m + (1 - b1) * g
    v = b2 * v + (1 - b2) * g * g
    denom = np.sqrt(v) / np.sqrt(1 - b2 ** step) + eps
    return p - lr / (1 - b1 ** step) * m / denom, m, v


def test_fused_adam_noise_against_float64_and_dev_variant_bitwise():
    sizes = [1, 5, 64, 1003, 4096, 70001, 70001, 9]
    has_grad = [True, False, True, True, False, True, False, True]
    seed, nstream, sigma = 99, 1, 1e-3
    rng = torch.Generator().manual_seed(4)
    offs = W.noise_offsets([torch.empty(n) for n in sizes])
    init = [torch.randn(n, generator=rng) for n in sizes]
    grads = [torch.randn(n, generator=rng) for n in sizes]
    runs = []
    for dev_variant in (False, True):
        bufs = [_guarded_tensors(sizes) for _ in range(4)]          # p, g, m, v
        P, Gr, Mm, V = [b[1] for b in bufs]
        for k in range(len(sizes)):
            P[k].copy_(init[k]); Gr[k].copy_(grads[k]); Mm[k].zero_(); V[k].zero_()
        rows = [(P[k].data_ptr(), Gr[k].data_ptr() if has_grad[k] else 0, Mm[k].data_ptr() if has_grad[k] else 0,
                 V[k].data_ptr() if has_grad[k] else 0, sizes[k], offs[k]) for k in range(len(sizes))]
        table = torch.tensor(rows, dtype=torch.int64).cuda()
        lib = L.lib()
        for step in (1, 2):
            if dev_variant:
                c0, c1 = G.FusedAdam.step_coefficients(2e-4, 0.5, 0.999, step)
                coef = torch.tensor([c0, c1, 0.0, 0.0])
                coef.view(torch.int32)[2] = step + 10
                coef = coef.cuda()
                L.check(lib.gode_adam_noise_multi_dev(table.data_ptr(), len(sizes), max(sizes), 0.5, 0.999, 1e-8, 1e-5, 1.0,
                                                      coef.data_ptr(), seed, nstream, sigma, stream()), "dev")
            else:
                L.check(lib.gode_adam_noise_multi(table.data_ptr(), len(sizes), max(sizes), 2e-4, 0.5, 0.999, 1e-8, 1e-5,
                                                  1.0, step, seed, nstream, step + 10, sigma, stream()), "eager")
        torch.cuda.synchronize()
        for b, views in bufs:                     # nothing written outside the tensors
            mask = torch.ones_like(b, dtype=torch.bool)
            for vw in views:
                o = (vw.data_ptr() - b.data_ptr()) // 4
                mask[o:o + vw.numel()] = False
            assert torch.isnan(b[mask]).all()
        for k in range(len(sizes)):
            if not has_grad[k]:
                assert torch.equal(Mm[k].cpu(), torch.zeros(sizes[k])) and torch.equal(V[k].cpu(), torch.zeros(sizes[k]))
        runs.append([t.cpu().clone() for t in P + Mm + V])
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    # float64 Adam + the restated noise (noise-only rows: p + fp32(z * sigma) exactly, on the kernel's own normals)
    for k, n in enumerate(sizes):
        p, m, v = init[k].double().numpy(), np.zeros(n), np.zeros(n)
        for step in (1, 2):
            if has_grad[k]:
                p, m, v = _adam64(p, grads[k].double().numpy(), m, v, step)
            p = p + sigma * W.noise_normals(seed, nstream, step + 10, offs[k], n)
        assert np.abs(runs[0][k].double().numpy() - p).max() < 2e-6, k
        if not has_grad[k]:
            q = init[k].clone()
            for step in (1, 2):
                q = q + _normals(seed, nstream, step + 10, offs[k], n).cpu() * np.float32(sigma)
            assert torch.equal(runs[0][k], q), k


def _nets(seed, ngf=16):
    seed_all(seed)
    gen, dv, di = G.build_mnist(ngf=ngf, ndf=ngf)
    ogen, odv, odi = M.build_mnist(ngf=ngf, ndf=ngf)
    for m, o in zip((gen, dv, di), (ogen, odv, odi)):
        o.load_state_dict(m.state_dict())
        m.cuda()
    return (gen, dv, di), (ogen, odv, odi)


def _data(B, seed, n=2):
    rng = torch.Generator().manual_seed(seed)
    return ([torch.rand(B, 1, 28, 28, generator=rng) for _ in range(n)],
            [torch.rand(B, 16, 1, 28, 28, generator=rng) for _ in range(n)])


@pytest.mark.parametrize("loss,sigma", [("wasserstein", 1e-4), ("bce", 1e-5)])
def test_trainer_iteration_batch32_against_reference_loop(loss, sigma):
    (gen, dv, di), (ogen, odv, odi) = _nets(81)
    tr = G.GanTrainer(gen, dv, di, loss=loss, param_noise=sigma, noise_seed=2024)
    opts = M.make_optimizers(ogen, odv, odi)
    imgs, vids = _data(32, 8)
    seed_all(82)
    got = [float(v) for v in tr.step([t.cuda() for t in imgs], [t.cuda() for t in vids])]
    seed_all(82)
    steps = [0, 0, 0]
    want = [float(v) for v in W.train_step(ogen, odv, odi, opts, imgs, vids, loss=loss, sigma=sigma, seed=2024,
                                           noise_steps=steps)]
    assert steps == [1, 2, 2]
    assert [tr.gen_opt.param_groups[0]["noise_step"], tr.vid_opt.param_groups[0]["noise_step"],
            tr.img_opt.param_groups[0]["noise_step"]] == steps
    # (a Wasserstein loss is a difference of means and may sit near zero: compare at the logits' scale)
    scale = 1.0 if loss == "wasserstein" else 0.0
    for a, b in zip(got, want):
        assert abs(a - b) <= 1e-4 * abs(b) + 1e-5 * scale, (got, want)
    for m, o in zip((gen, dv, di), (ogen, odv, odi)):
        osd = o.state_dict()
        for k, v in m.state_dict().items():
            w = osd[k]
            if v.dtype == torch.int64:
                assert int(v) == int(w), k
            elif "running_" in k:
                assert rel_err(v.cpu(), w) < 5e-3, k
            elif k.startswith("recurrent."):       # no gradient, noise only: the same fp32 operations on both sides
                assert (v.cpu() - w).abs().max() < 1e-7, k
            else:
                assert_weights_after_adam(v, w, k)


def _run_trainer(graph, iters=6, seed=31, **kw):
    seed_all(seed)
    gen, dv, di = G.build_mnist(ngf=16, ndf=16)
    gen.cuda(); dv.cuda(); di.cuda()
    tr = G.GanTrainer(gen, dv, di, graph=graph, **kw)
    rng = torch.Generator().manual_seed(10)
    losses = []
    for it in range(iters):
        imgs = [torch.rand(8, 1, 28, 28, generator=rng).cuda() for _ in range(2)]
        vids = [torch.rand(8, 16, 1, 28, 28, generator=rng).cuda() for _ in range(2)]
        seed_all(300 + it)
        losses.append([float(v) for v in tr.step(imgs, vids)])
    torch.cuda.synchronize()
    state = [v.detach().clone() for m in (gen, dv, di) for v in m.state_dict().values()]
    state += [tr.gen_opt.state[p]["exp_avg_sq"].clone() for p in gen.parameters() if tr.gen_opt.state.get(p)]
    return tr, losses, state


def test_graph_replay_is_bitwise_the_eager_schedule_with_noise():
    runs = []
    for graph in (True, False):
        tr, losses, state = _run_trainer(graph, loss="wasserstein", param_noise=1e-4, noise_seed=5)
        assert (tr._graph is not None) == graph
        runs.append((losses, state, [o.param_groups[0]["noise_step"] for o in (tr.gen_opt, tr.vid_opt, tr.img_opt)]))
    assert runs[0][0] == runs[1][0], (runs[0][0], runs[1][0])
    for a, b in zip(runs[0][1], runs[1][1]):
        assert torch.equal(a, b)
    assert runs[0][2] == runs[1][2] == [6, 12, 12]


def test_schedules_keep_their_equivalences_with_noise():
    """side stream, prefetch and arena gradients off: bitwise the default schedule; unpaired discriminator passes and
    separate generator calls: the same losses up to the summation order of the weight gradients (as for BCE)."""
    base = _run_trainer(False, iters=2, loss="wasserstein", param_noise=1e-4, noise_seed=5)
    serial = _run_trainer(False, iters=2, loss="wasserstein", param_noise=1e-4, noise_seed=5, overlap_image_d=False,
                          prefetch_latents=False, direct_grads=False)
    assert base[1] == serial[1]
    for a, b in zip(base[2], serial[2]):
        assert torch.equal(a, b)
    unpaired = _run_trainer(False, iters=2, loss="wasserstein", param_noise=1e-4, noise_seed=5, pair_d_passes=False,
                            joint_generator_passes=False)
    assert np.allclose(base[1][0], unpaired[1][0], rtol=1e-4, atol=1e-5), (base[1], unpaired[1])


def test_noisy_step_repacks_the_weights():
    seed_all(41)
    gen, dv, di = G.build_mnist(ngf=16, ndf=16)
    gen.cuda(); dv.cuda(); di.cuda()
    tr = G.GanTrainer(gen, dv, di, loss="wasserstein", param_noise=1e-4)
    imgs, vids = _data(8, 3)
    seed_all(42)
    tr.step([t.cuda() for t in imgs], [t.cuda() for t in vids])
    fresh, _, _ = G.build_mnist(ngf=16, ndf=16)
    fresh.load_state_dict(gen.state_dict())
    fresh.cuda()
    seed_all(43)
    with torch.no_grad():
        a, _ = gen.sample_videos(4)
    seed_all(43)
    with torch.no_grad():
        b, _ = fresh.sample_videos(4)
    assert torch.equal(a, b)


def test_checkpoint_resumes_the_same_noise_stream(tmp_path):
    imgs0, vids0 = _data(8, 20)
    imgs1, vids1 = _data(8, 21)
    seed_all(60)
    gen, dv, di = G.build_mnist(ngf=16, ndf=16)
    gen.cuda(); dv.cuda(); di.cuda()
    tr = G.GanTrainer(gen, dv, di, loss="wasserstein", param_noise=1e-4, noise_seed=77)
    seed_all(61)
    tr.step([t.cuda() for t in imgs0], [t.cuda() for t in vids0])
    path = tmp_path / "ck.pt"
    torch.save({"model_state_dict": [m.state_dict() for m in (gen, dv, di)],
                "optimizer_state_dict": [o.state_dict() for o in (tr.gen_opt, tr.vid_opt, tr.img_opt)]}, path)
    seed_all(62)
    want = [float(v) for v in tr.step([t.cuda() for t in imgs1], [t.cuda() for t in vids1])]
    ck = torch.load(path, map_location="cpu", weights_only=True)
    seed_all(999)                            # another process seed: the stream comes from the checkpoint
    gen2, dv2, di2 = G.build_mnist(ngf=16, ndf=16)
    for m, sd in zip((gen2, dv2, di2), ck["model_state_dict"]):
        m.load_state_dict(sd)
        m.cuda()
    tr2 = G.GanTrainer(gen2, dv2, di2, loss="wasserstein", param_noise=1e-4)
    for o, sd in zip((tr2.gen_opt, tr2.vid_opt, tr2.img_opt), ck["optimizer_state_dict"]):
        o.load_state_dict(sd)
    assert tr2.gen_opt.param_groups[0]["noise_seed"] == 77 and tr2.gen_opt.param_groups[0]["noise_step"] == 1
    seed_all(62)
    got = [float(v) for v in tr2.step([t.cuda() for t in imgs1], [t.cuda() for t in vids1])]
    assert got == want
    for a, b in zip([v for m in (gen, dv, di) for v in m.state_dict().values()],
                    [v for m in (gen2, dv2, di2) for v in m.state_dict().values()]):
        assert torch.equal(a, b)


def test_reference_driver_loop_body_through_the_drop_in_losses(monkeypatch):
    """mnist_moco_ode_wgan.py:13 imports the losses from torchgan.losses; with a stand-in module that re-exports
    gan_ode_amd's, the script's loop body (stock Adam + add_noise) runs on the GPU networks and agrees with the same
    body on the oracle networks with the restated torchgan losses."""
    pkg, mod = types.ModuleType("torchgan"), types.ModuleType("torchgan.losses")
    mod.WassersteinGeneratorLoss, mod.WassersteinDiscriminatorLoss = G.WassersteinGeneratorLoss, G.WassersteinDiscriminatorLoss
    pkg.losses = mod
    monkeypatch.setitem(sys.modules, "torchgan", pkg)
    monkeypatch.setitem(sys.modules, "torchgan.losses", mod)
    losses = importlib.import_module("torchgan.losses")
    (gen, dv, di), (ogen, odv, odi) = _nets(91, ngf=8)
    opts = M.make_optimizers(gen, dv, di)
    oopts = M.make_optimizers(ogen, odv, odi)
    imgs, vids = _data(8, 9)
    seed_all(92)
    got = [float(v) for v in W.train_step(gen, dv, di, opts, [t.cuda() for t in imgs], [t.cuda() for t in vids], sigma=1e-4,
                                          seed=3, gen_loss_fn=losses.WassersteinGeneratorLoss(),
                                          dis_loss_fn=losses.WassersteinDiscriminatorLoss())]
    seed_all(92)
    want = [float(v) for v in W.train_step(ogen, odv, odi, oopts, imgs, vids, sigma=1e-4, seed=3)]
    for a, b in zip(got, want):
        assert abs(a - b) <= 1e-4 * abs(b) + 1e-5, (got, want)
    for (k, v), (_, w) in zip(dv.state_dict().items(), odv.state_dict().items()):
        if v.dtype == torch.float32 and "running_" not in k:
            assert_weights_after_adam(v, w, k)
