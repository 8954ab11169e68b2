"""CPU: GANODETrainer's algebra on its plain-torch path (parameters off the GPU) -- the three step rules against the fp64
restatement of tests/odegan_ref.py and against the reference class's own results (tests/golden/odegan_tiny.npz), the
central-difference penalty against double backward in fp64, and the constructor's contract."""
import numpy as np
import pytest
import torch
import torch.nn as nn

import odegan_cases as K
import odegan_ref as R
from conftest import golden, seed_all

import gan_ode_amd as G

U = 2.0 ** -24


@pytest.fixture(scope="module")
def fix():
    return golden("odegan_tiny.npz")


def _quad(dtype):
    init = K.quad_init()
    return [init[n].to(dtype).clone().requires_grad_() for n in K.QUAD_NAMES]


@pytest.mark.parametrize("method", K.METHODS)
def test_step_rules_against_restatement_and_reference(fix, method):
    ps = _quad(torch.float32)
    tr = G.GANODETrainer(ps, [], None, lambda: K.quad_loss(*ps), None, None, lr=K.QUAD_LR, reg=0.0, method=method)
    p0 = [p.detach().clone() for p in ps]
    loss = tr.step(model="gen")
    assert float(loss.detach()) == float(K.quad_loss(*p0).detach())                # the first-stage loss
    # the closure's gradient is the closed form the bound below is built from
    for g, c in zip(torch.autograd.grad(K.quad_loss(*ps), ps, allow_unused=True), K.quad_grad(*[p.detach() for p in ps])):
        assert (g is None) == (c is None) and (g is None or torch.allclose(g, c, rtol=1e-5, atol=1e-6))
    r64 = _quad(torch.float64)
    assert float(R.ode_step(r64, lambda: K.quad_loss(*r64), method, K.QUAD_LR)) == pytest.approx(float(loss.detach()), rel=1e-6)
    stages = {"euler": 1, "rk2": 2, "rk4": 4}[method]
    g0 = K.quad_grad(*[p.double() for p in p0])
    for n, p, start, ref, g in zip(K.QUAD_NAMES, ps, p0, r64, g0):
        if g is None:
            assert torch.equal(p.detach(), start), n               # the unused tensor: bitwise untouched
            assert torch.equal(torch.from_numpy(fix[f"quad/{method}/{n}"]), start)
            continue
        # <= 4 roundings per stage on each side, each relative to a partial sum below |p| + lr * sum_k |g_k|; the stage
        # gradients stay within a factor 2 of the starting one on this problem (lr * curvature <= 0.4)
        tol = 16 * U * (ref.detach().abs() + K.QUAD_LR * stages * 2 * g.abs())
        for what, other in (("restatement", ref.detach()), ("reference", torch.from_numpy(fix[f"quad/{method}/{n}"]).double())):
            err = (p.detach().double() - other).abs()
            assert bool((err <= tol * (2 if what == "reference" else 1)).all()), (method, n, what, float(err.max()), float(tol.min()))
        assert float((p.detach() - start).abs().max()) > 1e-3      # (and it did move)


def test_stage_plan_keeps_the_references_two_quirks():
    from gan_ode_amd.ode_training import stage_plan
    lr, reg = 0.02, 0.01
    assert stage_plan("euler", lr, reg, True) == [({1: -lr}, -reg, 1)]                     # reg * gp: no lr factor
    assert stage_plan("rk2", lr, reg, True)[-1][1] == -reg * lr
    rk4 = stage_plan("rk4", lr, reg, True)
    assert rk4[-1][1] == -reg * lr and [s[2] for s in rk4] == [1, 1, 2, 1]                 # stage 3 checks g2
    assert all(s[1] is None for s in stage_plan("rk4", lr, reg, False))
    # the increments add up to the classical RK4 weights
    total = {k: 0.0 for k in range(1, 5)}
    for coefs, _, _ in rk4:
        for k, c in coefs.items():
            total[k] += c
    assert [total[k] / lr for k in range(1, 5)] == pytest.approx([-1 / 6, -1 / 3, -1 / 3, -1 / 6])


class _SmoothGen(nn.Module):
    """A small generator on stock modules with smooth activations; draws from BOTH host generators."""

    def __init__(self, bn=False):
        super().__init__()
        self.net = nn.Sequential(nn.Linear(8, 16), nn.BatchNorm1d(16) if bn else nn.Identity(), nn.Tanh(), nn.Linear(16, 64), nn.Tanh())
        self.unused = nn.Parameter(torch.ones(3))

    def sample(self, n):
        zc = torch.from_numpy(np.random.normal(0, 1, (n, 2))).to(self.net[0].weight.dtype)
        zm = torch.randn(n, 6).to(self.net[0].weight.dtype)
        return self.net(torch.cat([zc, zm], 1)).view(n, 1, 8, 8)


def _smooth_pair(bn=False, dtype=torch.float64):
    torch.manual_seed(3)
    gen = _SmoothGen(bn).to(dtype)
    dis = nn.Sequential(nn.Conv2d(1, 4, 3, 2, 1), nn.Tanh(), nn.Conv2d(4, 1, 4)).to(dtype)
    g_loss = lambda: K.bce(dis(gen.sample(4)).flatten(), 1.0)  # noqa: E731
    real = torch.randn(4, 1, 8, 8, dtype=dtype)
    d_loss = lambda: K.bce(dis(real).flatten(), 1.0) + K.bce(dis(gen.sample(4).detach()).flatten(), 0.0)  # noqa: E731
    return gen, dis, g_loss, d_loss


def test_penalty_central_difference_against_double_backward_fp64():
    gen, dis, g_loss, d_loss = _smooth_pair()
    gp_, dp_ = list(gen.parameters()), list(dis.parameters())
    seed_all(9)
    exact = R.exact_penalty(g_loss, gp_, dp_)
    seed_all(9)
    g_loss()
    after_one = R.rng_state()
    tr = G.GANODETrainer(gp_, dp_, None, g_loss, d_loss, None, lr=0.02, reg=0.01, method="rk4")
    assert tr.fd_h == pytest.approx(float(np.finfo(np.float32).eps) ** (1 / 3))
    before = [p.detach().clone() for p in gp_]
    errs = []
    for h in (tr.fd_h, tr.fd_h / 2):
        tr.fd_h = h
        seed_all(9)
        gp = tr.grad_penalty("dis_img")
        s = R.rng_state()
        assert torch.equal(s[0], after_one[0]) and all(np.array_equal(a, b) for a, b in zip(s[1], after_one[1]))
        assert all(torch.equal(p.detach(), b) for p, b in zip(gp_, before))          # generator: bitwise unchanged
        num = max(float((a - e).abs().max()) for a, e in zip(gp, exact))
        errs.append(num / max(float(e.abs().max()) for e in exact))
    print("central-difference error at h, h/2:", errs)
    assert errs[0] < 1e-3
    assert 3.0 <= errs[0] / errs[1] <= 5.0, errs                                      # the error is O(h^2)


@pytest.mark.parametrize("method", K.METHODS)
def test_penalised_step_is_the_restatement_with_the_same_penalty(method):
    gen, dis, g_loss, d_loss = _smooth_pair()
    gen2, dis2, g_loss2, d_loss2 = _smooth_pair()
    tr = G.GANODETrainer(gen.parameters(), dis.parameters(), None, g_loss, d_loss, None, lr=0.05, reg=0.3, method=method)
    seed_all(4)
    tr.step(model="dis_img")
    # the restatement, fed the same draws in the same order: loss1, then the penalty's single g_loss call, then the rest
    gp, n = [], [0]

    def loss_fn():
        loss = d_loss2()
        n[0] += 1
        if n[0] == 1:
            gp.extend(R.central_penalty(g_loss2, list(gen2.parameters()), list(dis2.parameters()), tr.fd_h)[0])
        return loss

    seed_all(4)
    R.ode_step(list(dis2.parameters()), loss_fn, method, 0.05, reg=0.3, gp=gp)
    for a, b in zip(dis.parameters(), dis2.parameters()):
        assert torch.allclose(a.detach(), b.detach(), rtol=0, atol=1e-12), float((a - b).abs().max())
    assert all(torch.equal(a.detach(), b.detach()) for a, b in zip(gen.parameters(), gen2.parameters()))
    # (Euler's penalty term carries no lr: with lr = 0.05 a reg * lr * gp update would miss the line above by 0.95 * reg * gp)
    assert max(float(g.abs().max()) for g in gp) * 0.3 * 0.95 > 1e-6


def test_constructor_contract():
    ps = _quad(torch.float32)
    with pytest.raises(AssertionError, match="euler"):
        G.GANODETrainer(ps, [], None, lambda: 0, None, None, method="heun")
    import inspect
    sig = inspect.signature(G.GANODETrainer.__init__)
    assert list(sig.parameters)[1:] == ["g_params", "dImg_params", "dVid_params", "g_loss", "dImg_loss", "dVid_loss", "lr",
                                        "reg", "method", "d_iter", "g_iter", "modules"]
    assert [sig.parameters[k].default for k in ("lr", "reg", "method", "d_iter", "g_iter", "modules")] == [0.02, 0.01, "rk4", 2, 1, None]
    from stage2.ode_training import GANODETrainer as shim
    assert shim is G.GANODETrainer
    noisy = G.PatchImageDiscriminator(1, ndf=8, use_noise=True, noise_sigma=0.1)
    gen = _SmoothGen()
    with pytest.raises(NotImplementedError, match="use_noise"):
        G.GANODETrainer(gen.parameters(), noisy.parameters(), None, None, None, None, reg=0.01, modules=(gen, noisy, None))
    G.GANODETrainer(gen.parameters(), noisy.parameters(), None, None, None, None, reg=0.0, modules=(gen, noisy, None))


def test_modules_restores_batchnorm_buffers():
    def buffers_after(modules):
        gen, dis, g_loss, d_loss = _smooth_pair(bn=True, dtype=torch.float32)
        tr = G.GANODETrainer(gen.parameters(), dis.parameters(), None, g_loss, d_loss, None, reg=0.01, method="euler",
                             modules=(gen, dis, None) if modules else None)
        seed_all(2)
        tr.step(model="dis_img")
        return [b.clone() for b in gen.buffers()]

    # what the reference leaves behind: one d_loss and ONE g_loss evaluation
    gen, dis, g_loss, d_loss = _smooth_pair(bn=True, dtype=torch.float32)
    seed_all(2)
    d_loss(); g_loss()
    want = [b.clone() for b in gen.buffers()]
    got = buffers_after(True)
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    assert not all(torch.equal(a, b) for a, b in zip(buffers_after(False), want))      # the documented deviation
