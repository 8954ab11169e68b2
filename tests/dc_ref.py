"""Test infrastructure: stock-torch restatement of stage 2's CIFAR DCGAN (stage2/test_ODE_training_with_cifar_GAN.ipynb) in
the dtype it is given, the fixed problems the host and GPU tests share, and the trainer problems on tests/odegan_ref.py.

Kinks decide the problems.  At the stock initialisation the discriminator's pre-activations have a standard deviation of
0.01-0.4, and at full width some hundreds of each layer's 10^5-10^6 LeakyReLU inputs lie within 1e-5 of zero at every seed: two
correct fp32 evaluations then disagree about slopes and a gradient comparison means nothing.  Hence three kinds of problem:

  (a) narrow, mixed sign, kink-clear: nz = 16, (ngf = ndf = 8, B in {1, 2, 3}) and (ngf = ndf = 16, B = 2); the notebook's
      initialisation at a seed with the discriminator's eight weights multiplied by D_GAINS (every pre-activation's standard
      deviation ~1-1.5), the seed being the first for which the fp64 run keeps every ReLU / LeakyReLU input 2e-5 away from zero
      (tests/test_host_dcgan.py asserts 1e-5; `python scripts/make_dcgan_goldens.py --search` finds the seeds again);
  (b) full-width discriminator, sign-definite: |W| with every layer rescaled so that its pre-activations have mean magnitude 1
      on the problem's own kind of input (unscaled the output reaches 3e10); a uniform [0.1, 1] input makes every
      pre-activation positive, its negative every one negative (slope 0.1 on every element of every layer);
  (c) full-width generator, kink-free: every BatchNorm with gamma = 1, beta = +6, so every ReLU input is ~6 +- 5 (the device of
      test_motion_latent_gradients_kink_free_full_width); the head's weight times C_HEAD_GAIN, because 576 inputs of ~6 would
      saturate the tanh at the Xavier scale (pre-activations ~8, 1 - tanh^2 ~ 1e-6: a gradient of rounding noise), and the three
      transposed convolutions' weights times C_CONVT_GAIN, for the eval-mode pass: after ONE train pass the running statistics
      are 0.1 mean and 0.9 + 0.1 var, and with inputs of ~6 the Xavier-scale outputs have per-channel means of ~+-3.5 (up to 10
      over 256 channels), which the running mean does not yet remove -- at a tenth of the scale the eval-mode ReLU inputs are
      6 +- 1.  Train-mode BatchNorm divides the gain out again.
"""
import functools
import os

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

import odegan_ref

NZ, NGF, NDF, NC, IMAGE = 128, 64, 64, 3, 32


# ---------------------------------------------------------------------------------------------------------------
# the networks
KINK = [float("inf")]         # smallest |ReLU / LeakyReLU input| seen since reset_kink()


def reset_kink():
    KINK[0] = float("inf")


def _run_main(main, x):
    """nn.Sequential's forward with the activations applied out of place and their inputs' distance from zero recorded"""
    for m in main:
        if isinstance(m, nn.LeakyReLU):
            KINK[0] = min(KINK[0], float(x.detach().abs().min()))
            x = F.leaky_relu(x, m.negative_slope)
        elif isinstance(m, nn.ReLU):
            KINK[0] = min(KINK[0], float(x.detach().abs().min()))
            x = F.relu(x)
        else:
            x = m(x)
    return x


def weights_init(m):
    """The notebook's initialisation, chosen by class name as it does: Xavier-uniform convolution weights; BatchNorm weights
    from N(1, 0.02) and zero BatchNorm biases."""
    name = type(m).__name__
    if "Conv" in name:
        nn.init.xavier_uniform_(m.weight, gain=1.0)
    elif "BatchNorm" in name:
        nn.init.normal_(m.weight, 1.0, 0.02)
        nn.init.zeros_(m.bias)


class Generator(nn.Module):
    def __init__(self, ngpu, nz=NZ, ngf=NGF, nc=NC):
        super().__init__()
        self.ngpu, self.ngf = ngpu, ngf
        self.project = nn.Conv2d(nz, ngf * 8 * 4 * 4, 1, 1, 0, bias=False)
        self.main = nn.Sequential(
            nn.ConvTranspose2d(ngf * 8, ngf * 4, 4, 2, 1, bias=False), nn.BatchNorm2d(ngf * 4), nn.ReLU(True),
            nn.ConvTranspose2d(ngf * 4, ngf * 2, 4, 2, 1, bias=False), nn.BatchNorm2d(ngf * 2), nn.ReLU(True),
            nn.ConvTranspose2d(ngf * 2, ngf, 4, 2, 1, bias=False), nn.BatchNorm2d(ngf), nn.ReLU(True),
            nn.Conv2d(ngf, nc, 3, 1, 1, bias=False), nn.Tanh())

    def forward(self, input):
        return _run_main(self.main, self.project(input).view(-1, self.ngf * 8, 4, 4))


class Discriminator(nn.Module):
    def __init__(self, ngpu, ndf=NDF, nc=NC):
        super().__init__()
        self.ngpu = ngpu
        self.main = nn.Sequential(
            nn.Conv2d(nc, ndf, 3, 1, 1, bias=False), nn.LeakyReLU(0.1, inplace=True),
            nn.Conv2d(ndf, ndf, 4, 2, 1, bias=False), nn.LeakyReLU(0.1, inplace=True),
            nn.Conv2d(ndf, ndf * 2, 3, 1, 1, bias=False), nn.LeakyReLU(0.1, inplace=True),
            nn.Conv2d(ndf * 2, ndf * 2, 4, 2, 1, bias=False), nn.LeakyReLU(0.1, inplace=True),
            nn.Conv2d(ndf * 2, ndf * 4, 3, 1, 1, bias=False), nn.LeakyReLU(0.1, inplace=True),
            nn.Conv2d(ndf * 4, ndf * 4, 4, 2, 1, bias=False), nn.LeakyReLU(0.1, inplace=True),
            nn.Conv2d(ndf * 4, ndf * 8, 3, 1, 1, bias=False), nn.LeakyReLU(0.1, inplace=True),
            nn.Conv2d(ndf * 8, 1, 4, 1, 0, bias=False))

    def forward(self, input):
        return _run_main(self.main, input).view(-1, 1).squeeze(1)


D_CONVS = tuple(f"main.{2 * i}.weight" for i in range(8))
G_BNS = (1, 4, 7)


@functools.lru_cache(maxsize=None)
def initial_weights(nz, ngf, ndf, seed):
    """(G state_dict, D state_dict) in fp32: the notebook's order under torch.manual_seed(seed) -- Generator, its
    weights_init, Discriminator, its weights_init."""
    torch.manual_seed(seed)
    G = Generator(1, nz, ngf)
    G.apply(weights_init)
    D = Discriminator(1, ndf)
    D.apply(weights_init)
    return ({k: v.clone() for k, v in G.state_dict().items()}, {k: v.clone() for k, v in D.state_dict().items()})


def _clone(sd):
    return {k: v.clone() for k, v in sd.items()}


def _rel_err(a, b):
    a, b = torch.as_tensor(a).double().flatten(), torch.as_tensor(b).double().flatten()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def _dev_dtype(net):
    p = next(net.parameters())
    return p.device, p.dtype


def _cpu(t):
    return t.detach().cpu().clone()


# ---------------------------------------------------------------------------------------------------------------
# (a) narrow, mixed sign, kink-clear: both networks, both losses
A_NZ = 16
D_GAINS = (3.5, 1.5, 2.1, 1.4, 1.2, 1.4, 1.9, 1.0)
A_CASES = ((8, 1), (8, 2), (8, 3), (16, 2))                      # (ngf = ndf, B)
A_SEED = {(8, 1): 1, (8, 2): 4, (8, 3): 4, (16, 2): 60}


def a_weights(w, seed):
    gsd, dsd = initial_weights(A_NZ, w, w, seed)
    gsd, dsd = _clone(gsd), _clone(dsd)
    for k, gain in zip(D_CONVS, D_GAINS):
        dsd[k] *= gain
    return gsd, dsd


def a_restated(w, seed, dtype):
    G, D = Generator(1, A_NZ, w), Discriminator(1, w)
    gsd, dsd = a_weights(w, seed)
    G.load_state_dict(gsd), D.load_state_dict(dsd)
    return G.to(dtype), D.to(dtype)


def a_load_product(G, D, w, seed):
    gsd, dsd = a_weights(w, seed)
    G.load_state_dict(gsd), D.load_state_dict(dsd)
    return G, D


def a_inputs(B, seed):
    """(z [B, nz, 1, 1], real [B, 3, 32, 32] uniform in [-1, 1]) in fp32"""
    g = torch.Generator().manual_seed(3000 + seed)
    return torch.randn(B, A_NZ, 1, 1, generator=g), torch.rand(B, NC, IMAGE, IMAGE, generator=g) * 2 - 1


def run_pair(G, D, criterion, z, real):
    """The arithmetic of the notebook's two closures on fixed inputs.  Pass 1 (dis_loss): G(z), D(real), D(G(z)) and the sum of
    the two criteria with labels in the data's dtype; pass 2 (gen_loss): D(G(z)) against ones with dtype=float.  Every parameter
    gradient of both networks from both losses, the gradients to z and to the real batch, and the generator's buffers after
    the two passes (two momentum updates with the same batch statistics).  -> {name: CPU tensor}"""
    dev, dt = _dev_dtype(G)
    B = z.shape[0]
    gp, dp = dict(G.named_parameters()), dict(D.named_parameters())
    names = ["G." + n for n in gp] + ["D." + n for n in dp]
    params = list(gp.values()) + list(dp.values())
    res = {}
    z1 = z.to(device=dev, dtype=dt).contiguous().requires_grad_(True)
    r1 = real.to(device=dev, dtype=dt).contiguous().requires_grad_(True)
    fake = G(z1)
    d_real, d_fake = D(r1), D(fake)
    loss_d = (criterion(d_real, torch.full((B,), 1, dtype=dt, device=dev))
              + criterion(d_fake, torch.full((B,), 0, dtype=dt, device=dev)))
    grads = torch.autograd.grad(loss_d, params + [z1, r1])
    res.update({"G(z)": _cpu(fake), "D(real)": _cpu(d_real), "D(G(z))": _cpu(d_fake), "loss_d": _cpu(loss_d).reshape(1)})
    res.update({"d/" + n: _cpu(g) for n, g in zip(names + ["z", "real"], grads)})
    z2 = z.to(device=dev, dtype=dt).contiguous().requires_grad_(True)
    loss_g = criterion(D(G(z2)), torch.full((B,), 1, dtype=float, device=dev))
    grads = torch.autograd.grad(loss_g, params + [z2])
    res["loss_g"] = _cpu(loss_g).reshape(1)
    res.update({"g/" + n: _cpu(g) for n, g in zip(names + ["z"], grads)})
    res.update({"buf/" + n: _cpu(b) for n, b in G.named_buffers()})
    return res


@functools.lru_cache(maxsize=None)
def a_reference(w, B, seed=None):
    """(fp64 results, fp32 CPU results, smallest |ReLU / LeakyReLU input| of the fp64 run)"""
    seed = A_SEED[w, B] if seed is None else seed
    z, real = a_inputs(B, seed)
    res = {}
    for dt in (torch.float64, torch.float32):
        G, D = a_restated(w, seed, dt)
        reset_kink()
        res[dt] = run_pair(G, D, nn.BCEWithLogitsLoss(), z, real)
        if dt == torch.float64:
            kink = KINK[0]
    return res[torch.float64], res[torch.float32], kink


# ---------------------------------------------------------------------------------------------------------------
# (b) full-width discriminator, sign-definite
B_CASES = (3, 64)
B_SEED = 0


def b_input(B, sign):
    """(x [B, 3, 32, 32] uniform in [0.1, 1] times sign, upstream weights r [B]: loss = sum(out * r)) in fp32"""
    g = torch.Generator().manual_seed(4000 + B)
    return (torch.rand(B, NC, IMAGE, IMAGE, generator=g) * 0.9 + 0.1) * sign, torch.randn(B, generator=g)


@functools.lru_cache(maxsize=None)
def b_weights(sign):
    """|W| of the notebook's initialisation at B_SEED, layer l times 1 / mean |pre-activation l| of the fp64 pass over the
    variant's B = 3 input with the layers before it already scaled.  fp32 state_dict."""
    dsd = _clone(initial_weights(NZ, NGF, NDF, B_SEED)[1])
    x = b_input(3, sign)[0].double()
    strides = (1, 2, 1, 2, 1, 2, 1, 1)
    pads = (1, 1, 1, 1, 1, 1, 1, 0)
    for l, k in enumerate(D_CONVS):
        W = dsd[k].abs().double()
        pre = F.conv2d(x, W, None, strides[l], pads[l])
        W = (W / float(pre.abs().mean())).float()
        dsd[k] = W
        x = F.leaky_relu(F.conv2d(x, W.double(), None, strides[l], pads[l]), 0.1)
    return dsd


def run_disc(D, x, r):
    """-> {'out', 'x': input gradient, '<param name>': gradient} as CPU tensors; x keeps the strides it comes with"""
    dev, dt = _dev_dtype(D)
    x = x.to(device=dev, dtype=dt).requires_grad_(True)
    out = D(x)
    params = dict(D.named_parameters())
    grads = torch.autograd.grad((out * r.to(device=dev, dtype=dt)).sum(), list(params.values()) + [x])
    res = {"out": _cpu(out)}
    res.update({n: _cpu(g) for n, g in zip(list(params) + ["x"], grads)})
    return res


@functools.lru_cache(maxsize=None)
def b_reference(B, sign, with_fp32=True):
    """(fp64 results, fp32 CPU results or None, smallest |pre-activation| of the fp64 run: every one has the sign of `sign`)"""
    x, r = b_input(B, sign)
    res = {}
    for dt in (torch.float64, torch.float32) if with_fp32 else (torch.float64,):
        D = Discriminator(1)
        D.load_state_dict(b_weights(sign))
        reset_kink()
        res[dt] = run_disc(D.to(dt), x, r)
        if dt == torch.float64:
            kink = KINK[0]
    return res[torch.float64], res.get(torch.float32), kink


# ---------------------------------------------------------------------------------------------------------------
# (c) full-width generator, kink-free
C_CASES = (3, 64)
C_SEED = 0
C_HEAD_GAIN = 0.05
C_CONVT_GAIN = 0.1


def c_weights():
    gsd = _clone(initial_weights(NZ, NGF, NDF, C_SEED)[0])
    for i in G_BNS:
        gsd[f"main.{i}.weight"].fill_(1.0)
        gsd[f"main.{i}.bias"].fill_(6.0)
        gsd[f"main.{i - 1}.weight"] *= C_CONVT_GAIN
    gsd["main.9.weight"] *= C_HEAD_GAIN
    return gsd


def c_input(B):
    """(z [B, nz, 1, 1], upstream weights r [B, 3, 32, 32]: loss = sum(out * r)) in fp32"""
    g = torch.Generator().manual_seed(5000 + B)
    return torch.randn(B, NZ, 1, 1, generator=g), torch.randn(B, NC, IMAGE, IMAGE, generator=g)


def run_gen(G, z, r):
    """-> {'out', 'z': its gradient, '<param name>': gradient, 'buf/<name>': buffers after the pass} as CPU tensors"""
    dev, dt = _dev_dtype(G)
    z = z.to(device=dev, dtype=dt).contiguous().requires_grad_(True)
    out = G(z)
    params = dict(G.named_parameters())
    grads = torch.autograd.grad((out * r.to(device=dev, dtype=dt)).sum(), list(params.values()) + [z])
    res = {"out": _cpu(out)}
    res.update({n: _cpu(g) for n, g in zip(list(params) + ["z"], grads)})
    res.update({"buf/" + n: _cpu(b) for n, b in G.named_buffers()})
    return res


def run_gen_train_then_eval(G, B):
    """One train-mode pass at B, then (B = 3 only) the same pass in eval mode on the running statistics it left."""
    z, r = c_input(B)
    G.train()
    res = {"train/" + k: v for k, v in run_gen(G, z, r).items()}
    if B == 3:
        G.eval()
        res.update({"eval/" + k: v for k, v in run_gen(G, z, r).items()})
        G.train()
    return res


@functools.lru_cache(maxsize=None)
def c_reference(B, with_fp32=True):
    """(fp64 results, fp32 CPU results or None, smallest |ReLU input| of the fp64 run)"""
    res = {}
    for dt in (torch.float64, torch.float32) if with_fp32 else (torch.float64,):
        G = Generator(1)
        G.load_state_dict(c_weights())
        reset_kink()
        res[dt] = run_gen_train_then_eval(G.to(dt), B)
        if dt == torch.float64:
            kink = KINK[0]
    return res[torch.float64], res.get(torch.float32), kink


# ---------------------------------------------------------------------------------------------------------------
# forward only, full width, stock initialisation (values are continuous across a kink; gradients are not compared)
F_B, F_SEED = 16, 0


def run_forward(G, D, criterion):
    dev, dt = _dev_dtype(G)
    z = torch.randn(F_B, NZ, 1, 1, generator=torch.Generator().manual_seed(6000)).to(device=dev, dtype=dt)
    with torch.no_grad():
        fake = G(z)
        out = D(fake)
        # dis_loss's criterion on the fake batch: labels in the data's dtype, so the fp32 restatement's loss is an fp32 number
        # (gen_loss's dtype=float labels make stock torch return the fp64 mean of these ~0.69 values, which an fp32 loss can
        # only match to half an ulp: that restatement's error says nothing about fp32 arithmetic)
        loss = criterion(out, torch.full((F_B,), 0, dtype=dt, device=dev))
    return {"G(z)": _cpu(fake), "D(G(z))": _cpu(out), "loss_fake": _cpu(loss).reshape(1)}


def f_load(G, D):
    gsd, dsd = initial_weights(NZ, NGF, NDF, F_SEED)
    G.load_state_dict(gsd), D.load_state_dict(dsd)
    return G, D


@functools.lru_cache(maxsize=None)
def f_reference():
    res = {}
    for dt in (torch.float64, torch.float32):
        G, D = f_load(Generator(1), Discriminator(1))
        res[dt] = run_forward(G.to(dt), D.to(dt), nn.BCEWithLogitsLoss())
    return res[torch.float64], res[torch.float32]


# ---------------------------------------------------------------------------------------------------------------
# trainer problems on (a) at ngf = ndf = 8, B = 2: the notebook's closures
T_W, T_B = 8, 2
TRAINER_LR = 0.01                                   # the notebook's step_size
TRAINER_SEED = {"euler": 13, "rk2": 41, "rk4": 41}
PENALTY_SEED = 0


def real_batch(seed):
    """the `data` of a CIFAR loader step: [images, labels]"""
    g = torch.Generator().manual_seed(7000 + seed)
    return [torch.rand(T_B, NC, IMAGE, IMAGE, generator=g) * 2 - 1, torch.zeros(T_B, dtype=torch.int64)]


def closures(G, D, criterion, device, dtype=torch.float32, randn=None):
    """dis_loss(data), gen_loss() of the notebook's closure cell.  randn(*shape): the noise source; by default torch's CPU
    generator, moved to the device (so that a restatement and the product see the same values); the notebook's own is
    torch.randn(..., device=device)."""
    if randn is None:
        def randn(*shape):
            return torch.randn(*shape).to(device=device, dtype=dtype)

    def dis_loss(data):
        D.zero_grad()
        real = data[0].to(device=device, dtype=dtype)
        n = real.size(0)
        loss_real = criterion(D(real), torch.full((n,), 1, dtype=real.dtype, device=device))
        fake = G(randn(n, A_NZ, 1, 1))
        loss_fake = criterion(D(fake), torch.full((n,), 0, dtype=real.dtype, device=device))
        return loss_real + loss_fake

    def gen_loss():
        G.zero_grad()
        noise = randn(T_B, A_NZ, 1, 1)
        label = torch.full((T_B,), 1, dtype=float, device=device)
        return criterion(D(G(noise)), label)

    return dis_loss, gen_loss


def seed_all(s):
    torch.manual_seed(s)
    np.random.seed(s)


def params_of(net):
    return {n: p.detach().cpu().clone() for n, p in net.named_parameters()}


def delta_of(net, before):
    return {n: p.detach().cpu().double() - before[n].double() for n, p in net.named_parameters()}


def reference_steps(method, dtype, seed=None):
    """One dis_img step, then one gen step (reg = 0) on the restatement: -> (D deltas, G deltas, kink along the whole step)."""
    seed = TRAINER_SEED[method] if seed is None else seed
    G, D = a_restated(T_W, seed, dtype)
    d_loss, g_loss = closures(G, D, nn.BCEWithLogitsLoss(), "cpu", dtype)
    x = real_batch(seed)
    bD, bG = params_of(D), params_of(G)
    reset_kink()
    seed_all(seed)
    odegan_ref.ode_step(list(D.parameters()), lambda: d_loss(x), method, TRAINER_LR)
    odegan_ref.ode_step(list(G.parameters()), g_loss, method, TRAINER_LR)
    return delta_of(D, bD), delta_of(G, bG), KINK[0]


@functools.lru_cache(maxsize=None)
def trainer_reference(method):
    d64, g64, kink = reference_steps(method, torch.float64)
    d32, g32, _ = reference_steps(method, torch.float32)
    return (d64, g64), (d32, g32), kink


def reference_penalty(dtype, h, seed=None):
    """odegan_ref.central_penalty of the restatement at the step h -> (gp per D parameter name, kink)."""
    seed = PENALTY_SEED if seed is None else seed
    G, D = a_restated(T_W, seed, dtype)
    _, g_loss = closures(G, D, nn.BCEWithLogitsLoss(), "cpu", dtype)
    reset_kink()
    seed_all(seed)
    gp, _ = odegan_ref.central_penalty(g_loss, list(G.parameters()), list(D.parameters()), h)
    return {n: g.detach() for (n, _), g in zip(D.named_parameters(), gp)}, KINK[0]


@functools.lru_cache(maxsize=None)
def penalty_reference(h):
    gp64, kink = reference_penalty(torch.float64, h)
    gp32, _ = reference_penalty(torch.float32, h)
    return gp64, gp32, kink


# ---------------------------------------------------------------------------------------------------------------
# the fp32 CPU restatement's own error against the fp64 one, per tensor (conftest.rel_err): what the GPU tests' 8x allowance is
# taken from.  The figure depends on the host's BLAS and thread count, so it is measured once (one thread) by
# scripts/make_dcgan_goldens.py and stored.
OWN_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dcgan_own.npz")


def measure_own(h):
    """Every figure of OWN_FILE, from the functions above (h: the trainer's central-difference step)."""
    out = {}
    for w, B in A_CASES:
        r64, r32, _ = a_reference(w, B)
        for n in r64:
            out[f"a/{w}/{B}/{n}"] = _rel_err(r32[n], r64[n])
    for B in B_CASES:
        for sign in (1, -1):
            r64, r32, _ = b_reference(B, sign)
            for n in r64:
                out[f"b/{B}/{sign}/{n}"] = _rel_err(r32[n], r64[n])
    for B in C_CASES:
        r64, r32, _ = c_reference(B)
        for n in r64:
            out[f"c/{B}/{n}"] = _rel_err(r32[n], r64[n])
    r64, r32 = f_reference()
    for n in r64:
        out[f"f/{n}"] = _rel_err(r32[n], r64[n])
    for m in TRAINER_SEED:
        (d64, g64), (d32, g32), _ = trainer_reference(m)
        for tag, q64, q32 in (("D", d64, d32), ("G", g64, g32)):
            for n in q64:
                out[f"step/{m}/{tag}/{n}"] = _rel_err(q32[n], q64[n])
    gp64, gp32, _ = penalty_reference(h)
    for n in gp64:
        out[f"penalty/{n}"] = _rel_err(gp32[n], gp64[n])
    return out


@functools.lru_cache(maxsize=None)
def stored_own():
    z = np.load(OWN_FILE)
    return {k: float(z[k]) for k in z.files}
