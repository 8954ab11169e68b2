"""Test infrastructure: stock-torch restatement of stage 2's fully-connected MNIST GAN
(stage2/test_ODE_training_with_MNIST_GAN.ipynb) in the dtype it is given, a NumPy restatement of the dropout stream of
include/gode.h (Philox4x32-10, the 23-bit uniform, the keep rule), and the fixed problems the host and GPU tests share.

The restatement's Discriminator makes the same torch.randint draw at the same point as the product's and takes its masks
from mask_fn(key, layer, shape) -- by default the NumPy stream, so both sides drop the same elements.

Weights: the notebook's initialisation at a seed, with the hidden layers' weights multiplied by GAINS.  At the stock
initialisation the pre-activations of the wide layers have a standard deviation of ~0.1, and among the ~10^5 LeakyReLU inputs
of a batch some lie within fp32 rounding of zero for every seed; the gains bring the standard deviation to ~1-2, where a seed
can be chosen for which no LeakyReLU input is closer to the kink than 1e-5 (tests/test_host_fcgan.py asserts it), so no two
correct fp32 evaluations can disagree about a slope.
"""
import functools
import os

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

import odegan_ref

DROP_P = np.float32(0.3)
Z_DIM, MNIST_DIM = 100, 784
DROP_TAG = 0x40000000
M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85


# ---------------------------------------------------------------------------------------------------------------
# the dropout stream
def philox4x32_10(c, k0, k1):
    """c: uint32 [4][n] counters -> uint32 [4][n] outputs (Salmon et al., 10 rounds)."""
    c = [np.asarray(x, dtype=np.uint64) for x in c]
    k0, k1 = int(k0), int(k1)
    mask = np.uint64(0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]
        hi0, lo0, hi1, lo1 = p0 >> np.uint64(32), p0 & mask, p1 >> np.uint64(32), p1 & mask
        c = [hi1 ^ c[1] ^ np.uint64(k0), lo1, hi0 ^ c[3] ^ np.uint64(k1), lo0]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return np.stack([x.astype(np.uint32) for x in c])


def uniform23(words):
    """((x >> 9) + 0.5) * 2^-23: exact in fp32, in (0, 1)"""
    return ((words >> np.uint32(9)).astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -23)


def keep_mask(key, layer, n, p=DROP_P):
    """bool [n]: element e is kept iff its uniform is >= p (fp32).  Counter (q lo, 0, tag | layer, q hi), q = e >> 2, lane e & 3."""
    key = int(key) & 0xFFFFFFFFFFFFFFFF
    q = np.arange((n + 3) // 4, dtype=np.uint64)
    zeros = np.zeros_like(q)
    out = philox4x32_10([q & np.uint64(0xFFFFFFFF), zeros, zeros + np.uint64(DROP_TAG | int(layer)), q >> np.uint64(32)],
                        key & 0xFFFFFFFF, key >> 32)
    return (uniform23(out.T.reshape(-1)[:n]) >= np.float32(p))


def mask_tensor(key, layer, shape, dtype=torch.float32):
    return torch.from_numpy(keep_mask(key, layer, int(np.prod(shape))).reshape(tuple(shape))).to(dtype)


# ---------------------------------------------------------------------------------------------------------------
# the networks
KINK = [float("inf")]         # smallest |LeakyReLU input| seen since reset_kink()


def reset_kink():
    KINK[0] = float("inf")


def _lrelu(x):
    KINK[0] = min(KINK[0], float(x.detach().abs().min()))
    return F.leaky_relu(x, 0.2)


class Generator(nn.Module):
    def __init__(self, g_input_dim, g_output_dim):
        super().__init__()
        self.fc1 = nn.Linear(g_input_dim, 256)
        self.fc2 = nn.Linear(self.fc1.out_features, self.fc1.out_features * 2)
        self.fc3 = nn.Linear(self.fc2.out_features, self.fc2.out_features * 2)
        self.fc4 = nn.Linear(self.fc3.out_features, g_output_dim)

    def forward(self, x):
        x = _lrelu(self.fc1(x))
        x = _lrelu(self.fc2(x))
        x = _lrelu(self.fc3(x))
        return torch.tanh(self.fc4(x))


class Discriminator(nn.Module):
    def __init__(self, d_input_dim, mask_fn=mask_tensor):
        super().__init__()
        self.fc1 = nn.Linear(d_input_dim, 1024)
        self.fc2 = nn.Linear(self.fc1.out_features, self.fc1.out_features // 2)
        self.fc3 = nn.Linear(self.fc2.out_features, self.fc2.out_features // 2)
        self.fc4 = nn.Linear(self.fc3.out_features, 1)
        self.mask_fn = mask_fn
        self.keys = []

    def _drop(self, x, key, layer):
        scale = 1.0 / (1.0 - float(DROP_P))                   # the product: fp32(1 / (1 - fp32(0.3)))
        return x * self.mask_fn(key, layer, x.shape, x.dtype) * scale

    def forward(self, x):
        key = int(torch.randint(0, 2 ** 62, (1,)))
        self.keys.append(key)
        x = self._drop(_lrelu(self.fc1(x)), key, 0)
        x = self._drop(_lrelu(self.fc2(x)), key, 1)
        x = self._drop(_lrelu(self.fc3(x)), key, 2)
        return torch.sigmoid(self.fc4(x))


GAINS = {"G": (2.0, 4.0, 3.0), "D": (4.0, 3.0, 2.0)}


@functools.lru_cache(maxsize=None)
def initial_weights(seed):
    """(G state_dict, D state_dict) in fp32: the notebook's construction order under torch.manual_seed(seed), hidden weights
    times GAINS."""
    torch.manual_seed(seed)
    nets = {"G": Generator(Z_DIM, MNIST_DIM), "D": Discriminator(MNIST_DIM)}
    out = []
    for tag in ("G", "D"):
        sd = {k: v.clone() for k, v in nets[tag].state_dict().items()}
        for fc, gain in zip(("fc1", "fc2", "fc3"), GAINS[tag]):
            sd[fc + ".weight"] *= gain
        out.append(sd)
    return tuple(out)


def restated(seed, dtype):
    """The pair (G, D) of this file's classes with initial_weights(seed), in dtype, on the CPU."""
    gsd, dsd = initial_weights(seed)
    G, D = Generator(Z_DIM, MNIST_DIM), Discriminator(MNIST_DIM)
    G.load_state_dict(gsd), D.load_state_dict(dsd)
    return G.to(dtype), D.to(dtype)


def load_product(G, D, seed):
    """The same weights into the product's modules (or any pair with the notebook's state_dict keys)."""
    gsd, dsd = initial_weights(seed)
    G.load_state_dict(gsd), D.load_state_dict(dsd)
    return G, D


# ---------------------------------------------------------------------------------------------------------------
# module problems: forward and every gradient at a batch size
MODULE_B = (1, 3, 100, 130)
# seeds: the first ones for which the fp64 run keeps every LeakyReLU input 2e-5 away from zero (asserted at 1e-5 by the host test)
MODULE_SEED = {("G", 1): 1, ("G", 3): 1, ("G", 100): 3, ("G", 130): 5, ("D", 1): 1, ("D", 3): 1, ("D", 100): 13, ("D", 130): 13}


def module_inputs(tag, B, seed):
    """(input [B, in], upstream weights r like the output): loss = sum(out * r).  fp32."""
    g = torch.Generator().manual_seed(1000 + seed)
    if tag == "G":
        return torch.randn(B, Z_DIM, generator=g), torch.randn(B, MNIST_DIM, generator=g)
    return torch.rand(B, MNIST_DIM, generator=g) * 2 - 1, torch.randn(B, 1, generator=g)


def run_module(net, tag, x, r, seed):
    """-> {'out', 'x' (D only), '<param name>': gradient} as CPU tensors.  The mask key comes from torch's CPU generator at
    `seed`."""
    dev = next(net.parameters()).device
    dt = next(net.parameters()).dtype
    x = x.to(device=dev, dtype=dt).contiguous().requires_grad_(tag == "D")
    torch.manual_seed(seed)
    out = net(x)
    loss = (out * r.to(device=dev, dtype=dt)).sum()
    params = dict(net.named_parameters())
    wanted = list(params.values()) + ([x] if tag == "D" else [])
    grads = torch.autograd.grad(loss, wanted)
    res = {"out": out.detach().cpu()}
    for n, g in zip(list(params) + ["x"], grads):
        res[n] = g.detach().cpu()
    return res


@functools.lru_cache(maxsize=None)
def module_reference(tag, B):
    """(fp64 results, fp32 CPU results, smallest |LeakyReLU input| of the fp64 run) of the restatement."""
    seed = MODULE_SEED[tag, B]
    x, r = module_inputs(tag, B, seed)
    res = {}
    for dt in (torch.float64, torch.float32):
        net = restated(seed, dt)[0 if tag == "G" else 1]
        reset_kink()
        res[dt] = run_module(net, tag, x, r, seed)
        if dt == torch.float64:
            kink = KINK[0]
    return res[torch.float64], res[torch.float32], kink


# ---------------------------------------------------------------------------------------------------------------
# trainer problems (batch 8): the closures of notebook cell 6
BS = 8
TRAINER_LR = 0.02
TRAINER_SEED = {"euler": 2, "rk2": 12, "rk4": 2}
PENALTY_SEED = 2
ADAM_SEED = 2
ADAM_LR = 2e-4


def real_batch(seed):
    return torch.rand(BS, 1, 28, 28, generator=torch.Generator().manual_seed(2000 + seed)) * 2 - 1


def closures(G, D, criterion, device, dtype=torch.float32):
    """d_loss(x), g_loss() of notebook cell 6 (Variable() dropped: it is the identity; dtype: the restatement's precision)."""
    bs, z_dim, mnist_dim = BS, Z_DIM, MNIST_DIM

    def d_loss(x):
        D.zero_grad()
        x_real, y_real = x.view(-1, mnist_dim), torch.ones(bs, 1)
        x_real, y_real = x_real.to(device=device, dtype=dtype), y_real.to(device=device, dtype=dtype)
        D_output_real = D(x_real)
        D_real_loss = criterion(D_output_real, y_real)
        z = torch.randn(bs, z_dim).to(device=device, dtype=dtype)
        x_fake, y_fake = G(z), torch.zeros(bs, 1).to(device=device, dtype=dtype)
        D_output_fake = D(x_fake)
        D_fake_loss = criterion(D_output_fake, y_fake)
        return D_real_loss + D_fake_loss

    def g_loss():
        G.zero_grad()
        z = torch.randn(bs, z_dim).to(device=device, dtype=dtype)
        y = torch.ones(bs, 1).to(device=device, dtype=dtype)
        G_output = G(z)
        D_output = D(G_output)
        return criterion(D_output, y)

    return d_loss, g_loss


def seed_all(s):
    torch.manual_seed(s)
    np.random.seed(s)


def _params(net):
    return {n: p.detach().cpu().clone() for n, p in net.named_parameters()}


def _delta(net, before):
    return {n: p.detach().cpu().double() - before[n].double() for n, p in net.named_parameters()}


def reference_steps(method, dtype):
    """One dis_img step, then one gen step (reg = 0) on the restatement: -> (D deltas, G deltas, kink)."""
    seed = TRAINER_SEED[method]
    G, D = restated(seed, dtype)
    d_loss, g_loss = closures(G, D, nn.BCELoss(), "cpu", dtype)
    x = real_batch(seed)
    bD, bG = _params(D), _params(G)
    reset_kink()
    seed_all(seed)
    odegan_ref.ode_step(list(D.parameters()), lambda: d_loss(x), method, TRAINER_LR)
    odegan_ref.ode_step(list(G.parameters()), g_loss, method, TRAINER_LR)
    return _delta(D, bD), _delta(G, bG), KINK[0]


@functools.lru_cache(maxsize=None)
def trainer_reference(method):
    d64, g64, kink = reference_steps(method, torch.float64)
    d32, g32, _ = reference_steps(method, torch.float32)
    return (d64, g64), (d32, g32), kink


def reference_penalty(dtype, h):
    """central_penalty of the restatement at the step h -> (gp per D parameter name, rng state after, kink)."""
    G, D = restated(PENALTY_SEED, dtype)
    _, g_loss = closures(G, D, nn.BCELoss(), "cpu", dtype)
    reset_kink()
    seed_all(PENALTY_SEED)
    gp, _ = odegan_ref.central_penalty(g_loss, list(G.parameters()), list(D.parameters()), h)
    return {n: g.detach() for (n, _), g in zip(D.named_parameters(), gp)}, odegan_ref.rng_state(), KINK[0]


@functools.lru_cache(maxsize=None)
def penalty_reference(h):
    gp64, state, kink = reference_penalty(torch.float64, h)
    gp32, _, _ = reference_penalty(torch.float32, h)
    return gp64, gp32, state, kink


def penalised_step_rng(h):
    """The generator states after the restatement's sequence of one penalised Euler dis_img step: d_loss(x), then the
    penalty (one g_loss call's worth of draws)."""
    G, D = restated(PENALTY_SEED, torch.float64)
    d_loss, g_loss = closures(G, D, nn.BCELoss(), "cpu", torch.float64)
    seed_all(PENALTY_SEED)
    d_loss(real_batch(PENALTY_SEED))
    odegan_ref.central_penalty(g_loss, list(G.parameters()), list(D.parameters()), h)
    return odegan_ref.rng_state()


def adam_iteration(G, D, criterion, device, dtype, x, lr=ADAM_LR):
    """One iteration of the notebook's Adam cell (cells 3 and 4): D_train(x), then G_train(x) -> (D loss, G loss)."""
    import torch.optim as optim
    bs, z_dim, mnist_dim = BS, Z_DIM, MNIST_DIM
    G_optimizer = optim.Adam(G.parameters(), lr=lr)
    D_optimizer = optim.Adam(D.parameters(), lr=lr)

    def D_train(x):
        D.zero_grad()
        x_real, y_real = x.view(-1, mnist_dim), torch.ones(bs, 1)
        x_real, y_real = x_real.to(device=device, dtype=dtype), y_real.to(device=device, dtype=dtype)
        D_output = D(x_real)
        D_real_loss = criterion(D_output, y_real)
        z = torch.randn(bs, z_dim).to(device=device, dtype=dtype)
        x_fake, y_fake = G(z), torch.zeros(bs, 1).to(device=device, dtype=dtype)
        D_output = D(x_fake)
        D_fake_loss = criterion(D_output, y_fake)
        D_loss = D_real_loss + D_fake_loss
        D_loss.backward()
        D_optimizer.step()
        return D_loss.data.item()

    def G_train(x):
        G.zero_grad()
        z = torch.randn(bs, z_dim).to(device=device, dtype=dtype)
        y = torch.ones(bs, 1).to(device=device, dtype=dtype)
        G_output = G(z)
        D_output = D(G_output)
        G_loss = criterion(D_output, y)
        G_loss.backward()
        G_optimizer.step()
        return G_loss.data.item()

    return D_train(x), G_train(x)


@functools.lru_cache(maxsize=None)
def adam_reference():
    """-> {dtype: (D loss, G loss, D weights after, G weights after)}, kink of the fp64 run"""
    res = {}
    for dt in (torch.float64, torch.float32):
        G, D = restated(ADAM_SEED, dt)
        reset_kink()
        seed_all(ADAM_SEED)
        dl, gl = adam_iteration(G, D, nn.BCELoss(), "cpu", dt, real_batch(ADAM_SEED))
        res[dt] = (dl, gl, _params(D), _params(G))
        if dt == torch.float64:
            kink = KINK[0]
    return res, kink


# ---------------------------------------------------------------------------------------------------------------
# the fp32 CPU restatement's own error against the fp64 one, per tensor (conftest.rel_err): what the GPU tests' 8x allowance
# is taken from.  The figure depends on the host's BLAS and thread count, so it is measured once (one thread) by
# scripts/make_fcgan_goldens.py and stored, as tests/golden/odegan_tiny.npz stores the figures of DESIGN section 14.
OWN_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fcgan_own.npz")


def _rel_err(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def measure_own(h):
    """Every figure of OWN_FILE, from the functions above (h: the trainer's central-difference step)."""
    out = {}
    for tag in ("G", "D"):
        for B in MODULE_B:
            r64, r32, _ = module_reference(tag, B)
            for n in r64:
                out[f"module/{tag}/{B}/{n}"] = _rel_err(r32[n], r64[n])
    for m in TRAINER_SEED:
        (d64, g64), (d32, g32), _ = trainer_reference(m)
        for tag, r64, r32 in (("D", d64, d32), ("G", g64, g32)):
            for n in r64:
                out[f"step/{m}/{tag}/{n}"] = _rel_err(r32[n], r64[n])
    gp64, gp32, _, _ = penalty_reference(h)
    for n in gp64:
        out[f"penalty/{n}"] = _rel_err(gp32[n], gp64[n])
    res, _ = adam_reference()
    out["adam/D_loss"] = abs(res[torch.float32][0] - res[torch.float64][0])
    out["adam/G_loss"] = abs(res[torch.float32][1] - res[torch.float64][1])
    return out


@functools.lru_cache(maxsize=None)
def stored_own():
    z = np.load(OWN_FILE)
    return {k: float(z[k]) for k in z.files}
