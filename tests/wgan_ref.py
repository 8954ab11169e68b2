"""Restatement of what mnist_moco_ode_wgan.py / mnist_moco_ode_noise.py compute beyond mnist_moco_ode.py, for the
tests of the Wasserstein loss and the parameter noise (tests/test_host_wgan.py, tests/test_gpu_wgan.py).

- torchgan's losses (torchgan/losses/wasserstein.py, functional.py: wasserstein_generator_loss = reduce(-1.0 * fgz),
  wasserstein_discriminator_loss = reduce(fgz - fx), reduce = torch.mean / torch.sum; defaults reduction="mean",
  clip=None).  torchgan itself is not a dependency.
- the parameter-noise stream of include/gode.h (Philox4x32-10, Box-Muller) in NumPy: the words exactly, the normals in
  float64.  The reference draws its noise from torch's CUDA generator; the stream is a documented deviation (DESIGN
  section 10), so the reference loop below takes its noise from this restatement.
- the reference loop body of mnist_moco_ode_wgan.py:121-178 (add_noise after every optimiser step) on stock torch.
"""
import numpy as np
import torch

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF


def philox4x32_10(ctr, key):
    """ctr: uint32 array [..., 4], key: uint32 array [..., 2] (broadcast) -> uint32 [..., 4]."""
    c = [np.asarray(ctr, dtype=np.uint64)[..., i] for i in range(4)]
    k = np.broadcast_to(np.asarray(key, dtype=np.uint64), np.asarray(ctr).shape[:-1] + (2,))
    k0, k1 = k[..., 0].copy(), k[..., 1].copy()
    for _ in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]
        hi0, lo0, hi1, lo1 = p0 >> 32, p0 & MASK, p1 >> 32, p1 & MASK
        c = [(hi1 ^ c[1] ^ k0) & MASK, lo1, (hi0 ^ c[3] ^ k1) & MASK, lo0]
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return np.stack(c, -1).astype(np.uint32)


def seed_key(seed):
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    return np.array([seed & MASK, seed >> 32], dtype=np.uint64)


def noise_words(seed, stream, step, noise_off, n):
    """The raw Philox word of every element e in [noise_off, noise_off + n) (lane e & 3 of quad e >> 2)."""
    e = np.arange(noise_off, noise_off + n, dtype=np.uint64)
    q0, q1 = int(noise_off) >> 2, (int(noise_off) + n - 1) >> 2
    q = np.arange(q0, q1 + 1, dtype=np.uint64)
    ctr = np.stack([q & MASK, np.full_like(q, step), np.full_like(q, stream), q >> 32], -1)
    words = philox4x32_10(ctr, seed_key(seed))           # [quads, 4]
    return words[(e >> 2) - q0, e & 3]


def uniforms(words):
    return ((np.asarray(words, dtype=np.uint32) >> 9).astype(np.float64) + 0.5) * 2.0 ** -23


def noise_normals(seed, stream, step, noise_off, n):
    """float64 Box-Muller of the stream over [noise_off, noise_off + n)."""
    q0, q1 = int(noise_off) >> 2, (int(noise_off) + n - 1) >> 2
    q = np.arange(q0, q1 + 1, dtype=np.uint64)
    ctr = np.stack([q & MASK, np.full_like(q, step), np.full_like(q, stream), q >> 32], -1)
    u = uniforms(philox4x32_10(ctr, seed_key(seed)))
    r0, r2 = np.sqrt(-2.0 * np.log(u[:, 0])), np.sqrt(-2.0 * np.log(u[:, 2]))
    z = np.stack([r0 * np.cos(2 * np.pi * u[:, 1]), r0 * np.sin(2 * np.pi * u[:, 1]),
                  r2 * np.cos(2 * np.pi * u[:, 3]), r2 * np.sin(2 * np.pi * u[:, 3])], -1)
    e = np.arange(noise_off, noise_off + n, dtype=np.uint64)
    return z[(e >> 2) - q0, e & 3]


def noise_offsets(params):
    """noise_off of every tensor of a param group: the running sum of roundup4(numel) in group order."""
    offs, off = [], 0
    for p in params:
        offs.append(off)
        off += (p.numel() + 3) // 4 * 4
    return offs


def add_noise(parameters, sigma, seed, stream, step):
    """mnist_moco_ode_noise.py's add_noise (param.add_(randn_like(param) * sigma), every parameter), with the normals of
    this stream in place of torch.randn_like: t = fp32(n * fp32(sigma)), p = fp32(p + t)."""
    params = list(parameters)
    with torch.no_grad():
        for p, off in zip(params, noise_offsets(params)):
            z = torch.from_numpy(noise_normals(seed, stream, step, off, p.numel()).astype(np.float32)).view_as(p)
            p.add_(z.to(p.device) * np.float32(sigma))


# -- torchgan's losses ------------------------------------------------------------------------------------------------
def _reduce(x, reduction):
    if reduction == "mean":
        return torch.mean(x)
    if reduction == "sum":
        return torch.sum(x)
    return x


def wasserstein_generator_loss(fgz, reduction="mean"):
    return _reduce(-1.0 * fgz, reduction)


def wasserstein_discriminator_loss(fx, fgz, reduction="mean"):
    return _reduce(fgz - fx, reduction)


class WassersteinGeneratorLoss(torch.nn.Module):
    def __init__(self, reduction="mean", override_train_ops=None):
        super().__init__()
        self.reduction = reduction

    def forward(self, fgz):
        return wasserstein_generator_loss(fgz, self.reduction)


class WassersteinDiscriminatorLoss(torch.nn.Module):
    def __init__(self, reduction="mean", clip=None, override_train_ops=None):
        super().__init__()
        self.reduction = reduction

    def forward(self, fx, fgz):
        return wasserstein_discriminator_loss(fx, fgz, self.reduction)


# -- the reference loop body ------------------------------------------------------------------------------------------
def train_step(gen, dis_vid, dis_img, opts, real_imgs, real_vids, loss="wasserstein", sigma=1e-4, seed=0, noise_steps=None,
               d_iters=2, gen_loss_fn=None, dis_loss_fn=None):
    """One outer iteration of mnist_moco_ode_wgan.py:121-178 (loss="wasserstein") or mnist_moco_ode_noise.py (loss="bce"),
    add_noise after every optimiser step with streams gen 0, dis_vid 1, dis_img 2.  noise_steps: a 3-list of the noise
    step counters [gen, vid, img], advanced in place (the counter of a step is its new value).  Returns the three losses
    of the last inner pass."""
    gen_opt, vid_opt, img_opt = opts
    gen_loss_fn = gen_loss_fn or WassersteinGeneratorLoss()
    dis_loss_fn = dis_loss_fn or WassersteinDiscriminatorLoss()
    bce = torch.nn.BCEWithLogitsLoss()
    steps = noise_steps if noise_steps is not None else [0, 0, 0]
    batch = real_imgs[0].shape[0]

    def noise(model, k):
        if sigma:
            steps[k] += 1
            add_noise(model.parameters(), sigma, seed, (0, 1, 2)[k], steps[k])

    for i in range(d_iters):
        img_opt.zero_grad()
        pr, _ = dis_img(real_imgs[i])
        with torch.no_grad():
            fake, _ = gen.sample_images(batch)
        pf, _ = dis_img(fake)
        li = dis_loss_fn(pr, pf) if loss == "wasserstein" else bce(pr, torch.ones_like(pr)) + bce(pf, torch.zeros_like(pf))
        li.backward()
        img_opt.step()
        noise(dis_img, 2)

        vid_opt.zero_grad()
        pr, _ = dis_vid(real_vids[i].transpose(1, 2))
        with torch.no_grad():
            fake, _ = gen.sample_videos(batch)
        pf, _ = dis_vid(fake)
        lv = dis_loss_fn(pr, pf) if loss == "wasserstein" else bce(pr, torch.ones_like(pr)) + bce(pf, torch.zeros_like(pf))
        lv.backward()
        vid_opt.step()
        noise(dis_vid, 1)

    gen_opt.zero_grad()
    fake_vid, _ = gen.sample_videos(batch)
    fake_img, _ = gen.sample_images(batch)
    pf_vid, _ = dis_vid(fake_vid)
    pf_img, _ = dis_img(fake_img)
    if loss == "wasserstein":
        lg = gen_loss_fn(pf_img) + gen_loss_fn(pf_vid)       # image term first (mnist_moco_ode_wgan.py:174)
    else:
        lg = bce(pf_vid, torch.ones_like(pf_vid)) + bce(pf_img, torch.ones_like(pf_img))
    lg.backward()
    gen_opt.step()
    noise(gen, 0)
    return li.detach(), lv.detach(), lg.detach()
