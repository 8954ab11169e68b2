"""Test infrastructure: the fixed problems of the ODE-GAN tests, shared by scripts/make_odegan_goldens.py (which runs the
reference's trainer on them) and the tests (which run this package's trainer on the same weights and inputs)."""
import numpy as np
import torch
import torch.nn.functional as F

METHODS = ("euler", "rk2", "rk4")
LR, QUAD_LR = 0.02, 0.1
GEN_SEED, PEN_SEED, GEN_VIDEOS, PEN_IMAGES = 77, 91, 2, 4
QUAD_NAMES = ("a", "b", "c", "d")


def quad_init():
    """Four small tensors; `c` is not used by quad_loss."""
    g = torch.Generator().manual_seed(5)
    return {"a": torch.randn(3, generator=g), "b": torch.randn(2, 3, generator=g), "c": torch.randn(5, generator=g),
            "d": torch.randn(7, generator=g)}


def quad_loss(a, b, c, d):
    """A polynomial with the closed-form gradient of quad_grad."""
    s = torch.tensor([1.0, 2.0, 0.5], dtype=a.dtype)
    return 0.5 * ((s * a) ** 2).sum() + 0.1 * (b ** 3).sum() / 3 + (a * b[1]).sum() + 0.15 * (d ** 2).sum() + 0.05 * d.sum() ** 2


def quad_grad(a, b, c, d):
    s = torch.tensor([1.0, 2.0, 0.5], dtype=a.dtype)
    gb = 0.1 * b ** 2
    gb[1] += a
    return s * s * a + b[1], gb, None, 0.3 * d + 0.1 * d.sum()


def bce(logits, target):
    return F.binary_cross_entropy_with_logits(logits, torch.full_like(logits, target))


def disc_loss(dis, real, fake, bce=bce):
    """A discriminator's closure over fixed real and fake batches (two forward calls, as the training scripts make).  bce: the loss
    op (the GPU tests pass the package's fused one)."""
    def loss():
        return bce(dis(real)[0], 1.0) + bce(dis(fake)[0], 0.0)
    return loss


def gen_video_loss(gen, dis_vid, bce=bce):
    def loss():
        vid, _ = gen.sample_videos(GEN_VIDEOS)
        return bce(dis_vid(vid)[0], 1.0)
    return loss


def gen_image_loss(gen, dis_img, bce=bce):
    def loss():
        img, _ = gen.sample_images(PEN_IMAGES)
        return bce(dis_img(img)[0], 1.0)
    return loss


def fake_like(x, seed):
    """A fixed 'generated' batch: fp16-representable normals squashed into the data range."""
    g = torch.Generator().manual_seed(seed)
    return torch.tanh(torch.randn(x.shape, generator=g)).half().float()


def delta_err(d, ref):
    """max |d - ref| / max |ref| of one tensor's parameter change"""
    d, ref = np.asarray(d, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.abs(d - ref).max() / max(np.abs(ref).max(), 1e-300))
