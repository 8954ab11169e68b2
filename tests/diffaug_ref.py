"""Restatement of the differentiable augmentation (gode_diffaug_op of include/gode.h) for
tests/test_host_diffaug.py and tests/test_gpu_diffaug.py, written from the definition:

- the parameter stream in NumPy on tests/wgan_ref.py's Philox (`params`);
- the transform and its backward in torch, in float64 by default and in any other dtype on request (`forward`, `backward`):
  the float32 run of the same code is the yardstick for the kernel's rounding error;
- `AugRef`, which puts the float32 transform in front of an oracle discriminator with the product's call counter.
"""
import numpy as np
import torch
import torch.nn as nn

import wgan_ref as W

MASK32 = 0xFFFFFFFF
BRIGHT, SAT, CONTRAST, TRANSLATE, CUTOUT = 1, 2, 4, 8, 16
BITS = {"color": BRIGHT | SAT | CONTRAST, "translation": TRANSLATE, "cutout": CUTOUT}


def mask_of(policy):
    m = 0
    for name in (policy or "").split(","):
        if name.strip():
            m |= BITS[name.strip()]
    return m


def tag(stream, field):
    """The third counter word: 0x20000000 | stream << 8 | field."""
    return 0x20000000 | (int(stream) << 8) | int(field)


def words(seed, stream, call, g, field):
    """The four Philox words of global sample g (array) for one field: counter (g low, call, tag, g high)."""
    g = np.asarray(g, dtype=np.uint64)
    ctr = np.stack([g & np.uint64(MASK32), np.full_like(g, int(call) & MASK32), np.full_like(g, tag(stream, field)),
                    g >> np.uint64(32)], -1)
    return W.philox4x32_10(ctr, W.seed_key(seed)).astype(np.uint64)


def sizes(H, W_):
    """Sx, Sy, cw, ch"""
    return (W_ + 4) // 8, (H + 4) // 8, (W_ + 1) // 2, (H + 1) // 2


def params(n, H, W_, seed, stream, call, g0=0):
    """(ints int32 [n, 4] = tx, ty, cx, cy; unis float32 [n, 3] = u_b, u_s, u_c) of samples g0 .. g0 + n - 1."""
    g = np.arange(n, dtype=np.uint64) + np.uint64(g0)
    w0, w1 = words(seed, stream, call, g, 0), words(seed, stream, call, g, 1)
    unis = (((w0[:, :3] >> np.uint64(9)).astype(np.float64) + 0.5) * 2.0 ** -23).astype(np.float32)
    Sx, Sy, cw, ch = sizes(H, W_)
    umulhi = lambda w, m: ((w * np.uint64(m)) >> np.uint64(32)).astype(np.int64)  # noqa: E731
    ints = np.stack([umulhi(w1[:, 0], 2 * Sx + 1) - Sx, umulhi(w1[:, 1], 2 * Sy + 1) - Sy,
                     umulhi(w1[:, 2], W_ + 1 - cw % 2), umulhi(w1[:, 3], H + 1 - ch % 2)], -1).astype(np.int32)
    return ints, unis


def box(ints_row, H, W_):
    """The cutout's rows [y0, y1) and columns [x0, x1), clipped to the map."""
    _, _, cw, ch = sizes(H, W_)
    cx, cy = int(ints_row[2]), int(ints_row[3])
    x0, y0 = cx - cw // 2, cy - ch // 2
    return max(y0, 0), min(y0 + ch, H), max(x0, 0), min(x0 + cw, W_)


def _shift(v, ty, tx):
    """y[..., h, w] = v[..., h - ty, w - tx] inside the map, else 0"""
    H, W_ = v.shape[-2], v.shape[-1]
    y = torch.zeros_like(v)
    h0, h1, w0, w1 = max(ty, 0), min(H + ty, H), max(tx, 0), min(W_ + tx, W_)
    if h0 < h1 and w0 < w1:
        y[..., h0:h1, w0:w1] = v[..., h0 - ty:h1 - ty, w0 - tx:w1 - tx]
    return y


def _cut(v, ints_row):
    H, W_ = v.shape[-2], v.shape[-1]
    y0, y1, x0, x1 = box(ints_row, H, W_)
    keep = torch.ones(H, W_, dtype=torch.bool)
    keep[y0:y1, x0:x1] = False
    return torch.where(keep, v, torch.zeros((), dtype=v.dtype))


def _as5(x):
    return x.unsqueeze(2) if x.dim() == 4 else x


def forward(x, ints, unis, mask, dtype=torch.float64):
    """x: [N, C, H, W] or [N, C, D, H, W] -> the augmented tensor of the same shape, every operation in `dtype`.
    Differentiable (torch ops only)."""
    x5 = _as5(x).to(dtype)
    out = []
    for n in range(x5.shape[0]):
        v = x5[n]                                               # [C, D, H, W]
        ub, us, uc = (torch.tensor(float(u), dtype=dtype) for u in unis[n])
        if mask & BRIGHT:
            v = v + (ub - 0.5)
        if mask & SAT:
            m = v.mean(0, keepdim=True)
            v = (v - m) * (2 * us) + m
        if mask & CONTRAST:
            M = v.mean()
            v = (v - M) * (uc + 0.5) + M
        if mask & TRANSLATE:
            v = _shift(v, int(ints[n][1]), int(ints[n][0]))
        if mask & CUTOUT:
            v = _cut(v, ints[n])
        out.append(v)
    y = torch.stack(out)
    return y.squeeze(2) if x.dim() == 4 else y


def backward(g, ints, unis, mask, dtype=torch.float64):
    """The cotangent of forward's input given the cotangent g of its output (same shapes), step by step as gode.h states it."""
    g5 = _as5(g).to(dtype)
    out = []
    for n in range(g5.shape[0]):
        v = g5[n]
        _, us, uc = (torch.tensor(float(u), dtype=dtype) for u in unis[n])
        if mask & CUTOUT:
            v = _cut(v, ints[n])
        if mask & TRANSLATE:
            v = _shift(v, -int(ints[n][1]), -int(ints[n][0]))
        if mask & CONTRAST:
            s = uc + 0.5
            v = s * v + (1 - s) * v.mean()
        if mask & SAT:
            s = 2 * us
            v = s * v + (1 - s) * v.mean(0, keepdim=True)
        out.append(v)
    y = torch.stack(out)
    return y.squeeze(2) if g.dim() == 4 else y


class AugRef(nn.Module):
    """An oracle discriminator behind the float32 transform: params_fn(n, H, W, seed, stream, call, g0) -> (ints, unis) (the
    library's host function, or `params`); the call counter advances by one per forward, as the product's."""

    def __init__(self, disc, policy, seed, stream, params_fn=params):
        super().__init__()
        self.disc = disc
        self.mask, self.seed, self.stream = mask_of(policy), seed, stream
        self.call, self.sample_offset = 0, 0
        self.params_fn = params_fn

    def forward(self, x):
        if self.training and self.mask:
            ints, unis = self.params_fn(x.shape[0], x.shape[-2], x.shape[-1], self.seed, self.stream, self.call,
                                        self.sample_offset)
            x = forward(x, ints, unis, self.mask, dtype=torch.float32)
            self.call = (self.call + 1) & MASK32
        return self.disc(x)

    # the oracle loop reads these through the module
    def state_dict(self, *a, **k):
        return self.disc.state_dict(*a, **k)

    def load_state_dict(self, *a, **k):
        return self.disc.load_state_dict(*a, **k)
