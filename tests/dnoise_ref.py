"""Restatement of the discriminators' instance noise (Noise(use_noise=True, sigma), models/mocogan.py:20-29) for
tests/test_host_dnoise.py and tests/test_gpu_dnoise.py.

- the stream of include/gode.h in NumPy (on tests/wgan_ref.py's Philox): the words exactly, the normals in float64;
- the oracle's VideoDisc / PatchImageDisc (oracle/mocogan_ref.py) with their nn.Identity noise slots replaced by a module
  that adds fp32(sigma * z), z taken from a caller-given source (the library's raw entry point on a GPU), and the call
  counter / sample offset of the product's modules.  The reference draws its noise from torch's CUDA generator; the
  stream is a documented deviation, so the reference loop runs with this one.
"""
import numpy as np
import torch
import torch.nn as nn

import wgan_ref as W

MASK = 0xFFFFFFFF


def tag(stream, layer):
    """The third counter word: 0x80000000 | stream << 8 | layer (disjoint from the parameter-noise streams 0 / 1 / 2)."""
    return 0x80000000 | (int(stream) << 8) | int(layer)


def counters(stream, layer, call, e):
    """The Philox counter of each element index e: (q low word, call, tag, q high word), q = e >> 2."""
    q = np.asarray(e, dtype=np.uint64) >> np.uint64(2)
    return np.stack([q & np.uint64(MASK), np.full_like(q, call & MASK), np.full_like(q, tag(stream, layer)),
                     q >> np.uint64(32)], -1)


def words(seed, stream, layer, call, offset, n):
    return W.noise_words(seed, tag(stream, layer), call & MASK, offset, n)


def normals(seed, stream, layer, call, offset, n):
    """float64 z of elements [offset, offset + n)"""
    return W.noise_normals(seed, tag(stream, layer), call & MASK, offset, n)


def noise_slots(disc):
    """Indices of the oracle's noise slots in `main`, in layer order."""
    return [i for i, m in enumerate(disc.main) if isinstance(m, (nn.Identity, RefNoise))]


class RefNoise(nn.Module):
    """x + fp32(sigma * z): z of this layer's channels-last element order, from owner.z_source(layer, call, offset, n)."""

    def __init__(self, owner, layer):
        super().__init__()
        self.layer = layer
        self.__dict__["owner"] = owner          # (not a submodule: no state_dict entries, no cycle in .modules())

    def forward(self, x):
        o = self.owner
        per = x.numel() // x.shape[0]
        perm = (0,) + tuple(range(2, x.dim())) + (1,)
        z = o.z_source(self.layer, o.call, o.sample_offset * per, x.numel())
        z = torch.as_tensor(z, dtype=torch.float32).to(x.device).view([x.shape[i] for i in perm])
        z = z.permute(*[perm.index(i) for i in range(x.dim())])
        return x + z * np.float32(o.sigma)


class NoisyRef(nn.Module):
    """An oracle discriminator with instance noise.  z_source(layer, call, e_offset, n) -> float32 array / tensor of n
    normals; default: the float64 restatement rounded to fp32."""

    def __init__(self, disc, sigma, seed, stream, z_source=None):
        super().__init__()
        self.disc = disc
        self.sigma, self.seed, self.stream = sigma, seed, stream
        self.call, self.sample_offset = 0, 0
        self.z_source = z_source or (lambda layer, call, off, n: normals(seed, stream, layer, call, off, n).astype(np.float32))
        for layer, i in enumerate(noise_slots(disc)):
            disc.main[i] = RefNoise(self, layer)

    def forward(self, x):
        out = self.disc(x)
        self.call = (self.call + 1) & MASK
        return out

    # the oracle loop reads these through the module
    def state_dict(self, *a, **k):
        return self.disc.state_dict(*a, **k)

    def load_state_dict(self, *a, **k):
        return self.disc.load_state_dict(*a, **k)
