"""Plain-torch restatement of the reference's stage-1 block (stage1/GResBlock.py), for CPU and GPU: the host tests hold it to
the fixtures written by scripts/make_gres_golden.py from the reference's own classes, the GPU tests and scripts/bench_gres.py
use it as the reference of the HIP path.  Same parameter names and initialisation order, so a fixture state_dict loads."""
import torch
import torch.nn as nn
import torch.nn.functional as F


def l2n(v, eps=1e-12):
    return v / (v.norm() + eps)


def sn_step(w_bar, u, v):
    """One power iteration (u, v: tensors, updated in place) -> (weight, sigma); u and v are constants of the graph."""
    m = w_bar.detach().reshape(w_bar.shape[0], -1)
    v.copy_(l2n(m.t().mv(u)))
    u.copy_(l2n(m.mv(v)))
    sigma = u.dot(w_bar.reshape(w_bar.shape[0], -1).mv(v))
    return w_bar / sigma, sigma


def sn_grad(G, w_bar, u, v, sigma):
    """dL/dw_bar from G = dL/dW for W = w_bar / sigma, sigma = u . (w_bar v)."""
    G64, s64 = G.double(), sigma.double()
    dot = (G64 * w_bar.double()).sum()
    return (G64 / s64 - dot / s64 ** 2 * torch.outer(u.double(), v.double()).view_as(G64)).float()


class SpectralNorm(nn.Module):
    def __init__(self, module, name="weight"):
        super().__init__()
        self.module, self.name = module, name
        w = getattr(module, name)
        u = w.data.new(w.shape[0]).normal_(0, 1)
        v = w.data.new(w[0].numel()).normal_(0, 1)
        del module._parameters[name]
        module.register_parameter(name + "_u", nn.Parameter(l2n(u), requires_grad=False))
        module.register_parameter(name + "_v", nn.Parameter(l2n(v), requires_grad=False))
        module.register_parameter(name + "_bar", nn.Parameter(w.data))

    def weight(self):
        m = self.module
        with torch.no_grad():
            u, v = getattr(m, self.name + "_u").data, getattr(m, self.name + "_v").data
        return sn_step(getattr(m, self.name + "_bar"), u, v)[0]

    def forward(self, x):
        setattr(self.module, self.name, self.weight())
        return self.module(x)


def cbn(x, gb, bn):
    """gamma[n] * BatchNorm(x) + beta[n] with gb = [gamma | beta][N][2C]; bn: an affine-free nn.BatchNorm2d."""
    C = x.shape[1]
    return gb[:, :C, None, None] * bn(x) + gb[:, C:, None, None]


class ConditionalNorm(nn.Module):
    def __init__(self, in_channel, n_condition=96):
        super().__init__()
        self.in_channel = in_channel
        self.bn = nn.BatchNorm2d(in_channel, affine=False)
        self.embed = nn.Linear(n_condition, 2 * in_channel)
        self.embed.weight.data[:, :in_channel].normal_(1, 0.02)
        self.embed.weight.data[:, in_channel:].zero_()

    def forward(self, x, class_id):
        return cbn(x, self.embed(class_id), self.bn)


def block_out(main, sc, b_main, b_sc, f, down):
    """main [N, C, H*f, W*f] and sc [N, C, H, W] (raw convolution outputs) -> the block output."""
    m = main + b_main[None, :, None, None]
    s = sc + b_sc[None, :, None, None]
    if f != 1:
        s = F.interpolate(s, scale_factor=f)
    if down != 1:
        m, s = F.avg_pool2d(m, down), F.avg_pool2d(s, down)
    return m + s


class GResBlock(nn.Module):
    def __init__(self, in_channel, out_channel, kernel_size=(3, 3), padding=1, n_class=96, bn=True, upsample_factor=2,
                 downsample_factor=1):
        super().__init__()
        self.up = upsample_factor if downsample_factor == 1 else 1
        self.down = downsample_factor
        self.bn = bn and downsample_factor == 1
        self.conv0 = SpectralNorm(nn.Conv2d(in_channel, out_channel, tuple(kernel_size), 1, padding))
        self.conv1 = SpectralNorm(nn.Conv2d(out_channel, out_channel, tuple(kernel_size), 1, padding))
        self.conv_sc = SpectralNorm(nn.Conv2d(in_channel, out_channel, 1, 1, 0))
        if bn:
            self.CBNorm1 = ConditionalNorm(in_channel, n_class)
            self.CBNorm2 = ConditionalNorm(out_channel, n_class)

    def forward(self, x, condition=None, keep=None):
        """keep (a dict): receives the pre-activations 'z0', 'z1' (for the fixtures' ReLU-kink margin)."""
        h = self.CBNorm1(x, condition) if self.bn else x
        if keep is not None:
            keep["z0"] = h
        h = F.relu(h)
        if self.up != 1:
            h = F.interpolate(h, scale_factor=self.up)
        h = self.conv0(h)
        if self.bn:
            h = self.CBNorm2(h, condition)
        if keep is not None:
            keep["z1"] = h
        h = self.conv1(F.relu(h))
        s = F.interpolate(x, scale_factor=self.up) if self.up != 1 else x
        s = self.conv_sc(s)
        if self.down != 1:
            h, s = F.avg_pool2d(h, self.down), F.avg_pool2d(s, self.down)
        return h + s
