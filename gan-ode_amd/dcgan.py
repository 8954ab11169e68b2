"""Stage 2's CIFAR DCGAN (stage2/test_ODE_training_with_cifar_GAN.ipynb, the ODE-GAN setting proper): a convolutional
generator and discriminator on 32x32 images and nn.BCEWithLogitsLoss against a target tensor, on libgode.

  Generator      z [B, nz, 1, 1] -> 1x1 convolution to 128 ngf channels, viewed as [8 ngf, 4, 4] -> three ConvTranspose2d(k4 s2 p1)
                 + train-mode BatchNorm + ReLU (4 ngf, 2 ngf, ngf channels; 8, 16, 32 pixels) -> Conv2d(ngf, nc, 3, 1, 1) -> tanh
  Discriminator  [B, nc, 32, 32] -> seven Conv2d + LeakyReLU(0.1), (k, s, p) alternating (3, 1, 1) and (4, 2, 1), channels ndf, ndf,
                 2 ndf, 2 ndf, 4 ndf, 4 ndf, 8 ndf -> Conv2d(8 ndf, 1, 4, 1, 0) -> logits [B]; no BatchNorm anywhere
  BCEWithLogitsLoss  mean-reduced, the target a tensor of the input's shape (gode_bce_logits_t)

The notebook reads nz, ngf, ndf and nc from globals; here they are keyword arguments with its values.  Attribute names,
construction order, state_dict keys and same-seed initial weights are the notebook's: `project` and the members of `main` are
stock torch.nn layers used as parameter containers only, so the notebook's weights_init applies to them.  Each network's
forward and backward is ONE ConvStack (engine.py) behind ONE autograd node, with a plan per batch size; there is no CPU path.

The generator's first layer: `project` followed by view(-1, 8 ngf, 4, 4) is one product [B, nz] x [nz, 128 ngf] whose output
columns are stored in (h, w, c) order (PackOp.co_perm), so that its output buffer IS the channels-last [B, 4, 4, 8 ngf] input of
the first transposed convolution; the weight gradient goes back through the same permutation into the parameter's own rows
c * 16 + h * 4 + w.  The discriminator reads its input in place through element strides: a contiguous NCHW batch or the
generator's channels-last view.

Deviation: the loss is fp32 whatever the target's dtype (stock torch returns fp64 for the fp64 labels of the notebook's gen_loss).
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import _lib as L
from .engine import ConvStack, LayerParams, LayerSpec, conv_out, dptr, make_geom, stream_ptr
from .modules import _DiscFn, _Pool, _flat_params, _require_gpu

IMAGE = 32          # the only image size of these two networks: 4 -> 8 -> 16 -> 32 up, 32 -> 16 -> 8 -> 4 -> 1 down


def _check_ngpu(ngpu):
    if ngpu != 1:
        raise ValueError(f"ngpu must be 1 (got {ngpu!r}): the reference's Generator raises for more, and this path is one device")


class _ConvNet(nn.Module):
    """One ConvStack per batch size behind one autograd node (modules._DiscFn: a stack over a caller-owned input)."""

    def _specs(self, B):
        raise NotImplementedError

    def _layer_params(self):
        raise NotImplementedError

    def _apply(self, fn, *a, **k):
        r = super()._apply(fn, *a, **k)
        if hasattr(self, "_pool"):
            self._pool.clear()   # parameter storage may have moved
        return r

    def invalidate_packs(self):
        """Forget the packed weights: after writing a weight behind autograd's back (p.data.copy_(), dist.broadcast(p.data))."""
        for k in [k for k in self._pool.pack_cache if k[0] == "ver"]:
            del self._pool.pack_cache[k]

    def _run_stack(self, x, what):
        """-> the stack's channels-last output [B, 1, Ho, Wo, C]"""
        lps = self._layer_params()
        params = _flat_params(lps)
        for t in params:
            _require_gpu(t, what + " parameter")
            if t.dtype != torch.float32 or not t.is_contiguous() or t.device != x.device:
                raise RuntimeError(f"{what}: contiguous float32 parameters on the input's device expected")
        B = x.shape[0]
        plan = self._pool.get((B,), lambda: ConvStack(self._specs(B), lps, x.device, owns_input=False,
                                                      pack_cache=self._pool.pack_cache))
        keep = torch.is_grad_enabled() and any(t.requires_grad for t in [x] + params)
        return _DiscFn.apply(plan, self.training, keep, None, None, x, None, *params)


class Generator(_ConvNet):
    """The notebook's Generator(ngpu): forward(z [B, nz, 1, 1]) -> [B, nc, 32, 32] in (-1, 1), a permuted view of the
    channels-last buffer the head writes."""

    def __init__(self, ngpu, nz=128, ngf=64, nc=3):
        super(Generator, self).__init__()
        _check_ngpu(ngpu)
        if min(nz, ngf, nc) < 1:
            raise ValueError("nz, ngf and nc must be positive")
        self.ngpu, self.nz, self.ngf, self.nc = ngpu, nz, ngf, nc
        self.project = nn.Conv2d(nz, ngf * 8 * 4 * 4, 1, 1, 0, bias=False)
        layers = []
        for c in (ngf * 8, ngf * 4, ngf * 2):
            layers += [nn.ConvTranspose2d(c, c // 2, 4, 2, 1, bias=False), nn.BatchNorm2d(c // 2), nn.ReLU(True)]
        layers += [nn.Conv2d(ngf, nc, 3, 1, 1, bias=False), nn.Tanh()]
        self.main = nn.Sequential(*layers)
        self._pool = _Pool()

    def _project_perm(self, device):
        """Internal output column (h * 4 + w) * 8 ngf + c of the first product is row c * 16 + h * 4 + w of project.weight."""
        perm = self.__dict__.get("_perm")
        if perm is None or perm.device != device:
            c8 = 8 * self.ngf
            perm = (torch.arange(c8, dtype=torch.int32).view(1, c8) * 16 + torch.arange(16, dtype=torch.int32).view(16, 1))
            perm = self.__dict__["_perm"] = perm.reshape(-1).contiguous().to(device)
        return perm

    def _specs(self, B):
        ngf, one = self.ngf, (1, 1, 1)
        dev = self.project.weight.device
        specs = [LayerSpec(make_geom(B, self.nz, ngf * 128, one, one, one, one, (0, 0, 0)), L.FPROP, L.ACT_NONE, False,
                           co_perm=self._project_perm(dev))]
        hw = 4
        for c in (ngf * 8, ngf * 4, ngf * 2):       # ConvTranspose2d(c, c / 2, 4, 2, 1): the DGRAD of a conv c / 2 -> c
            specs.append(LayerSpec(make_geom(B, c // 2, c, (1, hw * 2, hw * 2), (1, hw, hw), (1, 4, 4), (1, 2, 2), (0, 1, 1)),
                                   L.DGRAD, L.ACT_RELU, True))
            hw *= 2
        specs.append(LayerSpec(make_geom(B, ngf, self.nc, (1, hw, hw), (1, hw, hw), (1, 3, 3), one, (0, 1, 1)), L.FPROP,
                               L.ACT_NONE, False, epilogue=L.EPI_TANH))
        return specs

    def _layer_params(self):
        m = self.main
        out = [LayerParams(self.project.weight)]
        for i in (0, 3, 6):
            bn = m[i + 1]
            out.append(LayerParams(m[i].weight, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.num_batches_tracked))
        out.append(LayerParams(m[9].weight))
        return out

    def _apply(self, fn, *a, **k):
        self.__dict__.pop("_perm", None)
        return super()._apply(fn, *a, **k)

    def forward(self, input):
        if not torch.is_tensor(input):
            raise RuntimeError("Generator input: a tensor is expected")
        if input.dim() != 4 or tuple(input.shape[1:]) != (self.nz, 1, 1) or input.shape[0] < 1:
            raise ValueError(f"Generator input: [B, {self.nz}, 1, 1] expected, got {tuple(input.shape)}")
        _require_gpu(input, "Generator input")
        if input.dtype != torch.float32 or not input.is_contiguous():
            raise RuntimeError(f"Generator input: a contiguous float32 tensor expected, got {input.dtype} with strides "
                               f"{input.stride()}")
        out = self._run_stack(input, "Generator")               # [B, 1, 32, 32, nc]
        return out.squeeze(1).permute(0, 3, 1, 2)


class Discriminator(_ConvNet):
    """The notebook's Discriminator(ngpu): forward(x [B, nc, 32, 32], any strides) -> logits [B]."""

    LAYERS = ((3, 1, 1), (4, 2, 1)) * 3 + ((3, 1, 1),)          # (k, s, p) of the seven LeakyReLU(0.1) layers

    def __init__(self, ngpu, ndf=64, nc=3):
        super(Discriminator, self).__init__()
        _check_ngpu(ngpu)
        if min(ndf, nc) < 1:
            raise ValueError("ndf and nc must be positive")
        self.ngpu, self.ndf, self.nc = ngpu, ndf, nc
        layers = []
        for ci, co, (k, s, p) in zip(self._channels()[:-1], self._channels()[1:], self.LAYERS):
            layers += [nn.Conv2d(ci, co, k, s, p, bias=False), nn.LeakyReLU(0.1, inplace=True)]
        layers.append(nn.Conv2d(ndf * 8, 1, 4, 1, 0, bias=False))
        self.main = nn.Sequential(*layers)
        self._pool = _Pool()

    def _channels(self):
        ndf = self.ndf
        return (self.nc, ndf, ndf, ndf * 2, ndf * 2, ndf * 4, ndf * 4, ndf * 8)

    def _specs(self, B):
        ch, hw, specs = self._channels(), IMAGE, []
        for ci, co, (k, s, p) in zip(ch[:-1], ch[1:], self.LAYERS):
            ho = conv_out(hw, k, s, p)
            specs.append(LayerSpec(make_geom(B, ci, co, (1, hw, hw), (1, ho, ho), (1, k, k), (1, s, s), (0, p, p)), L.FPROP,
                                   L.ACT_LRELU01, False))
            hw = ho
        specs.append(LayerSpec(make_geom(B, ch[-1], 1, (1, hw, hw), (1, 1, 1), (1, 4, 4), (1, 1, 1), (0, 0, 0)), L.FPROP,
                               L.ACT_NONE, False))
        return specs

    def _layer_params(self):
        return [LayerParams(m.weight) for m in self.main if isinstance(m, nn.Conv2d)]

    def forward(self, input):
        if not torch.is_tensor(input):
            raise RuntimeError("Discriminator input: a tensor is expected")
        if input.dim() != 4 or tuple(input.shape[1:]) != (self.nc, IMAGE, IMAGE) or input.shape[0] < 1:
            raise ValueError(f"Discriminator input: [B, {self.nc}, {IMAGE}, {IMAGE}] expected (the network ends in a 4x4 "
                             f"convolution on a 4x4 map), got {tuple(input.shape)}")
        _require_gpu(input, "Discriminator input")
        if input.dtype != torch.float32:
            raise RuntimeError(f"Discriminator input: float32 expected, got {input.dtype}")
        return self._run_stack(input, "Discriminator").reshape(-1)          # [B, 1, 1, 1, 1] -> view(-1, 1).squeeze(1)


class _BCELogitsFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, t):
        x, t = x.detach().contiguous(), t.detach().to(torch.float32).contiguous()
        loss = torch.empty((), dtype=torch.float32, device=x.device)
        grad = torch.empty_like(x)
        L.run_one(L.BceTOp(logits=dptr(x), target=dptr(t), grad=dptr(grad), loss=dptr(loss), n=x.numel(), gscale=1.0,
                           accumulate=0), stream_ptr())
        ctx.save_for_backward(grad)
        return loss

    @staticmethod
    def backward(ctx, gout):
        (grad,) = ctx.saved_tensors
        return grad * gout, None


class BCEWithLogitsLoss(nn.Module):
    """nn.BCEWithLogitsLoss() on gode_bce_logits_t: float32 logits of any shape, a target tensor of the same shape (float32 or
    float64, converted to float32), mean reduction.  The loss is a float32 scalar."""

    def __init__(self, weight=None, size_average=None, reduce=None, reduction='mean', pos_weight=None):
        super().__init__()
        if (weight is not None or size_average is not None or reduce is not None or reduction != 'mean'
                or pos_weight is not None):
            raise ValueError("BCEWithLogitsLoss: only the default mean reduction without weights runs on the HIP kernel")
        self.reduction = reduction

    def forward(self, input, target):
        for t, what in ((input, "BCEWithLogitsLoss input"), (target, "BCEWithLogitsLoss target")):
            if not torch.is_tensor(t):
                raise RuntimeError(f"{what}: a tensor is expected")
        if input.shape != target.shape or input.numel() < 1:
            raise ValueError(f"BCEWithLogitsLoss: input and target of one non-empty shape expected, got {tuple(input.shape)} "
                             f"and {tuple(target.shape)}")
        _require_gpu(input, "BCEWithLogitsLoss input")
        _require_gpu(target, "BCEWithLogitsLoss target")
        if input.dtype != torch.float32:
            raise RuntimeError(f"BCEWithLogitsLoss input: float32 expected, got {input.dtype}")
        if target.dtype not in (torch.float32, torch.float64):
            raise RuntimeError(f"BCEWithLogitsLoss target: float32 or float64 expected, got {target.dtype}")
        if target.requires_grad:
            raise RuntimeError("BCEWithLogitsLoss: the target does not receive a gradient")
        return _BCELogitsFn.apply(input, target)
