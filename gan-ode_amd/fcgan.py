"""Stage 2's MNIST GAN (stage2/test_ODE_training_with_MNIST_GAN.ipynb, the only stage-2 experiment of the reference that
ran): a fully-connected generator and discriminator, and nn.BCELoss on the discriminator's probabilities, on libgode.

  Generator      100 -> 256 -> 512 -> 1024 -> 784, LeakyReLU(0.2) between the layers, tanh on the output
  Discriminator  784 -> 1024 -> 512 -> 256 -> 1, LeakyReLU(0.2) + F.dropout(x, 0.3) behind every hidden layer, sigmoid
  BCELoss        mean-reduced binary cross entropy on probabilities, torch's clamps

Same constructor signatures, attribute names, state_dict keys and same-seed initial weights as the notebook's classes: fc1..fc4
are stock nn.Linear parameter containers.  Each network's forward is ONE autograd node; per layer it runs gode_igemm (the
product, on the weight pack of the current weight version), then gode_fc_act in place (bias, activation, dropout), and in
the backward gode_fc_act_bwd (also the bias gradient), gode_wgrad and the DGRAD product.  There is no CPU path.

Dropout is the reference's: F.dropout(x, 0.3) leaves `training` at its default True, so the discriminator drops in .eval()
too.  Every Discriminator.forward draws ONE int64 key from torch's CPU default generator (torch.randint(0, 2**62, (1,))); its
three dropout layers are layers 0, 1, 2 of that key in the counter-based stream of include/gode.h.  GANODETrainer's
regulariser rewinds torch's CPU generator around its repeated g_loss calls, so all of them see the same masks.  Deviation: on a
GPU the reference draws its masks from the device generator; seeds cannot reproduce its masks either way.
"""
from __future__ import annotations

import ctypes as C

import torch
import torch.nn as nn

from . import _lib as L
from .engine import dptr, make_geom, stream_ptr, tensor_version
from .modules import _require_gpu

DROP_P = 0.3


def _check_input(x, width, what):
    if not torch.is_tensor(x):
        raise RuntimeError(f"{what}: a tensor is expected")
    _require_gpu(x, what)
    if x.dtype != torch.float32 or x.dim() != 2 or x.shape[1] != width or x.shape[0] < 1 or not x.is_contiguous():
        raise RuntimeError(f"{what}: a contiguous float32 tensor [B, {width}] is expected, got {x.dtype} "
                           f"{tuple(x.shape)} with strides {x.stride()}")


def _geom(M, Ci, Co):
    return make_geom(M, Ci, Co, (1, 1, 1), (1, 1, 1), (1, 1, 1), (1, 1, 1), (0, 0, 0))


def _f32(*shape, like):
    return torch.empty(shape, dtype=torch.float32, device=like.device)


def _run(op):
    L.run_one(op, stream_ptr())


class _Packs:
    """The weight packs gode_igemm reads, one per (layer, direction, batch rows), re-packed when the weight's version moved: torch's
    own counter (optimizer.step) or _gode_ver (updates through a raw pointer: GANODETrainer's fused step)."""

    def __init__(self):
        self.cache = {}

    def get(self, l, direction, w, ver, g):
        hit = self.cache.get((l, direction, g.N))
        if hit is not None and hit[0] == ver:
            return hit[1]
        lib = L.lib()
        n = lib.gode_pack_size(C.byref(g), direction)
        if n <= 0:
            raise RuntimeError(f"bad product geometry ({n})")
        wp = hit[1] if hit is not None and hit[1].numel() == n and hit[1].device == w.device else _f32(n, like=w)
        L.check(lib.gode_pack_weights(C.byref(g), direction, dptr(w), dptr(wp), None, 0, stream_ptr()), "gode_pack_weights")
        self.cache[(l, direction, g.N)] = (ver, wp)
        return wp


def _product(direction, g, src, wp, rows, cols):
    """src[M][K] x the packed weight -> out[M][cols] (FPROP: cols = Co, DGRAD: cols = Ci)."""
    out = _f32(rows, cols, like=src)
    op = L.IgemmOp(g=g, dir=direction, act=L.ACT_NONE, epilogue=L.EPI_RAW, tile=0, src=dptr(src), wpack=dptr(wp), out=dptr(out))
    need = L.lib().gode_igemm_work_size(C.byref(op))
    if need < 0:
        raise RuntimeError(f"gode_igemm_work_size failed ({need})")
    work = _f32(need, like=src) if need > 0 else None
    op.work = dptr(work)
    _run(op)
    return out


def _wgrad(g, x, gy, w):
    dw = torch.empty_like(w)
    op = L.WgradOp(g=g, act=L.ACT_NONE, xform_on_y=0, splits=0, accumulate=0, x=dptr(x), y=dptr(gy), dw=dptr(dw))
    work = _f32(max(L.lib().gode_wgrad_work_size(C.byref(op)), 1), like=x)
    op.work = dptr(work)
    _run(op)
    return dw


class _FcNetFn(torch.autograd.Function):
    """A stack of Linear + activation (+ dropout) layers.  args = (W1, b1, ..., Wn, bn); acts[l] / drops[l] per layer."""

    @staticmethod
    def forward(ctx, packs, vers, acts, drops, key, x, *args):
        x = x.detach()
        Ws, bs = [w.detach() for w in args[0::2]], [b.detach() for b in args[1::2]]
        M = x.shape[0]
        hs = [x]
        for l, (W, b) in enumerate(zip(Ws, bs)):
            Co, Ci = W.shape
            g = _geom(M, Ci, Co)
            y = _product(L.FPROP, g, hs[-1], packs.get(l, L.FPROP, W, vers[l], g), M, Co)
            _run(L.FcActOp(y=dptr(y), b=dptr(b), out=dptr(y), M=M, C=Co, act=acts[l], key=key, layer=l, p=drops[l]))
            hs.append(y)
        ctx.packs, ctx.vers, ctx.acts, ctx.drops, ctx.key = packs, vers, acts, drops, key
        ctx.save_for_backward(*hs, *Ws)
        return hs[-1]

    @staticmethod
    def backward(ctx, g_out):
        n = len(ctx.acts)
        hs, Ws = ctx.saved_tensors[:n + 1], ctx.saved_tensors[n + 1:]
        M = hs[0].shape[0]
        g = g_out.contiguous()
        if g.dtype != torch.float32:
            raise RuntimeError("fp32 gradient expected")
        grads = [None] * (2 * n)
        lib = L.lib()
        for l in range(n - 1, -1, -1):
            Co, Ci = Ws[l].shape
            geom = _geom(M, Ci, Co)
            # the caller's gradient tensor is read, never written; the products' own outputs are updated in place
            g_y = _f32(M, Co, like=g) if l == n - 1 else g
            db = _f32(Co, like=g)
            need = lib.gode_fc_act_bwd_work_size(M, Co)
            work = _f32(need, like=g) if need > 0 else None
            _run(L.FcActBwdOp(g_out=dptr(g), out=dptr(hs[l + 1]), g_y=dptr(g_y), db=dptr(db), work=dptr(work), M=M, C=Co,
                              act=ctx.acts[l], key=ctx.key, layer=l, p=ctx.drops[l], accumulate=0))
            grads[2 * l], grads[2 * l + 1] = _wgrad(geom, hs[l], g_y, Ws[l]), db
            g = None
            if l > 0 or ctx.needs_input_grad[5]:
                g = _product(L.DGRAD, geom, g_y, ctx.packs.get(l, L.DGRAD, Ws[l], ctx.vers[l], geom), M, Ci)
        return (None, None, None, None, None, g, *grads)


class _FcNet(nn.Module):
    ACTS, DROPS = (), ()

    def _layers(self):
        return (self.fc1, self.fc2, self.fc3, self.fc4)

    def invalidate_packs(self):
        """Forget the packed weights: after writing a weight behind autograd's back (p.data.copy_(), dist.broadcast(p.data))."""
        self.__dict__.pop("_packs", None)

    def _apply_net(self, x, key, what):
        _check_input(x, self.fc1.in_features, what)
        args, vers = [], []
        for fc in self._layers():
            vers.append(tensor_version(fc.weight))     # read off the Parameter: _gode_ver lives on that object
            for t in (fc.weight, fc.bias):
                _require_gpu(t, what + " parameter")
                if t.dtype != torch.float32 or not t.is_contiguous():
                    raise RuntimeError(f"{what}: contiguous float32 parameters expected")
                args.append(t)
        packs = self.__dict__.get("_packs")
        if packs is None:
            packs = self.__dict__["_packs"] = _Packs()        # a plain attribute: not a buffer, not in the state_dict
        return _FcNetFn.apply(packs, tuple(vers), self.ACTS, self.DROPS, key, x, *args)


class Generator(_FcNet):
    """The notebook's Generator(g_input_dim, g_output_dim): forward(z[B, g_input_dim]) -> [B, g_output_dim] in (-1, 1)."""
    ACTS, DROPS = (L.ACT_LRELU, L.ACT_LRELU, L.ACT_LRELU, L.ACT_TANH), (0.0, 0.0, 0.0, 0.0)

    def __init__(self, g_input_dim, g_output_dim):
        super(Generator, self).__init__()
        self.fc1 = nn.Linear(g_input_dim, 256)
        self.fc2 = nn.Linear(self.fc1.out_features, self.fc1.out_features * 2)
        self.fc3 = nn.Linear(self.fc2.out_features, self.fc2.out_features * 2)
        self.fc4 = nn.Linear(self.fc3.out_features, g_output_dim)

    def forward(self, x):
        return self._apply_net(x, 0, "Generator input")


class Discriminator(_FcNet):
    """The notebook's Discriminator(d_input_dim): forward(x[B, d_input_dim]) -> probabilities [B, 1].  Drops in train AND
    eval mode, as the reference's F.dropout(x, 0.3) does; one draw from torch's CPU generator per forward (module docstring)."""
    ACTS, DROPS = (L.ACT_LRELU, L.ACT_LRELU, L.ACT_LRELU, L.ACT_SIGMOID), (DROP_P, DROP_P, DROP_P, 0.0)

    def __init__(self, d_input_dim):
        super(Discriminator, self).__init__()
        self.fc1 = nn.Linear(d_input_dim, 1024)
        self.fc2 = nn.Linear(self.fc1.out_features, self.fc1.out_features // 2)
        self.fc3 = nn.Linear(self.fc2.out_features, self.fc2.out_features // 2)
        self.fc4 = nn.Linear(self.fc3.out_features, 1)

    def forward(self, x):
        _check_input(x, self.fc1.in_features, "Discriminator input")       # refuse before the generator is touched
        key = int(torch.randint(0, 2 ** 62, (1,)))
        return self._apply_net(x, key, "Discriminator input")


class _BCEProbFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, p, t):
        p, t = p.detach().contiguous(), t.detach().contiguous()
        loss = torch.empty((), dtype=torch.float32, device=p.device)
        grad = torch.empty_like(p)
        _run(L.BceProbOp(p=dptr(p), t=dptr(t), grad=dptr(grad), loss=dptr(loss), n=p.numel(), gscale=1.0, accumulate=0))
        ctx.save_for_backward(grad)
        return loss

    @staticmethod
    def backward(ctx, gout):
        (grad,) = ctx.saved_tensors
        return grad * gout, None


class BCELoss(nn.Module):
    """nn.BCELoss() on gode_bce_prob: input [B, 1] or [B] probabilities, target of the same shape, mean reduction."""

    def __init__(self, weight=None, size_average=None, reduce=None, reduction='mean'):
        super().__init__()
        if weight is not None or size_average is not None or reduce is not None or reduction != 'mean':
            raise ValueError("BCELoss: only the default mean reduction without weights runs on the HIP kernel")
        self.reduction = reduction

    def forward(self, input, target):
        for t, what in ((input, "BCELoss input"), (target, "BCELoss target")):
            if not torch.is_tensor(t):
                raise RuntimeError(f"{what}: a tensor is expected")
            _require_gpu(t, what)
            if t.dtype != torch.float32:
                raise RuntimeError(f"{what}: float32 expected, got {t.dtype}")
        if input.shape != target.shape or input.numel() < 1 or not (input.dim() == 1 or (input.dim() == 2 and input.shape[1] == 1)):
            raise ValueError(f"BCELoss: input and target of one shape [B, 1] or [B] expected, got {tuple(input.shape)} and "
                             f"{tuple(target.shape)}")
        if target.requires_grad:
            raise RuntimeError("BCELoss: the target does not receive a gradient")
        return _BCEProbFn.apply(input, target)
