"""Stage 1 of the reference: DVD-GAN's generator residual block (stage1/GResBlock.py) on libgode.

  SpectralNorm     :10-64   one power iteration around a module's weight (gode_sn_fwd / gode_sn_bwd)
  ConditionalNorm  :66-88   affine-free train-mode BatchNorm, gain / offset per sample from Linear(n_condition, 2C)
  GResBlock        :90-167  CBN -> ReLU -> nearest x2 -> 3x3 conv -> CBN -> ReLU -> 3x3 conv, + a 1x1 projected skip,
                            optional 2x2 average pool

Same constructor signatures, state_dict keys and RNG consumption as the reference.  The nn.Conv2d / nn.BatchNorm2d /
nn.Linear children are parameter containers; every forward runs on the HIP kernels of csrc/gres.hip around gode_igemm /
gode_wgrad and raises off the GPU.  Data flow and deviations: DESIGN section 15.
"""
from __future__ import annotations

import ctypes as C

import torch
import torch.nn as nn
from torch.nn import Parameter
from torch.nn import functional as F

from . import _lib as L
from .engine import dptr, make_geom, stream_ptr
from .modules import _require_gpu

BN_MOMENTUM, BN_EPS = 0.1, 1e-5


def l2normalize(v, eps=1e-12):
    return v / (v.norm() + eps)


def _f32(*shape, like):
    return torch.empty(shape, dtype=torch.float32, device=like.device)


def _dense(t):
    """A caller tensor that the kernels may read through its strides: an expanded tensor (a zero stride over a dimension of
    more than one element, e.g. the gradient of `.sum()`) is materialised first -- all-zero strides are the C ABI's
    spelling of "channels-last contiguous" and must never reach it as genuine strides."""
    if any(st == 0 and n > 1 for st, n in zip(t.stride(), t.shape)):
        return t.contiguous()
    return t


def _nhwc_strides(t):
    """Element strides {N, H, W, C} of an [N, C, H, W] tensor (see _dense); a size-1 dimension, whose stride is
    never used, reports at least 1, so the tuple is never the all-zero sentinel."""
    st = [t.stride(0), t.stride(2), t.stride(3), t.stride(1)]
    sz = [t.shape[0], t.shape[2], t.shape[3], t.shape[1]]
    assert all(v > 0 or n == 1 for v, n in zip(st, sz)), "expanded tensor: call _dense first"
    return tuple(v if n > 1 else max(v, 1) for v, n in zip(st, sz))


def _set(arr, vals):
    for i, v in enumerate(vals):
        arr[i] = int(v)


def _check_input(x, what):
    _require_gpu(x, what)
    if x.dtype != torch.float32:
        raise RuntimeError(f"{what}: fp32 expected, got {x.dtype}")


# ---------------------------------------------------------------------------------------------------------------
# spectral normalisation
class _SNFn(torch.autograd.Function):
    """weight_bar, u, v -> weight_bar / sigma; u and v are advanced in place (constants of the gradient)."""

    @staticmethod
    def forward(ctx, wbar, u, v, iterations):
        h = wbar.shape[0]
        w = wbar.numel() // h
        wb = wbar.detach().contiguous()
        wout, sigma, work = torch.empty_like(wb), _f32(1, like=wb), _f32(h + w, like=wb)
        op = L.SnOp(wbar=dptr(wb), u=dptr(u), v=dptr(v), wout=dptr(wout), sigma=dptr(sigma), work=dptr(work), h=h, w=w)
        for _ in range(iterations):
            L.run_one(op, stream_ptr())
        ctx.save_for_backward(wb, u.detach().clone(), v.detach().clone(), sigma)
        return wout

    @staticmethod
    def backward(ctx, G):
        wb, u, v, sigma = ctx.saved_tensors
        h = wb.shape[0]
        G = G.contiguous()
        out = torch.empty_like(wb)
        work = torch.empty(L.SN_BWD_BLOCKS, dtype=torch.float64, device=wb.device)
        L.run_one(L.SnBwdOp(G=dptr(G), wbar=dptr(wb), u=dptr(u), v=dptr(v), sigma=dptr(sigma), dwbar=dptr(out),
                            work=dptr(work), h=h, w=wb.numel() // h), stream_ptr())
        return out, None, None, None


class SpectralNorm(nn.Module):
    """stage1/GResBlock.py:10-64.  Around any module: every forward (train and eval mode alike) advances u and v in place
    and sets `<name>` to weight_bar / sigma through the kernels above, then calls the wrapped module's own forward -- stock
    torch, off the hot path (GResBlock runs its convolutions on gode_igemm instead)."""

    def __init__(self, module, name='weight', power_iterations=1):
        super().__init__()
        if power_iterations < 1:
            raise NotImplementedError("SpectralNorm: power_iterations >= 1")
        self.module, self.name, self.power_iterations = module, name, power_iterations
        if not all(hasattr(module, name + s) for s in ("_u", "_v", "_bar")):
            w = getattr(module, name)
            height = w.data.shape[0]
            width = w.data.numel() // height
            u = Parameter(l2normalize(w.data.new(height).normal_(0, 1)), requires_grad=False)
            v = Parameter(l2normalize(w.data.new(width).normal_(0, 1)), requires_grad=False)
            w_bar = Parameter(w.data)
            del module._parameters[name]
            module.register_parameter(name + "_u", u)
            module.register_parameter(name + "_v", v)
            module.register_parameter(name + "_bar", w_bar)

    def normalized_weight(self):
        m, n = self.module, self.name
        w_bar = getattr(m, n + "_bar")
        _check_input(w_bar, "SpectralNorm weight")
        return _SNFn.apply(w_bar, getattr(m, n + "_u"), getattr(m, n + "_v"), self.power_iterations)

    def _update_u_v(self):
        setattr(self.module, self.name, self.normalized_weight())

    def forward(self, *args):
        self._update_u_v()
        return self.module.forward(*args)


# ---------------------------------------------------------------------------------------------------------------
# building blocks shared by ConditionalNorm and GResBlock (all enqueue on the current stream)
def _run(op):
    L.run_one(op, stream_ptr())


def _embed(cond, W, b):
    N, K = cond.shape
    gb = _f32(N, W.shape[0], like=cond)
    _run(L.CbnEmbedOp(cond=dptr(cond), W=dptr(W), b=dptr(b), gb=dptr(gb), N=N, K=K, C2=W.shape[0]))
    return gb


def _embed_bwd(cond, W, dgb, need_cond):
    N, K = cond.shape
    dW, db = torch.empty_like(W), _f32(W.shape[0], like=W)
    dcond = _f32(N, K, like=cond) if need_cond else None
    _run(L.CbnEmbedBwdOp(cond=dptr(cond), W=dptr(W), dgb=dptr(dgb), dW=dptr(dW), db=dptr(db), dcond=dptr(dcond), N=N, K=K,
                         C2=W.shape[0]))
    return dW, db, dcond


def _finalize(bn, stats, rows, C_, count, training, like):
    """Partial sums -> (mean, invstd) and the running-statistics update; eval mode: the running statistics."""
    mean, invstd, scale, shift = (_f32(C_, like=like) for _ in range(4))
    _run(L.BnFinalizeOp(stats=dptr(stats), rows=rows, ncols=C_, C=C_, count=count, gamma=None, beta=None,
                        running_mean=dptr(bn.running_mean), running_var=dptr(bn.running_var),
                        num_batches_tracked=dptr(bn.num_batches_tracked), mean=dptr(mean), invstd=dptr(invstd),
                        scale=dptr(scale), shift=dptr(shift), momentum=BN_MOMENTUM, eps=BN_EPS, training=1 if training else 0))
    return mean, invstd


def _input_stats(x, bn, training):
    """Batch statistics of a caller tensor [N, C, H, W] read through its strides."""
    N, C_, H, W = x.shape
    stats, rows = None, 0
    if training:
        rows = L.lib().gode_chstats_rows(N * H * W)
        stats = _f32(2 * C_ * rows, like=x)
        op = L.ChstatsOp(x=dptr(x), stats=dptr(stats), N=N, H=H, W=W, C=C_, rows=rows)
        _set(op.xs, _nhwc_strides(x))
        _run(op)
    return _finalize(bn, stats, rows, C_, N * H * W, training, x)


def _apply(src, ss, dims, bias, mean, invstd, gb, f, act):
    N, H, W, C_ = dims
    out = _f32(N, H * f, W * f, C_, like=src)
    op = L.CbnApplyOp(src=dptr(src), bias=dptr(bias), mean=dptr(mean), invstd=dptr(invstd), gb=dptr(gb), out=dptr(out),
                      N=N, H=H, W=W, C=C_, f=f, act=act)
    _set(op.ss, ss)
    _run(op)
    return out


def _cbn_bwd(g_a, a, src, ss, dims, bias, mean, invstd, gb, gadd, want_dbias, g_out, gos, f, act, eval_mode):
    N, H, W, C_ = dims
    n = L.lib().gode_cbn_bwd_work_size(N, H, W, C_)
    work = torch.empty((n + 1) // 2, dtype=torch.float64, device=g_a.device)
    dgb = _f32(N, 2 * C_, like=g_a) if mean is not None else None
    dbias = _f32(C_, like=g_a) if want_dbias else None
    op = L.CbnBwdOp(g_a=dptr(g_a), a=dptr(a), src=dptr(src), bias=dptr(bias), mean=dptr(mean), invstd=dptr(invstd),
                    gb=dptr(gb), gadd=dptr(gadd), work=dptr(work), dgb=dptr(dgb), dbias=dptr(dbias), g_out=dptr(g_out),
                    N=N, H=H, W=W, C=C_, f=f, act=act, eval_mode=1 if eval_mode else 0)
    _set(op.ss, ss)
    _set(op.gos, gos)
    _run(op)
    return dgb, dbias


class _Conv:
    """One stride-1, size-preserving convolution of the block on gode_igemm / gode_wgrad: x[N, H, W, Ci] (given with its
    element strides) -> y[N, H, W, Co] channels-last."""

    def __init__(self, N, H, W, Ci, Co, k, p):
        self.g = make_geom(N, Ci, Co, (1, H, W), (1, H, W), (1, k[0], k[1]), (1, 1, 1), (0, p[0], p[1]))
        self.dims_y, self.dims_x = (N, H, W, Co), (N, H, W, Ci)

    def _pack(self, w, direction):
        n = L.lib().gode_pack_size(C.byref(self.g), direction)
        if n <= 0:
            raise RuntimeError(f"bad convolution geometry ({n})")
        wp = _f32(n, like=w)
        L.check(L.lib().gode_pack_weights(C.byref(self.g), direction, dptr(w), dptr(wp), None, 0, stream_ptr()),
                "gode_pack_weights")
        return wp

    def _igemm(self, direction, src, gs, w, out_dims, want_stats):
        lib = L.lib()
        wp = self._pack(w, direction)
        out = _f32(*out_dims, like=src)
        op = L.IgemmOp(g=self.g, dir=direction, act=L.ACT_NONE, epilogue=L.EPI_RAW, tile=0, src=dptr(src), wpack=dptr(wp),
                       out=dptr(out))
        if gs is not None:
            _set(op.gs, gs)
        stats, rows = None, 0
        if want_stats:
            rows = lib.gode_igemm_stats_rows(C.byref(op))
            if rows <= 0:
                raise RuntimeError(f"no partial-statistics layout for this geometry ({rows})")
            stats = _f32(2 * out_dims[3] * rows, like=src)
            op.stats = dptr(stats)
        need = lib.gode_igemm_work_size(C.byref(op))
        if need < 0:
            raise RuntimeError(f"gode_igemm_work_size failed ({need})")
        work = _f32(need, like=src) if need > 0 else None
        op.work = dptr(work)
        _run(op)
        return out, stats, rows

    def fprop(self, x, xs, w, want_stats=False):
        gs = None if xs is None else (xs[0], 0, xs[1], xs[2], xs[3])
        return self._igemm(L.FPROP, x, gs, w, self.dims_y, want_stats)

    def dgrad(self, gy, w):
        return self._igemm(L.DGRAD, gy, None, w, self.dims_x, False)[0]

    def wgrad(self, x, xs, gy, w):
        dw = torch.empty_like(w)
        op = L.WgradOp(g=self.g, act=L.ACT_NONE, xform_on_y=0, splits=0, accumulate=0, x=dptr(x), y=dptr(gy), dw=dptr(dw))
        if xs is not None:
            _set(op.xs, (xs[0], 0, xs[1], xs[2], xs[3]))
        work = _f32(max(L.lib().gode_wgrad_work_size(C.byref(op)), 1), like=x)
        op.work = dptr(work)
        _run(op)
        return dw


# ---------------------------------------------------------------------------------------------------------------
# ConditionalNorm
class _CBNFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, mod, x, cond, We, be):
        N, C_, H, W = x.shape
        training = mod.training
        xd, cd = _dense(x.detach()), cond.detach().contiguous()
        mean, invstd = _input_stats(xd, mod.bn, training)
        gb = _embed(cd, We.detach(), be.detach())
        ss = _nhwc_strides(xd)
        out = _apply(xd, ss, (N, H, W, C_), None, mean, invstd, gb, 1, L.ACT_NONE)
        ctx.save_for_backward(xd, cd, We.detach(), mean, invstd, gb, out)
        ctx.eval_mode = not training
        return out.permute(0, 3, 1, 2)

    @staticmethod
    def backward(ctx, g):
        x, cond, We, mean, invstd, gb, out = ctx.saved_tensors
        N, C_, H, W = x.shape
        g_a = g.permute(0, 2, 3, 1).contiguous()
        gx = torch.empty(x.shape, dtype=torch.float32, device=x.device)
        dgb, _ = _cbn_bwd(g_a, out, x, _nhwc_strides(x), (N, H, W, C_), None, mean, invstd, gb, None, False, gx,
                          _nhwc_strides(gx), 1, L.ACT_NONE, ctx.eval_mode)
        dW, db, dcond = _embed_bwd(cond, We, dgb, ctx.needs_input_grad[2])
        return None, gx, dcond, dW, db


class ConditionalNorm(nn.Module):
    """stage1/GResBlock.py:66-88: gamma[n] * BatchNorm(x) + beta[n], [gamma | beta] = embed(class_id)."""

    def __init__(self, in_channel, n_condition=96):
        super().__init__()
        self.in_channel = in_channel
        self.bn = nn.BatchNorm2d(self.in_channel, affine=False)
        self.embed = nn.Linear(n_condition, self.in_channel * 2)
        self.embed.weight.data[:, :self.in_channel].normal_(1, 0.02)
        self.embed.weight.data[:, self.in_channel:].zero_()

    def forward(self, x, class_id):
        _check_input(x, "ConditionalNorm input")
        _check_input(class_id, "ConditionalNorm condition")
        if x.dim() != 4 or x.shape[1] != self.in_channel or class_id.shape != (x.shape[0], self.embed.in_features):
            raise RuntimeError("ConditionalNorm: x [N, C, H, W] and class_id [N, n_condition] expected")
        return _CBNFn.apply(self, x, class_id, self.embed.weight, self.embed.bias)


# ---------------------------------------------------------------------------------------------------------------
# GResBlock
class _GResFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, blk, x, cond, W0, b0, W1, b1, Wsc, bsc, We1, be1, We2, be2):
        N, Ci, H, W = x.shape
        Co, f, d, bn, training = W0.shape[0], blk.upsample_factor, blk.downsample_factor, blk.bn, blk.training
        Hf, Wf = H * f, W * f
        x, W0, b0, W1, b1, Wsc, bsc = (t.detach() for t in (x, W0, b0, W1, b1, Wsc, bsc))
        x = _dense(x)
        xs = _nhwc_strides(x)
        c0, c1, csc = _Conv(N, Hf, Wf, Ci, Co, blk.kernel, blk.pad), _Conv(N, Hf, Wf, Co, Co, blk.kernel, blk.pad), \
            _Conv(N, H, W, Ci, Co, (1, 1), (0, 0))
        m1 = i1 = gb1 = m2 = i2 = gb2 = None
        if bn:
            cond = cond.detach().contiguous()
            We1, be1, We2, be2 = (t.detach() for t in (We1, be1, We2, be2))
            m1, i1 = _input_stats(x, blk.CBNorm1.bn, training)
            gb1 = _embed(cond, We1, be1)
        a0 = _apply(x, xs, (N, H, W, Ci), None, m1, i1, gb1, f, L.ACT_RELU)
        y0, stats, rows = c0.fprop(a0, None, W0, want_stats=bn and training)
        if bn:
            # conv0's bias only shifts the batch mean: statistics of the raw output, the bias goes into running_mean
            m2, i2 = _finalize(blk.CBNorm2.bn, stats, rows, Co, N * Hf * Wf, training, x)
            if training:
                rm = blk.CBNorm2.bn.running_mean
                L.call("gode_scale", lambda: L.check(L.lib().gode_scale(dptr(rm), dptr(b0), Co, BN_MOMENTUM, 1, stream_ptr()),
                                                     "gode_scale"))
            gb2 = _embed(cond, We2, be2)
        bias0 = b0 if (not bn or not training) else None
        a1 = _apply(y0, (0, 0, 0, 0), (N, Hf, Wf, Co), bias0, m2, i2, gb2, 1, L.ACT_RELU)
        y1, _, _ = c1.fprop(a1, None, W1)
        ysc, _, _ = csc.fprop(x, xs, Wsc)
        Ho, Wo = Hf // d, Wf // d
        y = _f32(N, Ho, Wo, Co, like=x)
        _run(L.GresOutOp(main=dptr(y1), sc=dptr(ysc), b_main=dptr(b1), b_sc=dptr(bsc), y=dptr(y), N=N, H=H, W=W, C=Co, f=f,
                         down=d))
        ctx.cfg, ctx.convs, ctx.eval_mode = (f, d, bn), (c0, c1, csc), not training
        ctx.save_for_backward(x, W0, W1, Wsc, a0, y0, a1, m1, i1, gb1, m2, i2, gb2, cond if bn else None, We1, We2, bias0)
        return y.permute(0, 3, 1, 2)

    @staticmethod
    def backward(ctx, gy):
        x, W0, W1, Wsc, a0, y0, a1, m1, i1, gb1, m2, i2, gb2, cond, We1, We2, bias0 = ctx.saved_tensors
        (f, d, bn), (c0, c1, csc) = ctx.cfg, ctx.convs
        N, Ci, H, W = x.shape
        Co = W0.shape[0]
        gy = _dense(gy)
        Hf, Wf = H * f, W * f
        xs = _nhwc_strides(x)
        lib = L.lib()
        # block output: bias gradients, skip-branch gradient at the input resolution, conv1's output gradient
        g_sc = _f32(N, H, W, Co, like=x)
        g_main = _f32(N, Hf, Wf, Co, like=x) if d == 1 else None
        db = _f32(Co, like=x)
        work = _f32(max(lib.gode_gres_out_bwd_work_size(N, H, W, Co, f, d), 1), like=x)
        op = L.GresOutBwdOp(g_y=dptr(gy), g_sc=dptr(g_sc), g_main=dptr(g_main), db=dptr(db), work=dptr(work), N=N, H=H, W=W,
                            C=Co, f=f, down=d)
        _set(op.gys, _nhwc_strides(gy))
        _run(op)
        g1 = g_main if d == 1 else g_sc
        dW1 = c1.wgrad(a1, None, g1, W1)
        g_a1 = c1.dgrad(g1, W1)
        dWsc = csc.wgrad(x, xs, g_sc, Wsc)
        g_xsc = csc.dgrad(g_sc, Wsc)
        g_y0 = _f32(N, Hf, Wf, Co, like=x)
        dgb2, db0 = _cbn_bwd(g_a1, a1, y0, (0, 0, 0, 0), (N, Hf, Wf, Co), bias0, m2, i2, gb2, None, True, g_y0,
                             (0, 0, 0, 0), 1, L.ACT_RELU, ctx.eval_mode)
        dW0 = c0.wgrad(a0, None, g_y0, W0)
        g_a0 = c0.dgrad(g_y0, W0)
        gx = torch.empty(x.shape, dtype=torch.float32, device=x.device)
        dgb1, _ = _cbn_bwd(g_a0, a0, x, xs, (N, H, W, Ci), None, m1, i1, gb1, g_xsc, False, gx, _nhwc_strides(gx), f,
                           L.ACT_RELU, ctx.eval_mode)
        dcond = dWe1 = dbe1 = dWe2 = dbe2 = None
        if bn:
            need_c = ctx.needs_input_grad[2]
            dWe1, dbe1, dcond = _embed_bwd(cond, We1, dgb1, need_c)
            dWe2, dbe2, dcond2 = _embed_bwd(cond, We2, dgb2, need_c)
            if need_c:
                L.call("gode_scale", lambda: L.check(lib.gode_scale(dptr(dcond), dptr(dcond2), dcond.numel(), 1.0, 1,
                                                                    stream_ptr()), "gode_scale"))
        return None, gx, dcond, dW0, db0, dW1, db, dWsc, db.clone(), dWe1, dbe1, dWe2, dbe2


def _pair(v, what):
    if isinstance(v, int):
        return (v, v)
    v = tuple(int(a) for a in v)
    if len(v) != 2:
        raise NotImplementedError(f"GResBlock: 2-D {what} expected, got {v}")
    return v


class GResBlock(nn.Module):
    """stage1/GResBlock.py:90-167.  forward(x[BT, C, H, W], condition[BT, n_class]) -> [BT, Cout, H', W'] (a channels-last
    view), fp32 on the GPU.  downsample_factor != 1 switches both CBNs off and forces upsample_factor = 1, as the reference
    does (the CBNorm modules then exist without ever receiving a gradient)."""

    def __init__(self, in_channel, out_channel, kernel_size=None, padding=1, stride=1, n_class=96, bn=True,
                 activation=F.relu, upsample_factor=2, downsample_factor=1):
        super().__init__()
        if activation is not F.relu:
            raise NotImplementedError("GResBlock: only activation=F.relu runs on the HIP kernels")
        if _pair(stride, "stride") != (1, 1):
            raise NotImplementedError("GResBlock: stride 1 only")
        if upsample_factor not in (1, 2) or downsample_factor not in (1, 2):
            raise NotImplementedError("GResBlock: up / down factors 1 or 2")
        if kernel_size is None:
            kernel_size = [3, 3]
        self.kernel, self.pad = _pair(kernel_size, "kernel_size"), _pair(padding, "padding")
        if any(k != 2 * p + 1 for k, p in zip(self.kernel, self.pad)):
            raise NotImplementedError("GResBlock: kernel_size / padding must preserve the map size (k = 2p + 1)")
        self.upsample_factor = upsample_factor if downsample_factor == 1 else 1
        self.downsample_factor = downsample_factor
        self.activation = activation
        self.bn = bn if downsample_factor == 1 else False
        self.conv0 = SpectralNorm(nn.Conv2d(in_channel, out_channel, kernel_size, stride, padding, bias=True))
        self.conv1 = SpectralNorm(nn.Conv2d(out_channel, out_channel, kernel_size, stride, padding, bias=True))
        self.skip_proj = True
        self.conv_sc = SpectralNorm(nn.Conv2d(in_channel, out_channel, 1, 1, 0))
        if bn:
            self.CBNorm1 = ConditionalNorm(in_channel, n_class)
            self.CBNorm2 = ConditionalNorm(out_channel, n_class)

    def forward(self, x, condition=None):
        _check_input(x, "GResBlock input")
        Ci = self.conv0.module.weight_bar.shape[1]
        if x.dim() != 4 or x.shape[1] != Ci:
            raise RuntimeError(f"GResBlock: x [BT, {Ci}, H, W] expected, got {tuple(x.shape)}")
        emb = (None, None, None, None)
        if self.bn:
            if condition is None:
                raise RuntimeError("GResBlock(bn=True) needs a condition")
            _check_input(condition, "GResBlock condition")
            if condition.shape != (x.shape[0], self.CBNorm1.embed.in_features):
                raise RuntimeError("GResBlock: condition [BT, n_class] expected")
            emb = (self.CBNorm1.embed.weight, self.CBNorm1.embed.bias, self.CBNorm2.embed.weight, self.CBNorm2.embed.bias)
        else:
            condition = None
        if self.downsample_factor == 2 and (x.shape[2] < 2 or x.shape[3] < 2):
            raise RuntimeError("GResBlock: a 2x2 pool needs a map of at least 2 x 2")
        ws = [c.normalized_weight() for c in (self.conv0, self.conv1, self.conv_sc)]
        for c, w in zip((self.conv0, self.conv1, self.conv_sc), ws):
            setattr(c.module, c.name, w)
        return _GResFn.apply(self, x, condition, ws[0], self.conv0.module.bias, ws[1], self.conv1.module.bias, ws[2],
                             self.conv_sc.module.bias, *emb)
