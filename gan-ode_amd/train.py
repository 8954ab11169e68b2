"""The training iteration of mnist_moco_ode.py:113-163 (== ucf_moco_ode.py:115-165) restated as `train_step`, with
the loss and optimiser lowered to libgode kernels, plus single-node data parallelism: one process per GPU, one RCCL
all-reduce of a flat fp32 gradient bucket per optimiser step (torch.distributed backend "nccl" is RCCL on ROCm).

The reference has no `train_step` function (the body is inline in train()); the call sequence, the RNG draws and
the d_iters=2 structure below follow that body line by line.
"""
from __future__ import annotations

import contextlib
from typing import List, Optional, Sequence

import torch
import torch.distributed as dist

from . import _lib as L
from .engine import PointerTable, bump_version, stream_ptr
from .modules import PatchImageDiscriminator, VideoDiscriminator, VideoGenerator, VideoGeneratorMNISTODE


def host_cpu_quota():
    """CPUs this process may actually use: the cgroup CPU quota if there is one, else the affinity mask size."""
    import os
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if quota != "max":
            n = min(n, max(1, int(int(quota) / int(period))))
    except Exception:
        pass
    return n


def limit_host_threads(n=None):
    """torch's intra-op pool defaults to one thread per visible core (128 on the MI355X host) while the container's
    cgroup quota is 16 CPUs: the idle pool spin-waits after every parallel region, the quota is exhausted and the
    whole process is throttled for the rest of the 100 ms period (seen as random 75-90 ms stalls in the host-side
    noise draws).  Call this once at start-up (bench.py does) to size the pool to the quota."""
    if n is None:
        import os
        # one process per GPU: the quota is shared by the ranks of this node
        local = int(os.environ.get("LOCAL_WORLD_SIZE", os.environ.get("WORLD_SIZE", "1")) or 1)
        n = max(1, min(16, host_cpu_quota() // max(1, local)))
    if torch.get_num_threads() > n:
        torch.set_num_threads(n)
    return n


def freeze_host_gc():
    """One full-heap (generation-2) pass of Python's cyclic garbage collector over the heap that `import torch` and
    the plans leave behind takes 75-100 ms, and the first one of a run lands after ~60 training iterations: one
    iteration of 106 ms among 12.6 ms ones (scripts/diag_iter_values.py; the GPU drains and idles meanwhile).  Moving
    the long-lived objects to the permanent generation after warm-up makes later passes walk only young objects.
    GanTrainer calls this once after its second iteration; bench.py before its timed loops."""
    import gc
    gc.collect()
    gc.freeze()


# ------------------------------------------------------------------------------------------------------------------
# loss
# ------------------------------------------------------------------------------------------------------------------
_UNIT = {}


def unit_grad(device):
    """A cached device scalar 1.0: `loss.backward(gradient=unit_grad(dev))` spares autograd's ones_like fill, and the
    loss nodes below recognise it (by address) and hand their stored gradients on without multiplying."""
    t = _UNIT.get(device)
    if t is None:
        t = _UNIT[device] = torch.ones((), dtype=torch.float32, device=device)
    return t


def _scaled(grad, gout):
    if gout.data_ptr() == unit_grad(gout.device).data_ptr():
        return grad
    return grad * gout      # a caller-supplied upstream gradient (not the training loop's path)


# Every loss of the training loops is ONE autograd node: its terms add into one device scalar (the first stores, the
# others accumulate: `bce(real, 1) + bce(fake, 0)`, mnist_moco_ode.py:126-128, needs no elementwise add) and write the
# upstream gradient of their inputs in place, so the backward launches nothing.
#
# A term is (op class, {pointer field: (input, first element)}, the op's other fields): the named field receives the
# input's data pointer and its gradient field (_GRAD_FIELD) the same place in the input's gradient -- the same element offset,
# so a term whose gradient rows are not laid out like its input rows (_ce with gld != ld) must start at element 0.  Terms are
# applied in order -- the order of the fp32 sum.  The terms of an input together write every element of its gradient.
_GRAD_FIELD = {"logits": "grad", "fake": "grad_fake", "real": "grad_real"}
_REDUCTIONS = {"mean": 0, "sum": 1}


def _bce(i, first, n, stride, target):
    """gode_bce_logits: mean BCEWithLogits of n elements of input i, `stride` apart from element `first`, against target."""
    return L.BceOp, {"logits": (i, first)}, dict(n=n, stride=stride, target=float(target))


def _ce(i, col0, ncls, rows, n_lab, labels, rows_per_label, ld, gld=None):
    """gode_ce_logits over the class columns col0 .. col0 + ncls of the [rows, ld] input i (gradient rows gld apart): the
    first n_lab rows are labelled, rows_per_label consecutive rows share a label; the others get zero gradient."""
    return L.CeOp, {"logits": (i, col0)}, dict(labels=None if labels is None else labels.data_ptr(), B=rows, n_lab=n_lab,
                                               C=ncls, ld=ld, gld=ld if gld is None else gld,
                                               rows_per_label=rows_per_label)


def _wgan(sign, reduction, n, fake, real=None):
    """gode_wgan_logits: sign * reduce(fake [- real]) over n elements; fake, real: (input, first element)."""
    return L.WganOp, ({"fake": fake} if real is None else {"real": real, "fake": fake}), dict(
        n=n, sign=sign, reduction=_REDUCTIONS[reduction])


class _LossFn(torch.autograd.Function):
    """sum of loss terms (see above) over 1..n input tensors.  There is one gradient tensor per input, in the layout of
    the contiguous input.  in_place: the inputs are read as they are (categorical_cross_entropy's strided view; its term
    carries the leading dimensions) instead of through .contiguous()."""

    @staticmethod
    def forward(ctx, terms, in_place, *xs):
        if not in_place:
            xs = [x.contiguous() for x in xs]
        loss = torch.empty((), dtype=torch.float32, device=xs[0].device)
        grads = [torch.empty_like(x, memory_format=torch.contiguous_format) for x in xs]
        st = stream_ptr()
        for k, (op_cls, ptrs, fields) in enumerate(terms):
            op = op_cls(loss=loss.data_ptr(), gscale=1.0, accumulate=1 if k else 0, **fields)
            for name, (i, first) in ptrs.items():
                setattr(op, name, xs[i].data_ptr() + 4 * first)
                setattr(op, _GRAD_FIELD[name], grads[i].data_ptr() + 4 * first)
            L.run_one(op, st)
        ctx.save_for_backward(*grads)
        return loss

    @staticmethod
    def backward(ctx, gout):
        return (None, None, *[_scaled(g, gout) for g in ctx.saved_tensors])


def bce_with_logits_const(logits: torch.Tensor, target: float) -> torch.Tensor:
    """nn.BCEWithLogitsLoss()(logits, full_like(logits, target)) -- mean reduction (mnist_moco_ode.py:89,126-128)."""
    if not logits.is_cuda:
        raise RuntimeError("bce_with_logits_const runs only on the GPU through libgode.so")
    return _LossFn.apply([_bce(0, 0, logits.numel(), 1, target)], False, logits)


def bce_with_logits_halves(joint: torch.Tensor, target_first: float, target_second: float) -> torch.Tensor:
    """nn.BCEWithLogitsLoss()(x[:B], t1) + nn.BCEWithLogitsLoss()(x[B:], t2) for the joint output of
    forward_pair_joint (mnist_moco_ode.py:126-128,145-147): each term is mean-reduced over its half, the gradient is one
    tensor in the joint layout."""
    if not joint.is_cuda or joint.shape[0] % 2:
        raise RuntimeError("bce_with_logits_halves: a CUDA tensor with an even leading dimension is expected")
    n = joint.numel() // 2
    return _LossFn.apply([_bce(0, 0, n, 1, target_first), _bce(0, n, n, 1, target_second)], False, joint)


def bce_with_logits_pair(logits_a, target_a: float, logits_b, target_b: float) -> torch.Tensor:
    """bce_with_logits_const(a, ta) + bce_with_logits_const(b, tb) as one node (same arithmetic: each term is
    mean-reduced on its own, the two means are added in fp32)."""
    if not (logits_a.is_cuda and logits_b.is_cuda):
        raise RuntimeError("bce_with_logits_pair runs only on the GPU through libgode.so")
    return _LossFn.apply([_bce(0, 0, logits_a.numel(), 1, target_a), _bce(1, 0, logits_b.numel(), 1, target_b)], False,
                         logits_a, logits_b)


# Categorical MoCoGAN (models/mocogan.py:167-182): nn.CrossEntropyLoss() on the class logits, alone or fused with the
# BCE terms of the same optimiser step.  A categorical head is ONE [B, 1 + C] tensor (column 0: the real/fake logit,
# columns 1..C: the class logits): its BCE term strides over column 0, its class term over the other columns.
def _check_labels(labels, rows, what):
    if not (torch.is_tensor(labels) and labels.is_cuda and labels.dtype == torch.int64 and labels.dim() == 1
            and labels.shape[0] == rows):
        raise RuntimeError(f"{what}: labels must be an int64 device tensor [{rows}]")
    return labels.contiguous()


def _check_head(head, what):
    """-> (videos, rows, width): a categorical head is [B, 1 + C], or channels-last [B, Do, Ho, Wo, 1 + C] as the stack
    writes it -- rows = B * Do * Ho * Wo positions of 1 + C columns each (a patch head when Do * Ho * Wo > 1: every
    position carries a real/fake logit and classifies its video)."""
    if not (torch.is_tensor(head) and head.is_cuda):
        raise RuntimeError(f"{what} runs only on the GPU through libgode.so")
    if head.dtype != torch.float32 or head.dim() not in (2, 5) or head.shape[-1] < 2:
        raise RuntimeError(f"{what}: a float32 categorical head [B, 1 + C] or [B, Do, Ho, Wo, 1 + C] is expected")
    W = head.shape[-1]
    return head.shape[0], head.numel() // W, W


def categorical_cross_entropy(categ: torch.Tensor, labels: torch.Tensor) -> torch.Tensor:
    """nn.CrossEntropyLoss()(categ, labels): categ [B, C] fp32 (a view of a categorical head is read in place), labels
    int64 [B] on the device; one launch, fixed summation order."""
    if not (torch.is_tensor(categ) and categ.is_cuda):
        raise RuntimeError("categorical_cross_entropy runs only on the GPU through libgode.so")
    if categ.dtype != torch.float32 or categ.dim() != 2:
        raise RuntimeError("categorical_cross_entropy: float32 class logits [B, C] are expected")
    labels = _check_labels(labels, categ.shape[0], "categorical_cross_entropy")
    B, C = categ.shape
    # rows stride(0) apart are read where they lie; the gradient is compact [B, C] either way
    in_place = categ.stride(1) == 1 and categ.stride(0) >= C
    return _LossFn.apply([_ce(0, 0, C, B, B, labels, 1, categ.stride(0) if in_place else C, C)], in_place, categ)


def bce_ce_head(head, target: float, labels) -> torch.Tensor:
    """BCEWithLogits(head[..., :1], target) + CrossEntropy(head[..., 1:], labels) on a categorical head (_check_head); a
    patch head's positions all take their video's label, each term is the mean over all positions."""
    B, R, W = _check_head(head, "bce_ce_head")
    labels = _check_labels(labels, B, "bce_ce_head")
    return _LossFn.apply([_bce(0, 0, R, W, target), _ce(0, 1, W - 1, R, R, labels, R // B, W)], False, head)


def bce_ce_head_pair(head, target: float, labels, logits_b, target_b: float) -> torch.Tensor:
    """bce_ce_head's two terms with BCEWithLogits(logits_b, target_b) between them (the generator step: video head, image
    logits, class term): BCE(head[:, :1]) + BCE(logits_b) + CE(head[:, 1:], labels), added in that order."""
    B, R, W = _check_head(head, "bce_ce_head_pair")
    if not logits_b.is_cuda:
        raise RuntimeError("bce_ce_head_pair runs only on the GPU through libgode.so")
    labels = _check_labels(labels, B, "bce_ce_head_pair")
    return _LossFn.apply([_bce(0, 0, R, W, target), _bce(1, 0, logits_b.numel(), 1, target_b),
                          _ce(0, 1, W - 1, R, R, labels, R // B, W)], False, head, logits_b)


def bce_ce_head_halves(joint, target_first: float, target_second: float, labels_first) -> torch.Tensor:
    """On the joint categorical head [2B, 1 + C] of forward_pair_joint(real, fake): BCE(first half, t1) + BCE(second
    half, t2) + CE(class logits of the first half, labels_first); the second half's class columns get zero gradient."""
    n2, R2, W = _check_head(joint, "bce_ce_head_halves")
    if n2 % 2:
        raise RuntimeError("bce_ce_head_halves: an even leading dimension is expected")
    B, R = n2 // 2, R2 // 2
    labels = _check_labels(labels_first, B, "bce_ce_head_halves")
    return _LossFn.apply([_bce(0, 0, R, W, target_first), _bce(0, R * W, R, W, target_second),
                          _ce(0, 1, W - 1, R2, R, labels, R // B, W)], False, joint)


def bce_ce_heads(head_a, target_a: float, labels_a, head_b, target_b: float) -> torch.Tensor:
    """bce_ce_head_halves for two separate passes: BCE(a, ta) + BCE(b, tb) + CE(class logits of a, labels_a)."""
    B, R, W = _check_head(head_a, "bce_ce_heads")
    _, Rb, Wb = _check_head(head_b, "bce_ce_heads")
    if Wb != W:
        raise RuntimeError("bce_ce_heads: both heads must have the same width")
    labels = _check_labels(labels_a, B, "bce_ce_heads")
    return _LossFn.apply([_bce(0, 0, R, W, target_a), _bce(1, 0, Rb, W, target_b),
                          _ce(0, 1, W - 1, R, R, labels, R // B, W), _ce(1, 1, W - 1, Rb, 0, None, 1, W)], False,
                         head_a, head_b)


# Wasserstein loss (torchgan.losses, mnist_moco_ode_wgan.py:13,97-98): generator -reduce(fgz), discriminator
# reduce(fgz - fx), no clipping, no gradient penalty.
def _wgan_check(*xs):
    for x in xs:
        if not x.is_cuda:
            raise RuntimeError("the Wasserstein losses run only on the GPU through libgode.so")


def wasserstein_generator_loss(fgz: torch.Tensor, reduction: str = "mean") -> torch.Tensor:
    """torchgan's wasserstein_generator_loss: reduce(-fgz)."""
    _wgan_check(fgz)
    return _LossFn.apply([_wgan(-1.0, reduction, fgz.numel(), (0, 0))], False, fgz)


def wasserstein_generator_loss_pair(fgz_a: torch.Tensor, fgz_b: torch.Tensor, reduction: str = "mean") -> torch.Tensor:
    """wasserstein_generator_loss(a) + wasserstein_generator_loss(b) as one node (each term reduced on its own, the two
    added in fp32: mnist_moco_ode_wgan.py:174)."""
    _wgan_check(fgz_a, fgz_b)
    return _LossFn.apply([_wgan(-1.0, reduction, fgz_a.numel(), (0, 0)), _wgan(-1.0, reduction, fgz_b.numel(), (1, 0))],
                         False, fgz_a, fgz_b)


def wasserstein_discriminator_loss(fx: torch.Tensor, fgz: torch.Tensor, reduction: str = "mean") -> torch.Tensor:
    """torchgan's wasserstein_discriminator_loss: reduce(fgz - fx), the difference taken per element."""
    _wgan_check(fx, fgz)
    if fx.shape != fgz.shape:
        raise RuntimeError(f"wasserstein_discriminator_loss: fx {tuple(fx.shape)} and fgz {tuple(fgz.shape)} differ in shape")
    return _LossFn.apply([_wgan(1.0, reduction, fgz.numel(), (1, 0), real=(0, 0))], False, fx, fgz)


def wasserstein_discriminator_loss_halves(joint: torch.Tensor, reduction: str = "mean") -> torch.Tensor:
    """wasserstein_discriminator_loss(x[:B], x[B:]) on the joint [real; fake] output of forward_pair_joint."""
    _wgan_check(joint)
    if joint.shape[0] % 2:
        raise RuntimeError("wasserstein_discriminator_loss_halves: a tensor with an even leading dimension is expected")
    n = joint.numel() // 2
    return _LossFn.apply([_wgan(1.0, reduction, n, (0, n), real=(0, 0))], False, joint)


def _wgan_args(reduction, override_train_ops, clip=None):
    if reduction == "none":
        raise ValueError("reduction='none' is not supported: the loss kernel reduces on the device (use 'mean' or 'sum')")
    if reduction not in _REDUCTIONS:
        raise ValueError(f"reduction must be 'mean' or 'sum', got {reduction!r}")
    if override_train_ops is not None:
        raise ValueError("override_train_ops is not supported: train with GanTrainer(loss='wasserstein') or a loop of "
                         "your own")
    if clip is not None:
        raise ValueError("weight clipping (clip=...) is not supported; the reference trains without it")


class WassersteinGeneratorLoss(torch.nn.Module):
    """torchgan.losses.WassersteinGeneratorLoss drop-in (constructor and forward signatures): -reduce(fgz)."""

    def __init__(self, reduction="mean", override_train_ops=None):
        super().__init__()
        _wgan_args(reduction, override_train_ops)
        self.reduction = reduction
        self.override_train_ops = None

    def forward(self, fgz):
        return wasserstein_generator_loss(fgz, self.reduction)


class WassersteinDiscriminatorLoss(torch.nn.Module):
    """torchgan.losses.WassersteinDiscriminatorLoss drop-in (constructor and forward signatures): reduce(fgz - fx)."""

    def __init__(self, reduction="mean", clip=None, override_train_ops=None):
        super().__init__()
        _wgan_args(reduction, override_train_ops, clip)
        self.reduction = reduction
        self.clip = None
        self.override_train_ops = None

    def forward(self, fx, fgz):
        return wasserstein_discriminator_loss(fx, fgz, self.reduction)


# ------------------------------------------------------------------------------------------------------------------
# optimiser
# ------------------------------------------------------------------------------------------------------------------
class FusedAdam(torch.optim.Optimizer):
    """torch.optim.Adam(lr, betas, eps, weight_decay) semantics (L2-coupled decay, parameters whose .grad is None
    are skipped -- the generator's dead GRU cell, models/mocogan.py:198) on libgode's Adam kernel.  state_dict()
    uses torch.optim.Adam's keys (step / exp_avg / exp_avg_sq) so checkpoints interchange."""

    def __init__(self, params, lr=2e-4, betas=(0.5, 0.999), eps=1e-8, weight_decay=1e-5, noise_sigma=0.0, noise_seed=None,
                 noise_stream=0):
        # the extra keys are torch.optim.Adam's remaining hyper-parameters at their defaults, carried so that a
        # state_dict saved here loads into torch.optim.Adam and vice versa (mnist_moco_ode.py:92-103,175-190)
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=False,
                                      maximize=False, foreach=None, capturable=False, differentiable=False,
                                      fused=None, decoupled_weight_decay=False))
        self._tables, self._keep = {}, {}         # per param group: its PointerTable, the gradients its last launch reads
        # noise_sigma > 0: add_noise of mnist_moco_ode_noise.py / _wgan.py (p += randn_like(p) * sigma on EVERY parameter,
        # gradient or not, right after the update) fused into the Adam launch.  The normals come from libgode's
        # counter-based stream (gode.h: Philox4x32-10 keyed by noise_seed, counter (element quad, noise step,
        # noise_stream)), not torch's generator.  The noise step counter and the stream parameters
        # live in each param group, so state_dict() / load_state_dict() resume the same stream.
        sigma = float(noise_sigma)
        if not (sigma >= 0.0 and sigma != float("inf")):
            raise ValueError(f"noise_sigma must be a finite number >= 0, got {noise_sigma!r}")
        if noise_seed is not None and (isinstance(noise_seed, bool) or not isinstance(noise_seed, int)):
            raise TypeError(f"noise_seed must be an int or None, got {type(noise_seed).__name__}")
        if isinstance(noise_stream, bool) or not isinstance(noise_stream, int) or not 0 <= noise_stream < 1 << 32:
            raise ValueError(f"noise_stream must be an int in [0, 2**32), got {noise_stream!r}")
        self._noise_defaults = None
        if sigma > 0.0:
            seed = torch.initial_seed() if noise_seed is None else noise_seed
            self._noise_defaults = dict(noise_sigma=sigma, noise_seed=int(seed) & 0xFFFFFFFFFFFFFFFF,
                                        noise_stream=int(noise_stream), noise_step=0)
            self._fill_noise_keys()

    def _fill_noise_keys(self):
        for group in self.param_groups:
            for k, v in self._noise_defaults.items():
                group.setdefault(k, v)

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        if self._noise_defaults is not None:      # a state saved without noise (stock torch.optim.Adam): stream from step 0
            self._fill_noise_keys()

    @staticmethod
    def noise_offsets(params):
        """noise_off of every tensor of a param group (gode.h): the running sum of roundup4(numel) in group order."""
        offs, off = [], 0
        for p in params:
            offs.append(off)
            off += (p.numel() + 3) // 4 * 4
        return offs

    @staticmethod
    def step_coefficients(lr, beta1, beta2, step):
        """(lr / (1 - beta1^step), sqrt(1 - beta2^step)) in gode_adam_multi's arithmetic: the hyper-parameters pass
        through C floats, the bias corrections are evaluated in double and rounded to float."""
        import numpy as np
        lr, b1, b2 = float(np.float32(lr)), float(np.float32(beta1)), float(np.float32(beta2))
        return (float(np.float32(lr / (1.0 - b1 ** float(step)))), float(np.float32((1.0 - b2 ** float(step)) ** 0.5)))

    @torch.no_grad()
    def step(self, closure=None, grads: Optional[dict] = None, gscale: float = 1.0, feed=None):
        """grads: optional {param: tensor} overriding .grad (views into an all-reduced bucket); gscale multiplies
        every gradient (1/world_size for data parallelism).  All tensors of a param group are updated by ONE launch
        (gode_adam_multi, with noise gode_adam_noise_multi) driven by a small device table of pointers, uploaded only
        when a pointer changed.
        feed: a HostFeed (graph capture): the step-dependent coefficients are then read from the feed's device block
        (the _dev entry points), so the recorded launch stays valid while the step count advances."""
        assert closure is None
        for gi, group in enumerate(self.param_groups):
            self._group_step(gi, group, grads, gscale, feed)
        return None

    def _group_step(self, gi, group, grads, gscale, feed):
        """One step of a param group.  Plain: a parameter without a gradient is skipped.  With noise every parameter gets
        its noise exactly once -- those with a gradient as Adam + noise rows, those without (the generator's dead GRU
        cell) as noise-only rows of the same launch, those on a different Adam step count through gode_adam_l2 +
        gode_param_noise."""
        lib = L.lib()
        b1, b2 = group["betas"]
        params = group["params"]
        noisy = group.get("noise_sigma", 0.0) > 0.0
        offs = [None] * len(params)
        if noisy:
            group["noise_step"] += 1
            nstep, seed, nstream, sigma = group["noise_step"], group["noise_seed"], group["noise_stream"], group["noise_sigma"]
            before = [p for g in self.param_groups[:gi] for p in g["params"]]      # the stream runs on through the groups
            offs = self.noise_offsets(before + params)[len(before):]
        rows, keep, step, max_n, dev = [], [], None, 0, None
        for p, off in zip(params, offs):
            g = grads.get(p) if grads is not None else p.grad
            if g is None and not noisy:
                continue
            if not p.is_cuda:
                raise RuntimeError("FusedAdam runs only on the GPU through libgode.so")
            row = None
            if g is None:
                row = (p.data_ptr(), 0, 0, 0, p.numel())         # noise-only row
            else:
                if not g.is_contiguous():
                    g = g.contiguous()
                st = self.state[p]
                if not st:
                    st["step"] = torch.tensor(0.0)
                    st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                st["step"] += 1
                s_now = int(st["step"].item())
                if step is None:
                    step = s_now
                if s_now != step:       # parameters on different step counts: fall back to one launch each
                    if feed is not None:
                        raise RuntimeError("graph capture needs all parameters of a group on the same Adam step")
                    L.run_one(L.AdamOp(p=p.data_ptr(), g=g.data_ptr(), m=st["exp_avg"].data_ptr(),
                                       v=st["exp_avg_sq"].data_ptr(), n=p.numel(), lr=group["lr"], beta1=b1, beta2=b2,
                                       eps=group["eps"], weight_decay=group["weight_decay"], gscale=gscale,
                                       step=s_now), stream_ptr())
                    if noisy:
                        L.call("param_noise", lambda: L.check(
                            lib.gode_param_noise(p.data_ptr(), p.numel(), seed, nstream, nstep, off, sigma, 1, stream_ptr()),
                            "gode_param_noise"))
                else:
                    row = (p.data_ptr(), g.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(), p.numel())
                keep.append(g)
            if row is not None:
                rows.append(row + (off,) if noisy else row)
                max_n = max(max_n, p.numel())
            bump_version(p)
            dev = p.device
        self._keep[gi] = keep            # (the launch reads the .contiguous() copies among them)
        if not rows:
            return
        # (the pointers of parameters, arena gradients and moments do not change from step to step: the table is uploaded
        # once, not per step)
        tbl = self._tables.get(gi)
        if tbl is None:
            tbl = self._tables[gi] = PointerTable(dev)
        if feed is not None and not tbl.matches(rows):
            raise RuntimeError("graph capture: the Adam pointer table must exist already (run eager iterations first)")
        table, n = tbl.upload(rows).data_ptr(), len(rows)
        if step is None:
            step = max(1, self.current_step(gi))                 # (noise-only launch: coefficients unused)
        tag = "adam_noise_multi" if noisy else "adam_multi"
        args = (b1, b2, group["eps"], group["weight_decay"], gscale)
        if feed is not None:         # the coefficients (and the noise step) come from the feed's device block
            coef = feed.adam_slot(self, gi, group["lr"], b1, b2, step, noise_step=nstep if noisy else None)
            name, args = f"gode_{tag}_dev", args + (coef,) + ((seed, nstream, sigma) if noisy else ())
        else:
            name, args = f"gode_{tag}", (group["lr"],) + args + (step,) + ((seed, nstream, nstep, sigma) if noisy else ())
        L.call(tag, lambda: L.check(getattr(lib, name)(table, n, max_n, *args, stream_ptr()), name))

    def pointer_table(self, group_index=0):
        """The PointerTable of a param group's launch (None before the group's first launch)."""
        return self._tables.get(group_index)

    def advance_steps(self, group_index=0):
        """Host-side bookkeeping of one optimiser step that a replayed graph performed on the device: the `step`
        entries of the state (checkpoints, the next coefficient upload) move on by one, and so does the noise step."""
        for p in self.param_groups[group_index]["params"]:
            st = self.state.get(p)
            if st:
                st["step"] += 1
        group = self.param_groups[group_index]
        if group.get("noise_sigma", 0.0) > 0.0:
            group["noise_step"] += 1

    def current_step(self, group_index=0):
        for p in self.param_groups[group_index]["params"]:
            st = self.state.get(p)
            if st:
                return int(st["step"].item())
        return 0


class HostFeed:
    """Everything the host contributes to one training iteration besides the launch itself -- the latent noise drawn
    from the NumPy / torch CPU generators (the reference's RNG contract) and Adam's step-dependent coefficients -- laid
    out in ONE pinned block that is uploaded with ONE copy into a static device block read by the captured graph.
    During capture the block's layout is recorded as a script (in program order); before every replay the script is
    walked again: same draws in the same order, coefficients for the new step counts."""

    FLOATS = 1 << 18

    def __init__(self, device):
        self.device = device
        self.dev = torch.zeros(self.FLOATS, dtype=torch.float32, device=device)
        self.pinned = [torch.zeros(self.FLOATS, dtype=torch.float32).pin_memory() for _ in range(2)]
        self.events = [None, None]
        self.parity = 0
        self.script, self.size = [], 0
        self.recording = False

    # -- capture ---------------------------------------------------------------------------------------------------
    def _reserve(self, n):
        off = self.size
        self.size = off + ((n + 3) // 4) * 4                 # 16-byte aligned regions
        if self.size > self.FLOATS:
            raise RuntimeError("HostFeed block too small")
        return off

    def noise_region(self, gen, select, num_samples, T, nfloats):
        """-> (pinned view to fill now, device view the captured copy reads)"""
        assert self.recording
        off = self._reserve(nfloats)
        self.script.append(("noise", gen, select, num_samples, T, off, nfloats))
        return self.pinned[self.parity][off:off + nfloats], self.dev[off:off + nfloats]

    def adam_slot(self, opt, group_index, lr, b1, b2, step, noise_step=None):
        """Adam's two step coefficients; with noise_step, the parameter-noise step counter follows as a raw 32-bit word."""
        assert self.recording
        off = self._reserve(2 if noise_step is None else 3)
        self.script.append(("adam", opt, group_index, lr, b1, b2, off, noise_step is not None))
        c = FusedAdam.step_coefficients(lr, b1, b2, step)
        self.pinned[self.parity][off], self.pinned[self.parity][off + 1] = c[0], c[1]
        if noise_step is not None:
            self.pinned[self.parity][off:off + 4].view(torch.int32)[2] = int(noise_step)
        return self.dev[off:off + 2].data_ptr()

    def dnoise_slot(self, model, call, ncalls):
        """A discriminator's instance-noise call index (raw 32 bits) for one captured forward; every replay writes the
        module's current counter and advances it by the forward's `ncalls`, as an eager forward does."""
        assert self.recording
        off = self._reserve(1)
        self.script.append(("dnoise", model, off, ncalls))
        self.pinned[self.parity][off:off + 4].view(torch.int32)[0] = int(call) - (1 << 32) if call >= 1 << 31 else int(call)
        return self.dev[off:off + 1].data_ptr()

    def latent_slot(self, gen, call, ncalls):
        """A device-mode generator's latent call index (raw 32 bits) for one captured sampling call, read by its
        gode_latent_draw op; every replay writes the generator's current counter and advances it by `ncalls`, as an eager
        call does.  Such a call has no "noise" entry: nothing of it is drawn on the host."""
        assert self.recording
        off = self._reserve(1)
        self.script.append(("latent", gen, off, ncalls))
        call = int(call) & 0xFFFFFFFF
        self.pinned[self.parity][off:off + 4].view(torch.int32)[0] = call - (1 << 32) if call >= 1 << 31 else call
        return self.dev[off:off + 1].data_ptr()

    # -- replay ----------------------------------------------------------------------------------------------------
    def begin(self):
        """Next pinned buffer (waits until the upload that last used it has been consumed)."""
        self.parity ^= 1
        ev = self.events[self.parity]
        if ev is not None:
            ev.synchronize()
        return self.pinned[self.parity]

    def fill_from_script(self):
        buf = self.begin()
        for ent in self.script:
            if ent[0] == "noise":
                _, gen, select, num_samples, T, off, nfloats = ent
                gen._fill_host_inputs(buf[off:off + nfloats], select, num_samples, T)
            elif ent[0] == "latent":
                _, gen, off, ncalls = ent
                call = gen.latent_call
                buf[off:off + 4].view(torch.int32)[0] = call - (1 << 32) if call >= 1 << 31 else call
                gen.latent_call = call + ncalls
            elif ent[0] == "dnoise":
                _, model, off, ncalls = ent
                call = model._noise_call
                buf[off:off + 4].view(torch.int32)[0] = call - (1 << 32) if call >= 1 << 31 else call
                model._noise_call = (call + ncalls) & 0xFFFFFFFF
            else:
                _, opt, gi, lr, b1, b2, off, noisy = ent
                opt.advance_steps(gi)
                c = FusedAdam.step_coefficients(lr, b1, b2, opt.current_step(gi))
                buf[off], buf[off + 1] = c[0], c[1]
                if noisy:
                    buf[off:off + 4].view(torch.int32)[2] = int(opt.param_groups[gi]["noise_step"])

    def upload(self):
        """One H2D copy of the used part of the block on the current stream (ordered before the replay that reads it,
        after the replay that read the previous contents)."""
        n = self.size
        self.dev[:n].copy_(self.pinned[self.parity][:n], non_blocking=True)
        if self.events[self.parity] is None:
            self.events[self.parity] = torch.cuda.Event()
        self.events[self.parity].record()


# ------------------------------------------------------------------------------------------------------------------
# data parallel gradient bucket
# ------------------------------------------------------------------------------------------------------------------
class GradBucket:
    """Flat fp32 bucket over the parameters of ONE network that received a gradient.  gather() packs the grads,
    all_reduce() sums them over the process group (one collective per optimiser step; RCCL over xGMI on the GPU box,
    gloo in the CPU tests), views() hands the reduced slices to the optimiser without copying back."""

    def __init__(self, params: Sequence[torch.nn.Parameter]):
        self.params = [p for p in params]
        self.flat = None
        self.live = []

    def gather(self):
        self.live = [p for p in self.params if p.grad is not None]
        if not self.live:
            return None
        n = sum(p.numel() for p in self.live)
        if self.flat is None or self.flat.numel() != n or self.flat.device != self.live[0].device:
            self.flat = torch.empty(n, dtype=torch.float32, device=self.live[0].device)
        off = 0
        for p in self.live:
            k = p.numel()
            self.flat[off:off + k].copy_(p.grad.reshape(-1))
            off += k
        return self.flat

    def all_reduce(self, group=None):
        if self.flat is not None and dist.is_initialized() and dist.get_world_size(group) > 1:
            dist.all_reduce(self.flat, op=dist.ReduceOp.SUM, group=group)

    def views(self):
        out, off = {}, 0
        for p in self.live:
            k = p.numel()
            out[p] = self.flat[off:off + k].view_as(p)
            off += k
        return out


class GradArena:
    """One flat fp32 gradient buffer per network, written by the backward kernels themselves: the first weight-gradient
    / BatchNorm-gradient / adjoint kernel that produces a parameter's gradient in a step stores it (and `p.grad`
    becomes a view of the arena), later ones (the second discriminator pass, the image path of the generator) add in
    place.  Replaces autograd's AccumulateGrad adds (64 small launches per iteration) and, under data parallelism,
    the pack-into-bucket copies: the arena IS the all-reduce bucket.  `order`: parameters in arena order (the
    generator puts its pre-net + ODEFunc tensors last, in the adjoint kernel's output order)."""

    def __init__(self, order: Sequence[torch.nn.Parameter]):
        self.params = list(order)
        dev = self.params[0].device
        n = sum(p.numel() for p in self.params)
        self.flat = torch.zeros(n, dtype=torch.float32, device=dev)
        self.views, off = {}, 0
        for p in self.params:
            self.views[p] = self.flat[off:off + p.numel()].view_as(p)
            off += p.numel()
        self.written = set()
        self.active = False

    def begin(self):
        """Start of an optimiser step (replaces zero_grad): every .grad is dropped, nothing is written yet."""
        for p in self.params:
            p.grad = None
        self.written.clear()
        self.active = True

    def end(self):
        self.active = False

    def target(self, p):
        """-> (tensor the kernel writes to, accumulate?) and binds p.grad to it on first use."""
        v = self.views[p]
        acc = p in self.written
        if not acc:
            self.written.add(p)
            p.grad = v
        return v, acc


# ------------------------------------------------------------------------------------------------------------------
# the iteration
# ------------------------------------------------------------------------------------------------------------------
def build_mnist(ngf=64, ndf=64, use_noise=False, noise_sigma=None):
    """The three networks of mnist_moco_ode.py:75-78 (use_noise / noise_sigma: the discriminators' instance noise)."""
    return VideoGeneratorMNISTODE(1, 50, 0, 16, 16, ngf=ngf), \
        VideoDiscriminator(1, ksize=2, ndf=ndf, use_noise=use_noise, noise_sigma=noise_sigma), \
        PatchImageDiscriminator(1, ndf=ndf, use_noise=use_noise, noise_sigma=noise_sigma)


def build_ucf(ngf=64, ndf=64, use_noise=False, noise_sigma=None):
    """ucf_moco_ode.py:77-80 with dim_hidden=16 (the shipped call omits it and raises)."""
    return VideoGenerator(3, 50, 0, 16, 16, dim_hidden=16, ngf=ngf), \
        VideoDiscriminator(3, ndf=ndf, use_noise=use_noise, noise_sigma=noise_sigma), \
        PatchImageDiscriminator(3, ndf=ndf, use_noise=use_noise, noise_sigma=noise_sigma)


def _shards(x):
    return list(x) if isinstance(x, (list, tuple)) else [x]


class GanTrainer:
    """Owns the three networks and their optimisers; step() is one outer iteration of the reference loop.

    Data parallelism: with an initialised process group every rank runs the whole iteration on its own
    shard with per-replica BatchNorm statistics and ONE all-reduce (sum) of each network's flat gradient arena per
    optimiser step; 1/world is folded into the Adam kernel.  Construction broadcasts rank 0's parameters and buffers so
    that replicas start (and, with identical updates, stay) equal.  The same semantics are available on ONE GPU as
    *virtual replicas*: pass a list of shard tensors instead of a tensor and every optimiser step accumulates the
    shards' gradients in the arena (each shard its own forward/backward, own BatchNorm statistics) and applies
    1/(world * shards) -- which is how BASELINE configs[2] (batch 256 = 8 x 32) is parity-tested on one device."""

    def __init__(self, gen, dis_vid, dis_img, lr=2e-4, betas=(0.5, 0.999), weight_decay=1e-5, d_iters=2,
                 process_group=None, freeze_d_in_g_step=True, freeze_gc=False, direct_grads=True, sync_replicas=True,
                 overlap_image_d=True, graph=False, pair_d_passes=True, prefetch_latents=True, overlap_allreduce=True,
                 joint_generator_passes=True, loss="bce", param_noise=0.0, noise_seed=None, diffaug=None,
                 diffaug_seed=None):
        self.gen, self.dis_vid, self.dis_img = gen, dis_vid, dis_img
        # loss: "bce" (mnist_moco_ode.py) or "wasserstein" (torchgan's losses, mnist_moco_ode_wgan.py: D minimises
        # mean(D(fake) - D(real)), G minimises -mean(D(fake)); no clipping, no gradient penalty)
        if loss not in ("bce", "wasserstein"):
            raise ValueError(f"GanTrainer(loss=...) must be 'bce' or 'wasserstein', got {loss!r}")
        self.loss = loss
        self.world = dist.get_world_size(process_group) if dist.is_initialized() else 1
        self.rank = dist.get_rank(process_group) if dist.is_initialized() else 0
        # categorical MoCoGAN: a generator with dim_z_category = C > 0 trains against a CategoricalVideoDiscriminator with
        # dim_categorical = C and one real/fake logit; the video-D and the G step gain a class term (see step())
        self.ncat = int(getattr(gen, "dim_z_category", 0) or 0)
        dcat = int(getattr(dis_vid, "dim_categorical", 0) or 0)
        if self.ncat != dcat:
            raise ValueError(f"GanTrainer: the generator has dim_z_category={self.ncat} but the video discriminator has "
                             f"dim_categorical={dcat}; they must match (0: unconditional)")
        if self.ncat:
            if getattr(dis_vid, "n_output_neurons", 1 + dcat) != 1 + dcat:
                raise ValueError("GanTrainer: the categorical video discriminator must have one real/fake logit "
                                 "(n_output_neurons=1)")
            if loss != "bce":
                raise NotImplementedError("GanTrainer: categorical training is implemented for loss='bce'")
            if graph:
                raise NotImplementedError("GanTrainer(graph=True) does not capture categorical training")
            if self.world > 1:
                raise NotImplementedError("GanTrainer: categorical training is single-process (no data parallelism)")
        # latents drawn on the device (gen.latent_rng == "device"): every rank takes its own stream of the generator's seed
        # (the ranks construct the generator under one torch seed), so the replicas' samples are disjoint
        if self.world > 1 and getattr(gen, "latent_rng", "host") == "device":
            gen.latent_stream = self.rank
        # discriminator instance noise (VideoDiscriminator / PatchImageDiscriminator(use_noise=True)): noise_seed, when given,
        # keys both discriminators' streams (default: each module's torch.initial_seed() at construction).  Replicas take
        # rank 0's seeds; each replica and virtual-replica shard draws the noise of its own samples (_noise_shard).
        dnoise = [m for m in (dis_vid, dis_img) if getattr(m, "use_noise", False)]
        if noise_seed is not None:
            for m in dnoise:
                m.noise_seed = int(noise_seed) & 0xFFFFFFFFFFFFFFFF
        if dnoise and self.world > 1 and sync_replicas:
            dev = next(gen.parameters()).device
            t = torch.tensor([[m.noise_seed & 0xFFFFFFFF, m.noise_seed >> 32] for m in dnoise], dtype=torch.int64, device=dev)
            dist.broadcast(t, src=0, group=process_group)
            for m, (lo, hi) in zip(dnoise, t.tolist()):
                m.noise_seed = int(lo) | (int(hi) << 32)
        # diffaug: a DiffAugment policy ('color,translation,cutout', any subset) for both discriminators -- every real and
        # every fake batch passes the same random transform in front of them, and the G step back-propagates through it
        # (DESIGN section 28).  diffaug_seed, when given, keys both streams (default: each module's torch.initial_seed() at
        # construction); replicas take rank 0's seeds, and each replica and virtual-replica shard draws the parameters of its
        # own samples (_noise_shard).  None leaves the discriminators as they are.
        from .modules import diffaug_mask
        if diffaug_mask(diffaug) or diffaug_seed is not None:   # (an unknown name is refused here, not in the first step)
            for m in (dis_vid, dis_img):
                m.diffaug = diffaug or m.diffaug
                if diffaug_seed is not None:
                    m.diffaug_seed = int(diffaug_seed) & 0xFFFFFFFFFFFFFFFF
        aug = [m for m in (dis_vid, dis_img) if diffaug_mask(getattr(m, "diffaug", None))]
        if aug and graph:
            raise NotImplementedError("GanTrainer(graph=True) does not capture a DiffAugment policy: use the eager "
                                      "schedule (graph=False)")
        if aug and self.world > 1 and sync_replicas:
            dev = next(gen.parameters()).device
            t = torch.tensor([[m.diffaug_seed & 0xFFFFFFFF, m.diffaug_seed >> 32] for m in aug], dtype=torch.int64, device=dev)
            dist.broadcast(t, src=0, group=process_group)
            for m, (lo, hi) in zip(aug, t.tolist()):
                m.diffaug_seed = int(lo) | (int(hi) << 32)
        # param_noise > 0: add_noise(model.parameters(), param_noise) after every optimiser step (mnist_moco_ode_noise.py
        # sigma 1e-5, mnist_moco_ode_wgan.py 1e-4), fused into the Adam launch; streams gen 0, dis_vid 1, dis_img 2 of
        # noise_seed (default torch.initial_seed(): nothing is drawn from the CPU generator, whose stream feeds the latent
        # noise in the reference's order).  Replicas take rank 0's seed.
        noise = float(param_noise)
        if noise > 0.0:
            if noise_seed is None:
                noise_seed = torch.initial_seed()
            if self.world > 1 and sync_replicas:
                dev = next(gen.parameters()).device
                t = torch.tensor([noise_seed & 0xFFFFFFFF, (noise_seed >> 32) & 0xFFFFFFFF], dtype=torch.int64, device=dev)
                dist.broadcast(t, src=0, group=process_group)
                noise_seed = int(t[0]) | (int(t[1]) << 32)
        self.param_noise, self.noise_seed = noise, (noise_seed if noise > 0.0 else None)
        mk = lambda m, k: FusedAdam(m.parameters(), lr=lr, betas=betas, weight_decay=weight_decay,  # noqa: E731
                                    noise_sigma=noise, noise_seed=self.noise_seed, noise_stream=k)
        self.gen_opt, self.vid_opt, self.img_opt = mk(gen, 0), mk(dis_vid, 1), mk(dis_img, 2)
        self.d_iters, self.group = d_iters, process_group
        self.freeze_d = freeze_d_in_g_step
        if self.world > 1 and sync_replicas:
            self.broadcast_state()
        self.buckets = {id(m): GradBucket(list(m.parameters())) for m in (gen, dis_vid, dis_img)}
        # overlap_image_d: inside step() the image discriminator's forward/backward/Adam (some 50 latency-bound
        # launches of 5-30 us each at batch 32) run on a side stream next to the video-discriminator step's big GEMMs.
        # Everything that touches the generator stays on the caller's stream in program order (its BatchNorm running
        # statistics are updated by every sample_* call), each stream executes the same kernels in the same order as
        # the serial schedule, so results are bit-identical to overlap_image_d=False.
        # pair_d_passes: in the discriminator steps D(real) and D(fake) run as ONE pass over [real; fake] with per-group
        # BatchNorm statistics (forward_pair_joint): same arithmetic per element, half the launches, fuller GEMM grids.
        self.pair_d = bool(pair_d_passes)
        # prefetch_latents: step() announces the iteration's sample_images / sample_videos calls to the generator up front
        # (VideoGenerator.prefetch_latents): the host draws are made in the same order, all latent solves go out at once on
        # a side stream.  Bit-identical results; what it buys is the ODE-RNN generator's six one-workgroup solves per
        # iteration running side by side in one launch, and the two adjoints of the G step likewise (flush_adjoints).
        self.prefetch = bool(prefetch_latents)
        # joint_generator_passes: the two generator calls between two generator updates (sample_images + sample_videos of
        # an inner discriminator pass; sample_videos + sample_images of the G step) are decoded in one pass over both
        # batches with per-call BatchNorm statistics (VideoGenerator.sample_pair)
        self.joint_g = bool(joint_generator_passes)
        self._paired_fake_vid = None
        # overlap_allreduce (world > 1): every all-reduce is issued asynchronously (the process group's own stream) and the
        # optimiser step that consumes it is DEFERRED to the point where that network is next needed -- a discriminator's
        # all-reduce then runs under the next no-grad generator forward, and the generator's arena goes out in two parts:
        # the decoder's 13 MB as soon as the last decoder backward kernel is queued (under the latent adjoint), the
        # ODEFunc / GRU tail after the adjoint.  Same kernels in the same per-stream order: bit-identical to the serial form.
        self.overlap_ar = bool(overlap_allreduce)
        self._pending = {}            # id(model) -> (opt, works, gscale, feed)
        self._early = {}              # id(model) -> (work, floats): the part of an arena whose all-reduce is already out
        self.skip_allreduce = False   # measurement only (bench.py): run the schedule without collectives
        self._side = None
        if overlap_image_d and next(dis_img.parameters()).is_cuda:
            self._side = torch.cuda.Stream(device=next(dis_img.parameters()).device)
        self._side_pending = False
        # graph: after two eager iterations (every plan, program and pointer table exists, the pack pattern is the
        # steady-state one) step() captures ONE whole iteration -- both streams, autograd's backward passes, the five
        # Adam launches -- in a HIP graph and from then on replays it: per iteration the host draws the latent noise
        # (same generators, same order: HostFeed), uploads it with one copy and launches the graph.  Measured at
        # BASELINE configs[1] the eager iteration is within ~25 % of being host-bound (scripts/host_floor.py: 7.5-8.2 ms
        # of Python + launch calls per iteration against ~11 ms of kernels); the replay needs ~2 ms of host time.
        # Single-process only (a captured RCCL all-reduce is not attempted); arena gradients required.
        self._graph_mode = bool(graph)
        self._graph = None
        self._feed = None
        if self._graph_mode and self.world > 1:
            raise NotImplementedError("GanTrainer(graph=True) is single-process; data-parallel runs use the eager schedule")
        if self._graph_mode and not getattr(gen, "_gode_graph_capture", True):
            raise NotImplementedError(f"GanTrainer(graph=True) does not capture {type(gen).__name__}: use the eager "
                                      "schedule (graph=False)")
        # freeze_gc: call freeze_host_gc() after the second iteration (process-global, hence opt-in; bench.py and
        # long training loops want it, see its docstring)
        self._iters, self._freeze_gc = 0, freeze_gc
        # direct_grads: backward kernels write into a per-network GradArena (see its docstring); CPU tensors (the gloo
        # tests) and direct_grads=False keep the stock autograd accumulation + GradBucket
        self.arenas = {}
        if direct_grads:
            for m in (gen, dis_vid, dis_img):
                ps = list(m.parameters())
                if ps and ps[0].is_cuda and getattr(m, "_gode_direct_grads", False):
                    tail = m._arena_tail() if hasattr(m, "_arena_tail") else []
                    ids = {id(p) for p in tail}
                    arena = GradArena([p for p in ps if id(p) not in ids] + tail)
                    self.arenas[id(m)] = arena
                    m._gode_arena = arena

    def broadcast_state(self, src=0):
        """Every replica takes rank `src`'s parameters and buffers (BatchNorm running statistics included)."""
        for m in (self.gen, self.dis_vid, self.dis_img):
            with torch.no_grad():
                for t in list(m.parameters()) + list(m.buffers()):
                    dist.broadcast(t.detach(), src=src, group=self.group)
            if hasattr(m, "invalidate_packs"):
                m.invalidate_packs()

    # -- collectives ---------------------------------------------------------------------------------------------------
    def _all_reduce(self, flat, async_op):
        """One sum over the replicas of a flat fp32 gradient buffer (RCCL over xGMI; gloo in the rehearsals)."""
        if self.skip_allreduce:
            return None
        return dist.all_reduce(flat, op=dist.ReduceOp.SUM, group=self.group, async_op=async_op)

    def _flush(self, model):
        """The deferred optimiser step of `model`, if one is pending: wait for its all-reduce(s), then Adam."""
        ent = self._pending.pop(id(model), None)
        if ent is None:
            return
        opt, works, gscale, feed = ent
        for w in works:
            if w is not None:
                w.wait()              # (the current stream waits; the host does not block with RCCL)
        opt.step(gscale=gscale, feed=feed)

    def _early_decoder_allreduce(self):
        a = self.arenas[id(self.gen)]
        tail = sum(p.numel() for p in (self.gen._arena_tail() if hasattr(self.gen, "_arena_tail") else []))
        head = a.flat.numel() - tail
        self._early[id(self.gen)] = (self._all_reduce(a.flat[:head], True), head)

    def flush_all(self):
        for m in (self.dis_img, self.dis_vid, self.gen):
            self._flush(m)

    def time_collectives(self, reps=10):
        """Milliseconds of each of the iteration's all-reduces on its own (same buffers, nothing else running): what the
        fabric charges for them; compare with the iteration time of a run with skip_allreduce to see what is exposed."""
        out = {}
        if self.world <= 1:
            return out
        for name, m in (("dis_img", self.dis_img), ("dis_vid", self.dis_vid), ("gen", self.gen)):
            a = self.arenas.get(id(m))
            if a is None:
                continue
            buf = torch.zeros_like(a.flat)
            for _ in range(2):
                dist.all_reduce(buf, group=self.group)
            torch.cuda.synchronize()
            dist.barrier(group=self.group)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                dist.all_reduce(buf, group=self.group)
            e1.record()
            torch.cuda.synchronize()
            out[name] = e0.elapsed_time(e1) / reps
        return out

    def _begin(self, model, opt):
        self._flush(model)            # the previous step's deferred update reads this arena
        a = self.arenas.get(id(model))
        if a is not None:
            # (re)bind: the autograd nodes look the arena up on the module, and a second trainer built on the same
            # networks (bench.py's graph-mode twin) would otherwise leave this trainer reducing an arena nobody writes
            model._gode_arena = a
            a.begin()
        else:
            opt.zero_grad()

    def _opt_step(self, model, opt, nshards=1):
        a = self.arenas.get(id(model))
        gscale = 1.0 / (self.world * nshards)
        if a is not None:
            if getattr(model, "_gode_arena", None) is not a:
                raise RuntimeError("another GanTrainer re-bound this network's gradient arena in the middle of an optimiser "
                                   "step: the backward kernels wrote into its arena, not this one")
            a.end()
            feed = getattr(opt, "_feed", None)
            feed = feed if (feed is not None and feed.recording) else None
            if self.world > 1 and self.overlap_ar and feed is None:
                # the arena is the bucket: no packing copies.  Parts that went out early (the generator's decoder block,
                # see g_step) are skipped here; the optimiser step waits in _flush, where the network is next needed
                early = self._early.pop(id(model), None)
                if early is None:
                    works = [self._all_reduce(a.flat, True)]
                else:
                    works = [early[0], self._all_reduce(a.flat[early[1]:], True)]
                self._pending[id(model)] = (opt, works, gscale, None)
                return
            if self.world > 1:       # serial form: one collective, then the update
                self._all_reduce(a.flat, False)
            opt.step(gscale=gscale, feed=feed)
            return
        if self.world > 1:
            b = self.buckets[id(model)]
            b.gather()
            b.all_reduce(self.group)
            opt.step(grads=b.views(), gscale=gscale)
        else:
            opt.step(gscale=gscale)

    def _d_loss(self, pr, pf):
        if self.loss == "wasserstein":
            return wasserstein_discriminator_loss(pr, pf)
        return bce_with_logits_pair(pr, 1.0, pf, 0.0)

    def _d_loss_joint(self, joint):
        """the discriminator loss on the [real; fake] output of forward_pair_joint"""
        if self.loss == "wasserstein":
            return wasserstein_discriminator_loss_halves(joint)
        return bce_with_logits_halves(joint, 1.0, 0.0)

    @staticmethod
    def _mean(losses):
        if len(losses) == 1:
            return losses[0]
        return torch.stack(losses).mean()

    def _noise_shard(self, model, k, B, nsh, call0):
        """Instance noise of shard k of nsh (batch B each): the shards of one step share the call index call0 and draw the
        noise of their own samples -- the offset is the shard's first sample in the global batch.  call0: the pair
        (instance-noise call, DiffAugment call) of _calls0; the augmentation's counter and offset follow the same rule."""
        if getattr(model, "use_noise", False):
            model._noise_call = call0[0]
            model._noise_sample_offset = (self.rank * nsh + k) * B
        if getattr(model, "diffaug", None):
            model.diffaug_call = call0[1]
            model._diffaug_sample_offset = (self.rank * nsh + k) * B

    @staticmethod
    def _calls0(model):
        return getattr(model, "_noise_call", 0), getattr(model, "diffaug_call", 0)

    def _gen_one_stream(self):
        """The discriminator steps' no-grad generator calls keep the one-stream path (VideoGenerator.one_stream): each
        follows other launches, so two lanes could hide nothing and would only add their event edges."""
        return getattr(self.gen, "one_stream", contextlib.nullcontext)()

    def d_image_step(self, real_img, _join=True, _defer=False, _pair_videos=0):
        """mnist_moco_ode.py:115-131.  real_img: [B,C,H,W], or a list of such shards (virtual replicas).
        _pair_videos (step() only): the batch size of the d_video_step that follows -- its fake videos are generated here,
        in the same decoder pass as this step's fake images (VideoGenerator.sample_pair), and kept for it."""
        shards = _shards(real_img)
        side = self._side
        main = torch.cuda.current_stream() if side is not None else None
        if side is not None and not self._side_pending:
            side.wait_stream(main)          # inputs prepared on the caller's stream; later passes only wait for `fake`
            self._side_pending = True
        on_side = (lambda: torch.cuda.stream(side)) if side is not None else contextlib.nullcontext
        with on_side():
            self._begin(self.dis_img, self.img_opt)
        losses = []
        call0 = self._calls0(self.dis_img)
        for k, x in enumerate(shards):
            B = x.shape[0]
            self._noise_shard(self.dis_img, k, B, len(shards), call0)
            if not self.pair_d:
                with on_side():
                    pr, _ = self.dis_img(x)
            with torch.no_grad(), self._gen_one_stream():    # generator work stays on the caller's stream
                if _pair_videos:
                    self._paired_fake_vid, (fake, _) = self.gen.sample_pair(_pair_videos, B, images_first=True)
                else:
                    fake, _ = self.gen.sample_images(B)
            if side is not None:
                ev = torch.cuda.Event()
                ev.record(main)
                side.wait_event(ev)
                fake.record_stream(side)
            with on_side():
                if self.pair_d:
                    loss = self._d_loss_joint(self.dis_img.forward_pair_joint(x, fake))
                else:
                    pf, _ = self.dis_img(fake)
                    loss = self._d_loss(pr, pf)
                loss.backward(gradient=unit_grad(loss.device))
            losses.append(loss.detach())
        with on_side():
            self._opt_step(self.dis_img, self.img_opt, len(shards))
            if not _defer:
                self._flush(self.dis_img)      # called on its own: the update has landed when the call returns
            out = self._mean(losses)
        if _join:
            self._join_side()
        return out

    def _join_side(self):
        """The caller's stream waits for the image-discriminator work queued on the side stream."""
        if self._side is not None and self._side_pending:
            torch.cuda.current_stream().wait_stream(self._side)
            self._side_pending = False

    def _labels_for(self, real_labels, B, what):
        """Categorical training: the int64 [B] device labels of a real video batch (None when categories are off)."""
        if not self.ncat:
            if real_labels is not None:
                raise ValueError(f"{what}: real_labels given, but the networks are unconditional (dim_z_category=0)")
            return None
        if real_labels is None:
            raise ValueError(f"{what}: categorical training (dim_z_category={self.ncat}) needs real_labels, the int64 "
                             "class of every real video")
        if not (torch.is_tensor(real_labels) and real_labels.dtype == torch.int64 and real_labels.dim() == 1
                and real_labels.shape[0] == B and real_labels.is_cuda):
            raise ValueError(f"{what}: real_labels must be an int64 device tensor [{B}]")
        return real_labels

    def d_video_step(self, real_vid, _defer=False, real_labels=None):
        """mnist_moco_ode.py:133-150.  real_vid: [B,T,C,H,W], or a list of such shards.  Categorical training:
        real_labels int64 [B]; the loss gains CE(categ(real), real_labels)."""
        shards = _shards(real_vid)
        if self.ncat and len(shards) > 1:
            raise NotImplementedError("categorical training does not take virtual-replica shards")
        labels = self._labels_for(real_labels, shards[0].shape[0], "d_video_step")
        losses = []
        begun = False
        call0 = self._calls0(self.dis_vid)
        for k, x in enumerate(shards):
            B = x.shape[0]
            self._noise_shard(self.dis_vid, k, B, len(shards), call0)
            real = x.transpose(1, 2)                            # [B,T,C,H,W] -> [B,C,T,H,W] view, read in place
            if not self.pair_d and not begun:
                self._begin(self.dis_vid, self.vid_opt)
                begun = True
            if not self.pair_d:
                pr = self.dis_vid.forward_head(real) if self.ncat else self.dis_vid(real)[0]
            with torch.no_grad(), self._gen_one_stream():
                fake, self._paired_fake_vid = self._paired_fake_vid, None
                if fake is not None:                     # generated by the d_image_step before (see _pair_videos)
                    fake = fake[0]
                    assert fake.shape[0] == B
                else:
                    fake, _ = self.gen.sample_videos(B)
            if not begun:
                # (paired pass) the generator forward above does not read this discriminator: its previous step's
                # all-reduce -- deferred, see overlap_allreduce -- has been running under it; now wait, update, begin
                self._begin(self.dis_vid, self.vid_opt)
                begun = True
            if self.ncat:          # BCE(real, 1) + BCE(fake, 0) + CE(categ(real), real_labels): one node
                if self.pair_d:
                    loss = bce_ce_head_halves(self.dis_vid.forward_pair_joint(real, fake), 1.0, 0.0, labels)
                else:
                    loss = bce_ce_heads(pr, 1.0, labels, self.dis_vid.forward_head(fake), 0.0)
            elif self.pair_d:
                loss = self._d_loss_joint(self.dis_vid.forward_pair_joint(real, fake))
            else:
                pf, _ = self.dis_vid(fake)
                loss = self._d_loss(pr, pf)
            loss.backward(gradient=unit_grad(loss.device))
            losses.append(loss.detach())
        self._opt_step(self.dis_vid, self.vid_opt, len(shards))
        if not _defer:
            self._flush(self.dis_vid)
        return self._mean(losses)

    def _can_pair(self, n_videos, n_images, images_first):
        return self.joint_g and hasattr(self.gen, "can_pair") and next(self.gen.parameters()).is_cuda and \
            self.gen.can_pair(n_videos, n_images, images_first)

    def g_step(self, B, shards=1):
        """mnist_moco_ode.py:153-163; `shards` virtual replicas of batch B each.  Categorical training: the loss gains
        CE(categ(D_vid(fake)), the classes the fake videos were generated for)."""
        if self.ncat and shards > 1:
            raise NotImplementedError("categorical training does not take virtual-replica shards")
        vid_head = (lambda v: self.dis_vid.forward_head(v)) if self.ncat else (lambda v: self.dis_vid(v)[0])
        self._begin(self.gen, self.gen_opt)
        frozen = []
        if self.freeze_d:
            # the reference lets this backward also fill the discriminators' .grad, which the next zero_grad()
            # discards unused (mnist_moco_ode.py:116,134,162); skipping those weight-gradient GEMMs changes nothing
            for m in (self.dis_vid, self.dis_img):
                for p in m.parameters():
                    if p.requires_grad:
                        p.requires_grad_(False)
                        frozen.append(p)
        losses = []
        batch_adj = self.prefetch and id(self.gen) in self.arenas and hasattr(self.gen, "flush_adjoints")
        early_ar = self.world > 1 and self.overlap_ar and id(self.gen) in self.arenas
        try:
            joint = shards == 1 and self._can_pair(B, B, False)
            calls0 = [self._calls0(m) for m in (self.dis_vid, self.dis_img)]
            for k in range(shards):
                for m, c0 in zip((self.dis_vid, self.dis_img), calls0):
                    self._noise_shard(m, k, B, shards, c0)
                if joint:          # both calls' rows in one decoder pass (two BatchNorm batches)
                    (fake_vid, classes), (fake_img, _) = self.gen.sample_pair(B, B)
                else:
                    fake_vid, classes = self.gen.sample_videos(B)
                    fake_img, _ = self.gen.sample_images(B)
                side = self._side if shards == 1 else None
                if side is not None:
                    # D_img(fake images) -- ~40 launches on grids of a few workgroups -- runs on the side stream, under the
                    # video discriminator's GEMMs; autograd replays each node's backward on the stream of its forward, so
                    # the input-gradient half overlaps the same way.  Same kernels on the same inputs: bit-identical.
                    main = torch.cuda.current_stream()
                    side.wait_stream(main)
                    fake_img.record_stream(side)
                    with torch.cuda.stream(side):
                        pi, _ = self.dis_img(fake_img)
                    pv = vid_head(fake_vid)
                    main.wait_stream(side)
                    pi.record_stream(main)
                else:
                    pv = vid_head(fake_vid)
                    pi, _ = self.dis_img(fake_img)
                if self.ncat:      # BCE(D_vid(fake), 1) + BCE(D_img(fake_img), 1) + CE(categ(fake), generated classes)
                    loss = bce_ce_head_pair(pv, 1.0, classes, pi, 1.0)
                elif self.loss == "wasserstein":
                    loss = wasserstein_generator_loss_pair(pi, pv)      # image term first (mnist_moco_ode_wgan.py:174)
                else:
                    loss = bce_with_logits_pair(pv, 1.0, pi, 1.0)
                if batch_adj:      # the video and the image path: two latent adjoints, one launch
                    self.gen._adjoint_batch = dict(expect=2, ops=[], keep=[])
                if early_ar and shards == 1:
                    # both generator passes' decoder backward queued -> the decoder block of the arena is complete: its
                    # all-reduce goes out now, under the latent adjoint(s)
                    self.gen._decoder_passes_left = 1 if joint else 2
                    self.gen._on_decoder_grads = self._early_decoder_allreduce
                loss.backward(gradient=unit_grad(loss.device))
                self.gen._on_decoder_grads = None
                if batch_adj:
                    self.gen.flush_adjoints()
                    self.gen._adjoint_batch = None
                losses.append(loss.detach())
        finally:
            if batch_adj:
                self.gen._adjoint_batch = None
            for p in frozen:
                p.requires_grad_(True)
        self._opt_step(self.gen, self.gen_opt, shards)
        self._flush(self.gen)              # weights are current when the step returns (checkpoints, the next prefetch)
        return self._mean(losses)

    def step(self, real_imgs: Sequence, real_vids: Sequence, real_labels: Optional[Sequence] = None):
        """real_imgs[i]: [B,C,H,W], real_vids[i]: [B,T,C,H,W] for i < d_iters (each may instead be a LIST of shard
        tensors: virtual replicas, see the class docstring).  Returns the three losses of the last inner pass as
        device scalars (the reference prints them every 100 iterations); with shards, their mean over the shards.
        In graph mode the returned scalars are static tensors that the next step() overwrites.
        real_labels (categorical training, dim_z_category > 0: required; else it must stay None): real_labels[i] is the
        int64 [B] device tensor of real_vids[i]'s classes.  MoCoGAN's objective: the video-D step minimises BCE(real, 1) +
        BCE(fake, 0) + CE(categ(real), real_labels), the G step BCE(D_vid(fake), 1) + BCE(D_img(fake_img), 1) +
        CE(categ(D_vid(fake)), generated classes); the image-D step is unchanged."""
        if self.ncat or real_labels is not None:
            if self.ncat and (real_labels is None or len(real_labels) < self.d_iters):
                raise ValueError(f"GanTrainer.step: categorical training (dim_z_category={self.ncat}) needs real_labels, one "
                                 "int64 [B] tensor per inner discriminator pass")
            for i in range(self.d_iters):
                v = real_vids[i]
                if isinstance(v, (list, tuple)):
                    raise NotImplementedError("categorical training does not take virtual-replica shards")
                self._labels_for(real_labels[i], v.shape[0], "GanTrainer.step")
        if self._graph_mode and self._iters >= 2 and not isinstance(real_imgs[0], (list, tuple)):
            return self._graph_step(real_imgs, real_vids)
        return self._eager_step(real_imgs, real_vids, real_labels)

    def _eager_step(self, real_imgs, real_vids, real_labels=None):
        first = _shards(real_imgs[0])
        B, nsh = first[0].shape[0], len(first)
        li = lv = None
        # (virtual replicas -- lists of shards, a parity-testing device -- repeat every call per shard: call by call there)
        # joint generator passes: the fake images of d_image_step i and the fake videos of d_video_step i come out of one
        # decoder pass (no generator update lies between the two calls), like the G step's two batches
        pair = [0] * self.d_iters
        if nsh == 1:
            for i in range(self.d_iters):
                nv, ni = _shards(real_vids[i])[0].shape[0], _shards(real_imgs[i])[0].shape[0]
                if len(_shards(real_vids[i])) == 1 and self._can_pair(nv, ni, True):
                    pair[i] = nv
        if self.prefetch and nsh == 1 and hasattr(self.gen, "prefetch_latents") and next(self.gen.parameters()).is_cuda:
            calls = []
            for i in range(self.d_iters):
                if pair[i]:
                    calls.append(("pair_iv", (pair[i], _shards(real_imgs[i])[0].shape[0])))
                    continue
                calls += [("images", x.shape[0]) for x in _shards(real_imgs[i])]
                calls += [("videos", x.shape[0]) for x in _shards(real_vids[i])]
            calls += [("pair_vi", (B, B))] if self._can_pair(B, B, False) else [("videos", B), ("images", B)]
            self.gen.prefetch_latents(calls)
        try:
            for i in range(self.d_iters):
                # (inside step() the discriminators' optimiser steps are deferred: see overlap_allreduce)
                li = self.d_image_step(real_imgs[i], _join=False, _defer=True, _pair_videos=pair[i])    # side stream
                lv = self.d_video_step(real_vids[i], _defer=True, real_labels=real_labels[i] if self.ncat else None)
            if self._pending:
                # the G step reads both discriminators: their deferred updates land now (the image discriminator's on its
                # side stream, where its step ran)
                if self._side is not None:
                    with torch.cuda.stream(self._side):
                        self._flush(self.dis_img)
                else:
                    self._flush(self.dis_img)
                self._flush(self.dis_vid)
            self._join_side()                                         # the G step reads the updated image discriminator
            lg = self.g_step(B, nsh)
        except BaseException:
            self._paired_fake_vid = None
            if hasattr(self.gen, "discard_prefetched"):
                self.gen.discard_prefetched()
            raise
        self._iters += 1
        if self._freeze_gc and self._iters == 2:     # every plan and program exists now
            freeze_host_gc()
        return li, lv, lg

    # -- HIP-graph replay of the iteration ---------------------------------------------------------------------------
    def _graph_step(self, real_imgs, real_vids):
        key = (tuple(real_imgs[0].shape), tuple(real_vids[0].shape))
        if self._graph is not None and self._graph["key"] != key:
            raise RuntimeError("GanTrainer(graph=True): batch shapes changed after capture "
                               f"({self._graph['key']} -> {key}); build a new trainer for the new shapes")
        if self._graph is None:
            self._capture(real_imgs, real_vids, key)
        else:
            g = self._graph
            for dst, src in zip(g["imgs"] + g["vids"], list(real_imgs) + list(real_vids)):
                if dst.data_ptr() != src.data_ptr():
                    dst.copy_(src, non_blocking=True)
            self._feed.fill_from_script()        # host draws + Adam coefficients for this iteration, in program order
            self._feed.upload()
            g["graph"].replay()
        for m in (self.gen, self.dis_vid, self.dis_img):
            m.invalidate_packs()                 # eager passes after a replay must re-pack (versions did not move)
        self._iters += 1
        return self._graph["losses"]

    def _capture(self, real_imgs, real_vids, key):
        dev = real_imgs[0].device
        for m in (self.gen, self.dis_vid, self.dis_img):
            if id(m) not in self.arenas:
                raise NotImplementedError("GanTrainer(graph=True) needs gradient arenas on all three networks "
                                          f"({type(m).__name__} has none)")
        imgs = [t.detach().clone() for t in real_imgs]      # static inputs: later iterations are copied into them
        vids = [t.detach().clone() for t in real_vids]
        # the graph must be self-contained with respect to the weights: every first-use pack of the iteration has to be
        # recorded.  Which panels are "stale" is host-side state -- an eager sample_videos() between the warm-up
        # iterations and this capture (or a load_state_dict / broadcast_state) would leave panels marked fresh, their
        # pack launches would be missing from the graph, and every replay would run that network on panels that are
        # never re-packed while Adam keeps moving the real weights.
        for m in (self.gen, self.dis_vid, self.dis_img):
            m.invalidate_packs()
        feed = self._feed = HostFeed(dev)
        self.gen._feed = feed
        self.dis_vid._feed = self.dis_img._feed = feed      # (instance noise: the call index of every captured forward)
        for o in (self.gen_opt, self.vid_opt, self.img_opt):
            o._feed = feed
        graph = torch.cuda.CUDAGraph()
        torch.cuda.synchronize()
        feed.begin()
        feed.recording = True
        try:
            with torch.cuda.graph(graph):
                losses = self._eager_step(imgs, vids)
        finally:
            feed.recording = False
        self._iters -= 1                        # _eager_step counted the capture pass; _graph_step counts it
        self._graph = dict(key=key, graph=graph, imgs=imgs, vids=vids, losses=losses)
        # nothing has executed yet: capture only recorded the launches.  The host inputs of THIS iteration were drawn
        # (and the Adam step counts advanced) while recording; upload them and run the iteration.
        feed.upload()
        graph.replay()


def train_step(trainer: GanTrainer, real_imgs, real_vids, real_labels=None):
    """Functional spelling of GanTrainer.step for parity tests that read like oracle.mocogan_ref.train_step."""
    return trainer.step(real_imgs, real_vids, real_labels)
