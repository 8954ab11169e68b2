"""ODE-GAN training: the reference's stage2/ode_training.py (GANODETrainer) on libgode's multi-tensor update kernels.

GAN training read as an ODE in parameter space: instead of Adam, each network takes an Euler, Heun ('rk2') or RK4 step
along its own negative loss gradient, and the discriminators are regularised by the gradient of ||grad_thetaG L_G||^2.
The stage algebra is the reference's, line for line (ode_training.py:59-201); every stage update of a network is ONE
launch of gode_ode_step, and the regulariser is evaluated from first-order passes only.

Parameters that are not on a CUDA device take the same algebra through plain torch ops (the host tests); CUDA
parameters run on the HIP kernels alone.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib as L
from .engine import PointerTable, bump_version, stream_ptr

METHODS = ("euler", "rk2", "rk4")
FD_H = float(np.finfo(np.float32).eps) ** (1.0 / 3.0)      # relative central-difference step for precision eps32


def stage_plan(method, lr, reg, penalty):
    """The updates of one step as [(coefficients {k: c_k}, cq, check)]: after gradient k = len(plan so far) + 1 has been
    taken, p += sum_k c_k * g_k + cq * gp, skipping tensors whose g_check is None.  Formed in double; cq is None on
    every stage but a penalised last one.  Two details are the reference's and stay: Euler's penalty term is reg * gp
    (no lr), and each update's None-check looks at the first gradient of its zip."""
    lr, reg = float(lr), float(reg)
    if method == "euler":
        return [({1: -lr}, -reg if penalty else None, 1)]
    if method == "rk2":
        return [({1: -lr}, None, 1),
                ({1: 0.5 * lr, 2: -0.5 * lr}, -reg * lr if penalty else None, 1)]
    if method == "rk4":
        return [({1: -lr / 2}, None, 1),
                ({1: lr / 2, 2: -lr / 2}, None, 1),
                ({2: lr / 2, 3: -lr}, None, 2),
                ({1: -lr / 6, 2: -lr / 3, 3: 2 * lr / 3, 4: -lr / 6}, -reg * lr if penalty else None, 1)]
    raise AssertionError("Choose method between 'euler', 'rk2' and 'rk4'")


def _f32(x):
    return float(np.float32(x))


class _Device:
    """The fused path of one parameter list: layout of the concatenated index space (fixed: parameters do not move),
    pointer tables per launch site, scratch of the penalty.  Everything is allocated on first use and kept."""

    def __init__(self, params):
        self.params = [p for p in params if p.numel() > 0]
        for p in self.params:
            if p.dtype != torch.float32 or not p.is_contiguous():
                raise RuntimeError("GANODETrainer's fused path takes contiguous fp32 parameters")
        self.device = self.params[0].device
        self.sites = {}
        self._layout_key = None
        self._layout()

    def _layout(self):
        key = tuple(p.data_ptr() for p in self.params)
        if key != self._layout_key:
            lib = L.lib()
            chunks = [int(lib.gode_ode_step_chunks(p.data_ptr(), p.numel())) for p in self.params]
            self.chunk0 = np.concatenate([[0], np.cumsum(chunks)[:-1]]).astype(np.int64)
            self.chunks = int(sum(chunks))
            self.numel = np.asarray([p.numel() for p in self.params], dtype=np.int64)
            self._layout_key = key
        return key

    def _site(self, name):
        s = self.sites.get(name)
        if s is None:
            s = self.sites[name] = PointerTable(self.device)
        return s

    @staticmethod
    def _ptr(t, like):
        if t is None:
            return 0, None
        if t.dtype != torch.float32 or t.device != like.device or t.numel() != like.numel():
            raise RuntimeError("gradient does not match its parameter (fp32, same device, same size expected)")
        if not t.is_contiguous():
            t = t.contiguous()
        return t.data_ptr(), t

    def _bump(self):
        for p in self.params:
            bump_version(p)

    def step(self, site, coefs, grads, cq=None, q=None, cq_dev=None):
        """p += sum_k coefs[k] * grads[k] + cq * (q[0] - q[1]) [* cq_dev[0]] on every parameter, one launch."""
        pk = self._layout()
        rows = np.zeros((len(self.params), 9), dtype=np.int64)
        rows[:, 0], rows[:, 7], rows[:, 8] = pk, self.numel, self.chunk0
        keep, terms, c = [], 0, [0.0] * 4
        for k, ck in coefs.items():
            terms |= 1 << (k - 1)
            c[k - 1] = _f32(ck)
            for i, p in enumerate(self.params):
                rows[i, k], t = self._ptr(grads[k][i], p)
                keep.append(t)
        if q is not None:
            terms |= 16
            for col, lst in ((5, q[0]), (6, q[1])):
                for i, p in enumerate(self.params):
                    rows[i, col], t = self._ptr(lst[i], p)
                    keep.append(t)
        tbl = self._site(site).upload(rows)
        lib = L.lib()
        L.call("ode_step", lambda: L.check(
            lib.gode_ode_step(tbl.data_ptr(), len(self.params), self.chunks, terms, c[0], c[1], c[2], c[3],
                              _f32(cq) if q is not None else 0.0, cq_dev.data_ptr() if cq_dev is not None else None,
                              stream_ptr()), "gode_ode_step"))
        self._keep = keep
        self._bump()

    def _scratch(self):
        if not hasattr(self, "sums"):
            self.sums = torch.zeros(2, dtype=torch.float64, device=self.device)
            self.fd = torch.zeros(2, dtype=torch.float32, device=self.device)        # [eps, 1 / eps]
            self.work = torch.empty(2 * 512, dtype=torch.float64, device=self.device)
            self.saved = [torch.empty_like(p) for p in self.params]

    def axpy(self, site, dst, base, v, a, a_dev=None, h=None):
        """dst = base + a [* a_dev[0]] * v per tensor (v None: copy), one launch; h given: also the two norms and the
        difference step into self.sums / self.fd.  dst's layout is the parameters' (same alignment by construction:
        torch allocations are 512-byte aligned, so `saved` may only add vector lanes, and the chunk count is an upper bound)."""
        self._scratch()
        self._layout()
        rows = np.zeros((len(self.params), 5), dtype=np.int64)
        rows[:, 3] = self.numel
        keep = []
        lib = L.lib()
        chunk = 0
        for i, p in enumerate(self.params):
            rows[i, 0], rows[i, 1] = dst[i].data_ptr(), base[i].data_ptr()
            if v is not None:
                rows[i, 2], t = self._ptr(v[i], p)
                keep.append(t)
            rows[i, 4] = chunk
            chunk += int(lib.gode_ode_step_chunks(dst[i].data_ptr(), p.numel()))
        tbl = self._site(site).upload(rows)
        want = h is not None
        L.call("axpy_multi", lambda: L.check(
            lib.gode_axpy_multi(tbl.data_ptr(), len(self.params), chunk, _f32(a), a_dev.data_ptr() if a_dev is not None else None,
                                self.sums.data_ptr() if want else None, _f32(h) if want else 0.0,
                                self.fd.data_ptr() if want else None, self.work.data_ptr(), stream_ptr()), "gode_axpy_multi"))
        self._keep_axpy = keep


def _torch_update(params, coefs, grads, check, cq=None, gp=None):
    """The same p += sum c_k g_k (+ cq * gp) in torch ops, for parameters off the GPU."""
    with torch.no_grad():
        for i, p in enumerate(params):
            if grads[check][i] is None:
                continue
            u = None
            for k, ck in coefs.items():
                t = grads[k][i] * ck
                u = t if u is None else u + t
            if gp is not None:
                u = u + gp[i] * cq
            p.add_(u)


class GANODETrainer(object):
    """Drop-in for the reference's GANODETrainer (same constructor, same step()).

    modules=(gen, dis_img, dis_vid): optional.  The regulariser evaluates g_loss two more times than the reference
    does; with `modules` the buffers of these networks (BatchNorm running statistics) are put back afterwards, without
    it they see two extra momentum updates per penalised step (eval-mode sampling only).  The closures must draw their
    randomness from torch's CPU generator, NumPy's global state (as the generators of this package do) or the CUDA
    generator of the parameters' device (torch.randn(..., device=device), as the CIFAR notebook's closures do): the
    regulariser rewinds these three.
    """

    def __init__(self, g_params, dImg_params, dVid_params, g_loss, dImg_loss, dVid_loss, lr=0.02, reg=0.01, method='rk4',
                 d_iter=2, g_iter=1, modules=None):
        self.g_params = list(g_params)
        self.dImg_params = list(dImg_params)
        self.dVid_params = list(dVid_params) if dVid_params is not None else None
        self.g_loss, self.dImg_loss, self.dVid_loss = g_loss, dImg_loss, dVid_loss
        self.lr, self.reg, self.method = lr, reg, method
        assert self.method in METHODS, "Choose method between 'euler', 'rk2' and 'rk4'"
        self.penalty = self.reg > 0
        self.d_iter, self.g_iter = d_iter, g_iter
        self.modules = tuple(m for m in modules if m is not None) if modules is not None else None
        if self.penalty and self.modules is not None:
            for m in self.modules:
                if getattr(m, "use_noise", False):
                    raise NotImplementedError(
                        "reg > 0 with use_noise=True: the instance noise is a counter-based device stream that the "
                        "regulariser's repeated g_loss evaluations cannot rewind (DESIGN section 14)")
        self.fd_h = FD_H
        self._dev = {}
        self._buffers = None

    # -- plumbing --------------------------------------------------------------------------------------------------------
    def _fused(self, name, params):
        d = self._dev.get(name)
        if d is None:
            d = self._dev[name] = _Device(params)
        return d

    @staticmethod
    def _on_gpu(params):
        cuda = [p.is_cuda for p in params]
        if any(cuda) and not all(cuda):
            raise RuntimeError("a parameter list must live on one device")
        return bool(cuda) and cuda[0]

    def _save_buffers(self):
        if self.modules is None:
            return
        bufs = [b for m in self.modules for b in m.buffers()]
        if self._buffers is None or len(self._buffers[0]) != len(bufs):
            self._buffers = (bufs, [torch.empty_like(b) for b in bufs])
        with torch.no_grad():
            for b, s in zip(*self._buffers):
                s.copy_(b)

    def _restore_buffers(self):
        if self.modules is None:
            return
        with torch.no_grad():
            for b, s in zip(*self._buffers):
                b.copy_(s)

    # -- the regulariser ---------------------------------------------------------------------------------------------------
    def _penalty_pair(self, params):
        """q+ and q- = grad_params g_loss at thetaG +- eps * v, v = grad_thetaG g_loss; the generator's parameters, the
        random generators (torch's CPU one, NumPy's and the CUDA one of the parameters' device: left as after ONE g_loss call)
        and, with `modules`, all buffers are as before on return.
        Returns (q+, q-, 1/eps as a device float or None, 1/eps as a Python float or None)."""
        cuda_dev = self.g_params[0].device if self._on_gpu(self.g_params) else None

        def rng_state():
            return (torch.get_rng_state(), np.random.get_state(),
                    torch.cuda.get_rng_state(cuda_dev) if cuda_dev is not None else None)

        def rewind(state):
            torch.set_rng_state(state[0]); np.random.set_state(state[1])
            if cuda_dev is not None:
                torch.cuda.set_rng_state(state[2], cuda_dev)

        rng = rng_state()
        v = torch.autograd.grad(self.g_loss(), self.g_params, allow_unused=True)
        rng_after = rng_state()
        self._save_buffers()
        gpu = self._on_gpu(self.g_params)
        if gpu:
            G = self._fused("gen", self.g_params)
            vv = [v[i] for i, p in enumerate(self.g_params) if p.numel() > 0]
            G._scratch()
            G.axpy("save", G.saved, G.params, vv, 0.0, h=self.fd_h)          # thetaG0, both norms and eps in one launch
            inv_host = None
        else:
            with torch.no_grad():
                saved = [p.detach().clone() for p in self.g_params]
                nv = sum(float(g.double().square().sum()) for g in v if g is not None) ** 0.5
                nt = sum(float(p.double().square().sum()) for p in saved) ** 0.5
            eps = self.fd_h * (1.0 + nt) / nv if nv > 0 else 0.0
            inv_host = 1.0 / eps if eps > 0 else 0.0
        q = []
        for k, sign in enumerate((1.0, -1.0)):
            rewind(rng)
            if gpu:
                G.axpy("shift%d" % k, G.params, G.saved, vv, sign, a_dev=G.fd)
                G._bump()
            else:
                with torch.no_grad():
                    for p, s, g in zip(self.g_params, saved, v):
                        if g is not None:
                            p.copy_(s + (sign * eps) * g)
            q.append(torch.autograd.grad(self.g_loss(), params, allow_unused=True))
        if gpu:
            G.axpy("restore", G.params, G.saved, None, 0.0)
            G._bump()
        else:
            with torch.no_grad():
                for p, s in zip(self.g_params, saved):
                    p.copy_(s)
        rewind(rng_after)
        self._restore_buffers()
        return q[0], q[1], (G.fd[1:2] if gpu else None), inv_host

    def grad_penalty(self, model='dis_img'):
        """The regulariser's gradient grad_thetaD ||grad_thetaG L_G||^2 ~ (q+ - q-) / eps as a list of tensors (None where
        g_loss does not reach a parameter).  A diagnostic: step() fuses this expression into its last update."""
        params = self.dImg_params if model == 'dis_img' else self.dVid_params
        qp, qm, inv_dev, inv = self._penalty_pair(params)
        scale = inv_dev if inv_dev is not None else inv
        return [None if a is None else (a - b) * scale for a, b in zip(qp, qm)]

    # -- the step ------------------------------------------------------------------------------------------------------------
    def step(self, x=None, model='gen'):
        assert model in ['gen', 'dis_img', 'dis_vid']
        if model == 'gen':
            return self._ode_step('gen', self.g_params, self.g_loss, x, False)
        if model == 'dis_img':
            return self._ode_step('dis_img', self.dImg_params, self.dImg_loss, x, self.penalty)
        return self._ode_step('dis_vid', self.dVid_params, self.dVid_loss, x, self.penalty)

    def _ode_step(self, name, params, loss_fn, x, penalty):
        plan = stage_plan(self.method, self.lr, self.reg, penalty)
        gpu = self._on_gpu(params)
        dev = self._fused(name, params) if gpu else None
        live = [i for i, p in enumerate(params) if p.numel() > 0]
        grads, loss1, q = {}, None, None
        for s, (coefs, cq, check) in enumerate(plan, start=1):
            loss = loss_fn(x) if x is not None else loss_fn()
            if s == 1:
                loss1 = loss
            grads[s] = torch.autograd.grad(loss, params, allow_unused=True)
            if s == 1 and penalty:
                q = self._penalty_pair(params)         # at the step's starting point, before the first update
            for i in live:
                if grads[check][i] is not None and any(grads[k][i] is None for k in coefs):
                    raise RuntimeError("a parameter lost its gradient between two stages of one step")
            if cq is None:
                if gpu:
                    dev.step("s%d" % s, coefs, {k: [grads[k][i] for i in live] for k in coefs})
                else:
                    _torch_update(params, coefs, grads, check)
            else:
                qp, qm, inv_dev, inv = q
                if any(qp[i] is None or qm[i] is None for i in live):
                    raise RuntimeError("the regulariser does not reach every parameter of this discriminator")
                if gpu:
                    dev.step("s%d" % s, coefs, {k: [grads[k][i] for i in live] for k in coefs}, cq=cq,
                             q=([qp[i] for i in live], [qm[i] for i in live]), cq_dev=inv_dev)
                else:
                    gp = [(a - b) * inv for a, b in zip(qp, qm)]
                    _torch_update(params, coefs, grads, check, cq=cq, gp=gp)
        return loss1
