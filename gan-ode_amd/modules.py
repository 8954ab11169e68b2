"""nn.Module surface of the hot path, mirroring the reference's classes (same names, constructor signatures,
state_dict keys, RNG consumption and return conventions) with all device arithmetic lowered to libgode.so.

Reference: models/mocogan.py (Noise :20-29, PatchImageDiscriminator :66-93, VideoDiscriminator :129-164,
VideoGenerator :185-301) and models/mocogan_ode.py (ODEFunc :6-17, VideoGenerator :20-54, VideoGeneratorMNIST
:57-111, VideoGeneratorMNISTODE :114-148).

The child modules under ``main`` / ``ode_fn`` / ``linear`` / ``recurrent`` are stock torch.nn layers used ONLY as
parameter containers (default init, state_dict keys, .cuda()/.to()); they are never called.  Every forward goes
through the HIP kernels and raises if the tensors are not on the GPU or libgode.so is missing.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import functools
import math
import os
from typing import Optional

import numpy as np
import torch
import torch.nn as nn

from . import _lib as L
from .engine import (LANE_ORDERED, LANE_OVERLAP, LANE_SINGLE, ConvStack, LayerParams, LayerSpec, conv_out, dptr, lane_gate,
                     lane_mode, make_geom, pair_turn, stream_ptr, tensor_version)

Z_COLS = 96  # latent row: [motion 16 | content 50 | zero pad 30]: K % 32 == 0 puts the first decoder GEMM on the FAST path
Z_CATEG0 = 66        # dim_z_category = C > 0: the one-hot lives in the first C pad columns (gode_categ_onehot)
MAX_CATEG = Z_COLS - Z_CATEG0
ODE_METHODS = L.ODE_METHODS      # gen.ode_method -> the latent ops' `method` code
# GODE_SAMPLE_LANES=0 (read once): no-grad sampling calls stay on one stream (_GenPlan._forward_lanes); per generator:
# gen.sample_lanes = False
_SAMPLE_LANES_ENV = os.environ.get("GODE_SAMPLE_LANES", "1") != "0"
# What gen.sample_lanes = True selects behind its gate: pair mode (_GenPlan._forward_pair) or the two-lane front
# (_forward_lanes).  DESIGN section 24 holds the measurement that decides it.
_PAIR_DEFAULT = True


def ode_method_code(name):
    """The `method` code of gen.ode_method = name on the plain Neural-ODE generators (NotImplementedError: no kernel)."""
    return L.ode_method_code(name)


def _require_gpu(t: torch.Tensor, what: str):
    if not t.is_cuda:
        raise RuntimeError(f"{what}: this implementation runs only on an MI355X through libgode.so; move the module "
                           "to the GPU with .cuda() (there is no CPU or PyTorch fallback)")


class _Pool:
    """Plans own their activation buffers; a plan stays checked out between a forward that saved state for autograd
    and its backward, so two overlapping passes of the same shape (D(real), D(fake)) get distinct plans.  A forward
    whose backward never comes (loss dropped) gives its plan back when its autograd node is freed (_Lease).  Every
    forward bumps the plan's generation and its autograd node remembers it: a backward that arrives after the plan's
    buffers were reused (retain_graph second pass, or more than MAX_PLANS forwards of one shape kept alive) raises
    instead of computing on overwritten activations."""

    MAX_PLANS = 6

    def __init__(self):
        self.plans = {}
        self.pack_cache = {}     # packed weight panels shared by every plan of the module

    def get(self, key, factory):
        lst = self.plans.setdefault(key, [])
        for p in lst:
            if not p.busy:
                return p
        if len(lst) >= self.MAX_PLANS:
            # all checked out: reuse the oldest; its pending backward (if it ever comes) fails the generation check
            p = lst.pop(0)
            p.busy = False
            lst.append(p)
            return p
        p = factory()
        lst.append(p)
        return p

    def clear(self):
        self.plans.clear()
        self.pack_cache.clear()


class _Lease:
    """Held by an autograd node: identifies the forward (plan generation) whose buffers the node will need, and gives
    the plan back if the node dies without having run its backward."""

    __slots__ = ("plan", "generation")

    def __init__(self, plan):
        self.plan, self.generation = plan, _plan_generation(plan)

    def check(self, what):
        if _plan_generation(self.plan) != self.generation:
            raise RuntimeError(
                f"{what}: the activation buffers of this forward pass were reused by a later forward of the same shape "
                "before backward() ran (a second backward through a retained graph, or more than "
                f"{_Pool.MAX_PLANS} grad-enabled forwards of one shape kept alive at once); run the forward again")

    def __del__(self):
        try:
            if self.plan.busy and _plan_generation(self.plan) == self.generation:
                self.plan.busy = False
        except Exception:
            pass


def _plan_generation(plan):
    return plan.stack.generation if hasattr(plan, "stack") else plan.generation


# The parameters of a ConvStack cross autograd in one order: per layer the weight, then gamma and beta where the layer has a
# BatchNorm.  The nodes below take the parameters (_flat_params) and return the gradients (_flat_grads) in it.
def _flat_grads(views):
    """ConvStack.backward's per-layer (weight, gamma, beta) gradient views -> the flat list."""
    out = []
    for w, g, b in views:
        out.append(w)
        if g is not None:
            out += [g, b]
    return out


def _flat_params(layer_params):
    return _flat_grads((lp.weight, lp.gamma, lp.beta) for lp in layer_params)


def _grads_into(arena, layer_params):
    """Per layer (weight, gamma, beta gradient targets, accumulate?) inside the trainer's arena, ConvStack.backward's
    `into`: the first writer of an optimiser step stores, later ones add."""
    into = []
    for lp in layer_params:
        wt, acc = arena.target(lp.weight)
        gt = bt = None
        if lp.gamma is not None:
            gt, _ = arena.target(lp.gamma)
            bt, _ = arena.target(lp.beta)
        into.append((wt, gt, bt, acc))
    return into


def _strides5(x):
    """Element strides {N, D, H, W, C} of an [N, C, H, W] or [N, C, D, H, W] tensor."""
    if x.dim() == 5:
        return (x.stride(0), x.stride(2), x.stride(3), x.stride(4), x.stride(1))
    return (x.stride(0), 0, x.stride(2), x.stride(3), x.stride(1))


# ==================================================================================================================
# generator
# ==================================================================================================================
class ODEFunc(nn.Module):
    """Right-hand side f(t, x) = W2 tanh(W1 x + b1) + b2 (models/mocogan_ode.py:6-17).  Evaluated inside the fused
    ODE kernels; calling it directly is not part of the hot path."""

    def __init__(self, dim, dim_hidden):
        super().__init__()
        self.fn = nn.Sequential(nn.Linear(dim, dim_hidden), nn.Tanh(), nn.Linear(dim_hidden, dim))

    def forward(self, t, x):
        raise RuntimeError("ODEFunc is evaluated inside libgode's fused RK4 kernels (gode_ode_fwd/bwd)")


class ODEFuncTanh(nn.Module):
    """Right-hand side f(t, x) = tanh(W x + b) (models/mocogan_mnist.py:6-16: the ODEFunc(dim) of that file).  Evaluated
    inside the fused fixed-grid ODE kernels (the ops' rhs = 1), like ODEFunc."""

    def __init__(self, dim):
        super().__init__()
        self.fn = nn.Sequential(nn.Linear(dim, dim), nn.Tanh())

    def forward(self, t, x):
        raise RuntimeError("ODEFuncTanh is evaluated inside libgode's fused fixed-grid kernels (gode_ode_fwd/bwd, rhs = 1)")


ODE_BACKPROPS = {"adjoint": 0, "discrete": 1}      # gen.ode_backprop -> gode_ode_bwd_op.backprop
_DISCRETE_METHODS = ("rk4", "euler", "midpoint")


def ode_backprop_code(gen):
    """The `backprop` code of gen.ode_backprop (a generator without the attribute: the adjoint).  "discrete" -- the exact
    gradient of the fixed-grid solve -- is served by the plain Neural-ODE generators with the three fixed-grid methods."""
    name = getattr(gen, "ode_backprop", "adjoint")
    try:
        code = ODE_BACKPROPS[name]
    except (KeyError, TypeError):
        raise ValueError(f"ode_backprop {name!r}: " + " or ".join(repr(k) for k in ODE_BACKPROPS)) from None
    if code:
        served = ", ".join(repr(k) for k in _DISCRETE_METHODS)
        if not getattr(gen, "_discrete_ok", True):
            raise NotImplementedError(f"ode_backprop 'discrete' is implemented for the plain Neural-ODE generators (ode_method "
                                      f"{served}), not for {type(gen).__name__}: its latent kernels already back-propagate "
                                      "through their own steps or integrate an adaptive adjoint")
        if gen.ode_method not in _DISCRETE_METHODS:
            raise NotImplementedError(f"ode_backprop 'discrete' with ode_method {gen.ode_method!r}: back-propagating through "
                                      f"adaptive steps is not implemented; the fixed-grid methods {served} are served")
    return code


def _is_one_layer(ode_fn):
    """Is ode_fn (a class or an instance) the one-layer right-hand side?"""
    return issubclass(ode_fn, ODEFuncTanh) if isinstance(ode_fn, type) else isinstance(ode_fn, ODEFuncTanh)


def _ode_fn_tensors(fn):
    """The tensors of an ODEFunc / ODEFuncTanh in the kernels' order: W1, b1[, W2, b2]."""
    return [t for m in fn.fn if isinstance(m, nn.Linear) for t in (m.weight, m.bias)]


def solver_grid_arrays(T, step_size):
    """torchdiffeq options={'step_size': h} (FixedGridODESolver) for t = linspace(0, 1, T): the solver walks its own
    grid arange(niters)*h + t0 (last point clamped to t_end) and interpolates the requested outputs linearly; the
    adjoint pass solves every output interval on the grid built the same way for the reversed span.  All arithmetic
    is fp32 torch on the host, operation for operation what torchdiffeq executes, so the device gets bit-identical
    step sizes and interpolation weights.  Returns CPU tensors: grid_dt[G], emit_at[T] (grid step after which output
    j is produced), emit_w[T] (interpolation weight; 0 / 1 = an end point itself), bstep_off[T], bstep_dt[...]."""
    t = torch.linspace(0, 1, T).float()

    def grid_of(tt):
        start, end = tt[0], tt[-1]
        niters = int(torch.ceil((end - start) / step_size + 1).item())
        gr = torch.arange(0, niters, dtype=tt.dtype) * step_size + start
        gr[-1] = end
        return gr

    gr = grid_of(t)
    gdt = gr[1:] - gr[:-1]
    emit_at = torch.full((T,), -1, dtype=torch.int32)
    emit_w = torch.zeros(T, dtype=torch.float32)
    j = 1
    for i in range(len(gr) - 1):
        a, b = gr[i], gr[i + 1]
        while j < T and bool(b >= t[j]):
            emit_at[j] = i
            emit_w[j] = 0.0 if bool(t[j] == a) else (1.0 if bool(t[j] == b) else (t[j] - a) / (b - a))
            j += 1
    assert j == T
    off, steps = [0], []
    for i in range(1, T):                      # adjoint of output interval i -> i-1: reversed span, t -> -t
        rg = grid_of(-t[i - 1:i + 1].flip(0))
        d = rg[1:] - rg[:-1]
        steps.append(d)
        off.append(off[-1] + len(d))
    return dict(G=len(gdt), grid_dt=gdt, emit_at=emit_at, emit_w=emit_w,
                bstep_off=torch.tensor(off, dtype=torch.int32), bstep_dt=torch.cat(steps))


def latent_co_perm(n_categ=0):
    """Latent column -> row of the first decoder weight (the reference's z = cat([content, category, motion]),
    models/mocogan.py:264-267): columns [motion 16 | content 50 | one-hot C | pad] -> rows [50+C .. 65+C | 0 .. 49 |
    50 .. 49+C | -1 (no row: the column multiplies zeros)]."""
    C_ = int(n_categ)
    return ([50 + C_ + i for i in range(16)] + list(range(50)) + [50 + i for i in range(C_)]
            + [-1] * (Z_COLS - Z_CATEG0 - C_))


def _input_slices(nx, n):
    """The host-drawn inputs of a call travel as ONE block of floats, so that a call stages them with a single H2D
    copy: [x (nx) | content 50 per trajectory | sel 1 per trajectory | class 1 per trajectory], sel and class as int32
    bits (sel: sample_images only; class: dim_z_category > 0 only, the block then ends one word per trajectory later)."""
    a, b = nx + n * 50, nx + n * 51
    return slice(0, nx), slice(nx, a), slice(a, b), slice(b, b + n)


def _pack_inputs(buf, x_host, content_host, sel_host=None, cls_host=None):
    sx, sc, ss, sk = _input_slices(x_host.numel(), content_host.shape[0])
    buf[sx].copy_(x_host.reshape(-1))
    buf[sc].copy_(content_host.reshape(-1))
    if sel_host is not None:
        buf[ss].view(torch.int32).copy_(sel_host)
    if cls_host is not None:
        buf[sk].view(torch.int32).copy_(torch.from_numpy(cls_host.astype(np.int32)))


def _run_multi(ops, op_type, name, stream):
    """gode_<name>(ops, count, stream): several latent solves (or adjoints) side by side, at most 8 per launch."""
    fn = getattr(L.lib(), "gode_" + name)
    for k in range(0, len(ops), 8):
        chunk = ops[k:k + 8]
        arr = (op_type * len(chunk))(*chunk)
        L.call(name, lambda: L.check(fn(arr, len(chunk), stream), "gode_" + name))


_ODE_GRAD_OFFS = [(0, 1024, (64, 16)), (1024, 64, (64,)), (1088, 1024, (16, 64)), (2112, 16, (16,)),
                  (2128, 256, (16, 16)), (2384, 16, (16,)), (2400, 256, (16, 16)), (2656, 16, (16,))]
_PRENET_NPARAM = 2128      # the pre-net's four tensors: the head of the ODE and SDE gradient blocks when it is present


class _DeviceLatents:
    """Stands in for the host-drawn inputs of a sampling call whose latents are drawn on the device: the call index of the
    latent stream (include/gode.h) the plan's draw op takes."""

    __slots__ = ("call",)

    def __init__(self, call):
        self.call = int(call)


class _GenPlan:
    """ODE solve + decoder for `n_traj` trajectories.  full: rows = n_traj*T; select: rows = n_traj (one chosen
    time per trajectory, sample_images).  The subclasses swap the motion latent: each states its buffers (_alloc), its
    parameters (_params), its ops (_programs) and the class attributes below; the algorithm around them lives here."""

    zcols = 68                   # row width of a latent-only plan (sample_z_m); plans with a decoder write Z_COLS
    rows_in_traj = True          # sample_z_m's rows: the kernel's trajectory buffer (else the first 16 latent columns)
    # the adjoint kernel's gradient block.  One-layer right-hand side (ODEFuncTanh, the ops' rhs = 1): the block ends behind
    # b1 -- six tensors, 2400 floats; the kernels neither read nor write a float of `grads` from there on
    rhs = property(lambda self: L.ode_rhs_code("tanh" if _is_one_layer(self.gen.ode_fn) else "mlp"))
    nparam = property(lambda self: L.ODE_RHS_TANH_NPARAM if self.rhs else L.ODE_NPARAM)
    grad_offs = property(lambda self: _ODE_GRAD_OFFS[:6] if self.rhs else _ODE_GRAD_OFFS)
    # no pre-net: this kernel keeps its offsets (the block's first _PRENET_NPARAM floats stay unwritten); the SDE
    # kernel's block starts at the first tensor present
    grads_from_first_present = False
    # gode_<stem>_fwd_multi / _bwd_multi launch several solves at once (None: no such entry); multi_always False: only
    # the adaptive solver's, and its adjoints only when they are adaptive too
    multi, multi_always = ("ode", L.OdeFwdOp, L.OdeBwdOp), False

    def __init__(self, gen: "VideoGenerator", n_traj: int, T: int, select: bool, zbuf=None, x=None, lanes=None):
        """zbuf: latent rows of a joint pass (_GenJointPlan) -- the plan then is the latent half only (no decoder stack).
        x: the motion noise on the device -- sample_z_m's plan: the latent half alone on its own [n_traj*T, zcols] rows, no
        content, no classes, nothing staged."""
        dev = gen.main[0].weight.device
        self.gen, self.n, self.T, self.select, self.device = gen, n_traj, T, select, dev
        self.rows = n_traj if select else n_traj * T
        f32 = dict(dtype=torch.float32, device=dev)
        self.ncat = int(getattr(gen, "dim_z_category", 0)) if x is None else 0
        self.labels = None           # int64 classes of the staged call (written by the one-hot op; full mode only)
        self.x, self.content, self.sel, self.cls = x, None, None, None
        self._in = None              # the input block [x | content | sel | cls] (None: a latent-only plan, x is the caller's)
        self.draw_op = None          # gode_latent_draw in front of the latent program (gen.latent_rng == "device")
        self._draw_evs, self._draw_ev_i = [None] * 4, 0
        self._ring = []
        if x is None:
            xs = self._x_shape(n_traj, T)
            sx, sc, ss, sk = _input_slices(int(np.prod(xs)), n_traj)
            nin = sk.stop if self.ncat else sk.start
            self._in = torch.zeros(nin, **f32)
            self.x, self.content = self._in[sx].view(xs), self._in[sc].view(n_traj, 50)
            self.sel = self._in[ss].view(torch.int32) if select else None
            self.cls = self._in[sk].view(torch.int32) if self.ncat else None
            # pinned staging ring for the host-drawn noise: a pageable H2D copy would block the host until the stream
            # drains (no host/GPU overlap between consecutive calls); slots are recycled behind an event
            self._ring = [dict(buf=torch.zeros(nin).pin_memory(), ev=None) for _ in range(4)]
        self._ring_i = 0
        # the latent rows the kernels write: the decoder's input, the caller's, or the plan's own
        self.stack = None
        if x is not None:
            self._zbuf, self._zcols = torch.empty(n_traj * T, self.zcols, **f32), self.zcols
        elif zbuf is not None:
            self._zbuf, self._zcols = zbuf, Z_COLS
        else:
            self.stack = ConvStack(gen._decoder_specs(self.rows), gen._decoder_params(), dev, owns_input=True,
                                   pack_cache=gen._pool.pack_cache, two_lane_backward=True)
            self._zbuf, self._zcols = self.stack.x_in, Z_COLS
        self._alloc()
        self._ode_ptrs = None
        self.busy = False
        # two-lane sampling (_forward_lanes): the gode_lanes object and its side stream, the cached two-lane program, what
        # the previous call saw (None: it was no lanes call), and the calls counted by the path they took
        self._lanes = self._side = self._lane_prog = self._lane_prev = None
        self.lane_calls = {LANE_OVERLAP: 0, LANE_ORDERED: 0, LANE_SINGLE: 0}
        # pair mode (_forward_pair): the second plan of this shape (built when the first streak starts: it doubles the
        # activation memory), this plan's pair-mode program, what the previous pair call saw (None: the previous forward was
        # no pair call), the pair calls counted by mode, and the staging-copy events of the last two calls of either plan
        # (lane_gate's evidence).  A second plan is driven by the first (_owner) and never enters the pool.
        self._peer = self._pair_prog = self._pair_prev = None
        self._pair_refused = False
        self._owner = self
        self.pair_calls = {LANE_OVERLAP: 0, LANE_ORDERED: 0}
        self._copies = []
        # The one kind of plan that can take the two lanes gets its lanes object now, not at its first lanes call: the side
        # stream takes its hardware queue when it is created, and measured a stream created behind a
        # replayed training graph sat on the caller's queue, 17 us per step slower than one stream.  With gen.sample_lanes
        # off at this point the object is made at the plan's first lanes call after the switch (_lanes_possible).
        self._lanes_ok = type(self) is _GenPlan and self.stack is not None and not self.ncat and _SAMPLE_LANES_ENV
        self.lanes_made_late = False
        self._peer_lanes = None
        if lanes is not None:        # a second plan (pair mode): the lanes object its first plan made for it
            self._make_lanes(lanes)
        elif self._lanes_ok and gen.sample_lanes:
            self._make_lanes()

    @staticmethod
    def _x_shape(n_traj, T):
        """Shape of the host-drawn noise block: the ODE's initial states."""
        return (n_traj, 16)

    def _alloc(self):
        """The solver's own device buffers."""
        f32 = dict(dtype=torch.float32, device=self.device)
        self.traj = torch.empty(self.n, self.T, 16, **f32)
        tt = torch.linspace(0, 1, self.T).float()       # models/mocogan_ode.py:143 -- fp32 grid built on the host
        self.dt = (tt[1:] - tt[:-1]).to(self.device) if self.T > 1 else torch.zeros(1, **f32)
        self.ode_work = torch.empty(L.lib().gode_ode_bwd_work_size(self.n), **f32)

    def _params(self):
        """The latent's tensors in the adjoint kernel's output order (None: an absent pre-net tensor)."""
        g = self.gen
        lin = g.linear
        if isinstance(lin, nn.Identity):
            pre = (None, None, None, None)
        else:
            pre = (lin[0].weight, lin[0].bias, lin[2].weight, lin[2].bias)
        return pre + tuple(_ode_fn_tensors(g.ode_fn))

    @classmethod
    def multi_ok(cls, gen, adjoint):
        """Do this generator's solves (adjoint: their backward passes) go out through the gode_*_multi entries?"""
        if cls.multi is None:
            return False
        return cls.multi_always or (gen.ode_method == "dopri5" and not (adjoint and gen.adjoint_substeps != 0))

    def check_solve(self):
        """Host-side look at a finished solve (the CDE plan's: it raises when the kernel stopped early)."""

    def latent_rows(self):
        """sample_z_m's result [n*T, 16] of a latent-only plan: the ODE kernel writes its trajectory in that very order; the
        other kernels' latent rows hold it in their first 16 columns."""
        if self.rows_in_traj:
            return self.traj.view(self.n * self.T, 16)
        return self._zbuf if self._zcols == 16 else self._zbuf[:, :16].contiguous()

    def _solver_grid(self, step_size):
        gd = solver_grid_arrays(self.T, step_size)
        return {k: (v.to(self.device) if torch.is_tensor(v) else v) for k, v in gd.items()}

    def _programs(self):
        ps = self._params()
        discrete = getattr(self.gen, "ode_backprop", "adjoint") != "adjoint"
        ptrs = tuple(dptr(p) for p in ps) + (self.gen.ode_step_size, self.gen.ode_method, self.gen.ode_rtol,
                                             self.gen.ode_atol, self._draws_on_device(),
                                             getattr(self.gen, "ode_backprop", "adjoint"),
                                             self.gen.ode_substeps if discrete else None)    # (discrete: sizes ysteps)
        if ptrs != self._ode_ptrs:
            method = ode_method_code(self.gen.ode_method)
            backprop = ode_backprop_code(self.gen)
            rhs = self.rhs
            if rhs and method == ODE_METHODS["dopri5"]:
                raise NotImplementedError("ode_method 'dopri5' with the one-layer right-hand side (ODEFuncTanh): libgode's "
                                          "adaptive kernels integrate the two-layer ODEFunc only; the one-layer function "
                                          "is served by 'rk4', 'euler' and 'midpoint'")
            self._ode_ptrs = ptrs
            op = L.OdeParams(*ptrs[:len(ps)])       # (one-layer: six tensors -- W2 / b2 stay NULL, never dereferenced)
            prenet = 0 if ps[0] is None else 1
            zbuf, zcols = self._zbuf, self._zcols
            self.fwd_op = L.OdeFwdOp(p=op, x=dptr(self.x), content=dptr(self.content), dt=dptr(self.dt),
                                     sel_t=dptr(self.sel), z=dptr(zbuf), traj=dptr(self.traj), N=self.n,
                                     T=self.T, substeps=self.gen.ode_substeps, prenet=prenet, zcols=zcols, rhs=rhs)
            self.bwd_op = L.OdeBwdOp(p=op, x=dptr(self.x), traj=dptr(self.traj), dt=dptr(self.dt),
                                     sel_t=dptr(self.sel), gz=None, work=dptr(self.ode_work), grads=None, N=self.n,
                                     T=self.T, substeps=self.gen.ode_substeps, prenet=prenet, accumulate=0, zcols=zcols,
                                     rhs=rhs)
            self._grid = None
            if self.gen.ode_method == "dopri5":
                # torchdiffeq's adaptive solver over the output times; the adjoint call is integrated adaptively too
                # (adjoint_substeps == 0, gode_ode_bwd method 1) or with `adjoint_substeps` fixed Kutta-3/8 steps
                self._tout = torch.linspace(0, 1, self.T).float().to(self.device)
                self._nsteps = torch.zeros((self.n + 63) // 64, dtype=torch.int32, device=self.device)
                # more than one workgroup (32 trajectories each): whole-batch error norm through these words
                ns = L.lib().gode_odernn_sync_size(self.n)
                self._sync_f = torch.zeros(ns, dtype=torch.int32, device=self.device) if ns else None
                self._sync_b = torch.zeros(ns, dtype=torch.int32, device=self.device) if ns else None
                self.fwd_op.sync, self.bwd_op.sync = dptr(self._sync_f), dptr(self._sync_b)
                self.fwd_op.method, self.fwd_op.rtol, self.fwd_op.atol = 1, float(self.gen.ode_rtol), float(self.gen.ode_atol)
                self.fwd_op.tout, self.fwd_op.nsteps = dptr(self._tout), dptr(self._nsteps)
                self.bwd_op.method, self.bwd_op.rtol, self.bwd_op.atol = 1, float(self.gen.ode_rtol), float(self.gen.ode_atol)
                self.bwd_op.tout = dptr(self._tout)
                self._nsteps_bwd = torch.zeros((self.n + 63) // 64, dtype=torch.int32, device=self.device)
                self.bwd_op.nsteps = dptr(self._nsteps_bwd)
            else:
                # the fixed-grid solvers (rk4: the reference's call; euler, midpoint): one grid, whichever steps on it
                self.fwd_op.method = self.bwd_op.method = method
            if self.gen.ode_method != "dopri5" and self.gen.ode_step_size is not None and self.T > 1:
                gd = self._grid = self._solver_grid(float(self.gen.ode_step_size))
                self.fwd_op.G = gd["G"]
                self.fwd_op.grid_dt, self.fwd_op.emit_at, self.fwd_op.emit_w = dptr(gd["grid_dt"]), dptr(gd["emit_at"]), dptr(gd["emit_w"])
                self.bwd_op.bstep_off, self.bwd_op.bstep_dt = dptr(gd["bstep_off"]), dptr(gd["bstep_dt"])
            self._ysteps = None
            if backprop:
                # the exact gradient of the forward's steps, on the forward's grid; off the reference's grid (substeps > 1 or
                # a step_size grid) the kernel re-runs the forward and keeps every step's start state in ysteps
                assert not self.multi_ok(self.gen, True)     # (discrete ops never enter the trainer's _adjoint_batch)
                self.bwd_op.backprop = backprop
                self.bwd_op.G = self.fwd_op.G
                self.bwd_op.grid_dt, self.bwd_op.emit_at, self.bwd_op.emit_w = self.fwd_op.grid_dt, self.fwd_op.emit_at, self.fwd_op.emit_w
                ny = L.lib().gode_ode_bwd_steps_size(self.n, self.T, self.gen.ode_substeps, self.fwd_op.G)
                if ny:
                    self._ysteps = torch.empty(ny, dtype=torch.float32, device=self.device)
                    self.bwd_op.ysteps = dptr(self._ysteps)
            self.categ_op = None
            if self.ncat:
                # the one-hot columns follow the solve in the same program (the solve's content broadcast zeroes the pad)
                self.categ_op = L.CategOp(cls=dptr(self.cls), z=dptr(zbuf), labels_out=None, n_traj=self.n,
                                          rows_per=1 if self.select else self.T, C=self.ncat, zcols=zcols, col0=Z_CATEG0)
            self.fwd_prog = self._latent_program([self.fwd_op] + ([self.categ_op] if self.ncat else []))
        self.fwd_op.substeps = self.bwd_op.substeps = self.gen.ode_substeps
        if self.gen.ode_method == "dopri5":
            self.bwd_op.substeps = self.gen.adjoint_substeps

    # -- latents drawn on the device (gen.latent_rng == "device") ---------------------------------------
    def _draws_on_device(self):
        # (getattr: the host tests drive _programs on bare plans and stand-in generators)
        return getattr(self, "_in", None) is not None and getattr(self.gen, "latent_rng", "host") == "device"

    def _latent_program(self, ops):
        """The latent program: `ops`, behind gode_latent_draw when this plan's input block is drawn on the device.  The op
        writes the block's four sub-blocks in place; its seed, stream and call are set call by call (_set_draw)."""
        self.draw_op = None
        if self._draws_on_device():
            xs = tuple(self.x.shape)
            outer, inner = (xs[0], xs[2]) if len(xs) == 3 else (1, xs[1])
            self.draw_op = L.LatentDrawOp(x=dptr(self.x), content=dptr(self.content), sel_t=dptr(self.sel),
                                          cls=dptr(self.cls), call_dev=None, seed=0, traj0=0, n=self.n, outer=outer,
                                          inner=inner, T=self.T, n_all=self.n * self.T * 2 if self.select else 0,
                                          C=self.ncat, stream=0, call=0)
            ops = [self.draw_op] + list(ops)
        return L.Program(ops)

    def _set_draw(self, latents):
        """Points the draw op at the call `latents` (a _DeviceLatents) stands for.  Under graph capture the call index
        travels in the trainer's HostFeed block (one word, rewritten before every replay), as the discriminators' does."""
        op, gen = self.draw_op, self.gen
        if op is None:
            raise RuntimeError("latent_rng was switched between a sampling call's draw and its launch")
        seed = int(gen.latent_seed) & 0xFFFFFFFFFFFFFFFF
        op.seed = seed - (1 << 64) if seed >= 1 << 63 else seed
        op.stream = int(gen.latent_stream)
        feed = getattr(gen, "_feed", None)
        if feed is not None and feed.recording:
            op.call_dev, op.call = feed.latent_slot(gen, latents.call, 1), 0
        else:
            call = latents.call & 0xFFFFFFFF
            op.call_dev, op.call = None, call - (1 << 32) if call >= 1 << 31 else call

    def _draw_event(self):
        """An event for the place where a host-mode call records its staging copy's (lane_gate's evidence)."""
        i = self._draw_ev_i
        self._draw_ev_i = (i + 1) % len(self._draw_evs)
        if self._draw_evs[i] is None:
            self._draw_evs[i] = torch.cuda.Event()
        return self._draw_evs[i]

    def stage_inputs(self, x_host, content_host, sel_host, cls_host=None):
        """Host-drawn inputs -> the plan's device block, on the current stream (one H2D copy).  cls_host: the trajectories'
        classes (dim_z_category > 0).  x_host a _DeviceLatents: nothing is staged, the latent program's draw op writes the
        block."""
        self._programs()
        device_draw = isinstance(x_host, _DeviceLatents)
        if self.ncat:
            if cls_host is None and not device_draw:
                raise RuntimeError("a categorical generator plan needs the classes of its trajectories")
            if getattr(self.gen, "_feed", None) is not None and self.gen._feed.recording:
                raise NotImplementedError("categorical latents are not captured in a graph (GanTrainer(graph=True))")
            if not self.select:      # a fresh tensor per call: it leaves the plan as sample_videos' second result
                self.labels = torch.empty(self.n, dtype=torch.int64, device=self.device)
            self.categ_op.labels_out = dptr(self.labels) if not self.select else None
        if device_draw:
            self._set_draw(x_host)
            if not torch.cuda.is_current_stream_capturing():
                ev = self._draw_event()
                ev.record()
                self._note_copy(ev)
            return
        feed = getattr(self.gen, "_feed", None)
        if feed is not None and feed.recording:
            # graph capture (GanTrainer(graph=True)): the inputs travel in the trainer's HostFeed block; the recorded
            # copy is device -> device from the block's static region for this call site
            nfl = self._in.numel()
            pin, dev = feed.noise_region(self.gen, self.select, self.n, self.T, nfl)
            _pack_inputs(pin, x_host, content_host, sel_host, cls_host)
            self._in.copy_(dev)
        else:
            slot = self._ring[self._ring_i]
            self._ring_i = (self._ring_i + 1) % len(self._ring)
            if slot["ev"] is not None:
                slot["ev"].synchronize()
            _pack_inputs(slot["buf"], x_host, content_host, sel_host, cls_host)
            self._in.copy_(slot["buf"], non_blocking=True)
            if slot["ev"] is None:
                slot["ev"] = torch.cuda.Event()
            slot["ev"].record()
            self._note_copy(slot["ev"])

    def _note_copy(self, ev):
        own = self._owner
        own._copies = own._copies[-1:] + [ev]

    def forward(self, x_host, content_host, sel_host, training, keep, cls_host=None, no_grad=False):
        """x_host None: the latent rows of this call were produced ahead of time by VideoGenerator.prefetch_latents (on
        its own stream); only the decoder runs here, after the latent's event.  no_grad: the caller's gradient mode is off
        (inside an autograd Function it always is, so the caller has to say)."""
        if x_host is None:
            torch.cuda.current_stream().wait_event(self._latent_ev)
            out = self.stack.forward(training)
            self._lane_prev = self._pair_prev = None
        elif self._lanes_possible(keep, no_grad):
            knob = self.gen.sample_lanes
            if (knob == "pair" or (_PAIR_DEFAULT and knob != "always")) and self._pair_possible(training):
                self._lane_prev = None
                out = self._forward_pair(x_host, content_host, sel_host, training)
            else:
                self._pair_prev = None
                out = self._forward_lanes(x_host, content_host, sel_host, training)
        else:
            self.stage_inputs(x_host, content_host, sel_host, cls_host)
            out = self.stack.forward(training, pre_ops_program=self.fwd_prog)
            self._lane_prev = self._pair_prev = None
            self.lane_calls[LANE_SINGLE] += 1
        self.busy = keep
        return out

    # -- two-lane sampling: the next call's front under this call's decoder ------------------------------------------------
    # A no-grad sampling call's H2D copy, latent solve and layer-0 GEMM (the front) depend on nothing the previous call
    # computed, and write only buffers of this plan: _in, the latent rows, y[0], stats[0].  They go to the side stream of a
    # gode_lanes object, where they wait for the previous call's LAST READER of those buffers (release_after) instead of
    # its last kernel -- so in a loop of calls they run under the previous decoder's GEMMs.  BatchNorm finalize of layer 0
    # stays on the caller's stream: it read-modify-writes the module's running statistics, which a state_dict() clone queued
    # between two calls must see as it does on one stream.  Same kernels on the same inputs: bit-identical.
    # Only a call that finds the GPU behind the host takes the two lanes (lane_mode's gpu_behind): a caller that consumes
    # each result before its next call stays on one stream.
    def _lanes_possible(self, keep, no_grad):
        """The conditions of lane_mode's first group that are known before the decoder pass is prepared, cheapest first."""
        gen = self.gen
        if (not no_grad or keep or not gen.sample_lanes or gen._one_stream or not self._lanes_ok or L.TRACE is not None
                or gen.ode_method == "dopri5"):
            return False
        # lane_mode's gpu_behind (engine.lane_gate), asked before anything dearer so that a call on an idle GPU pays two
        # event queries and nothing else
        if gen.sample_lanes not in ("always", "pair") and not lane_gate(
                self._lane_prev is not None or self._pair_prev is not None, self._copy_pending(1), self._copy_pending(2)):
            return False
        feed = getattr(gen, "_feed", None)
        if (feed is not None and feed.recording) or torch.cuda.is_current_stream_capturing():
            return False
        if self._lanes is None:
            # the plan was built with gen.sample_lanes off: its side stream takes whatever hardware queue is the least used
            # NOW, which may be the caller's (see __init__); gen.lane_stats() counts such late objects
            self._make_lanes()
            self.lanes_made_late = True
        return True

    def _copy_pending(self, back):
        """Has the staging copy of the call `back` calls ago (1: the previous one) not completed yet?"""
        ev = self._copies[-back] if len(self._copies) >= back else None
        return ev is not None and not ev.query()

    def _make_lanes(self, lanes=None):
        """This plan's lanes object: the device's shared one for first plans (L.Lanes.shared says why sharing is safe) --
        and, where the knob can select pair mode, the device's shared one for second plans: a second plan is built only
        when a streak starts, but its stream has to take its hardware queue now, next to this plan's (see __init__;
        measured in DESIGN section 24: made behind a training iteration it shared a queue, the two passes ran one after
        the other and the step was 43 us slower than on two lanes).  Two objects per device whatever the number of plans:
        a process with a trainer's two sampling plans holds as many streams as it did with one object per plan."""
        with torch.cuda.device(self.device):
            self._lanes = lanes if lanes is not None else L.Lanes.shared(torch.cuda.current_device(), False)
            knob = self.gen.sample_lanes
            if lanes is None and (knob == "pair" or (_PAIR_DEFAULT and knob != "always")):
                self._peer_lanes = L.Lanes.shared(torch.cuda.current_device(), True)
        self._side = torch.cuda.ExternalStream(self._lanes.stream_ptr, device=self.device)

    def _front_versions(self):
        """What tells that a tensor the front reads was written: the ODE function's and the pre-net's parameters, and the
        layer-0 weight (torch's version counter, FusedAdam's, the storage).  A write through `.data` shows in none of them:
        VideoGenerator.invalidate_packs is the call that tells."""
        ts = [t for t in self._params() if t is not None] + [self.stack.params[0].weight]
        return tuple(tensor_version(t) for t in ts)

    def _forward_lanes(self, x_host, content_host, sel_host, training):
        """forward() of a call that _lanes_possible let through: the mode is decided once, behind begin_forward."""
        self._programs()
        prev, self._lane_prev = self._lane_prev, None        # (an exception below leaves the next call ORDERED)
        between = L.LAUNCHES - prev["mark"] if prev is not None else -1
        prog, out, repacked = self.stack.begin_forward(training)
        st = stream_ptr()
        cache = self._lane_prog
        if cache is None or cache[0] is not prog or cache[1] is not self.fwd_prog:
            # a rebuilt latent program comes with new grid tensors, uploaded on the caller's stream: no overlap past them
            split = self.stack.front_split(prog, self.fwd_prog.ops)
            cache = self._lane_prog = (prog, self.fwd_prog, None if split is None else L.LanesProgram(*split))
            prev = None
        lp = cache[2]
        versions = self._front_versions()
        mode = lane_mode(enabled=True, trace=False, recording=False, categorical=False, grad=False, keep=False,
                         fixed_grid_ode=True, splittable=lp is not None, prev_lanes=prev is not None,
                         launches_between=between, repacked=repacked,
                         versions_same=prev is not None and prev["versions"] == versions,
                         same_stream=prev is not None and prev["stream"] == st,
                         gpu_behind=True)
        self.lane_calls[mode] += 1
        if mode == LANE_SINGLE:
            self.stage_inputs(x_host, content_host, sel_host)
            self.fwd_prog.run(st)
            prog.run(st)
        else:
            self._stage_on_side(mode == LANE_ORDERED, x_host, content_host, sel_host)
            lp.run_lanes(self._lanes, L.LANES_OVERLAP if mode == LANE_OVERLAP else L.LANES_ORDERED, st)
            self._lane_prev = dict(mark=L.LAUNCHES, versions=versions, stream=st)
        return self.stack.end_forward(out, training)

    def _stage_on_side(self, ordered, x_host, content_host, sel_host):
        """stage_inputs' ring copy on the side lane.  _in is read by the side lane only, so the copy needs no edge of its own
        behind a lanes call; behind anything else (ordered) the last reader may sit on the caller's stream.  Latents drawn
        on the device: the draw op rides in the front of the program; only the event is recorded where the copy's was."""
        if isinstance(x_host, _DeviceLatents):
            self._programs()
            self._set_draw(x_host)
            if ordered:
                self._side.wait_stream(torch.cuda.current_stream())
            ev = self._draw_event()
            ev.record(self._side)
            self._note_copy(ev)
            return
        slot = self._ring[self._ring_i]
        self._ring_i = (self._ring_i + 1) % len(self._ring)
        if slot["ev"] is not None:
            slot["ev"].synchronize()
        _pack_inputs(slot["buf"], x_host, content_host, sel_host)
        if ordered:
            self._side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(self._side):
            self._in.copy_(slot["buf"], non_blocking=True)
            if slot["ev"] is None:
                slot["ev"] = torch.cuda.Event()
            slot["ev"].record()
        self._note_copy(slot["ev"])

    # -- pair mode: two whole decoder passes in flight, on two plans used in turn --------------------------------------------
    # With the BatchNorm finalizes in their deferred form (ConvStack.pair_program) nothing but the trailing gode_bn_running
    # op touches state that two calls share, so a call's whole program runs on its plan's lanes stream and only that op on
    # the caller's stream, behind it (gode_run_pair).  The lane of call m starts behind the caller's stream at the entry
    # of call m-1: the BatchNorm passes and the head of one call then run next to the GEMMs of the other.  Eligible exactly
    # where the two lanes are; a call that cannot overlap (lane_mode's second group, over every parameter the program reads)
    # is ordered behind everything queued.  Same kernels on the same inputs, the running statistics updated in call order on
    # the caller's stream: bit-identical.
    def _pair_possible(self, training):
        """Has this plan's stack a pair-mode program for this pass (a training-mode pass of a plain stack)?  What only
        ConvStack.pair_program can tell (the number of BatchNorm layers) it tells once: _forward_pair then notes the
        refusal and the plan's calls take the two-lane front from there on."""
        return training and not self._pair_refused and self.stack._G2 is False and not self.stack.noisy

    def _pair_versions(self):
        """_front_versions over every tensor the program reads: the whole pass now runs off the caller's stream."""
        ts = [t for t in self._params() if t is not None]
        for p in self.stack.params:
            ts += [t for t in (p.weight, p.gamma, p.beta) if t is not None]
        return tuple(tensor_version(t) for t in ts)

    def _forward_pair(self, x_host, content_host, sel_host, training):
        """forward() of a call that _lanes_possible and _pair_possible let through, on the plan whose turn it is."""
        prev, self._pair_prev = self._pair_prev, None        # (an exception below leaves the next call ordered, on this plan)
        turn = pair_turn(None if prev is None else prev["turn"])
        if turn == 1 and self._peer is None:
            if self._peer_lanes is None:         # (the knob was switched to "pair" after this plan was built)
                with torch.cuda.device(self.device):
                    self._peer_lanes = L.Lanes.shared(torch.cuda.current_device(), True)
            peer = self._peer = type(self)(self.gen, self.n, self.T, self.select, lanes=self._peer_lanes)
            peer._owner = self
        plan = self._peer if turn else self
        plan._programs()
        between = L.LAUNCHES - prev["mark"] if prev is not None else -1
        prog, out, repacked = plan.stack.begin_forward(training, out_stream=plan._side)
        st = stream_ptr()
        cache = plan._pair_prog
        if cache is None or cache[0] is not prog or cache[1] is not plan.fwd_prog:
            # (a rebuilt latent program comes with new grid tensors, uploaded on the caller's stream: no overlap past them)
            ops = plan.stack.pair_program(prog, plan.fwd_prog.ops)
            if ops is None:          # (decided at a plan's first pair call, which runs on the first plan)
                self._pair_refused = True
                return self._forward_lanes(x_host, content_host, sel_host, training)
            cache = plan._pair_prog = (prog, plan.fwd_prog, L.PairProgram(ops, 1))
            prev = None
        versions = self._pair_versions()
        mode = lane_mode(enabled=True, trace=False, recording=False, categorical=False, grad=False, keep=False,
                         fixed_grid_ode=True, splittable=True, prev_lanes=prev is not None, launches_between=between,
                         repacked=repacked, versions_same=prev is not None and prev["versions"] == versions,
                         same_stream=prev is not None and prev["stream"] == st, gpu_behind=True)
        self.pair_calls[mode] += 1
        plan._stage_on_side(mode == LANE_ORDERED, x_host, content_host, sel_host)
        other = self if turn else self._peer
        cache[2].run_pair(plan._lanes, None if other is None else other._lanes,
                          L.LANES_OVERLAP if mode == LANE_OVERLAP else L.LANES_ORDERED, st)
        self._pair_prev = dict(mark=L.LAUNCHES, versions=versions, stream=st, turn=turn)
        return plan.stack.end_forward(out, training)

    def _decoder_pass_done(self):
        """The trainer may ask to be told when the LAST decoder backward of a generator step has been queued (the decoder
        block of the gradient arena is then complete and its all-reduce can start under the latent adjoint)."""
        cb = getattr(self.gen, "_on_decoder_grads", None)
        if cb is not None:
            self.gen._decoder_passes_left -= 1
            if self.gen._decoder_passes_left == 0:
                cb()

    def backward(self, gout, arena=None):
        if arena is not None:
            into = _grads_into(arena, self.gen._decoder_params())
            _, _, gz = self.stack.backward(gout, need_input_grad=True, into=into)
            self._decoder_pass_done()
            self.latent_backward(gz.data_ptr(), arena, gz)
            self.busy = False
            return None, None
        flat, views, gz = self.stack.backward(gout, need_input_grad=True)
        motion = self.latent_backward(gz.data_ptr(), None, gz)
        self.busy = False
        return views, motion

    def latent_backward(self, gz_ptr, arena, keep):
        """Adjoint of the latent half given the gradient wrt its latent rows (gz_ptr: first row, the op's zcols floats per
        row).  arena: gradients go straight into the trainer's arena, whose tail holds the latent's tensors contiguously in
        the kernel's output order (first writer of a step stores, later ones add), and the launch may be deferred into the
        trainer's batch; else -> list of gradient tensors in _params order (those present)."""
        op = self.bwd_op
        op.gz = gz_ptr
        ps = self._params()
        absent = _PRENET_NPARAM if ps[0] is None else 0          # floats of the block that belong to no tensor
        cut = absent if self.grads_from_first_present else 0     # ... and how many of them the kernel leaves out
        if arena is not None:
            tgt = [arena.target(q) for q in ps if q is not None]      # (every tensor: marks its .grad as written)
            base, acc = tgt[0]
            op.grads = base.data_ptr() - 4 * (absent - cut)
            op.accumulate = 1 if acc else 0
            batch = getattr(self.gen, "_adjoint_batch", None)
            if batch is not None and self.multi_ok(self.gen, True):
                # the trainer announced how many generator passes this backward holds (video + image path of the G step):
                # their adjoints -- one workgroup each -- go out as ONE launch once the last decoder backward is through
                batch["ops"].append(op)
                batch["keep"].append(keep)
                if len(batch["ops"]) >= batch["expect"]:
                    self.gen.flush_adjoints()
            else:
                L.run_one(op, stream_ptr())
            return None
        grads = torch.empty(self.nparam - cut, dtype=torch.float32, device=self.device)
        op.grads = grads.data_ptr()
        op.accumulate = 0
        L.run_one(op, stream_ptr())
        return [grads[o - cut:o - cut + n].view(shp) for o, n, shp in self.grad_offs[4 if absent else 0:]]


class _GenJointPlan:
    """sample_videos(nv) and sample_images(ni) of one generator step decoded in ONE pass: latent rows [nv*T video rows | ni
    image rows], two BatchNorm batches (ConvStack(split_images=nv*T)): the reference calls `main` on the 512-row and on
    the 32-row batch separately (models/mocogan.py:276,293) -- same arithmetic per element, but the image path's GEMMs
    (M = 32 rows: 45-65 TFLOP/s on their own) ride along in the video path's launches and every elementwise / reduction
    launch is issued once.  `vid` / `img`: the latent halves (plans without a decoder) writing into the joint buffer.
    images_first: the reference called sample_images first (the discriminator steps), so its BatchNorm momentum update
    comes first."""

    def __init__(self, gen, nv, ni, T, images_first):
        dev = gen.main[0].weight.device
        self.gen, self.nv, self.ni, self.T, self.device = gen, nv, ni, T, dev
        self.rows_v, self.rows_i = nv * T, ni
        self.stack = ConvStack(gen._decoder_specs(self.rows_v + self.rows_i), gen._decoder_params(), dev, owns_input=True,
                               pack_cache=gen._pool.pack_cache, split_images=self.rows_v, split_order=1 if images_first else 0,
                               two_lane_backward=True)       # (UCF G step 4.43 -> 4.34 ms, MNIST neutral)
        self.vid = gen._plan_cls(gen, nv, T, False, zbuf=self.stack.x_in[:self.rows_v])
        self.img = gen._plan_cls(gen, ni, T, True, zbuf=self.stack.x_in[self.rows_v:])
        self.images_first = images_first
        self.busy = False
        self._latent_ev = None

    def subplans(self):
        """in the order of the reference's calls (= the order of the host draws)"""
        return (self.img, self.vid) if self.images_first else (self.vid, self.img)

    def forward(self, host, training, keep):
        """host: [(x, content, sel) per sub-plan in call order], or None when the latents were prefetched."""
        if host is None:
            torch.cuda.current_stream().wait_event(self._latent_ev)
        else:
            subs = self.subplans()
            for sub, h in zip(subs, host):
                sub.stage_inputs(*h)
            self.gen._launch_latents(list(subs))
        out = self.stack.forward(training)
        self.busy = keep
        return out

    def backward(self, g_joint, arena):
        subs = (self.vid, self.img)
        offs = (0, 4 * self.rows_v * Z_COLS)
        if arena is not None:
            into = _grads_into(arena, self.gen._decoder_params())
            _, _, gz = self.stack.backward(g_joint, need_input_grad=True, into=into)
            self.vid._decoder_pass_done()
            for sub, off in zip(subs, offs):
                sub.latent_backward(gz.data_ptr() + off, arena, gz)
            self.busy = False
            return None, None
        flat, views, gz = self.stack.backward(g_joint, need_input_grad=True)
        motion = None
        for sub, off in zip(subs, offs):
            m = sub.latent_backward(gz.data_ptr() + off, None, gz)
            motion = m if motion is None else [a + b for a, b in zip(motion, m)]
        self.busy = False
        return views, motion


def _gen_backward(ctx, plan, gout, n_other):
    """The tail of both generator nodes' backward: the plan's backward, then one gradient per forward argument (n_other
    non-parameter arguments first) -- all None when the kernels wrote into the trainer's arena."""
    arena = getattr(plan.gen, "_gode_arena", None)
    if arena is not None and arena.active:
        plan.backward(gout, arena)
        return (None,) * (n_other + ctx.n_params)
    views, motion = plan.backward(gout, None)
    grads = _flat_grads(views)
    assert len(grads) == ctx.n_dec and len(motion) == ctx.n_params - ctx.n_dec
    return (None,) * n_other + (*grads, *motion)


class _GenJointFn(torch.autograd.Function):
    """The joint generator pass as one autograd node with two outputs (video frames, image frames)."""

    @staticmethod
    def forward(ctx, plan, host, training, keep, n_dec, *params):
        out = plan.forward(host, training, keep)
        ctx.plan, ctx.n_dec, ctx.n_params = plan, n_dec, len(params)
        ctx.lease = _Lease(plan)
        ctx.out_shape = tuple(out.shape)
        return out.narrow(0, 0, plan.rows_v), out.narrow(0, plan.rows_v, plan.rows_i)

    @staticmethod
    def backward(ctx, gv, gi):
        plan = ctx.plan
        ctx.lease.check(type(plan.gen).__name__ + " (joint pass)")
        g = torch.empty(ctx.out_shape, dtype=torch.float32, device=plan.device)
        for part, gg in ((g.narrow(0, 0, plan.rows_v), gv), (g.narrow(0, plan.rows_v, plan.rows_i), gi)):
            if gg is None:
                part.zero_()
            else:
                part.copy_(gg)
        return _gen_backward(ctx, plan, g, 5)


class _GenFn(torch.autograd.Function):
    """Whole generator pass (pre-net + RK4 + decoder) as one autograd node; backward = decoder backward + adjoint."""

    @staticmethod
    def forward(ctx, plan, x_host, content_host, sel_host, cls_host, training, keep, no_grad, n_dec, *params):
        out = plan.forward(x_host, content_host, sel_host, training, keep, cls_host, no_grad=no_grad)
        ctx.plan, ctx.n_dec, ctx.n_params = plan, n_dec, len(params)
        ctx.lease = _Lease(plan)
        return out

    @staticmethod
    def backward(ctx, gout):
        plan = ctx.plan
        ctx.lease.check(type(plan.gen).__name__)
        return _gen_backward(ctx, plan, gout, 9)


class _LatentFn(torch.autograd.Function):
    """sample_z_m as its own autograd node: the generator's latent kernel alone on a latent-only plan, rows [N*T, 16] in
    the reference's transpose(0, 1).reshape(-1, 16) order (row n*T + t); backward = the plan's adjoint."""

    @staticmethod
    def forward(ctx, gen, x_host, n, T, *params):
        lp = gen._plan_cls(gen, n, T, False, x=x_host.to(gen.main[0].weight.device))
        lp._programs()
        lp.fwd_prog.run(stream_ptr())
        lp.check_solve()
        ctx.lp = lp
        return lp.latent_rows()

    @staticmethod
    def backward(ctx, gout):
        lp = ctx.lp
        g = gout.contiguous()
        lp.bwd_op.zcols = 16
        return (None, None, None, None, *lp.latent_backward(g.data_ptr(), None, g))


class VideoGenerator(nn.Module):
    """MoCoGAN generator whose motion latent is a Neural ODE (models/mocogan_ode.py:20-54), 64x64 decoder
    (models/mocogan.py:200-215).  `ode_substeps` (build extension, default 1 = the reference's one RK4 step per
    output interval) sub-divides each interval."""

    mnist = False
    _plan_cls = None   # set below (_GenPlan)
    # no-grad sampling calls: True -- whenever a call finds the GPU behind the host, the two-lane front
    # (_GenPlan._forward_lanes) or, with _PAIR_DEFAULT, pair mode (_GenPlan._forward_pair: two decoder passes in flight on
    # two plans); "always" -- the two-lane front and "pair" -- pair mode at every call, also on an idle GPU (tests and
    # traces: the mode then depends on no timing); False -- one stream (A/B runs).  Read at every call; a plan built while it is False makes its lanes object at its first lanes call after
    # the switch.
    sample_lanes = True
    _one_stream = 0            # > 0: inside one_stream()
    _categorical_ok = True     # dim_z_category > 0 is served (the other motion latents switch it off)
    _one_layer_ok = True       # ode_fn=ODEFuncTanh is served (the ODE-RNN generator, whose kernels are two-layer, refuses it)
    # the reference passes method='rk4' (models/mocogan_ode.py:50,144); 'dopri5' is what BASELINE configs[3] words;
    # 'euler' and 'midpoint' are torchdiffeq's other two fixed-grid solvers, on rk4's grid (ODE_METHODS: all served names)
    ode_method = "rk4"
    # How the fixed-grid solve is back-propagated.  "adjoint": torchdiffeq's odeint_adjoint, the reference's call -- the
    # continuous adjoint re-integrated backwards, which differs from the gradient of the computed solve by the solver's
    # truncation error.  "discrete": the exact reverse-mode gradient of the forward's steps (what autograd through
    # torchdiffeq's odeint gives), for 'rk4', 'euler' and 'midpoint' (DESIGN section 29).  Read at every call.
    ode_backprop = "adjoint"
    _discrete_ok = True        # (the SDE / CDE / GRU / ODE-RNN generators switch it off)
    # adjoint_substeps (dopri5 only): 0 = the adjoint is integrated adaptively with the same controller and
    # torchdiffeq's mixed norm, as odeint_adjoint does; k > 0 = k fixed Kutta-3/8 steps per output interval
    ode_rtol, ode_atol, adjoint_substeps = 1e-7, 1e-9, 0
    # Where sample_videos / sample_images / sample_pair / prefetch_latents take their latents from.  "host": the reference's
    # NumPy / torch CPU draws, uploaded (the RNG contract every fixture rests on).  "device": one gode_latent_draw launch in
    # front of the latent solve, from the counter-based latent stream of include/gode.h keyed by latent_seed (default:
    # torch.initial_seed() at construction), latent_stream (0; GanTrainer sets the rank) and latent_call, which every
    # sampling call advances by one -- no host draw, no upload, the global generators untouched; it matches no torch or
    # NumPy generator.  Plain attributes, no buffers.  sample_z_m / sample_z_content / sample_z_categ / sample_z_video, the
    # reference's surface, draw on the host in both modes.
    latent_rng = "host"
    latent_stream = 0
    _latent_call = 0

    def __init__(self, n_channels, dim_z_content, dim_z_category, dim_z_motion, video_length, ode_fn=ODEFunc,
                 dim_hidden=None, linear=True, ngf=64):
        super().__init__()
        self.latent_seed = torch.initial_seed() & 0xFFFFFFFFFFFFFFFF
        if not self._categorical_ok and dim_z_category != 0:
            raise NotImplementedError(f"categorical latents (dim_z_category={dim_z_category}) are implemented for the "
                                      f"Neural-ODE generators only, not for {type(self).__name__}")
        if not (0 <= int(dim_z_category) <= MAX_CATEG) or int(dim_z_category) != dim_z_category:
            raise NotImplementedError(f"dim_z_category={dim_z_category}: the categorical one-hot lives in the {MAX_CATEG} pad "
                                      f"columns of the {Z_COLS}-column latent row (0 <= dim_z_category <= {MAX_CATEG})")
        if dim_z_motion != 16 or dim_z_content != 50:
            raise NotImplementedError("libgode's fused ODE kernels are specialised for dim_z_motion=16, "
                                      "dim_z_content=50 (mnist_moco_ode.py:78, ucf_moco_ode.py:80)")
        self.n_channels, self.dim_z_content, self.dim_z_category = n_channels, dim_z_content, dim_z_category
        self.dim_z_motion, self.video_length, self.ngf = dim_z_motion, video_length, ngf
        self.ode_substeps = 1
        self.ode_step_size = None    # = torchdiffeq options={'step_size': h}; None: the reference's call (grid = outputs)
        dim_z = dim_z_motion + dim_z_category + dim_z_content
        # construction order == the reference's, so that a given torch seed yields the same initial weights
        self.recurrent = nn.GRUCell(dim_z_motion, dim_z_motion)       # models/mocogan.py:198 (unused by ODE path)
        self.main = self._make_main(dim_z, ngf, n_channels, mnist=False)  # base class always builds the 64x64 stack
        self._init_ode_parts(ode_fn, dim_hidden, linear, dim_z, ngf)
        self._pool = _Pool()

    def _init_ode_parts(self, ode_fn, dim_hidden, linear, dim_z, ngf):
        if dim_hidden is None and not (isinstance(ode_fn, type) and _is_one_layer(ode_fn)):
            # the reference passes no dim_hidden here and its ODEFunc then raises TypeError;
            # keep the failure mode but say why.  (The one-layer ODEFuncTanh takes none: ucf_moco_ode.py:80's call
            # constructs against models/mocogan_mnist.py.)
            raise TypeError("ODEFunc.__init__() missing 1 required positional argument: 'dim_hidden' "
                            "(pass dim_hidden=16; ucf_moco_ode.py:80 omits it and fails the same way)")
        self.ode_fn = self._make_ode_fn(ode_fn, dim_hidden)
        self.linear = self._make_prenet(linear)

    def _make_ode_fn(self, ode_fn, dim_hidden):
        """The fused RK4 / adjoint kernels hard-code ODEFunc's 16 -> 16 -> 16 tanh MLP (one MFMA tile per mat-vec):
        anything else would be integrated with the wrong right-hand side, so it is refused here.  The one exception is the
        one-layer ODEFuncTanh (tanh(W x + b), models/mocogan_mnist.py): the fixed-grid kernels are compiled for it too."""
        if isinstance(ode_fn, type) and _is_one_layer(ode_fn):
            if not self._one_layer_ok:
                raise NotImplementedError(f"{type(self).__name__} does not serve the one-layer ODEFuncTanh: only the plain "
                                          "Neural-ODE generators' fixed-grid kernels integrate tanh(W x + b)")
            if dim_hidden:
                # models/mocogan_mnist.py:23-24 would call ode_fn(dim=..., dim_hidden=...) on an __init__(self, dim)
                raise TypeError("ODEFunc.__init__() got an unexpected keyword argument 'dim_hidden' (the one-layer "
                                "ODEFunc of models/mocogan_mnist.py takes dim only)")
            fn = ode_fn(dim=self.dim_z_motion)
            lin = [m for m in fn.fn] if hasattr(fn, "fn") else []
            if not (len(lin) == 2 and isinstance(lin[0], nn.Linear) and isinstance(lin[1], nn.Tanh)
                    and tuple(lin[0].weight.shape) == (16, 16) and lin[0].bias is not None):
                raise NotImplementedError("ode_fn.fn must be Sequential(Linear(16,16), Tanh())")
            return fn
        hid = dim_hidden if dim_hidden else self.dim_z_motion
        if hid != 16:
            raise NotImplementedError(f"dim_hidden={hid}: libgode's fused ODE kernels are specialised for the "
                                      "16-16-16 ODEFunc of mnist_moco_ode.py:78 (dim_hidden=None -> dim_z_motion=16)")
        if not (isinstance(ode_fn, type) and issubclass(ode_fn, ODEFunc)):
            raise NotImplementedError("ode_fn must be gan_ode_amd's ODEFunc (W2 tanh(W1 x + b1) + b2, "
                                      "models/mocogan_ode.py:6-17): the right-hand side is evaluated inside the "
                                      "fused HIP kernels, an arbitrary Python callable cannot be")
        fn = ode_fn(dim=self.dim_z_motion, dim_hidden=hid)
        lin = [m for m in fn.fn] if hasattr(fn, "fn") else []
        if not (len(lin) == 3 and isinstance(lin[0], nn.Linear) and isinstance(lin[1], nn.Tanh)
                and isinstance(lin[2], nn.Linear) and tuple(lin[0].weight.shape) == (16, 16)
                and tuple(lin[2].weight.shape) == (16, 16)):
            raise NotImplementedError("ode_fn.fn must be Sequential(Linear(16,16), Tanh(), Linear(16,16))")
        return fn

    def _make_prenet(self, linear):
        if not linear:
            return nn.Identity()
        d = self.dim_z_motion
        return nn.Sequential(nn.Linear(d, 64), nn.LeakyReLU(0.2), nn.Linear(64, d), nn.LeakyReLU(0.2))

    @staticmethod
    def _make_main(dim_z, ngf, n_channels, mnist):
        w = [dim_z, ngf * 8, ngf * 4, ngf * 2, ngf]
        layers = []
        for i in range(4):
            st, pd = (1, 0) if i == 0 else (2, 1)
            layers += [nn.ConvTranspose2d(w[i], w[i + 1], 4, st, pd, bias=False), nn.BatchNorm2d(w[i + 1]), nn.ReLU(True)]
        if mnist:
            layers.append(nn.ConvTranspose2d(ngf, n_channels, kernel_size=1, stride=1, padding=2, bias=False))
        else:
            layers.append(nn.ConvTranspose2d(ngf, n_channels, 4, 2, 1, bias=False))
        layers.append(nn.Tanh())
        return nn.Sequential(*layers)

    # -- plan description ----------------------------------------------------------------------------------------
    def _decoder_specs(self, rows):
        ngf, nc = self.ngf, self.n_channels
        dev = self.main[0].weight.device
        perm = torch.tensor(latent_co_perm(self.dim_z_category), dtype=torch.int32, device=dev)
        one = (1, 1, 1)
        specs = [LayerSpec(make_geom(rows, ngf * 8, Z_COLS, (1, 4, 4), one, (1, 4, 4), one, (0, 0, 0)), L.DGRAD,
                           L.ACT_RELU, True, co_perm=perm)]
        hw = 4
        for ci, co in ((ngf * 4, ngf * 8), (ngf * 2, ngf * 4), (ngf, ngf * 2)):
            specs.append(LayerSpec(make_geom(rows, ci, co, (1, hw * 2, hw * 2), (1, hw, hw), (1, 4, 4), (1, 2, 2),
                                             (0, 1, 1)), L.DGRAD, L.ACT_RELU, True))
            hw *= 2
        if self.mnist:   # ConvTranspose2d(ngf, C, 1, 1, padding=2): a 1x1 conv on the centre 28x28 crop
            specs.append(LayerSpec(make_geom(rows, nc, ngf, (1, 28, 28), (1, 32, 32), one, one, (0, 2, 2)), L.DGRAD,
                                   L.ACT_NONE, False, epilogue=L.EPI_TANH))
        else:
            specs.append(LayerSpec(make_geom(rows, nc, ngf, (1, 64, 64), (1, 32, 32), (1, 4, 4), (1, 2, 2), (0, 1, 1)),
                                   L.DGRAD, L.ACT_NONE, False, epilogue=L.EPI_TANH))
        return specs

    def _decoder_params(self):
        m = self.main
        out = []
        for i in range(4):
            conv, bn = m[3 * i], m[3 * i + 1]
            out.append(LayerParams(conv.weight, bn.weight, bn.bias, bn.running_mean, bn.running_var,
                                   bn.num_batches_tracked))
        out.append(LayerParams(m[12].weight))
        return out

    def _decoder_list(self):
        return _flat_params(self._decoder_params())

    def _param_list(self):
        ode = []
        if not isinstance(self.linear, nn.Identity):
            ode += [self.linear[0].weight, self.linear[0].bias, self.linear[2].weight, self.linear[2].bias]
        ode += _ode_fn_tensors(self.ode_fn)
        return self._decoder_list(), ode

    def _apply(self, fn, *a, **k):
        r = super()._apply(fn, *a, **k)
        if hasattr(self, "_pool"):
            self._pool.clear()   # parameter storage may have moved
            self.__dict__.pop("_labels", None)
            self.__dict__.pop("_latent_plans", None)
            self.__dict__.pop("_prefetched", None)
        return r

    def lane_stats(self):
        """How this generator's no-grad sampling calls ran, summed over its plans: {"overlap", "ordered", "single"} -> calls,
        and how many plans hold a lanes object (made late: after the plan, on a switch of sample_lanes to a true value).
        A loop of calls that counts overlaps but gains nothing has its side stream on the caller's hardware queue (the
        runtime shares a few queues among all streams of the process): two lanes then only cost; sample_lanes = False."""
        out = {LANE_OVERLAP: 0, LANE_ORDERED: 0, LANE_SINGLE: 0, "lanes_objects": 0, "lanes_objects_made_late": 0,
               "pair_overlap": 0, "pair_ordered": 0, "pair_plans": 0}
        for plans in self._pool.plans.values():
            for p in plans:
                for k, v in getattr(p, "lane_calls", {}).items():
                    out[k] += v
                for k, v in getattr(p, "pair_calls", {}).items():
                    out["pair_" + k] += v
                out["pair_plans"] += getattr(p, "_peer", None) is not None
                out["lanes_objects"] += getattr(p, "_lanes", None) is not None
                out["lanes_objects_made_late"] += bool(getattr(p, "lanes_made_late", False))
        return out

    @contextlib.contextmanager
    def one_stream(self):
        """Sampling calls inside stay on the caller's stream, as with sample_lanes = False (the trainers' discriminator
        steps, whose generator calls always follow other launches)."""
        self._one_stream += 1
        try:
            yield
        finally:
            self._one_stream -= 1

    def invalidate_packs(self):
        """Call after writing ANY parameter of the generator behind autograd's back (`p.data.copy_()`, `p.data.clamp_()`,
        `dist.broadcast(p.data)`): such writes bump neither torch's version counter nor FusedAdam's.  Conv weights: the
        packed weight panels would stay stale.  The ODE function's and the pre-net's parameters and the first conv weight:
        a two-lane sampling call (_GenPlan._forward_lanes) would let its front, which reads them, start under the
        previous call's decoder, ahead of a write queued on the caller's stream in between; after this call the next
        sampling call of every plan orders its front behind everything queued.  In-place ops on the parameter itself,
        optimiser steps, load_state_dict and .to()/.cuda() are tracked automatically."""
        for k in [k for k in self._pool.pack_cache if k[0] == "ver"]:
            del self._pool.pack_cache[k]
        for plans in self._pool.plans.values():
            for p in plans:
                if getattr(p, "_lane_prev", None) is not None:
                    p._lane_prev = None
                if getattr(p, "_pair_prev", None) is not None:
                    p._pair_prev = None

    def _zero_labels(self, n, device):
        """np.zeros(B) -> torch.from_numpy -> .cuda() of the reference (models/mocogan.py:235,279): float64 zeros,
        never written by anyone, so one cached tensor per batch size serves every call (no fill kernel per call)."""
        key = (n, device)
        t = self.__dict__.setdefault("_labels", {}).get(key)
        if t is None:
            t = self._labels[key] = torch.zeros(n, dtype=torch.float64, device=device)
        return t

    _gode_direct_grads = True      # the backward kernels can write into a trainer-owned GradArena

    def _arena_tail(self):
        """Pre-net + ODEFunc tensors in the adjoint kernel's output order (they must be contiguous in the arena)."""
        return self._param_list()[1]

    # -- host-side latent draws: RNG call order is part of the contract ---------------------------------------
    def _draw(self, num_samples, video_len):
        """NumPy normal for the content code first (models/mocogan.py:252), then torch.randn on the CPU generator
        for the ODE's initial noise (models/mocogan_ode.py:136)."""
        content = np.random.normal(0, 1, (num_samples, self.dim_z_content)).astype(np.float32)
        x = torch.randn(num_samples, self.dim_z_motion)
        return torch.from_numpy(content), x

    def _run(self, n_traj, T, select, x, content, sel, cls=None, plan=None):
        # (cls before plan: callers splat _host_inputs' three or four values into x, content, sel[, cls])
        ode_backprop_code(self)
        _require_gpu(self.main[0].weight, type(self).__name__)
        if plan is None:
            plan = self._pool.get((n_traj, T, select), lambda: self._plan_cls(self, n_traj, T, select))
        dec, ode = self._param_list()
        # (grad mode is off inside Function.forward, so decide here whether the plan must be kept for a backward)
        keep = torch.is_grad_enabled() and any(p.requires_grad for p in dec + ode)
        no_grad = not torch.is_grad_enabled()
        return _GenFn.apply(plan, x, content, sel, cls, self.training, keep, no_grad, len(dec), *dec, *ode)

    # -- latents ahead of time ----------------------------------------------------------------------------------------
    def prefetch_latents(self, calls):
        """calls: [("videos" | "images", num_samples), ...] -- the sample_videos / sample_images calls that will follow,
        in order, with no optimiser step on THIS network in between (one training iteration: the generator's weights
        change only at its end).  All host draws are made now, in call order (the same NumPy / torch CPU generator
        consumption as the calls themselves would make), and the latent solves of all calls are issued at once on a side
        stream; the calls then only wait for the latents and run the decoder.  For the ODE-RNN generator the solves --
        one workgroup of a 256-CU GPU each, ~100 us of dependent arithmetic -- become ONE launch whose workgroups run side
        by side (gode_odernn_fwd_multi) instead of six launches back to back.  Results are bit-identical to the calls
        without prefetch.  latent_rng == "device": nothing is drawn on the host; each announced call takes the next index of
        the latent stream, in announcement order, and its plan's draw op runs ahead of the solves."""
        ode_backprop_code(self)
        _require_gpu(self.main[0].weight, type(self).__name__)
        if self.__dict__.get("_prefetched"):
            raise RuntimeError("prefetch_latents: the previous prefetch has not been consumed "
                               f"({len(self._prefetched)} calls left)")
        for kind, n in calls:
            if kind not in ("videos", "images", "pair_vi", "pair_iv"):
                raise ValueError(f"prefetch_latents: unknown call kind {kind!r}")
        main = torch.cuda.current_stream()
        lat = self.__dict__.get("_latent_stream")
        if lat is None or lat.device != main.device:
            lat = self._latent_stream = torch.cuda.Stream(device=main.device)
        plans, queue = [], []
        T = self.video_length
        per_shape = {}
        for kind, n in calls:
            per_shape[(kind, n)] = per_shape.get((kind, n), 0) + 1
        if max(per_shape.values(), default=0) > _Pool.MAX_PLANS:
            raise RuntimeError(f"prefetch_latents: more than {_Pool.MAX_PLANS} calls of one shape ahead (each holds its own "
                               "plan and buffers); announce fewer calls at a time")
        for kind, n in calls:                  # (plans are created on the caller's stream, like every other plan)
            if kind.startswith("pair"):        # n = (n_videos, n_images): sample_pair -- one joint plan, two latent halves
                plan = self._joint_plan(n[0], n[1], T, kind == "pair_iv")
                if plan is None:
                    raise RuntimeError(f"prefetch_latents: {kind}{n} cannot be decoded jointly; announce the two calls")
                plan.busy = True
                plans.append(plan)
                queue.append((kind, n, T, plan))
                continue
            select = kind == "images"
            plan = self._pool.get((n, T, select), lambda: self._plan_cls(self, n, T, select))
            plan.busy = True                   # reserved: a second call of the same shape gets its own plan and buffers
            plans.append(plan)
            queue.append((select, n, T, plan))
        lat.wait_stream(main)                  # weights written on the caller's stream (Adam) are complete
        with torch.cuda.stream(lat):
            latent_plans = []
            for plan, (select, n, _, _) in zip(plans, queue):
                # draw and stage call by call: a generator may hand out a reused host buffer (the ODE-RNN noise stack)
                for sub in (plan.subplans() if isinstance(plan, _GenJointPlan) else (plan,)):
                    sub.stage_inputs(*self._inputs(sub.select, sub.n, T))
                    latent_plans.append(sub)
            self._launch_latents(latent_plans)
            ev = torch.cuda.Event()
            ev.record(lat)
        for p in plans:
            p._latent_ev = ev
        self._prefetched = queue

    def _launch_latents(self, plans):
        """The latent solves of `plans`: through the plan class's gode_*_fwd_multi entry where it has one -- solves of one
        workgroup each at the config sizes run side by side instead of back to back -- else program by program."""
        st = stream_ptr()
        pc = self._plan_cls
        if pc.multi_ok(self, False):
            draws = [p.draw_op for p in plans if p.draw_op is not None]
            if draws:                        # the plans' latents, drawn on this stream ahead of the solves that read them
                L.Program(draws).run(st)
            _run_multi([p.fwd_op for p in plans], pc.multi[1], pc.multi[0] + "_fwd_multi", st)
            if self.dim_z_category:          # the one-hot columns of every solve, behind the solves
                L.Program([p.categ_op for p in plans]).run(st)
        else:
            for p in plans:
                p.fwd_prog.run(st)
        for p in plans:
            p.check_solve()

    def flush_adjoints(self):
        """Launch the adjoints collected during a backward pass (GanTrainer.g_step: video + image path)."""
        batch = getattr(self, "_adjoint_batch", None)
        if not batch or not batch["ops"]:
            return
        pc = self._plan_cls
        _run_multi(batch["ops"], pc.multi[2], pc.multi[0] + "_bwd_multi", stream_ptr())
        batch["ops"], batch["keep"] = [], []

    def discard_prefetched(self):
        """Drop latents that were prefetched but will not be consumed (an exception in the middle of an iteration)."""
        for _, _, _, plan in self.__dict__.get("_prefetched") or []:
            plan.busy = False
        self._prefetched = []

    def _take_prefetched(self, select, n, T):
        q = self.__dict__.get("_prefetched")
        if not q:
            return None
        s0, n0, T0, plan = q[0]
        if (s0, n0, T0) != (select, n, T):
            name = lambda k: k if isinstance(k, str) else ("sample_images" if k else "sample_videos")      # noqa: E731
            raise RuntimeError(f"prefetch_latents promised {name(s0)}({n0}) next, got {name(select)}({n}, video_len={T})")
        q.pop(0)
        return plan

    # -- latents drawn on the device ---------------------------------------------------------------------------------
    @property
    def latent_call(self):
        """The call index the next device-mode sampling call takes (wraps at 2^32)."""
        return self._latent_call

    @latent_call.setter
    def latent_call(self, v):
        self._latent_call = int(v) & 0xFFFFFFFF

    @contextlib.contextmanager
    def latents_at(self, call):
        """Device-mode sampling calls inside start from call index `call`; the previous counter comes back on exit (the same
        sample grid every epoch, without touching any global generator)."""
        prev = self._latent_call
        self.latent_call = call
        try:
            yield self
        finally:
            self._latent_call = prev

    def _inputs(self, select, num_samples, T):
        """The inputs of one sampling call: _host_inputs' draws, or (latent_rng == "device") the call's index in the latent
        stream -- the plan's draw op then writes what the host would have staged."""
        mode = self.latent_rng
        if mode == "host":
            return self._host_inputs(select, num_samples, T)
        if mode != "device":
            raise ValueError(f"latent_rng={mode!r}: 'host' (the reference's draws) or 'device' (the counter-based stream)")
        self._check_len(T)
        call = self._latent_call
        self._latent_call = (call + 1) & 0xFFFFFFFF
        return _DeviceLatents(call), None, None

    # -- reference API ---------------------------------------------------------------------------------------------
    def _host_inputs(self, select, num_samples, T):
        """The host-drawn inputs of one sample_videos (select False) / sample_images (select True) call, consuming the
        NumPy and torch CPU generators exactly as the reference does: -> (x [n_traj, 16], content [n_traj, 50],
        sel int32 [n_traj] or None), and dim_z_category > 0: + the trajectories' classes, drawn between the content and the
        motion noise (models/mocogan.py:259-262).  sample_images: the reference integrates B*T*2 trajectories and decodes
        B randomly chosen rows of the B*T*2*T latent rows (models/mocogan.py:287-295); all draws are made, only the
        chosen trajectories are kept."""
        self._check_len(T)
        n_all = num_samples * T * 2 if select else num_samples
        if self.dim_z_category:
            content, cls, x = self._draw_categorical(n_all)
        else:
            (content, x), cls = self._draw(n_all, T), None
        sel = None
        if select:
            j = np.sort(np.random.choice(n_all * T, num_samples, replace=False)).astype(np.int64)
            traj = torch.from_numpy(j // T)
            sel = torch.from_numpy((j % T).astype(np.int32))
            x, content = self._take_trajectories(x, traj), content[traj].contiguous()
            cls = cls[j // T] if cls is not None else None
        return (x, content, sel) if cls is None else (x, content, sel, cls)

    def _draw_categorical(self, num_samples):
        """_draw with the class draw at the reference's place: content (NumPy normal), classes (ONE np.random.randint(C,
        size=n), models/mocogan.py:237), motion noise (torch.randn)."""
        content = np.random.normal(0, 1, (num_samples, self.dim_z_content)).astype(np.float32)
        cls = np.random.randint(self.dim_z_category, size=num_samples)
        x = torch.randn(num_samples, self.dim_z_motion)
        return torch.from_numpy(content), cls, x

    @staticmethod
    def _take_trajectories(x, traj):
        return x[traj].contiguous()

    def _check_len(self, T):
        """Refuses a video length the motion latent cannot serve, before anything is drawn (VideoGeneratorCDE)."""

    def _fill_host_inputs(self, buf, select, num_samples, T):
        """Graph replay (HostFeed): the same draws, written straight into the feed block's region for this call site."""
        _pack_inputs(buf, *self._host_inputs(select, num_samples, T))

    def sample_videos(self, num_samples, video_len=None):
        """-> (videos [B, C, T, H, W] fp32, float64 zero labels [B]); models/mocogan.py:271-285.  dim_z_category > 0: the
        second result is the int64 classes the videos were generated for (on the device, as the reference's)."""
        T = video_len if video_len is not None else self.video_length
        plan = self._take_prefetched(False, num_samples, T)
        if plan is not None:
            h = self._run(num_samples, T, False, None, None, None, plan=plan)
        else:
            if self.dim_z_category:          # the plan is needed here: its `labels` are the call's int64 classes
                _require_gpu(self.main[0].weight, type(self).__name__)
                plan = self._pool.get((num_samples, T, False), lambda: self._plan_cls(self, num_samples, T, False))
            h = self._run(num_samples, T, False, *self._inputs(False, num_samples, T), plan=plan)  # [B*T, 1, H, W, C]
        H, W = h.size(2), h.size(3)
        h = h.view(num_samples, T, H, W, self.n_channels).permute(0, 4, 1, 2, 3)
        if self.dim_z_category:
            return h, plan.labels
        return h, self._zero_labels(num_samples, h.device)

    def sample_images(self, num_samples):
        """-> (images [B, C, H, W], None); models/mocogan.py:287-295.  The reference integrates B*T*2 trajectories
        and decodes B randomly chosen rows of the B*T*2*T latent rows; the draws are reproduced exactly on the host
        and only the chosen trajectories are integrated.  For the fixed-grid rk4 call of the reference this is exact
        (trajectories are independent and unselected rows receive no gradient).  With ode_method="dopri5" it is a
        documented deviation: torchdiffeq accepts/rejects steps on an error norm over ALL B*T*2 trajectories, here
        the norm is taken over the selected ones, so the accepted step sequence differs (both solutions are within
        rtol 1e-7 of the exact flow; tests/test_gpu_modules.py::test_dopri5_method_against_oracle pins the size).
        latent_rng == "device": the selection and the chosen trajectories' latents come from the latent stream, whose values
        are a function of the trajectory's index -- only the chosen ones are ever drawn, bit for bit what drawing all gives."""
        T = self.video_length
        plan = self._take_prefetched(True, num_samples, T)
        if plan is not None:
            h = self._run(num_samples, T, True, None, None, None, plan=plan)
        else:
            h = self._run(num_samples, T, True, *self._inputs(True, num_samples, T))
        return h.view(num_samples, h.size(2), h.size(3), self.n_channels).permute(0, 3, 1, 2), None

    def sample_pair(self, n_videos, n_images, images_first=False):
        """(sample_videos(n_videos), sample_images(n_images)) -- or, images_first, the same two calls in the other order --
        with the host draws of those two calls in that order, decoded in ONE pass over [video rows | image rows] with
        per-call BatchNorm batch statistics (_GenJointPlan): -> ((videos, labels), (images, None)).  Falls back to the two
        calls when the layers' statistics rows do not split at the batch boundary (unusual batch sizes)."""
        T = self.video_length
        ode_backprop_code(self)
        _require_gpu(self.main[0].weight, type(self).__name__)
        plan = self._take_prefetched("pair_iv" if images_first else "pair_vi", (n_videos, n_images), T)
        host = None
        if plan is None:
            plan = self._joint_plan(n_videos, n_images, T, images_first)
            if plan is None:
                if images_first:
                    im = self.sample_images(n_images)
                    return self.sample_videos(n_videos), im
                vd = self.sample_videos(n_videos)
                return vd, self.sample_images(n_images)
            host = [self._inputs(sub.select, sub.n, T) for sub in plan.subplans()]
        dec, ode = self._param_list()
        keep = torch.is_grad_enabled() and any(p.requires_grad for p in dec + ode)
        hv, hi = _GenJointFn.apply(plan, host, self.training, keep, len(dec), *dec, *ode)
        H, W = hv.size(2), hv.size(3)
        vid = hv.view(n_videos, T, H, W, self.n_channels).permute(0, 4, 1, 2, 3)
        img = hi.view(n_images, H, W, self.n_channels).permute(0, 3, 1, 2)
        return (vid, plan.vid.labels if self.dim_z_category else self._zero_labels(n_videos, vid.device)), (img, None)

    def can_pair(self, n_videos, n_images, images_first=False):
        """Can sample_pair decode these two batches in one pass?  (Builds the plan on first use.)"""
        key = ("pair", n_videos, n_images, self.video_length, images_first)
        if key in self.__dict__.get("_no_joint", ()):
            return False
        return bool(self._pool.plans.get(key)) or self._joint_plan(n_videos, n_images, self.video_length, images_first) is not None

    def _joint_plan(self, nv, ni, T, images_first):
        """A free joint plan for this shape, or None when the shape cannot be decoded jointly."""
        key = ("pair", nv, ni, T, images_first)
        bad = self.__dict__.setdefault("_no_joint", set())
        if key in bad:
            return None
        try:
            return self._pool.get(key, lambda: _GenJointPlan(self, nv, ni, T, images_first))
        except ValueError:
            bad.add(key)
            return None

    def sample_z_content(self, num_samples, video_len=None):
        """models/mocogan.py:249-257 -> [N*T, 50], the same code on all T rows of a video."""
        T = video_len if video_len is not None else self.video_length
        c = np.repeat(np.random.normal(0, 1, (num_samples, self.dim_z_content)).astype(np.float32), T, axis=0)
        return torch.from_numpy(c).to(self.main[0].weight.device)

    def sample_z_categ(self, num_samples, video_len=None):
        """models/mocogan.py:231-247: dim_z_category == 0 -> (None, np.zeros(N)); else ONE np.random.randint(C, size=N)
        -> (one-hot [N*T, C] on the device, the same row on all T rows of a video; the classes as a NumPy array)."""
        if self.dim_z_category <= 0:
            return None, np.zeros(num_samples)
        T = video_len if video_len is not None else self.video_length
        classes = np.random.randint(self.dim_z_category, size=num_samples)
        one_hot = np.zeros((num_samples, self.dim_z_category), dtype=np.float32)
        one_hot[np.arange(num_samples), classes] = 1
        return torch.from_numpy(np.repeat(one_hot, T, axis=0)).to(self.main[0].weight.device), classes

    def sample_z_m(self, num_samples, video_len=None):
        """models/mocogan_ode.py:133-148 (UCF class :39-54): torch.randn(N, 16) on the CPU generator -> pre-net ->
        odeint(rk4 on linspace(0, 1, T)) -> transpose(0, 1).reshape(-1, 16): [N*T, 16], row n*T + t -- and the same for the
        other motion latents (mocogan_ode_rnn.py:39-51 and mocogan.py:217-229: row n*T + t = h_{t+1}; mocogan_sde.py:49-64;
        mocogan_cde.py:60-84), each with its own noise (_draw_motion).  One launch of the generator's fused latent
        kernel, differentiable through its adjoint kernel.  sample_videos()/sample_images() do NOT go through here -- they
        fuse the solve with the content broadcast and the decoder -- this method exists for the reference's public
        surface (and is what sample_z_video calls)."""
        T = video_len if video_len is not None else self.video_length
        self._check_len(T)
        ode_backprop_code(self)
        _require_gpu(self.main[0].weight, type(self).__name__)
        x = self._draw_motion(num_samples, T)
        return _LatentFn.apply(self, x, num_samples, T, *self._param_list()[1])

    def _draw_motion(self, num_samples, T):
        return torch.randn(num_samples, self.dim_z_motion)

    def sample_z_video(self, num_samples, video_len=None):
        """models/mocogan.py:259-269: (cat([content, motion], dim=1) [N*T, 66], np.zeros(N)); RNG order: NumPy normal
        for the content first, then torch.randn for the motion noise."""
        z_content = self.sample_z_content(num_samples, video_len)
        z_category, z_category_labels = self.sample_z_categ(num_samples, video_len)
        z_motion = self.sample_z_m(num_samples, video_len)
        if z_category is not None:
            return torch.cat([z_content, z_category, z_motion], dim=1), z_category_labels
        return torch.cat([z_content, z_motion], dim=1), z_category_labels

    def forward(self, *a, **k):
        raise RuntimeError("use sample_videos()/sample_images() (the reference never calls forward())")


VideoGenerator._plan_cls = _GenPlan


class VideoGeneratorMNIST(VideoGenerator):
    """28x28 decoder variant (models/mocogan_ode.py:57-111)."""

    mnist = True

    def _init_ode_parts(self, ode_fn, dim_hidden, linear, dim_z, ngf):
        self.ode_fn = self._make_ode_fn(ode_fn, dim_hidden)
        self.main = self._make_main(dim_z, ngf, self.n_channels, mnist=True)
        self.linear = self._make_prenet(linear)


class VideoGeneratorMNISTODE(VideoGeneratorMNIST):
    """The class mnist_moco_ode.py:6 imports (models/mocogan_ode.py:114-148)."""

    def _init_ode_parts(self, ode_fn, dim_hidden, linear, dim_z, ngf):
        super()._init_ode_parts(ode_fn, dim_hidden, linear, dim_z, ngf)
        self.ode_fn = self._make_ode_fn(ode_fn, dim_hidden)   # re-created, as the reference does
        self.linear = self._make_prenet(linear)


class _OneLayerDefault:
    """The constructor of models/mocogan_mnist.py's three generators: ode_fn defaults to that file's one-layer ODEFunc
    (ODEFuncTanh), built with dim alone when dim_hidden is falsy (:23-26, :60-63, :117-120)."""

    def __init__(self, n_channels, dim_z_content, dim_z_category, dim_z_motion, video_length, ode_fn=ODEFuncTanh,
                 dim_hidden=None, linear=True, ngf=64):
        super().__init__(n_channels, dim_z_content, dim_z_category, dim_z_motion, video_length, ode_fn=ode_fn,
                         dim_hidden=dim_hidden, linear=linear, ngf=ngf)


class VideoGeneratorTanh(_OneLayerDefault, VideoGenerator):
    """models/mocogan_mnist.py:19-53: the 64x64 generator; VideoGenerator(n_channels, 50, 0, 16, 16), the UCF driver's
    own call (ucf_moco_ode.py:80), constructs here.  Built in the reference's order: recurrent, main, ode_fn, linear."""


class VideoGeneratorMNISTTanh(_OneLayerDefault, VideoGeneratorMNIST):
    """models/mocogan_mnist.py:56-110: recurrent, the 64x64 main, ode_fn, the 28x28 main, linear."""


class VideoGeneratorMNISTODETanh(_OneLayerDefault, VideoGeneratorMNISTODE):
    """models/mocogan_mnist.py:113-147.  Its super().__init__ call hands none of ode_fn / dim_hidden / linear on, so the
    parent builds its defaults first (a one-layer ODEFunc, the 28x28 main, a pre-net); ode_fn and linear are then built
    again from the arguments."""

    def _init_ode_parts(self, ode_fn, dim_hidden, linear, dim_z, ngf):
        VideoGeneratorMNIST._init_ode_parts(self, ODEFuncTanh, None, True, dim_z, ngf)
        self.ode_fn = self._make_ode_fn(ode_fn, dim_hidden)
        self.linear = self._make_prenet(linear)


_RNN_GRAD_OFFS = [(0, 256, (16, 16)), (256, 16, (16,)), (272, 256, (16, 16)), (528, 16, (16,)),
                  (544, 768, (48, 16)), (1312, 768, (48, 16)), (2080, 48, (48,)), (2128, 48, (48,))]


class _RnnGenPlan(_GenPlan):
    """ODE-RNN latent (gode_odernn_fwd/bwd) + decoder.  x_host carries the noise stack [T+1, n, 16]."""

    rows_in_traj = False
    nparam, grad_offs = L.ODERNN_NPARAM, _RNN_GRAD_OFFS
    multi, multi_always = ("odernn", L.OdeRnnFwdOp, L.OdeRnnBwdOp), True

    def _alloc(self):
        n_traj, T = self.n, self.T
        f32 = dict(dtype=torch.float32, device=self.device)
        self.noise = self.x        # [T+1, n, 16]: h_0 and the per-frame GRU inputs (staged by the base class)
        self.hp = torch.empty(n_traj, T, 16, **f32)
        self.nsteps = torch.zeros(T, dtype=torch.int32, device=self.device)          # dopri5 trial steps per frame
        self.nsteps_bwd = torch.zeros(T, dtype=torch.int32, device=self.device)      # ... of each frame's adjoint call
        self.rnn_work = torch.empty(L.lib().gode_odernn_bwd_work_size(n_traj), **f32)
        # more than one workgroup (32 trajectories each): the whole-batch error norm is exchanged through these words
        ns = L.lib().gode_odernn_sync_size(n_traj)
        self.sync_f = torch.zeros(ns, dtype=torch.int32, device=self.device) if ns else None
        self.sync_b = torch.zeros(ns, dtype=torch.int32, device=self.device) if ns else None

    @staticmethod
    def _x_shape(n_traj, T):
        return (T + 1, n_traj, 16)

    def _params(self):
        g = self.gen
        f, r = g.ode_fn.fn, g.recurrent
        return (f[0].weight, f[0].bias, f[2].weight, f[2].bias, r.weight_ih, r.weight_hh, r.bias_ih, r.bias_hh)

    def _programs(self):
        ptrs = tuple(dptr(p) for p in self._params())
        if ptrs + (self._draws_on_device(),) != self._ode_ptrs:
            self._ode_ptrs = ptrs + (self._draws_on_device(),)
            op = L.OdeRnnParams(*ptrs)
            self.fwd_op = L.OdeRnnFwdOp(p=op, noise=dptr(self.noise), content=dptr(self.content), sel_t=dptr(self.sel),
                                        z=dptr(self._zbuf), hs=None, hp=dptr(self.hp), nsteps=dptr(self.nsteps),
                                        N=self.n, T=self.T, rtol=self.gen.ode_rtol, atol=self.gen.ode_atol, zcols=self._zcols,
                                        sync=dptr(self.sync_f))
            self.bwd_op = L.OdeRnnBwdOp(p=op, noise=dptr(self.noise), hp=dptr(self.hp), sel_t=dptr(self.sel), gz=None,
                                        work=dptr(self.rnn_work), grads=None, N=self.n, T=self.T,
                                        substeps=self.gen.adjoint_substeps, accumulate=0, zcols=self._zcols,
                                        rtol=self.gen.ode_rtol, atol=self.gen.ode_atol, sync=dptr(self.sync_b),
                                        nsteps=dptr(self.nsteps_bwd))
            self.fwd_prog = self._latent_program([self.fwd_op])
        self.fwd_op.rtol, self.fwd_op.atol = self.gen.ode_rtol, self.gen.ode_atol
        self.bwd_op.rtol, self.bwd_op.atol = self.gen.ode_rtol, self.gen.ode_atol
        self.bwd_op.substeps = self.gen.adjoint_substeps


class VideoGeneratorMNISTODERNN(VideoGeneratorMNIST):
    """ODE-RNN generator (models/mocogan_ode_rnn.py:21-53): per frame the hidden state is evolved by the Neural ODE
    over a unit interval (torchdiffeq default solver: dopri5, rtol 1e-7, atol 1e-9) and then updated by the GRU cell
    with fresh noise.  The pre-net `linear` is constructed (state_dict parity) but unused, as in the reference.
    Noise: the reference calls T.FloatTensor(n, d).normal_() (models/mocogan.py:297-301), i.e. the DEVICE generator on
    a GPU; here it is always drawn from the global torch CPU generator in the same order and copied to the device, so
    that runs are comparable with the CPU oracle at identical seeds ("ROCm .cuda() semantics")."""

    _categorical_ok = False     # dim_z_category > 0 is refused: categorical latents exist for the Neural-ODE generators only
    _one_layer_ok = False

    _plan_cls = _RnnGenPlan
    _discrete_ok = False
    ode_rtol, ode_atol = 1e-7, 1e-9
    adjoint_substeps = 0      # 0: adaptive adjoint (torchdiffeq's behaviour); 32 was round 1's fixed discretisation

    def _init_ode_parts(self, ode_fn, dim_hidden, linear, dim_z, ngf):
        super()._init_ode_parts(ode_fn, dim_hidden, linear, dim_z, ngf)
        self.ode_fn = self._make_ode_fn(ode_fn, dim_hidden)
        self.linear = self._make_prenet(linear)

    def _param_list(self):
        f, r = self.ode_fn.fn, self.recurrent
        return self._decoder_list(), [f[0].weight, f[0].bias, f[2].weight, f[2].bias,
                                      r.weight_ih, r.weight_hh, r.bias_ih, r.bias_hh]

    def _draw(self, num_samples, video_len):
        """content (NumPy) first, then h_0 and one e_t per frame from FloatTensor(...).normal_()
        (models/mocogan.py:252,297-301; mocogan_ode_rnn.py:44-47)."""
        content = np.random.normal(0, 1, (num_samples, self.dim_z_content)).astype(np.float32)
        # filled in place into a reused host buffer: the draws consume the generator exactly like the reference's
        # fresh FloatTensor(n, d).normal_() calls, without a ~1 MB malloc/free per call (large transient host
        # allocations next to a live HIP context showed up as 75-90 ms stalls on the GPU box)
        key = (num_samples, video_len)
        buf = self.__dict__.setdefault("_noise_bufs", {}).get(key)
        if buf is None:
            buf = self._noise_bufs[key] = torch.empty(video_len + 1, num_samples, self.dim_z_motion)
        for i in range(video_len + 1):
            buf[i].normal_()
        return torch.from_numpy(content), buf

    @staticmethod
    def _take_trajectories(noise, traj):
        return noise[:, traj].contiguous()        # noise stack [T+1, n, 16]: trajectories are the middle axis

    def _draw_motion(self, num_samples, T):
        """h_0 and one e_t per frame, each a fresh FloatTensor(n, d).normal_() on the global torch CPU generator
        (models/mocogan.py:297-301; call order of models/mocogan_ode_rnn.py:42-46) -> [T+1, n, 16]."""
        buf = torch.empty(T + 1, num_samples, self.dim_z_motion)
        for i in range(T + 1):
            buf[i].normal_()
        return buf


# ------------------------------------------------------------------------------------------------------------------
# GRU motion latent: the original MoCoGAN generator (models/mocogan.py:185-301)
# ------------------------------------------------------------------------------------------------------------------
_GRU_GRAD_OFFS = [(0, 768, (48, 16)), (768, 768, (48, 16)), (1536, 48, (48,)), (1584, 48, (48,))]


class _GruGenPlan(_GenPlan):
    """GRU latent (gode_gru_fwd/bwd) + decoder.  x_host carries the noise stack [T+1, n, 16] (h_0, e_0 .. e_{T-1})."""

    rows_in_traj = False
    zcols = 16
    nparam, grad_offs = L.GRU_NPARAM, _GRU_GRAD_OFFS
    multi, multi_always = ("gru", L.GruFwdOp, L.GruBwdOp), True

    def _alloc(self):
        f32 = dict(dtype=torch.float32, device=self.device)
        self.noise = self.x        # [T+1, n, 16], staged by the base class
        self.hs = torch.empty(self.n, self.T + 1, 16, **f32)             # every h_t, kept for the backward
        self.gru_work = torch.empty(L.lib().gode_gru_bwd_work_size(self.n), **f32)

    @staticmethod
    def _x_shape(n_traj, T):
        return (T + 1, n_traj, 16)

    def _params(self):
        r = self.gen.recurrent
        return (r.weight_ih, r.weight_hh, r.bias_ih, r.bias_hh)

    def _programs(self):
        ptrs = tuple(dptr(p) for p in self._params())
        if ptrs + (self._draws_on_device(),) != self._ode_ptrs:
            self._ode_ptrs = ptrs + (self._draws_on_device(),)
            op = L.GruParams(*ptrs)
            self.fwd_op = L.GruFwdOp(p=op, noise=dptr(self.noise), content=dptr(self.content), sel_t=dptr(self.sel),
                                     z=dptr(self._zbuf), hs=dptr(self.hs), N=self.n, T=self.T, zcols=self._zcols)
            self.bwd_op = L.GruBwdOp(p=op, noise=dptr(self.noise), hs=dptr(self.hs), sel_t=dptr(self.sel), gz=None,
                                     work=dptr(self.gru_work), grads=None, N=self.n, T=self.T, accumulate=0,
                                     zcols=self._zcols)
            self.fwd_prog = self._latent_program([self.fwd_op])


class VideoGeneratorGRU(VideoGenerator):
    """The original MoCoGAN generator (models/mocogan.py:185-301; `from models.mocogan import VideoGenerator` resolves
    here): the motion latent is a GRUCell(16, 16) driven by fresh noise every frame, h_{t+1} = GRUCell(e_t, h_t), latent
    row n*T + t = h_{t+1}; the 64x64 decoder is the one the UCF ODE generator inherits.  The module holds exactly
    `recurrent` and `main`, built in the reference's order (same seeded weights and state_dict).
    Deviation: h_0 and the e_t are drawn on the global torch CPU generator in the reference's order (content (NumPy),
    then h_0, e_0 .. e_{T-1}, each a FloatTensor(n, 16).normal_()) and copied to the device; the reference draws them on
    the device generator on a GPU (models/mocogan.py:297-301), which cannot be reproduced bit for bit."""

    _plan_cls = _GruGenPlan
    _discrete_ok = False
    _gode_graph_capture = False     # GanTrainer(graph=True) refuses this generator (not captured / verified)

    def __new__(cls, *args, **kwargs):
        # __init__ keeps the reference's signature (no ode_fn); a caller that hands this class one is told why not
        if kwargs.get("ode_fn") is not None:
            raise NotImplementedError("the GRU generator integrates no ODE: it takes no ode_fn (ODEFunc and ODEFuncTanh are "
                                      "served by the Neural-ODE generators)")
        return super().__new__(cls)

    def __init__(self, n_channels, dim_z_content, dim_z_category, dim_z_motion, video_length, ngf=64):
        if dim_z_category != 0:
            raise NotImplementedError("categorical latents are not implemented (dim_z_category=0: no reference script "
                                      "uses them)")
        if dim_z_motion != 16 or dim_z_content != 50:
            raise NotImplementedError("libgode's fused GRU kernels are specialised for dim_z_motion=16, "
                                      "dim_z_content=50 (the reference scripts' latent sizes)")
        super().__init__(n_channels, dim_z_content, dim_z_category, dim_z_motion, video_length, ngf=ngf)

    def _init_ode_parts(self, ode_fn, dim_hidden, linear, dim_z, ngf):
        pass                        # recurrent + main only, as the reference's class

    def _param_list(self):
        r = self.recurrent
        return self._decoder_list(), [r.weight_ih, r.weight_hh, r.bias_ih, r.bias_hh]

    def _draw(self, num_samples, video_len):
        """content (NumPy) first, then h_0 and one e_t per frame (models/mocogan.py:252,297-301) as ONE normal_() over
        the reused [T+1, n, 16] host stack: torch's CPU normal_ draws the uniforms in order and transforms them in blocks
        of 16, so with rows of n*16 values this is bitwise the T+1 separate FloatTensor(n, 16).normal_() calls of the
        reference (tests/test_host_gru.py pins it) for a third of the host time -- sample_images draws n*T*2 trajectories."""
        content = np.random.normal(0, 1, (num_samples, self.dim_z_content)).astype(np.float32)
        key = (num_samples, video_len)
        buf = self.__dict__.setdefault("_noise_bufs", {}).get(key)
        if buf is None:
            buf = self._noise_bufs[key] = torch.empty(video_len + 1, num_samples, self.dim_z_motion)
        buf.normal_()
        return torch.from_numpy(content), buf

    _take_trajectories = staticmethod(VideoGeneratorMNISTODERNN._take_trajectories)

    def _draw_motion(self, num_samples, T):
        """h_0 and one e_t per frame -> [T+1, n, 16] (see _draw)"""
        return torch.empty(T + 1, num_samples, self.dim_z_motion).normal_()


# ------------------------------------------------------------------------------------------------------------------
# Neural-SDE motion latent (models/mocogan_sde.py)
# ------------------------------------------------------------------------------------------------------------------
class SDEFunc(nn.Module):
    """Drift f(y) = Wf2 tanh(Wf1 y + bf1) + bf2 and diagonal Ito diffusion g(y) = Wg2 tanh(Wg1 y + bg1) + bg2
    (models/mocogan_sde.py:6-28).  Evaluated inside the fused SDE kernels; calling f / g directly is not part of the
    hot path."""

    def __init__(self, dim, dim_hidden):
        super().__init__()
        self.drift_fn = nn.Sequential(nn.Linear(dim, dim_hidden), nn.Tanh(), nn.Linear(dim_hidden, dim))
        self.diffusion_fn = nn.Sequential(nn.Linear(dim, dim_hidden), nn.Tanh(), nn.Linear(dim_hidden, dim))
        self.noise_type = "diagonal"
        self.sde_type = "ito"

    def f(self, t, x):
        raise RuntimeError("SDEFunc is evaluated inside libgode's fused Euler-Maruyama kernels (gode_sde_fwd/bwd)")

    def g(self, t, x):
        raise RuntimeError("SDEFunc is evaluated inside libgode's fused Euler-Maruyama kernels (gode_sde_fwd/bwd)")


def sde_grid_arrays(T, dt):
    """torchsde's fixed-step loop (BaseSDESolver.integrate + linear_interp, method='euler') for ts = linspace(0, 1, T):
    the solver steps from t to min(t + dt, ts[-1]) while t is short of the next output time and produces that output by
    linear interpolation between the last two states.  All arithmetic is fp32 torch on the host, operation for
    operation the loop's own.  Returns CPU tensors: S (number of steps), dt[S], sqrt_dt[S] (the Brownian increment of
    step k is sqrt_dt[k] * xi_k), emit_at[T] (step after which output j is produced; -1 for output 0, which is the
    initial state), w0[T], w1[T] (output j = w0[j] y_k + w1[j] y_{k+1})."""
    ts = torch.linspace(0, 1, T).float()
    t = ts[0]
    steps = []
    emit_at = torch.full((T,), -1, dtype=torch.int32)
    w0 = torch.zeros(T, dtype=torch.float32)
    w1 = torch.zeros(T, dtype=torch.float32)
    w1[0] = 1.0
    prev_t = t
    for j in range(1, T):
        out_t = ts[j]
        while bool(t < out_t):
            cand = t + dt
            nt = ts[-1] if bool(ts[-1] < cand) else cand         # min(t + dt, ts[-1])
            prev_t = t
            steps.append(nt - t)
            t = nt
        emit_at[j] = len(steps) - 1
        w0[j] = (t - out_t) / (t - prev_t)
        w1[j] = (out_t - prev_t) / (t - prev_t)
    dts = torch.stack(steps) if steps else torch.zeros(0, dtype=torch.float32)
    return dict(S=len(steps), dt=dts, sqrt_dt=torch.sqrt(dts), emit_at=emit_at, w0=w0, w1=w1)


_SDE_GRAD_OFFS = [(0, 1024, (64, 16)), (1024, 64, (64,)), (1088, 1024, (16, 64)), (2112, 16, (16,)),
                  (2128, 256, (16, 16)), (2384, 16, (16,)), (2400, 256, (16, 16)), (2656, 16, (16,)),
                  (2672, 256, (16, 16)), (2928, 16, (16,)), (2944, 256, (16, 16)), (3200, 16, (16,))]


class _SdeGenPlan(_GenPlan):
    """Neural-SDE latent (gode_sde_fwd/bwd) + decoder.  x_host carries [x0 | xi_0 .. xi_{S-1}] = [1+S, n, 16]."""

    rows_in_traj = False
    zcols = 16
    nparam, grad_offs = L.SDE_NPARAM, _SDE_GRAD_OFFS
    grads_from_first_present = True      # no pre-net: the block starts at drift_fn's first weight, nothing in front of it
    multi = None

    def _alloc(self):
        self._sched = self.gen._sde_schedule(self.T, self.device)
        self.S = self._sched["S"]
        f32 = dict(dtype=torch.float32, device=self.device)
        self.states = torch.empty(self.n, self.S + 1, 16, **f32)      # every Euler state, kept for the backward
        self.sde_work = torch.empty(L.lib().gode_sde_bwd_work_size(self.n), **f32)

    def _x_shape(self, n_traj, T):
        return (1 + self.gen._sde_schedule(T, self.device)["S"], n_traj, 16)

    def _params(self):
        g = self.gen
        lin = g.linear
        pre = (None,) * 4 if isinstance(lin, nn.Identity) else (lin[0].weight, lin[0].bias, lin[2].weight, lin[2].bias)
        d, s = g.ode_fn.drift_fn, g.ode_fn.diffusion_fn
        return pre + (d[0].weight, d[0].bias, d[2].weight, d[2].bias, s[0].weight, s[0].bias, s[2].weight, s[2].bias)

    def _programs(self):
        ps = self._params()
        ptrs = tuple(dptr(p) for p in ps)
        if ptrs + (self._draws_on_device(),) != self._ode_ptrs:
            self._ode_ptrs = ptrs + (self._draws_on_device(),)
            prenet = 0 if ps[0] is None else 1
            sc = self._sched
            common = dict(p=L.SdeParams(*ptrs), x=dptr(self.x), sel_t=dptr(self.sel), dt=dptr(sc["dt"]),
                          sqrt_dt=dptr(sc["sqrt_dt"]), emit_at=dptr(sc["emit_at"]), emit_w0=dptr(sc["w0"]),
                          emit_w1=dptr(sc["w1"]), N=self.n, T=self.T, S=self.S, prenet=prenet,
                          zcols=self._zcols)
            self.fwd_op = L.SdeFwdOp(content=dptr(self.content), z=dptr(self._zbuf), states=dptr(self.states), **common)
            self.bwd_op = L.SdeBwdOp(states=dptr(self.states), gz=None, work=dptr(self.sde_work), grads=None,
                                     accumulate=0, **common)
            self.fwd_prog = self._latent_program([self.fwd_op])


class VideoGeneratorSDE(VideoGeneratorMNIST):
    """The class mnist_moco_sde.py:6 imports (models/mocogan_sde.py:31-64): the MNIST generator whose motion latent is
    the Ito SDE dy = f(y) dt + g(y) dW (SDEFunc, diagonal noise) integrated with torchsde's fixed-step Euler-Maruyama
    loop (dt = sde_dt = 2.5e-2) on linspace(0, 1, T), outputs linearly interpolated.  Deviations ("Neural-SDE
    motion latent"): the Brownian increment of step k is sqrt(dt_k) xi_k with xi drawn on the global torch CPU
    generator (torchsde's BrownianInterval cannot be reproduced), x0 is drawn on the CPU generator too, and the
    gradient is the exact gradient of the discrete forward instead of torchsde's continuous adjoint.
    RNG order: sample_videos(n): content (NumPy), x0 = randn(n, 16), xi = randn(S, n, 16); sample_images(n): content and
    x0 of all n*T*2 trajectories, np.random.choice, then xi for the kept trajectories only ([S, n, 16])."""

    _categorical_ok = False     # dim_z_category > 0 is refused: categorical latents exist for the Neural-ODE generators only

    _plan_cls = _SdeGenPlan
    _discrete_ok = False
    _sde_dt = 2.5e-2
    _gode_graph_capture = False     # GanTrainer(graph=True) refuses this generator (not captured / verified)

    def __init__(self, n_channels, dim_z_content, dim_z_category, dim_z_motion, video_length, ode_fn=SDEFunc,
                 dim_hidden=None, linear=True, ngf=64):
        super().__init__(n_channels, dim_z_content, dim_z_category, dim_z_motion, video_length, ode_fn=ode_fn,
                         dim_hidden=dim_hidden, linear=linear, ngf=ngf)

    def _init_ode_parts(self, ode_fn, dim_hidden, linear, dim_z, ngf):
        hid = dim_hidden if dim_hidden else self.dim_z_motion
        if hid != 16:
            raise NotImplementedError(f"dim_hidden={hid}: libgode's fused SDE kernels are specialised for the 16-16-16 "
                                      "drift and diffusion nets of mnist_moco_sde.py:77 (dim_hidden=None -> 16)")
        if not (isinstance(ode_fn, type) and issubclass(ode_fn, SDEFunc)):
            raise NotImplementedError("ode_fn must be gan_ode_amd's SDEFunc (models/mocogan_sde.py:6-28): drift and "
                                      "diffusion are evaluated inside the fused HIP kernels, an arbitrary Python callable "
                                      "cannot be")
        # construction order == the reference's: VideoGeneratorMNIST with its defaults (ODEFunc(16, 16), the 28x28
        # `main`, a pre-net), then the SDEFunc replaces ode_fn and `linear` is built again
        super()._init_ode_parts(ODEFunc, None, True, dim_z, ngf)
        fn = ode_fn(dim=self.dim_z_motion, dim_hidden=hid)
        for net in (getattr(fn, "drift_fn", None), getattr(fn, "diffusion_fn", None)):
            lin = list(net) if isinstance(net, nn.Sequential) else []
            if not (len(lin) == 3 and isinstance(lin[0], nn.Linear) and isinstance(lin[1], nn.Tanh)
                    and isinstance(lin[2], nn.Linear) and tuple(lin[0].weight.shape) == (16, 16)
                    and tuple(lin[2].weight.shape) == (16, 16)):
                raise NotImplementedError("ode_fn.drift_fn / diffusion_fn must be Sequential(Linear(16,16), Tanh(), "
                                          "Linear(16,16))")
        if getattr(fn, "noise_type", None) != "diagonal" or getattr(fn, "sde_type", None) != "ito":
            raise NotImplementedError("libgode integrates diagonal-noise Ito SDEs only")
        self.ode_fn = fn
        self.linear = self._make_prenet(linear)

    @property
    def sde_dt(self):
        """torchsde's dt (models/mocogan_sde.py:59); changing it rebuilds the plans (the step count changes)."""
        return self._sde_dt

    @sde_dt.setter
    def sde_dt(self, v):
        self._sde_dt = float(v)
        self.__dict__.pop("_sde_grids", None)
        if hasattr(self, "_pool"):
            self._pool.clear()

    def _sde_schedule(self, T, device):
        """sde_grid_arrays(T, sde_dt) on `device`, cached per (T, device)."""
        key = (T, device)
        cache = self.__dict__.setdefault("_sde_grids", {})
        if key not in cache:
            gd = sde_grid_arrays(T, self._sde_dt)
            cache[key] = {k: (v.to(device) if torch.is_tensor(v) else v) for k, v in gd.items()}
        return cache[key]

    def _apply(self, fn, *a, **k):
        r = super()._apply(fn, *a, **k)
        self.__dict__.pop("_sde_grids", None)
        return r

    def _param_list(self):
        sde = []
        if not isinstance(self.linear, nn.Identity):
            sde += [self.linear[0].weight, self.linear[0].bias, self.linear[2].weight, self.linear[2].bias]
        for net in (self.ode_fn.drift_fn, self.ode_fn.diffusion_fn):
            sde += [net[0].weight, net[0].bias, net[2].weight, net[2].bias]
        return self._decoder_list(), sde

    def _steps(self, T):
        return self._sde_schedule(T, torch.device("cpu"))["S"]

    def _with_noise(self, x0, T):
        """[x0 | xi]: xi = randn(S, n, 16) on the global torch CPU generator, drawn now."""
        n = x0.shape[0]
        buf = torch.empty(1 + self._steps(T), n, self.dim_z_motion)
        buf[0].copy_(x0)
        buf[1:].normal_()                      # == torch.randn(S, n, 16): the same generator consumption and values
        return buf

    def _host_inputs(self, select, num_samples, T):
        """_draw (inherited) gives content (NumPy) and x0 = torch.randn(n, 16); the noise stack xi is drawn after it."""
        if select:        # content and x0 of all n*T*2 trajectories, the choice, then xi of the kept ones (below)
            return super()._host_inputs(True, num_samples, T)
        content, x0 = self._draw(num_samples, T)
        return self._with_noise(x0, T), content, None

    def _take_trajectories(self, x, traj):
        return self._with_noise(x[traj], self.video_length)

    def _draw_motion(self, num_samples, T):
        return self._with_noise(torch.randn(num_samples, self.dim_z_motion), T)


# ------------------------------------------------------------------------------------------------------------------
# Neural-CDE motion latent (models/mocogan_cde.py)
# ------------------------------------------------------------------------------------------------------------------
class CDEFunc(nn.Module):
    """The CDE vector field z -> tanh(linear2(relu(linear1(z)))).view(hidden, input) (models/mocogan_cde.py:13-29),
    Linear(16, 128) and Linear(128, 32) for the reference's call.  Evaluated inside the fused CDE kernels; calling it
    directly is not part of the hot path."""

    def __init__(self, dim, dim_hidden):
        super().__init__()
        self.input_dim = dim
        self.hidden_dim = dim_hidden
        self.linear1 = nn.Linear(dim_hidden, 128)
        self.linear2 = nn.Linear(128, dim * dim_hidden)

    def forward(self, t, z):
        raise RuntimeError("CDEFunc is evaluated inside libgode's fused CDE kernels (gode_cde_fwd/bwd)")


def cde_time_slopes(T):
    """The time channel's per-interval slopes: the fp32 differences of linspace(0, 1, T) (the knots torchcde's spline
    interpolates; the spline's own knots are at t = 0, 1, ..., T-1, so these are its derivatives)."""
    tt = torch.linspace(0, 1, T).float()
    return tt[1:] - tt[:-1]


_CDE_GRAD_OFFS = [(0, 128, (64, 2)), (128, 64, (64,)), (192, 1024, (16, 64)), (1216, 16, (16,)),
                  (1232, 2048, (128, 16)), (3280, 128, (128,)), (3408, 4096, (32, 128)), (7504, 32, (32,))]


class _CdeGenPlan(_GenPlan):
    """Neural-CDE latent (gode_cde_fwd/bwd) + decoder.  x_host carries the noise channel's knots [n, T]."""

    rows_in_traj = False
    zcols = 16
    nparam, grad_offs = L.CDE_NPARAM, _CDE_GRAD_OFFS
    multi = None

    def __init__(self, gen, n_traj, T, select, zbuf=None, x=None):
        if x is None and n_traj > L.CDE_MAX_N:       # (sample_z_m's plan: gode_cde_fwd itself refuses)
            raise ValueError(f"{type(gen).__name__}: {n_traj} trajectories in one solve; the whole-batch error norm of "
                             f"gode_cde_fwd needs all workgroups co-resident, at most {L.CDE_MAX_N} trajectories")
        super().__init__(gen, n_traj, T, select, zbuf=zbuf, x=x)

    def _alloc(self):
        f32 = dict(dtype=torch.float32, device=self.device)
        self.S_cap = int(self.gen.cde_max_steps)
        self.tslope = cde_time_slopes(self.T).to(self.device)
        self.states = torch.empty(self.n, self.S_cap + 1, 16, **f32)      # the state at every accepted step
        self.sched = torch.zeros(2 * self.S_cap, dtype=torch.float64, device=self.device)
        self.counts = torch.zeros(2, dtype=torch.int32, device=self.device)
        ns = L.lib().gode_cde_sync_size(self.n)
        self.sync = torch.zeros(ns, dtype=torch.int32, device=self.device) if ns else None
        self.cde_work = torch.empty(L.lib().gode_cde_bwd_work_size(self.n), **f32)
        self.last_counts = None

    def _x_shape(self, n_traj, T):
        return (n_traj, T)

    def _params(self):
        g = self.gen
        f, fn = g.f, g.ode_fn
        return (f[0].weight, f[0].bias, f[2].weight, f[2].bias, fn.linear1.weight, fn.linear1.bias,
                fn.linear2.weight, fn.linear2.bias)

    def _programs(self):
        ps = self._params()
        key = tuple(dptr(p) for p in ps) + (self.gen.cde_rtol, self.gen.cde_atol, self._draws_on_device())
        if key != self._ode_ptrs:
            self._ode_ptrs = key
            common = dict(p=L.CdeParams(*key[:8]), x=dptr(self.x), tslope=dptr(self.tslope), sel_t=dptr(self.sel),
                          states=dptr(self.states), sched=dptr(self.sched), counts=dptr(self.counts), N=self.n,
                          T=self.T, S_cap=self.S_cap, zcols=self._zcols)
            self.fwd_op = L.CdeFwdOp(content=dptr(self.content), z=dptr(self._zbuf), sync=dptr(self.sync),
                                     rtol=float(self.gen.cde_rtol), atol=float(self.gen.cde_atol), **common)
            self.bwd_op = L.CdeBwdOp(gz=None, work=dptr(self.cde_work), grads=None, accumulate=0, **common)
            self.fwd_prog = self._latent_program([self.fwd_op])

    def check_solve(self):
        """Reads the solve's {accepted, trials} (a host synchronisation with the current stream) and raises when the
        kernel stopped early: more than cde_max_steps accepted steps, the trial limit or a step-size underflow."""
        c = self.counts.cpu().tolist()
        self.last_counts = c
        if c[0] < 0:
            raise RuntimeError(f"{type(self.gen).__name__}: the dopri5 CDE solve stopped after {-c[0] - 1} accepted steps "
                               f"({c[1]} trials): more than cde_max_steps = {self.S_cap} accepted steps, or the step "
                               "size underflowed; raise cde_max_steps or loosen cde_rtol / cde_atol")
        return c

    def forward(self, x_host, content_host, sel_host, training, keep, cls_host=None, no_grad=False):
        if x_host is None:                     # prefetched (checked by _launch_latents)
            return super().forward(None, content_host, sel_host, training, keep)
        self.stage_inputs(x_host, content_host, sel_host, cls_host)
        self.fwd_prog.run(stream_ptr())
        self.check_solve()
        out = self.stack.forward(training)
        self.busy = keep
        return out


class VideoGeneratorCDE(VideoGeneratorMNIST):
    """The class mnist_moco_cde.py:6 imports (models/mocogan_cde.py:32-84): the MNIST generator whose motion latent is
    the Neural CDE dz = F(z) dX, X the backward-difference Hermite cubic spline of [linspace(0, 1, T), x] (x = the
    [n, 16] motion noise, one knot per frame, so video_len must equal dim_z_motion), z0 = f([0, x_0]), solved by
    torchdiffeq's dopri5 (rtol cde_rtol = 1e-4, atol cde_atol = 1e-6: torchcde's defaults) with dense output at
    t = 0..T-1.  Deviations ("Neural-CDE motion latent"): x is drawn on the global torch CPU generator (the
    reference's device generator cannot be reproduced); sample_images integrates only the selected trajectories, so
    its whole-batch error norm runs over those (as VideoGenerator.sample_images with ode_method="dopri5"); and the
    gradient is the exact gradient of the discrete forward instead of torchdiffeq's continuous adjoint.
    RNG order: sample_videos(n): content (NumPy), x = randn(n, 16); sample_images(n): content and x of all n*T*2
    trajectories, then np.random.choice.  Dead parameters (never used by sample_z_m, no gradient): recurrent.*,
    linear.*."""

    _categorical_ok = False     # dim_z_category > 0 is refused: categorical latents exist for the Neural-ODE generators only

    _plan_cls = _CdeGenPlan
    _discrete_ok = False
    _gode_graph_capture = False     # GanTrainer(graph=True) refuses this generator (not captured / verified)
    cde_rtol, cde_atol = 1e-4, 1e-6
    cde_max_steps = 512             # accepted-step capacity of a solve's stored schedule and states

    def __init__(self, n_channels, dim_z_content, dim_z_category, dim_z_motion, video_length, ode_fn=CDEFunc,
                 cde_input_dim=2, dim_hidden=None, linear=True, ngf=64):
        self._cde_args = (cde_input_dim, dim_hidden)
        super().__init__(n_channels, dim_z_content, dim_z_category, dim_z_motion, video_length, ode_fn=ode_fn,
                         dim_hidden=None, linear=linear, ngf=ngf)

    def _init_ode_parts(self, ode_fn, dim_hidden, linear, dim_z, ngf):
        cde_input_dim, dim_hidden = self._cde_args
        del self._cde_args
        if cde_input_dim != 2:
            raise NotImplementedError(f"cde_input_dim={cde_input_dim}: the path of models/mocogan_cde.py is [time, noise] "
                                      "(2 channels), the only one libgode's fused CDE kernels integrate")
        if dim_hidden not in (None, 16):
            raise NotImplementedError(f"dim_hidden={dim_hidden}: libgode's fused CDE kernels are specialised for the "
                                      "16-dimensional state of mnist_moco_cde.py (dim_hidden=None -> dim_z_motion=16)")
        if not (isinstance(ode_fn, type) and issubclass(ode_fn, CDEFunc)):
            raise NotImplementedError("ode_fn must be gan_ode_amd's CDEFunc (models/mocogan_cde.py:13-29): the vector "
                                      "field is evaluated inside the fused HIP kernels, an arbitrary Python callable cannot be")
        # construction order == the reference's: VideoGeneratorMNIST with its defaults (ODEFunc(16, 16), the 28x28
        # `main`, `linear`), then the CDEFunc, `linear` again and the pre-net `f`
        super()._init_ode_parts(ODEFunc, None, True, dim_z, ngf)
        fn = ode_fn(dim=cde_input_dim, dim_hidden=dim_hidden if dim_hidden else self.dim_z_motion)
        l1, l2 = getattr(fn, "linear1", None), getattr(fn, "linear2", None)
        if not (isinstance(l1, nn.Linear) and isinstance(l2, nn.Linear) and tuple(l1.weight.shape) == (128, 16)
                and l1.bias is not None and tuple(l2.weight.shape) == (32, 128) and l2.bias is not None):
            raise NotImplementedError("ode_fn must hold linear1 = Linear(16, 128) and linear2 = Linear(128, 32)")
        self.ode_fn = fn
        self.linear = self._make_prenet(linear)
        d = self.dim_z_motion
        self.f = nn.Sequential(nn.Linear(cde_input_dim, 64), nn.LeakyReLU(0.2), nn.Linear(64, d), nn.LeakyReLU(0.2))

    def _param_list(self):
        fn = self.ode_fn
        cde = [self.f[0].weight, self.f[0].bias, self.f[2].weight, self.f[2].bias, fn.linear1.weight, fn.linear1.bias,
               fn.linear2.weight, fn.linear2.bias]
        return self._decoder_list(), cde

    def _check_len(self, T):
        if T != self.dim_z_motion:
            raise ValueError(f"video_len={T}: models/mocogan_cde.py views the [n, {self.dim_z_motion}] motion noise as "
                             f"[n, video_len, 1], which needs video_len == dim_z_motion ({self.dim_z_motion})")


# ==================================================================================================================
# discriminators
# ==================================================================================================================
def _noise_sigma(use_noise, sigma):
    """The reference takes any sigma and fails deep in forward (None * tensor); here a bad one is refused up front."""
    if not use_noise:
        return sigma
    if sigma is None or isinstance(sigma, bool):
        raise ValueError(f"use_noise=True needs a finite noise sigma >= 0, got {sigma!r}")
    try:
        s = float(sigma)
    except (TypeError, ValueError):
        raise ValueError(f"use_noise=True needs a finite noise sigma >= 0, got {sigma!r}") from None
    if not math.isfinite(s) or s < 0.0:
        raise ValueError(f"use_noise=True needs a finite noise sigma >= 0, got {sigma!r}")
    return s


def dnoise_normals(n, seed, stream, layer, call, offset=0, device="cuda", raw=False):
    """The instance-noise stream of gode.h alone: z of elements [offset, offset + n) for (seed, stream,
    layer, call) as a float32 device tensor (raw=True: the Philox words, as int32)."""
    out = torch.empty(int(n), dtype=torch.float32, device=device)
    L.check(L.lib().gode_dnoise_normals(out.data_ptr(), int(n), int(seed) & 0xFFFFFFFFFFFFFFFF, int(stream), int(layer),
                                        int(call) & 0xFFFFFFFF, int(offset), 1 if raw else 0, stream_ptr()),
            "gode_dnoise_normals")
    return out.view(torch.int32) if raw else out


class Noise(nn.Module):
    """models/mocogan.py:20-29: x + sigma * N(0, 1) when use_noise (train and eval mode alike, gradient the identity), else
    the identity.  The discriminators never call these modules: their plans apply the noise (gode_dnoise_op).  A standalone
    Noise(True, sigma) on a device tensor draws from the same stream with its own seed (torch.initial_seed() at
    construction), stream 0, layer 0 and call counter, over the tensor's channels-last element order."""

    def __init__(self, use_noise, sigma=0.2):
        super().__init__()
        self.use_noise, self.sigma = use_noise, _noise_sigma(use_noise, sigma)
        self.noise_seed, self.noise_stream, self.noise_call = torch.initial_seed() & 0xFFFFFFFFFFFFFFFF, 0, 0

    def forward(self, x):
        if not self.use_noise:
            return x
        _require_gpu(x, "Noise input")
        if x.dtype != torch.float32 or x.dim() < 2:
            raise RuntimeError("Noise: fp32 input [N, C, ...] expected")
        perm = (0,) + tuple(range(2, x.dim())) + (1,)
        shape = tuple(x.shape[i] for i in perm)
        z = dnoise_normals(x.numel(), self.noise_seed, self.noise_stream, 0, self.noise_call, device=x.device)
        self.noise_call += 1
        inv = [perm.index(i) for i in range(x.dim())]
        return x + z.view(shape).permute(*inv) * self.sigma      # fp32(x + fp32(sigma * z)): two roundings, as gode.h


# -- differentiable augmentation (DiffAugment; gode_diffaug_op) -------------------------------------------
DIFFAUG_BITS = {"color": 1 | 2 | 4, "translation": 8, "cutout": 16}


def diffaug_mask(policy):
    """'color,translation,cutout' in any order -> the op's mask bits; None or an empty string: 0 (off)."""
    if policy is None:
        return 0
    if not isinstance(policy, str):
        raise ValueError(f"DiffAugment policy must be a string of comma-separated names or None, got {policy!r}")
    return _diffaug_mask_of(policy)


@functools.lru_cache(maxsize=32)
def _diffaug_mask_of(policy):
    mask = 0
    for name in (s.strip() for s in policy.split(",")):
        if not name:
            continue
        if name not in DIFFAUG_BITS:
            raise ValueError(f"DiffAugment policy {policy!r}: unknown component {name!r} (known: "
                             + ", ".join(DIFFAUG_BITS) + ")")
        mask |= DIFFAUG_BITS[name]
    return mask


def diffaug_params(n, H, W, seed, stream, call, g0=0):
    """The parameters of samples g0 .. g0 + n - 1 of an H x W map, from the library's host function (no launch, no GPU):
    (ints int32 [n, 4] = tx, ty, cx, cy; unis float32 [n, 3] = u_b, u_s, u_c)."""
    ints, unis = np.empty((int(n), 4), dtype=np.int32), np.empty((int(n), 3), dtype=np.float32)
    L.check(L.lib().gode_diffaug_params(ints.ctypes.data, unis.ctypes.data, int(n), int(seed) & 0xFFFFFFFFFFFFFFFF, int(stream),
                                        int(call) & 0xFFFFFFFF, int(g0), int(H), int(W)), "gode_diffaug_params")
    return ints, unis


# (shape, strides, mask, backward) -> (op struct with the layout filled in, output shape, floats of the output, float offset of
# the workspace, floats of the workspace).  The discriminators see a handful of layouts; the struct is copied at launch.
_DIFFAUG_OPS = {}


def _diffaug_run(x, backward, mask, seed, stream, call, g0):
    """One gode_diffaug launch (two with contrast) over x [N, C, H, W] / [N, C, D, H, W] of any strides -> the contiguous
    channels-last result [N, D, H, W, C].  The result and the sums' workspace behind it are one allocation."""
    key = (x.shape, x.stride(), mask, backward)
    ent = _DIFFAUG_OPS.get(key)
    if ent is None:
        if len(_DIFFAUG_OPS) >= 64:
            _DIFFAUG_OPS.clear()
        N, Cc = x.shape[0], x.shape[1]
        D, H, W = (x.shape[2], x.shape[3], x.shape[4]) if x.dim() == 5 else (1, x.shape[2], x.shape[3])
        n = x.numel()
        op = L.DiffAugOp(xs=(C.c_int64 * 5)(*_strides5(x)), N=N, C=Cc, D=D, H=H, W=W, mask=mask, backward=int(backward))
        ent = _DIFFAUG_OPS[key] = (op, (N, D, H, W, Cc), n, n + (n & 1), L.lib().gode_diffaug_work_size(N, D, H, W, mask))
    op, oshape, n, woff, nwork = ent
    buf = torch.empty(woff + nwork if nwork else n, dtype=torch.float32, device=x.device)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    call = int(call) & 0xFFFFFFFF
    op.x, op.out = x.data_ptr(), buf.data_ptr()
    op.work = buf.data_ptr() + 4 * woff if nwork else None          # (8-byte aligned: woff is even)
    op.seed, op.g0, op.stream = seed - (1 << 64) if seed >= 1 << 63 else seed, int(g0), int(stream)
    op.call = call - (1 << 32) if call >= 1 << 31 else call
    L.run_one(op, stream_ptr())
    return (buf[:n] if nwork else buf).view(oshape)


def _from_channels_last(t, ndim):
    """[N, D, H, W, C] -> the [N, C, D, H, W] (ndim 5) or [N, C, H, W] (ndim 4) permuted view."""
    return t.permute(0, 4, 1, 2, 3) if ndim == 5 else t.squeeze(1).permute(0, 3, 1, 2)


class _DiffAugFn(torch.autograd.Function):
    """The augmentation as one autograd node; its backward is the same op in its other direction, on the same parameters."""

    @staticmethod
    def forward(ctx, x, mask, seed, stream, call, g0):
        ctx.args = (mask, seed, stream, call, g0)
        return _from_channels_last(_diffaug_run(x, 0, mask, seed, stream, call, g0), x.dim())

    @staticmethod
    def backward(ctx, g):
        return _from_channels_last(_diffaug_run(g, 1, *ctx.args), g.dim()), None, None, None, None, None


def _diffaug_apply(x, mask, seed, stream, call, g0, what):
    _require_gpu(x, what)
    if x.dtype != torch.float32 or x.dim() not in (4, 5):
        raise RuntimeError(f"{what}: fp32 input [N, C, H, W] or [N, C, D, H, W] expected")
    if torch.is_grad_enabled() and x.requires_grad:
        return _DiffAugFn.apply(x, mask, seed, stream, call, g0)
    return _from_channels_last(_diffaug_run(x, 0, mask, seed, stream, call, g0), x.dim())      # (no node to record)


class DiffAugment(nn.Module):
    """Differentiable augmentation (Zhao et al., NeurIPS 2020) as one HIP op: `policy` is a comma-separated subset of 'color'
    (brightness, saturation, contrast), 'translation' (up to 1/8 of the map, zero fill) and 'cutout' (half the map), applied to
    fp32 device tensors [N, C, H, W] or [N, C, D, H, W] of any strides with ONE parameter set per sample (a clip stays
    temporally consistent).  Returns a permuted view of the channels-last result with the input's shape; gradients flow
    through it.  The parameters are a pure function of (seed, stream, call, sample_offset + position in the batch) -- see
    include/gode.h and diffaug_params; `call` advances by one per forward.  Plain attributes, no buffers.  An empty policy
    returns its input."""

    def __init__(self, policy, seed=None, stream=0):
        super().__init__()
        self.policy, self.mask = policy, diffaug_mask(policy)
        self.seed = (torch.initial_seed() if seed is None else int(seed)) & 0xFFFFFFFFFFFFFFFF
        self.stream, self.call, self.sample_offset = int(stream), 0, 0

    def forward(self, x):
        if not self.mask:
            return x
        y = _diffaug_apply(x, self.mask, self.seed, self.stream, self.call, self.sample_offset, "DiffAugment input")
        self.call = (self.call + 1) & 0xFFFFFFFF
        return y


class _DiscFn(torch.autograd.Function):
    """One pass of a discriminator as one autograd node: over x1 alone (x2 None; x1 may want its gradient), or over
    [x1; x2] (real and fake batches of equal shape, detached) with per-group BatchNorm statistics on a groups=2 plan.
    Returns the raw channels-last output [B, Do, Ho, Wo, C] ([2B, ...] for the pair, x1's group first)."""

    @staticmethod
    def forward(ctx, plan, training, keep, arena, noise, x1, x2, *params):
        out = plan.forward(training, x=x1, x_strides=_strides5(x1), x2=x2,
                           x2_strides=None if x2 is None else _strides5(x2), noise=noise)
        plan.busy = keep
        ctx.plan, ctx.lease, ctx.arena = plan, _Lease(plan), arena
        ctx.x_dim, ctx.paired = x1.dim(), x2 is not None
        return out

    @staticmethod
    def backward(ctx, gout):
        plan, arena = ctx.plan, ctx.arena
        ctx.lease.check("discriminator (paired pass)" if ctx.paired else "discriminator")
        need_x = ctx.needs_input_grad[5]
        if ctx.paired and (need_x or ctx.needs_input_grad[6]):
            raise NotImplementedError("the paired discriminator pass is for discriminator updates (detached inputs)")
        need_p = any(ctx.needs_input_grad[7:])
        into = _grads_into(arena, plan.params) if need_p and arena is not None and arena.active else None
        _, views, g_in = plan.backward(gout, need_input_grad=need_x, need_param_grad=need_p, into=into)
        grads = _flat_grads(views) if need_p and into is None else [None] * (len(ctx.needs_input_grad) - 7)
        gx = None
        if need_x:      # g_in: [N, D, H, W, C] channels-last, allocated for this call
            gx = g_in.permute(0, 4, 1, 2, 3) if ctx.x_dim == 5 else g_in.squeeze(1).permute(0, 3, 1, 2)
        return (None, None, None, None, None, gx, None, *grads)


class _DiscBase(nn.Module):
    # ConvStack(two_lane_backward=...): the weight gradients of a backward pass on a second stream next to the input-gradient
    # chain.  UCF iteration 16.83 -> 16.53 ms, MNIST / ODE-RNN -0.3 / -0.5 % (same box, same run).
    two_lane_backward = True

    _gode_direct_grads = True

    def _specs(self, x_shape):
        raise NotImplementedError

    # -- instance noise -------------------------------------------------------------------------------
    # Plain attributes, not buffers: the state_dict keys stay the reference's.  noise_seed / noise_stream pick the stream,
    # _noise_call counts the reference's forward calls (forward: one, forward_pair_joint: two), _noise_sample_offset is the
    # first global sample of the batch this module sees (data-parallel ranks, virtual-replica shards: GanTrainer sets it).
    NOISED_LAYERS = ()

    def _init_noise(self, use_noise, noise_sigma, stream):
        self.use_noise = bool(use_noise)
        self.noise_sigma = _noise_sigma(use_noise, noise_sigma)
        self.noise_seed = torch.initial_seed() & 0xFFFFFFFFFFFFFFFF
        self.noise_stream = stream
        self._noise_call, self._noise_sample_offset = 0, 0
        # differentiable augmentation, off by default: `diffaug` is a DiffAugment policy string applied to
        # every input in train mode, in front of the instance noise; plain attributes as above.  diffaug_call counts the
        # forwards (a paired pass: two), _diffaug_sample_offset is the first global sample of the batch (GanTrainer sets it).
        self.diffaug = None
        self.diffaug_seed = torch.initial_seed() & 0xFFFFFFFFFFFFFFFF
        self.diffaug_stream = stream
        self.diffaug_call, self._diffaug_sample_offset = 0, 0

    def _noise_active(self):
        """sigma 0 adds exact zeros: the plan then stays the noise-free one (the call counter still advances)."""
        return self.use_noise and self.noise_sigma > 0.0

    def _noise_args(self, ncalls):
        """This call's noise arguments (forward: ncalls 1, forward_pair_joint: 2); advances the call counter.  Inside a graph
        capture the base call is read from the HostFeed, which rewrites it before every replay."""
        if not self.use_noise:
            return None
        call = self._noise_call
        self._noise_call = (call + ncalls) & 0xFFFFFFFF
        if not self._noise_active():
            return None
        feed = getattr(self, "_feed", None)
        dev = feed.dnoise_slot(self, call, ncalls) if (feed is not None and feed.recording) else None
        return dict(seed=self.noise_seed, stream=self.noise_stream, sigma=self.noise_sigma, call=call, call_dev=dev,
                    sample_offset=self._noise_sample_offset)

    def _layer_params(self):
        out = []
        mods = list(self.main)
        for i, m in enumerate(mods):
            if isinstance(m, (nn.Conv2d, nn.Conv3d)):
                nxt = mods[i + 1] if i + 1 < len(mods) else None
                if isinstance(nxt, (nn.BatchNorm2d, nn.BatchNorm3d)):
                    out.append(LayerParams(m.weight, nxt.weight, nxt.bias, nxt.running_mean, nxt.running_var,
                                           nxt.num_batches_tracked))
                else:
                    out.append(LayerParams(m.weight))
        return out

    def _apply(self, fn, *a, **k):
        r = super()._apply(fn, *a, **k)
        if hasattr(self, "_pool"):
            self._pool.clear()
        return r

    def invalidate_packs(self):
        """See VideoGenerator.invalidate_packs."""
        for k in [k for k in self._pool.pack_cache if k[0] == "ver"]:
            del self._pool.pack_cache[k]

    @staticmethod
    def _logits(out, ndim):
        """The stack's channels-last output -> the reference's squeezed logits for an ndim-dimensional input."""
        h = out.permute(0, 4, 1, 2, 3)
        if ndim == 4:
            h = h.squeeze(2)       # (a squeeze, not h[:, :, 0]: select's backward allocates a zero tensor and copies)
        return h.squeeze()

    def forward(self, input):
        return self._logits(self._forward_raw(input), input.dim()), None

    def _forward_raw(self, first, second=None):
        """The stack's output as written, channels-last [B, Do, Ho, Wo, C]: one pass over `first`, or (forward_pair_joint)
        over [first; second] on a groups=2 plan."""
        _require_gpu(self.main[1].weight, type(self).__name__)
        xs = [first] if second is None else [first, second]
        for t in xs:
            _require_gpu(t, type(self).__name__ + " input")
            if t.dtype != torch.float32:
                raise RuntimeError("fp32 input expected")
        shape, n = tuple(first.shape), len(xs)
        if second is not None:
            if shape != tuple(second.shape):
                raise RuntimeError("paired pass: both inputs must have the same shape")
            if first.requires_grad or second.requires_grad:
                raise RuntimeError("paired pass: inputs must be detached (it is the discriminator-update pass)")
        mask = diffaug_mask(self.diffaug) if self.training and self.diffaug else 0
        if mask:           # one op per input (call c for `first`, c + 1 for `second`: what two forwards draw)
            call = self.diffaug_call
            xs = [_diffaug_apply(t, mask, self.diffaug_seed, self.diffaug_stream, call + i, self._diffaug_sample_offset,
                                 type(self).__name__ + " input") for i, t in enumerate(xs)]
            self.diffaug_call = (call + n) & 0xFFFFFFFF
            first, second = xs[0], (xs[1] if n == 2 else None)
        key = (("pair",) if n == 2 else ()) + shape + (("noise",) if self._noise_active() else ())
        plan = self._pool.get(key, lambda: ConvStack(self._specs((n * shape[0],) + shape[1:]), self._layer_params(),
                                                     self.main[1].weight.device, owns_input=False,
                                                     pack_cache=self._pool.pack_cache, groups=n,
                                                     two_lane_backward=self.two_lane_backward))
        params = _flat_params(self._layer_params())
        keep = torch.is_grad_enabled() and any(t.requires_grad for t in xs + params)
        noise = self._noise_args(n)
        return _DiscFn.apply(plan, self.training, keep, getattr(self, "_gode_arena", None), noise, first, second, *params)

    def forward_pair_joint(self, first, second):
        """D(first) and D(second) in ONE pass -- the same launches over [first; second] with PER-GROUP BatchNorm batch
        statistics, i.e. the arithmetic of the reference's two calls `dis(real)`, `dis(fake)` (mnist_moco_ode.py:119-124,
        137-143): running statistics receive first's update, then second's.  Returns the joint raw logits
        [2B, Do, Ho, Wo, 1] (first group first); GanTrainer feeds them to bce_with_logits_halves.  Twice the rows per
        launch fill the GPU better (video-D GEMMs +14 %) and every elementwise / reduction launch is issued once."""
        return self._forward_raw(first, second)

    def forward_pair(self, first, second):
        """-> ((logits_first, None), (logits_second, None)) with forward()'s shapes."""
        out = self.forward_pair_joint(first, second)
        B = first.shape[0]
        return tuple((self._logits(h, first.dim()), None) for h in (out[:B], out[B:]))


class PatchImageDiscriminator(_DiscBase):
    """models/mocogan.py:66-93: Conv2d k4 s2 p1 x4 (C->ndf->2ndf->4ndf->1), BN on layers 2-3, LeakyReLU(0.2)."""

    NOISED_LAYERS = (0, 1, 2, 3)        # every convolution's input, the head's included (models/mocogan.py:72-89)

    def __init__(self, n_channels, ndf=64, use_noise=False, noise_sigma=None):
        super().__init__()
        self._init_noise(use_noise, noise_sigma, stream=2)
        self.n_channels, self.ndf = n_channels, ndf
        self.main = nn.Sequential(
            Noise(use_noise, sigma=noise_sigma), nn.Conv2d(n_channels, ndf, 4, 2, 1, bias=False),
            nn.LeakyReLU(0.2, inplace=True),
            Noise(use_noise, sigma=noise_sigma), nn.Conv2d(ndf, ndf * 2, 4, 2, 1, bias=False), nn.BatchNorm2d(ndf * 2),
            nn.LeakyReLU(0.2, inplace=True),
            Noise(use_noise, sigma=noise_sigma), nn.Conv2d(ndf * 2, ndf * 4, 4, 2, 1, bias=False),
            nn.BatchNorm2d(ndf * 4), nn.LeakyReLU(0.2, inplace=True),
            Noise(use_noise, sigma=noise_sigma), nn.Conv2d(ndf * 4, 1, 4, 2, 1, bias=False))
        self._pool = _Pool()

    def _specs(self, x_shape):
        B, Cc, H, W = x_shape
        ndf = self.ndf
        chans = [Cc, ndf, ndf * 2, ndf * 4, 1]
        specs = []
        for i in range(4):
            Ho, Wo = conv_out(H, 4, 2, 1), conv_out(W, 4, 2, 1)
            specs.append(LayerSpec(make_geom(B, chans[i], chans[i + 1], (1, H, W), (1, Ho, Wo), (1, 4, 4), (1, 2, 2),
                                             (0, 1, 1)), L.FPROP, L.ACT_LRELU if i < 3 else L.ACT_NONE, i in (1, 2),
                                   noise=self._noise_active() and i in self.NOISED_LAYERS))
            H, W = Ho, Wo
        return specs


class VideoDiscriminator(_DiscBase):
    """models/mocogan.py:129-164: Conv3d ksize^3, stride (1,2,2), pad (0,1,1) x4 + a final ksize^3 s1 p0 conv."""

    NOISED_LAYERS = (0, 1, 2, 3)        # the final ndf*8 -> 1 convolution has no Noise in front (models/mocogan.py:138-159)

    def __init__(self, n_channels, n_output_neurons=1, bn_use_gamma=True, use_noise=False, noise_sigma=None, ndf=64,
                 ksize=4):
        super().__init__()
        if int(n_output_neurons) != n_output_neurons or not (1 <= n_output_neurons <= 1 + MAX_CATEG):
            raise NotImplementedError(f"n_output_neurons={n_output_neurons}: 1 (the reference's scripts) up to "
                                      f"{1 + MAX_CATEG} (CategoricalVideoDiscriminator with {MAX_CATEG} classes)")
        self._init_noise(use_noise, noise_sigma, stream=1)
        self.n_channels, self.n_output_neurons = n_channels, n_output_neurons
        self.bn_use_gamma, self.ndf, self.ksize = bn_use_gamma, ndf, ksize
        st, pd = (1, 2, 2), (0, 1, 1)
        self.main = nn.Sequential(
            Noise(use_noise, sigma=noise_sigma), nn.Conv3d(n_channels, ndf, ksize, stride=st, padding=pd, bias=False),
            nn.LeakyReLU(0.2, inplace=True),
            Noise(use_noise, sigma=noise_sigma), nn.Conv3d(ndf, ndf * 2, ksize, stride=st, padding=pd, bias=False),
            nn.BatchNorm3d(ndf * 2), nn.LeakyReLU(0.2, inplace=True),
            Noise(use_noise, sigma=noise_sigma), nn.Conv3d(ndf * 2, ndf * 4, ksize, stride=st, padding=pd, bias=False),
            nn.BatchNorm3d(ndf * 4), nn.LeakyReLU(0.2, inplace=True),
            Noise(use_noise, sigma=noise_sigma), nn.Conv3d(ndf * 4, ndf * 8, ksize, stride=st, padding=pd, bias=False),
            nn.BatchNorm3d(ndf * 8), nn.LeakyReLU(0.2, inplace=True),
            nn.Conv3d(ndf * 8, n_output_neurons, ksize, 1, 0, bias=False))
        self._pool = _Pool()

    def _specs(self, x_shape):
        B, Cc, D, H, W = x_shape
        ndf, k = self.ndf, self.ksize
        chans = [Cc, ndf, ndf * 2, ndf * 4, ndf * 8]
        specs = []
        for i in range(4):
            Do, Ho, Wo = conv_out(D, k, 1, 0), conv_out(H, k, 2, 1), conv_out(W, k, 2, 1)
            specs.append(LayerSpec(make_geom(B, chans[i], chans[i + 1], (D, H, W), (Do, Ho, Wo), (k, k, k), (1, 2, 2),
                                             (0, 1, 1)), L.FPROP, L.ACT_LRELU, i > 0,
                                   noise=self._noise_active() and i in self.NOISED_LAYERS))
            D, H, W = Do, Ho, Wo
        Do, Ho, Wo = conv_out(D, k, 1, 0), conv_out(H, k, 1, 0), conv_out(W, k, 1, 0)
        specs.append(LayerSpec(make_geom(B, chans[4], self.n_output_neurons, (D, H, W), (Do, Ho, Wo), (k, k, k), (1, 1, 1),
                                         (0, 0, 0)), L.FPROP, L.ACT_NONE, False))
        return specs


class CategoricalVideoDiscriminator(VideoDiscriminator):
    """models/mocogan.py:167-182: a VideoDiscriminator whose final convolution has n_output_neurons + dim_categorical
    outputs; forward -> (labels [B, n_output_neurons], categ [B, dim_categorical]), two views of the ONE [B, 1 + C] head
    buffer the stack wrote (autograd sums their gradients into one upstream tensor and the stack's backward runs once).
    Where the stack's output is not 1x1x1 (the 28x28 MNIST videos with ksize=2: 11x2x2 positions) the reference's
    squeeze() + split give labels [B, n_out, Do, Ho, Wo] and categ [B, C, Do, Ho, Wo], and so does this class.
    The head (<= 31 columns, K = 8 ndf k^3) runs on the stack's generic implicit-GEMM and weight-gradient kernels (DESIGN
    section 13).  `ndf`, `ksize` are keyword extensions, as on VideoDiscriminator."""

    def __init__(self, n_channels, dim_categorical, n_output_neurons=1, use_noise=False, noise_sigma=None, ndf=64, ksize=4):
        if int(dim_categorical) != dim_categorical or not (1 <= dim_categorical <= MAX_CATEG):
            raise NotImplementedError(f"dim_categorical={dim_categorical}: 1 .. {MAX_CATEG} classes")
        super().__init__(n_channels=n_channels, n_output_neurons=n_output_neurons + dim_categorical, use_noise=use_noise,
                         noise_sigma=noise_sigma, ndf=ndf, ksize=ksize)
        self.dim_categorical = dim_categorical

    def split(self, input):
        return input[:, :input.size(1) - self.dim_categorical], input[:, input.size(1) - self.dim_categorical:]

    def forward_head(self, input):
        """The raw head as ONE channels-last tensor [B, Do, Ho, Wo, n_output_neurons] (labels | categ columns per output
        position) -- what the fused losses (train.bce_ce_head*) read; [B, n_output_neurons] when the output is 1x1x1."""
        out = self._forward_raw(input)
        return out.view(out.shape[0], out.shape[4]) if out.numel() == out.shape[0] * out.shape[4] else out

    def forward(self, input):
        h = self.forward_head(input)
        return self.split(h if h.dim() == 2 else h.permute(0, 4, 1, 2, 3))
