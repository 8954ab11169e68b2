"""Restatement of the Neural-SDE motion latent (gode_sde_fwd / gode_sde_bwd) for the SDE tests: torchsde's fixed-step
Euler-Maruyama loop on the schedule of sde_grid_arrays, Brownian increments sqrt(dt_k) xi_k, in the dtype of the
parameters (float64 for the reference, float32 for the reference's own rounding error); gradients come from torch
autograd.  restate() and _params() run on the CPU; _sched_dev() and _ops() put a schedule and the two op structs on the
GPU.  Shared by tests/test_gpu_sde.py, tests/test_gpu_latent_schedules.py and tests/test_host_latent_schedules.py."""
import torch
import torch.nn.functional as F

import gan_ode_amd._lib as L


def restate(params, x, grid, prenet):
    """params: [Wa ba Wb bb] (prenet) + [Wf1 bf1 Wf2 bf2 Wg1 bg1 Wg2 bg2]; x [1+S, N, 16] = x0, xi.
    -> states [N, S+1, 16], outputs [N, T, 16] in the dtype of the parameters."""
    dt_ = params[-1].dtype
    Wf1, bf1, Wf2, bf2, Wg1, bg1, Wg2, bg2 = params[-8:]
    y = x[0].to(dt_)
    if prenet:
        Wa, ba, Wb, bb = params[:4]
        y = F.leaky_relu(F.leaky_relu(y @ Wa.t() + ba, 0.2) @ Wb.t() + bb, 0.2)
    Y = [y]
    for k in range(grid["S"]):
        h = grid["dt"][k].to(dt_)
        dw = grid["sqrt_dt"][k].to(dt_) * x[1 + k].to(dt_)
        f = torch.tanh(y @ Wf1.t() + bf1) @ Wf2.t() + bf2
        g = torch.tanh(y @ Wg1.t() + bg1) @ Wg2.t() + bg2
        y = y + f * h + g * dw
        Y.append(y)
    outs = [Y[0]]
    for j in range(1, len(grid["emit_at"])):
        k = int(grid["emit_at"][j])
        outs.append(grid["w0"][j].to(dt_) * Y[k] + grid["w1"][j].to(dt_) * Y[k + 1])
    return torch.stack(Y, 1), torch.stack(outs, 1)


def _params(prenet, gen=None, scale=0.4):
    gen = gen or torch.Generator().manual_seed(3)
    shapes = ([(64, 16), (64,), (16, 64), (16,)] if prenet else []) + [(16, 16), (16,), (16, 16), (16,)] * 2
    return [torch.randn(s, generator=gen) * scale for s in shapes]


def _sched_dev(grid):
    return {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in grid.items()}


def _ops(P, prenet, N, T, sd, x, content, sel, z, states, zcols):
    """-> (SdeFwdOp, SdeBwdOp).  states None: the forward stores no states (the backward op is then not runnable)."""
    ptrs = [p.data_ptr() for p in P]
    prm = L.SdeParams(*(ptrs if prenet else [None] * 4 + ptrs))
    common = dict(p=prm, x=x.data_ptr(), sel_t=None if sel is None else sel.data_ptr(), dt=sd["dt"].data_ptr(),
                  sqrt_dt=sd["sqrt_dt"].data_ptr(), emit_at=sd["emit_at"].data_ptr(), emit_w0=sd["w0"].data_ptr(),
                  emit_w1=sd["w1"].data_ptr(), N=N, T=T, S=sd["S"], prenet=int(prenet), zcols=zcols)
    st = None if states is None else states.data_ptr()
    fop = L.SdeFwdOp(content=None if content is None else content.data_ptr(), z=z.data_ptr(), states=st, **common)
    bop = L.SdeBwdOp(states=st, gz=None, work=None, grads=None, accumulate=0, **common)
    return fop, bop


def grads_of(loss, params):
    """autograd gradients of `loss` w.r.t. `params`, zeros for tensors the loss does not depend on (S = 0: the drift and
    diffusion nets; S = 0 without the pre-net: everything)."""
    if not loss.requires_grad:
        return [torch.zeros_like(p) for p in params]
    gs = torch.autograd.grad(loss, params, retain_graph=True, allow_unused=True)
    return [torch.zeros_like(p) if g is None else g for g, p in zip(gs, params)]
