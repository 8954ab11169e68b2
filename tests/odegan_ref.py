"""Test infrastructure: restatement of ODE-GAN training (stage2/ode_training.py of the reference) on stock torch, in the
precision of the tensors it is given (the tests feed it fp64), and of its gradient penalty both ways: exactly, by
double backward (create_graph=True), and by the central difference of DESIGN section 14.

The step rules are written from the Runge-Kutta tableaux, not from the reference's incremental updates: with
f(theta) = -grad L(theta), Euler is theta + lr f(theta); Heun averages f at theta and at the Euler point; RK4 takes
its four slopes at theta, theta + lr/2 k1, theta + lr/2 k2, theta + lr k3 and combines them with weights 1/6, 1/3,
1/3, 1/6 (the reference reaches the same point by increments from wherever the parameters stand).
The penalty enters the final update only: -reg * gp for Euler, -reg * lr * gp for the other two.
"""
import numpy as np
import torch


def _grads(loss, params):
    return torch.autograd.grad(loss, params, allow_unused=True)


def ode_step(params, loss_fn, method, lr, reg=0.0, gp=None):
    """One step on `params` in place; tensors the loss does not reach stay untouched.  gp: the penalty gradient per
    parameter (taken at the starting point) or None.  Returns the loss at the starting point."""
    start = [p.detach().clone() for p in params]

    def slope():
        loss = loss_fn()
        return loss, [None if g is None else -g for g in _grads(loss, params)]

    def move_to(combo):
        """theta = start + sum_j w_j * k_j for combo = [(w_j, k_j)]"""
        with torch.no_grad():
            for i, p in enumerate(params):
                if combo[0][1][i] is None:
                    continue
                p.copy_(start[i] + sum(w * k[i] for w, k in combo))

    loss1, k1 = slope()
    if method == "euler":
        final, pen = [(lr, k1)], reg
    elif method == "rk2":
        move_to([(lr, k1)])
        _, k2 = slope()
        final, pen = [(lr / 2, k1), (lr / 2, k2)], reg * lr
    elif method == "rk4":
        move_to([(lr / 2, k1)])
        _, k2 = slope()
        move_to([(lr / 2, k2)])
        _, k3 = slope()
        move_to([(lr, k3)])
        _, k4 = slope()
        final, pen = [(lr / 6, k1), (lr / 3, k2), (lr / 3, k3), (lr / 6, k4)], reg * lr
    else:
        raise AssertionError(method)
    move_to(final)
    if gp is not None:
        with torch.no_grad():
            for p, g in zip(params, gp):
                p.sub_(pen * g)
    return loss1


def exact_penalty(g_loss, g_params, d_params):
    """grad_{d_params} || grad_{g_params} g_loss ||^2 by double backward (one g_loss call)."""
    v = torch.autograd.grad(g_loss(), g_params, create_graph=True, allow_unused=True)
    mag = sum(g.square().sum() for g in v if g is not None)
    return [g.detach() for g in torch.autograd.grad(mag, d_params)]


def rng_state():
    return torch.get_rng_state(), np.random.get_state()


def set_rng_state(s):
    torch.set_rng_state(s[0])
    np.random.set_state(s[1])


def central_penalty(g_loss, g_params, d_params, h):
    """The same quantity from first-order passes: 2 d/d eps [grad_{d} g_loss(thetaG + eps v)] with v = grad_{thetaG} g_loss
    fixed, as (q+ - q-) / eps, eps = h (1 + |thetaG|) / |v|.  Every evaluation sees the same random draws; the generators
    are left as after one g_loss call and thetaG as found.  Returns (gp list, eps)."""
    s0 = rng_state()
    v = _grads(g_loss(), g_params)
    s1 = rng_state()
    saved = [p.detach().clone() for p in g_params]
    nv = float(sum(g.double().square().sum() for g in v if g is not None)) ** 0.5
    nt = float(sum(p.double().square().sum() for p in saved)) ** 0.5
    if nv == 0.0:
        return [torch.zeros_like(p) for p in d_params], 0.0
    eps = h * (1.0 + nt) / nv
    q = []
    for sign in (1.0, -1.0):
        set_rng_state(s0)
        with torch.no_grad():
            for p, s, g in zip(g_params, saved, v):
                if g is not None:
                    p.copy_(s + sign * eps * g)
        q.append(torch.autograd.grad(g_loss(), d_params))
    with torch.no_grad():
        for p, s in zip(g_params, saved):
            p.copy_(s)
    set_rng_state(s1)
    return [(a - b) / eps for a, b in zip(*q)], eps


def ode_step_sum64(p, terms, cq=None, qp=None, qm=None):
    """fp64 value of p + sum c_k g_k + cq (q+ - q-) and the magnitude |p| + sum |c_k g_k| + |cq| (|q+| + |q-|), from fp32
    arrays and fp32-rounded coefficients."""
    out, mag = p.astype(np.float64), np.abs(p.astype(np.float64))
    for c, g in terms:
        c = float(np.float32(c))
        out = out + c * g.astype(np.float64)
        mag = mag + np.abs(c * g.astype(np.float64))
    if cq is not None:
        cq = float(np.float32(cq))
        out = out + cq * (qp.astype(np.float64) - qm.astype(np.float64))
        mag = mag + abs(cq) * (np.abs(qp.astype(np.float64)) + np.abs(qm.astype(np.float64)))
    return out, mag
