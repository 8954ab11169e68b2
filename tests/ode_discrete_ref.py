"""Discrete backprop through the fixed-grid latent solve, restated in float64 torch WITHOUT autograd (what
gode_ode_bwd computes with backprop = 1, include/gode.h), and the references it is compared with: autograd through
oracle.ode_ref.odeint, and oracle.ode_ref.odeint_adjoint (the continuous adjoint, backprop = 0).

theta = (W1, b1, W2, b2) for f(y) = W2 tanh(W1 y + b1) + b2, or (W1, b1) for f(y) = tanh(W1 y + b1).  States are [N, 16];
gout [T, N, 16] is dL/d(solution).  A grid is (dts [S], emits): emits[s] = [(output j, weight w)] -- output j is
y0 + w (y1 - y0) of step s (w = 1: y1 itself, w = 0: y0)."""
import torch

from oracle import ode_ref

METHODS = ("rk4", "euler", "midpoint")


def solver_grid(tt, step_size=None, substeps=1):
    """The forward solve's steps: the output times split into `substeps` equal steps each, or torchdiffeq's step_size grid
    with its linear interpolation of the outputs (oracle.ode_ref.fixed_grid_solve's own loop)."""
    T = len(tt)
    if step_size is None:
        dts, emits = [], []
        for j in range(T - 1):
            for ss in range(substeps):
                dts.append((tt[j + 1] - tt[j]) / substeps)
                emits.append([(j + 1, 1.0)] if ss == substeps - 1 else [])
        return dts, emits
    grid = ode_ref._grid_from_step_size(tt, step_size)
    dts, emits, j = [], [], 1
    for a, b in zip(grid[:-1], grid[1:]):
        here = []
        while j < T and b >= tt[j]:
            here.append((j, 0.0 if tt[j] == a else (1.0 if tt[j] == b else float((tt[j] - a) / (b - a)))))
            j += 1
        dts.append(b - a)
        emits.append(here)
    assert j == T
    return dts, emits


def _h(theta, u):
    return torch.tanh(u @ theta[0].T + theta[1])


def _k(theta, h):
    return h @ theta[2].T + theta[3] if len(theta) == 4 else h


def _vjp(theta, grads, g, u, h):
    """J^T g at u (h = tanh(W1 u + b1)); the stage's parameter VJP is added to `grads` (same order as theta)."""
    if len(theta) == 4:
        grads[3] += g.sum(0)
        grads[2] += g.T @ h
        du = (g @ theta[2]) * (1 - h * h)
    else:
        du = g * (1 - h * h)
    grads[1] += du.sum(0)
    grads[0] += du.T @ u
    return du @ theta[0]


def reverse_step(theta, grads, method, y0, dt, lam):
    """lambda = dL/dy1 -> dL/dy0 of ONE solver step from y0; the three recurrences of include/gode.h."""
    if method == "euler":
        return lam + _vjp(theta, grads, dt * lam, y0, _h(theta, y0))
    if method == "midpoint":
        h1 = _h(theta, y0)
        u2 = y0 + dt / 2 * _k(theta, h1)
        gu2 = _vjp(theta, grads, dt * lam, u2, _h(theta, u2))
        return lam + gu2 + _vjp(theta, grads, dt / 2 * gu2, y0, h1)
    h1 = _h(theta, y0)
    k1 = _k(theta, h1)
    u2 = y0 + dt * k1 / 3
    h2 = _h(theta, u2)
    k2 = _k(theta, h2)
    u3 = y0 + dt * (k2 - k1 / 3)
    h3 = _h(theta, u3)
    k3 = _k(theta, h3)
    u4 = y0 + dt * (k1 - k2 + k3)
    h4 = _h(theta, u4)
    gu4 = _vjp(theta, grads, dt / 8 * lam, u4, h4)
    gu3 = _vjp(theta, grads, 3 * dt / 8 * lam + dt * gu4, u3, h3)
    gu2 = _vjp(theta, grads, 3 * dt / 8 * lam - dt * gu4 + dt * gu3, u2, h2)
    gu1 = _vjp(theta, grads, dt / 8 * lam + dt * gu4 - dt / 3 * gu3 + dt / 3 * gu2, y0, h1)
    return lam + gu1 + gu2 + gu3 + gu4


def forward_step(theta, method, y0, dt):
    f = lambda y: _k(theta, _h(theta, y))   # noqa: E731
    if method == "euler":
        return y0 + dt * f(y0)
    if method == "midpoint":
        return y0 + dt * f(y0 + dt / 2 * f(y0))
    k1 = f(y0)
    k2 = f(y0 + dt * k1 / 3)
    k3 = f(y0 + dt * (k2 - k1 / 3))
    k4 = f(y0 + dt * (k1 - k2 + k3))
    return y0 + (k1 + 3 * (k2 + k3) + k4) * dt * 0.125


def discrete_backprop(theta, method, y0, tt, gout, step_size=None, substeps=1):
    """-> dL/dy0 [N, 16], [dL/dtheta] for L = sum(solution * gout), by the explicit reverse steps (no autograd)."""
    with torch.no_grad():
        theta = [p.detach() for p in theta]
        dts, emits = solver_grid(tt, step_size, substeps)
        starts, y = [], y0.detach()
        for dt in dts:                              # the forward re-run: every step's start state
            starts.append(y)
            y = forward_step(theta, method, y, dt)
        grads = [torch.zeros_like(p) for p in theta]
        lam = torch.zeros_like(y0)
        for s in range(len(dts) - 1, -1, -1):
            after = torch.zeros_like(lam)
            for j, w in emits[s]:                   # an interpolated output: w gz before the reverse step, (1 - w) gz after
                lam = lam + w * gout[j]
                after = after + (1 - w) * gout[j]
            lam = reverse_step(theta, grads, method, starts[s], dts[s], lam) + after
        return lam + gout[0], grads


def solve(f, y0, tt, method, step_size=None, substeps=1, adjoint=False):
    """The float64 oracle's solution [T, N, 16], differentiable: autograd through ode_ref.odeint, or (adjoint) through
    ode_ref.odeint_adjoint.  substeps = k: the same call per output interval on the k-fold refined grid."""
    if substeps == 1:
        opts = None if step_size is None else {"step_size": step_size}
        return (ode_ref.odeint_adjoint if adjoint else ode_ref.odeint)(f, y0, tt, method=method, options=opts)
    assert step_size is None and not adjoint
    sol = [y0]
    for j in range(len(tt) - 1):
        a, b = tt[j], tt[j + 1]
        fine = torch.cat([a + (b - a) / substeps * torch.arange(substeps, dtype=tt.dtype), b.reshape(1)])
        sol.append(ode_ref.odeint(f, sol[-1], fine, method=method)[-1])
    return torch.stack(sol)


def autograd_reference(f, y0, tt, method, gout, step_size=None, substeps=1, adjoint=False):
    """-> solution, dL/dy0, [dL/dtheta in f.parameters() order] of L = sum(solution * gout) on the float64 oracle."""
    y0 = y0.detach().requires_grad_(True)
    f.zero_grad()
    sol = solve(f, y0, tt, method, step_size, substeps, adjoint)
    (sol * gout).sum().backward()
    # (T = 1: no step, the function is never called and its parameters get no gradient)
    return sol.detach(), y0.grad.clone(), [torch.zeros_like(p) if p.grad is None else p.grad.clone() for p in f.parameters()]
